// The crowd demo's front end on the device (include/p2m.h, "The crowd demo's front end"): p2m_crowd_select - add_pelvis /
// add_neck, the score filter and the greedy suppression of duplicate detections of demo/run.py:127-146, 276-306 for a batch of
// images - and p2m_person_colours, run.py:314's random hue per person from the project's Philox stream.
// One block per image.  The image's detections are staged in LDS once (fp32 inputs as they are, the float64 midpoints beside
// them); the P (P - 1) / 2 pair tests, which are independent, are spread over the block's waves, one pair per lane, and a
// ballot turns a row of them into the 64-bit mask "earlier slots this one matches"; the greedy scan, which is serial by
// definition, then runs on ONE wave over those masks with the masks in registers (readlane, scalar bit operations: 64 short
// iterations at most), and the compaction is a popcount of the accepted mask below each bit.  No atomics.
// This file is compiled with -ffp-contract=off (build.py): the header defines every operation as rounded once, unfused.
#include "p2m_common.h"
#include "p2m_philox.h"

#pragma STDC FP_CONTRACT OFF

namespace p2m {

constexpr int CROWD_THREADS = 256;
constexpr int CROWD_MAX_MID = 8;
constexpr uint32_t ST_PERSON_COLOUR = 11;

struct CrowdArgs {
  const float* dets;
  const int* num;
  int B, P, J, n_mid;
  uint64_t mid_a, mid_b;           // byte m = the two input joints of midpoint m
  double pose_thr, score_thr, min_diff;
  float* joints;
  int* count;
  int* index;
  int8_t* reason;
  int* dup_of;
  double* score;
  uint8_t* keep;
};

// LDS image of one image's detections.  Person stride of the fp32 coordinates: an ODD number of 8-byte units, so that the 32
// lanes of a ds_read_b64 group, which read the same joint of 32 different people, fall on 32 different bank pairs.
struct CrowdLds {
  int stride8;
  size_t xm, cm, valid, match, elig, xf, cf, bad, src, cnt, bytes;
};
__host__ __device__ inline CrowdLds crowd_lds(int P, int J, int n_mid) {
  CrowdLds l;
  l.stride8 = J | 1;
  size_t o = 0;
  l.xm = o;    o += (size_t)16 * P * n_mid;       // double2 [P][n_mid]
  l.cm = o;    o += (size_t)8 * P * n_mid;        // double  [P][n_mid]
  l.valid = o; o += (size_t)8 * P;                // uint64  [P]   bit j: conf_j > pose_thr
  l.match = o; o += (size_t)8 * P;                // uint64  [P]   bit d < p: the pair (p, d) tests as a duplicate
  l.elig = o;  o += 8;                            // uint64        bit p: finite and not low: takes part in the scan
  l.xf = o;    o += (size_t)8 * P * l.stride8;    // float2  [P][stride8]
  l.cf = o;    o += (size_t)4 * P * J;            // float   [P][J]
  l.bad = o;   o += (size_t)4 * P;                // int     [P]   a non-finite input value
  l.src = o;   o += (size_t)4 * P;                // int     [P]   input slot of compacted person k
  l.cnt = o;   o += 4;
  l.bytes = (o + 15) & ~(size_t)15;
  return l;
}

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < __builtin_inff(); }

__global__ __launch_bounds__(CROWD_THREADS) void k_crowd_select(const CrowdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char crowd_smem[];
  const int P = a.P, J = a.J, n_mid = a.n_mid, Jo = J + n_mid;
  const CrowdLds L = crowd_lds(P, J, n_mid);
  double2* xm = (double2*)(crowd_smem + L.xm);
  double* cm = (double*)(crowd_smem + L.cm);
  uint64_t* valid = (uint64_t*)(crowd_smem + L.valid);
  uint64_t* match = (uint64_t*)(crowd_smem + L.match);
  uint64_t* eligp = (uint64_t*)(crowd_smem + L.elig);
  float2* xf = (float2*)(crowd_smem + L.xf);
  float* cf = (float*)(crowd_smem + L.cf);
  int* bad = (int*)(crowd_smem + L.bad);
  int* src = (int*)(crowd_smem + L.src);
  int* cntp = (int*)(crowd_smem + L.cnt);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  int Pn = a.num ? a.num[b] : P;
  Pn = __builtin_amdgcn_readfirstlane(min(max(Pn, 0), P));
  const float* det = a.dets + (size_t)b * P * J * 3;

  // 1. stage the filled slots: fp32 as they are (widening to float64 later is exact)
  for (int p = tid; p < P; p += CROWD_THREADS) bad[p] = 0;
  __syncthreads();
  for (int e = tid; e < Pn * J; e += CROWD_THREADS) {
    const int p = e / J, j = e - p * J;
    const float x = det[(size_t)e * 3], y = det[(size_t)e * 3 + 1], c = det[(size_t)e * 3 + 2];
    xf[p * L.stride8 + j] = make_float2(x, y);
    cf[p * J + j] = c;
    if (!(finitef(x) && finitef(y) && finitef(c))) bad[p] = 1;        // (every writer writes the same value)
  }
  __syncthreads();
  // 2. midpoints, float64
  for (int e = tid; e < Pn * n_mid; e += CROWD_THREADS) {
    const int p = e / n_mid, m = e - p * n_mid;
    const int ja = (int)((a.mid_a >> (8 * m)) & 0xFF), jb = (int)((a.mid_b >> (8 * m)) & 0xFF);
    const float2 va = xf[p * L.stride8 + ja], vb = xf[p * L.stride8 + jb];
    xm[e] = make_double2(((double)va.x + (double)vb.x) * 0.5, ((double)va.y + (double)vb.y) * 0.5);
    cm[e] = (double)cf[p * J + ja] * (double)cf[p * J + jb];
  }
  __syncthreads();
  // 3. per slot (wave 0, lane = slot): the score, sequential in index order, the validity bits, and what kind of slot it is
  const double qnan = __longlong_as_double(0x7FF8000000000000LL);
  double my_score = qnan;
  int my_kind = -1;                      // -1 at or beyond num, 0 takes part in the scan, 1 low score, 3 non-finite
  if (wave == 0) {
    if (lane < Pn) {
      double sc = 0.0;
      uint64_t vb = 0;
      for (int j = 0; j < J; ++j) {
        const double c = (double)cf[lane * J + j];
        sc = sc + c;
        vb |= (uint64_t)(c > a.pose_thr) << j;
      }
      for (int m = 0; m < n_mid; ++m) {
        const double c = cm[lane * n_mid + m];
        sc = sc + c;
        vb |= (uint64_t)(c > a.pose_thr) << (J + m);
      }
      valid[lane] = vb;
      if (bad[lane]) my_kind = 3;
      else {
        my_score = sc;
        my_kind = sc < a.score_thr ? 1 : 0;
      }
    }
    const uint64_t el = __ballot(my_kind == 0);
    if (lane == 0) *eligp = el;
  }
  __syncthreads();
  // 4. the pair tests.  Rows r and Pn - 1 - r share a wave step: lanes [0, r) hold the pairs (r, d), lanes [r, Pn - 1) the
  //    pairs (Pn - 1 - r, d): Pn - 1 <= 63 lanes busy whatever the row.
  const uint64_t elig = *eligp;
  for (int r = wave; r < (Pn + 1) / 2; r += CROWD_THREADS / 64) {
    const int r2 = Pn - 1 - r;
    int pi = -1, pd = 0;
    if (lane < r) { pi = r; pd = lane; }
    else if (r2 != r && lane - r < r2) { pi = r2; pd = lane - r; }
    bool dup = false;
    if (pi >= 0 && (elig >> pi & 1) && (elig >> pd & 1)) {
      const uint64_t vm = valid[pi] & valid[pd];
      const float2* xi = xf + pi * L.stride8;
      const float2* xd = xf + pd * L.stride8;
      double S = 0.0;
      int n = 0;
      for (int j = 0; j < J; ++j) {
        const bool on = vm >> j & 1;
        const float2 u = xi[j], w = xd[j];
        const double tx = on ? fabs((double)u.x - (double)w.x) : 0.0;
        const double ty = on ? fabs((double)u.y - (double)w.y) : 0.0;
        S = S + tx;                       // (adding the +0 of a left-out term changes no bit of S >= 0)
        n += tx != 0.0;
        S = S + ty;
        n += ty != 0.0;
      }
      for (int m = 0; m < n_mid; ++m) {
        const bool on = vm >> (J + m) & 1;
        const double2 u = xm[pi * n_mid + m], w = xm[pd * n_mid + m];
        const double tx = on ? fabs(u.x - w.x) : 0.0;
        const double ty = on ? fabs(u.y - w.y) : 0.0;
        S = S + tx;
        n += tx != 0.0;
        S = S + ty;
        n += ty != 0.0;
      }
      dup = n == 0 || S / (double)n < a.min_diff;
    }
    const uint64_t bal = __ballot(dup);
    if (lane == 0) {
      match[r] = bal & ((uint64_t(1) << r) - 1);                                    // r < 32
      if (r2 != r) match[r2] = (bal >> r) & ((uint64_t(1) << r2) - 1);              // r2 <= 63
    }
  }
  __syncthreads();
  // 5. the greedy scan (wave 0; lane = slot), serial over the slots on the scalar unit
  if (wave == 0) {
    const uint64_t my_match = lane < Pn ? match[lane] : 0;
    const int m_lo = (int)(uint32_t)my_match, m_hi = (int)(uint32_t)(my_match >> 32);
    uint64_t acc = 0;
    for (int p = 0; p < Pn; ++p) {
      const uint64_t mp = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(m_lo, p) |
                          (uint64_t)(uint32_t)__builtin_amdgcn_readlane(m_hi, p) << 32;
      const int kp = __builtin_amdgcn_readlane(my_kind, p);
      if (kp == 0 && (mp & acc) == 0) acc |= uint64_t(1) << p;
    }
    const int cnt = __popcll(acc);
    if (lane < P) {
      const bool acc_me = acc >> lane & 1;
      const int reason = my_kind != 0 ? my_kind : (acc_me ? 0 : 2);
      const size_t o = (size_t)b * P + lane;
      a.reason[o] = (int8_t)reason;
      a.keep[o] = reason == 0;
      a.dup_of[o] = reason == 2 ? __ffsll((unsigned long long)(my_match & acc)) - 1 : -1;
      a.score[o] = my_score;
      if (acc_me) src[__popcll(acc & ((uint64_t(1) << lane) - 1))] = lane;
    }
    if (lane == 0) {
      *cntp = cnt;
      a.count[b] = cnt;
    }
  }
  __syncthreads();
  // 6. the compacted people; every other slot is NaN
  const int cnt = *cntp;
  for (int p = tid; p < P; p += CROWD_THREADS) a.index[(size_t)b * P + p] = p < cnt ? src[p] : -1;
  float* out = a.joints + (size_t)b * P * Jo * 3;
  const float fnan = __int_as_float(0x7FC00000);
  for (int e = tid; e < P * Jo; e += CROWD_THREADS) {
    const int k = e / Jo, j = e - k * Jo;
    float x = fnan, y = fnan, c = fnan;
    if (k < cnt) {
      const int p = src[k];
      if (j < J) {
        const float2 v = xf[p * L.stride8 + j];
        x = v.x;
        y = v.y;
        c = cf[p * J + j];
      } else {
        const double2 v = xm[p * n_mid + (j - J)];
        x = (float)v.x;
        y = (float)v.y;
        c = (float)cm[p * n_mid + (j - J)];
      }
    }
    out[(size_t)e * 3] = x;
    out[(size_t)e * 3 + 1] = y;
    out[(size_t)e * 3 + 2] = c;
  }
}

// ---- p2m_person_colours -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_person_colours(const uint64_t* __restrict__ state, int n, double s, double v,
                                                        float* __restrict__ rgb, uint8_t* __restrict__ u8) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const Philox4 d = philox_draw(state[0], state[1] + (uint64_t)k, 0, ST_PERSON_COLOUR, 0);
  const double h = (double)(d.w[0] >> 8) * 0x1p-24;
  double c0 = v, c1 = v, c2 = v;
  if (s != 0.0) {
    const double h6 = h * 6.0;
    const int i = (int)h6;
    const double f = h6 - (double)i;
    const double p = v * (1.0 - s), q = v * (1.0 - s * f), t = v * (1.0 - s * (1.0 - f));
    switch (i % 6) {
      case 0: c0 = v; c1 = t; c2 = p; break;
      case 1: c0 = q; c1 = v; c2 = p; break;
      case 2: c0 = p; c1 = v; c2 = t; break;
      case 3: c0 = p; c1 = q; c2 = v; break;
      case 4: c0 = t; c1 = p; c2 = v; break;
      default: c0 = v; c1 = p; c2 = q; break;
    }
  }
  if (rgb) {
    rgb[(size_t)k * 3] = (float)c0;
    rgb[(size_t)k * 3 + 1] = (float)c1;
    rgb[(size_t)k * 3 + 2] = (float)c2;
  }
  if (u8) {
    u8[(size_t)k * 3] = (uint8_t)(int)rint(255.0 * c0);
    u8[(size_t)k * 3 + 1] = (uint8_t)(int)rint(255.0 * c1);
    u8[(size_t)k * 3 + 2] = (uint8_t)(int)rint(255.0 * c2);
  }
}

}  // namespace p2m

using namespace p2m;

static inline bool finite64(double v) { return v - v == 0.0; }

extern "C" int p2m_crowd_select(const float* dets, const int32_t* num, int32_t B, int32_t P, int32_t J, const int32_t* midpoints,
                                int32_t n_mid, double pose_thr, double score_thr, double min_diff, float* joints,
                                int32_t* count, int32_t* index, int8_t* reason, int32_t* dup_of, double* score, uint8_t* keep,
                                void* stream) {
  P2M_CHECK_ARG(dets && joints && count && index && reason && dup_of && score && keep, "null pointer");
  P2M_CHECK_ARG(B >= 1 && B <= (1 << 24), "B outside [1, 2^24]");
  P2M_CHECK_ARG(P >= 1 && P <= 64, "P outside [1, 64]");
  P2M_CHECK_ARG(J >= 1, "J < 1");
  P2M_CHECK_ARG(n_mid >= 0 && n_mid <= CROWD_MAX_MID, "n_mid outside [0, 8]");
  P2M_CHECK_ARG(J <= 64 - n_mid, "J + n_mid > 64");
  P2M_CHECK_ARG(n_mid == 0 || midpoints, "null midpoints");
  P2M_CHECK_ARG(finite64(pose_thr) && finite64(score_thr) && finite64(min_diff), "a threshold is not finite");
  P2M_CHECK_ARG((uintptr_t)score % 8 == 0, "misaligned score");
  CrowdArgs a;
  a.mid_a = a.mid_b = 0;
  for (int m = 0; m < n_mid; ++m) {
    const int32_t ja = midpoints[2 * m], jb = midpoints[2 * m + 1];
    P2M_CHECK_ARG(ja >= 0 && ja < J && jb >= 0 && jb < J, "a midpoint index outside [0, J)");
    a.mid_a |= (uint64_t)ja << (8 * m);
    a.mid_b |= (uint64_t)jb << (8 * m);
  }
  a.dets = dets;
  a.num = num;
  a.B = B;
  a.P = P;
  a.J = J;
  a.n_mid = n_mid;
  a.pose_thr = pose_thr;
  a.score_thr = score_thr;
  a.min_diff = min_diff;
  a.joints = joints;
  a.count = count;
  a.index = index;
  a.reason = reason;
  a.dup_of = dup_of;
  a.score = score;
  a.keep = keep;
  const CrowdLds L = crowd_lds(P, J, n_mid);        // at most 57.4 KB (P = 64, J = 56, n_mid = 8): under the 64 KB default
  hipLaunchKernelGGL(k_crowd_select, dim3(B), dim3(CROWD_THREADS), L.bytes, (hipStream_t)stream, a);
  return check_launch("p2m_crowd_select");
}

extern "C" int p2m_person_colours(const uint64_t* state, int32_t n, double s, double v, float* rgb, uint8_t* u8, void* stream) {
  P2M_CHECK_ARG(state, "null state");
  P2M_CHECK_ARG((uintptr_t)state % 8 == 0, "misaligned state");
  P2M_CHECK_ARG(rgb || u8, "rgb and u8 are both NULL");
  P2M_CHECK_ARG(n >= 1 && n <= (1 << 24), "n outside [1, 2^24]");
  P2M_CHECK_ARG(s >= 0.0 && s <= 1.0 && v >= 0.0 && v <= 1.0, "s, v outside [0, 1]");
  hipLaunchKernelGGL(k_person_colours, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, state, n, s, v, rgb, u8);
  return check_launch("p2m_person_colours");
}
