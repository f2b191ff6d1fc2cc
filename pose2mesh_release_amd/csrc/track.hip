// People across video frames on the device (include/p2m.h, "Tracking people across frames"): p2m_pose_track - which person of
// this frame is which person of the frames before.  A small state machine per video stream: gated greedy assignment of the
// frame's people to the stream's track slots by a masked, size-normalised mean joint distance, births into free slots,
// retirement after max_missed frames without a detection.
// One block per stream; the frames of a call are walked in order inside the kernel.  Per frame: one wave per person / per
// track stages the (x, y) of the Jo joints in LDS (lane = joint; the validity mask and the "all finite" test are ballots,
// the track's extent a wave reduction of exact fp32 max / min); the P T pair costs, which are independent, are spread over
// the block, one pair per thread, each a sequential float64 loop over the joints as the contract orders it, and stay in LDS;
// a greedy round is a block-wide arg-min of (cost, track, person) - shuffles inside a wave, one LDS slot per wave, ONE barrier
// per round (the slots alternate) - after which every thread holds the same winner and the same taken-masks in registers;
// births and the per-slot bookkeeping are popcounts over 64-bit masks on wave 0; the pose copy is a flat coalesced loop.
// No atomics.  This file is compiled with -ffp-contract=off (build.py): the header defines every operation as rounded once.
#include <mutex>

#include "p2m_common.h"

#pragma STDC FP_CONTRACT OFF

namespace p2m {

constexpr int TRACK_THREADS = 256;
constexpr int TRACK_WAVES = TRACK_THREADS / 64;
constexpr int TRACK_MAX = 64;                     // people per frame, track slots, joints

struct TrackArgs {
  const float* people;
  int F, S, P, T, Jo;
  double pose_thr, gate;
  int min_common, max_missed;
  float* st_pose;
  int* st_uid;
  int* st_missed;
  int* st_next;
  float* joints;
  int* slot_of;
  int* person_of;
  int* uid;
  uint8_t* flags;
  double* cost;
  int* dropped;
};

// LDS image of one stream's frame.  Row stride of the float2 coordinates: an ODD number of 8-byte units, so that the 32 lanes
// of a ds_read_b64 group, which read the same joint of 32 different people, fall on 32 different bank pairs (the track of
// those lanes is one address: a broadcast).  The small per-slot arrays are sized for the caps.
struct TrackLds {
  int stride8;
  size_t cost, pxy, txy, tsize, pvalid, tvalid, mcost, wcost, widx, pflag, slot, person, uid, missed, bytes;
};
__host__ __device__ inline TrackLds track_lds(int P, int T, int Jo) {
  TrackLds l;
  l.stride8 = Jo | 1;
  size_t o = 0;
  l.cost = o;   o += (size_t)8 * P * T;             // double [T][P]  the pair's cost, +inf where there is no candidate
  l.pxy = o;    o += (size_t)8 * P * l.stride8;     // float2 [P][stride8]
  l.txy = o;    o += (size_t)8 * T * l.stride8;     // float2 [T][stride8]
  o = (o + 15) & ~(size_t)15;
  l.tsize = o;  o += 8 * TRACK_MAX;                 // double [T]
  l.pvalid = o; o += 8 * TRACK_MAX;                 // uint64 [P]     bit j: conf_j > pose_thr
  l.tvalid = o; o += 8 * TRACK_MAX;                 // uint64 [T]
  l.mcost = o;  o += 8 * TRACK_MAX;                 // double [T]     cost of the slot's matched pair, NaN otherwise
  l.wcost = o;  o += 8 * 2 * TRACK_WAVES;           // double [2][waves]  a round's best per wave (the halves alternate)
  l.widx = o;   o += 4 * 2 * TRACK_WAVES;           // int    [2][waves]
  l.pflag = o;  o += 4 * TRACK_MAX;                 // int    [P]     present: all 3 Jo values finite
  l.slot = o;   o += 4 * TRACK_MAX;                 // int    [P]     matched slot, -1
  l.person = o; o += 4 * TRACK_MAX;                 // int    [T]     the slot's person this frame, -1
  l.uid = o;    o += 4 * TRACK_MAX;                 // int    [T]     state, kept here over the frames of a call
  l.missed = o; o += 4 * TRACK_MAX;                 // int    [T]
  l.bytes = (o + 15) & ~(size_t)15;
  return l;
}

__device__ __forceinline__ bool track_finite(float v) { return fabsf(v) < __builtin_inff(); }
__device__ __forceinline__ uint64_t below(int b) { return (uint64_t(1) << b) - 1; }        // b <= 63
__device__ __forceinline__ int kth_bit(uint64_t m, int k) {                                 // k < popcount(m)
  for (int i = 0; i < k; ++i) m &= m - 1;
  return __ffsll((unsigned long long)m) - 1;
}

// One wave stages one pose: lane = joint.  Returns (wave-uniform) the validity mask; *all_finite likewise.
__device__ __forceinline__ uint64_t track_stage(const float* src, int Jo, int lane, double pose_thr, float2* row,
                                                bool* all_finite, float* x_out, float* y_out) {
  float x = 0.f, y = 0.f, c = 0.f;
  if (lane < Jo) {
    x = src[lane * 3];
    y = src[lane * 3 + 1];
    c = src[lane * 3 + 2];
    row[lane] = make_float2(x, y);
  }
  const uint64_t bad = __ballot(!(track_finite(x) && track_finite(y) && track_finite(c)));
  *all_finite = bad == 0;
  *x_out = x;
  *y_out = y;
  return __ballot(lane < Jo && (double)c > pose_thr);
}

__global__ __launch_bounds__(TRACK_THREADS) void k_pose_track(const TrackArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char track_smem[];
  const int P = a.P, T = a.T, Jo = a.Jo, PT = P * T;
  const TrackLds L = track_lds(P, T, Jo);
  double* cost = (double*)(track_smem + L.cost);
  float2* pxy = (float2*)(track_smem + L.pxy);
  float2* txy = (float2*)(track_smem + L.txy);
  double* tsize = (double*)(track_smem + L.tsize);
  uint64_t* pvalid = (uint64_t*)(track_smem + L.pvalid);
  uint64_t* tvalid = (uint64_t*)(track_smem + L.tvalid);
  double* mcost = (double*)(track_smem + L.mcost);
  double* wcost = (double*)(track_smem + L.wcost);
  int* widx = (int*)(track_smem + L.widx);
  int* pflag = (int*)(track_smem + L.pflag);
  int* slot_l = (int*)(track_smem + L.slot);
  int* person_l = (int*)(track_smem + L.person);
  int* uid_l = (int*)(track_smem + L.uid);
  int* missed_l = (int*)(track_smem + L.missed);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x;
  const size_t pose_sz = (size_t)Jo * 3;
  float* st_pose = a.st_pose + (size_t)s * T * pose_sz;
  const double inf = __builtin_inf();
  const double qnan = __longlong_as_double(0x7FF8000000000000LL);
  const float fnan = __int_as_float(0x7FC00000);
  const uint64_t t_mask = T == 64 ? ~uint64_t(0) : below(T);
  const int max_rounds = min(P, T);

  if (tid < T) {
    uid_l[tid] = a.st_uid[(size_t)s * T + tid];
    missed_l[tid] = a.st_missed[(size_t)s * T + tid];
  }
  int next_uid = a.st_next[s];                     // (used by wave 0 alone)
  __syncthreads();

  for (int f = 0; f < a.F; ++f) {
    const size_t fs = (size_t)f * a.S + s;
    const float* people = a.people + fs * P * pose_sz;
    // 1. stage the frame's people and the stream's alive tracks: one wave per pose, lane = joint
    for (int p = wave; p < P; p += TRACK_WAVES) {
      bool ok;
      float x, y;
      const uint64_t v = track_stage(people + (size_t)p * pose_sz, Jo, lane, a.pose_thr, pxy + p * L.stride8, &ok, &x, &y);
      if (lane == 0) {
        pvalid[p] = v;
        pflag[p] = ok;
      }
    }
    for (int t = wave; t < T; t += TRACK_WAVES) {
      if (uid_l[t] < 0) continue;                  // (wave-uniform)
      bool ok;
      float x, y;
      const uint64_t v = track_stage(st_pose + (size_t)t * pose_sz, Jo, lane, a.pose_thr, txy + t * L.stride8, &ok, &x, &y);
      // the track's extent over its valid joints: fp32 max / min are exact, so the order of the reduction decides nothing
      const bool on = v >> lane & 1;
      float hx = on ? x : -__builtin_inff(), lx = on ? x : __builtin_inff();
      float hy = on ? y : -__builtin_inff(), ly = on ? y : __builtin_inff();
      for (int o = 32; o >= 1; o >>= 1) {
        hx = fmaxf(hx, __shfl_xor(hx, o));
        lx = fminf(lx, __shfl_xor(lx, o));
        hy = fmaxf(hy, __shfl_xor(hy, o));
        ly = fminf(ly, __shfl_xor(ly, o));
      }
      if (lane == 0) {
        const double w = (double)hx - (double)lx, h = (double)hy - (double)ly;
        double size = w > h ? w : h;
        if (!(size >= 1.0)) size = 1.0;            // (also a track without a valid joint: -inf)
        tsize[t] = size;
        tvalid[t] = v;
      }
    }
    if (tid < TRACK_MAX) {
      slot_l[tid] = -1;
      person_l[tid] = -1;
      mcost[tid] = qnan;
    }
    __syncthreads();
    const uint64_t present = __ballot(lane < P && pflag[lane < P ? lane : 0] != 0);
    const uint64_t alive = __ballot(lane < T && uid_l[lane < T ? lane : 0] >= 0);

    // 2. the pair costs, pair e = t P + p: the lanes of a wave share a track (or two) and differ in the person
    for (int e = tid; e < PT; e += TRACK_THREADS) {
      const int t = e / P, p = e - t * P;
      double c = inf;
      if ((present >> p & 1) && (alive >> t & 1)) {
        const uint64_t vm = pvalid[p] & tvalid[t];
        const float2* xp = pxy + p * L.stride8;
        const float2* xt = txy + t * L.stride8;
        double S = 0.0;
        for (int j = 0; j < Jo; ++j) {
          const float2 u = xp[j], w = xt[j];
          const double tx = fabs((double)u.x - (double)w.x), ty = fabs((double)u.y - (double)w.y);
          if (vm >> j & 1) {
            S = S + tx;
            S = S + ty;
          }
        }
        const int n = 2 * __popcll(vm);
        if (n >= 2 * a.min_common) {
          const double v = (S / (double)n) / tsize[t];
          if (v < a.gate) c = v;
        }
      }
      cost[e] = c;
    }
    __syncthreads();

    // 3. greedy, globally ascending: the least (cost, t, p) among the persons and tracks not yet taken, until none is left.
    //    Every thread ends a round with the same winner, so the taken-masks live in registers and the loop's exit is uniform.
    uint64_t p_taken = 0, t_taken = 0;
    for (int r = 0; r < max_rounds; ++r) {
      double bc = inf;
      int be = 0x7FFFFFFF;
      for (int e = tid; e < PT; e += TRACK_THREADS) {       // (ascending e: a strict < keeps the lowest index of a tie)
        const int t = e / P, p = e - t * P;
        const double c = cost[e];
        if (c < bc && !(p_taken >> p & 1) && !(t_taken >> t & 1)) {
          bc = c;
          be = e;
        }
      }
      for (int o = 32; o >= 1; o >>= 1) {
        const double oc = __shfl_xor(bc, o);
        const int oe = __shfl_xor(be, o);
        if (oc < bc || (oc == bc && oe < be)) {
          bc = oc;
          be = oe;
        }
      }
      double* wc = wcost + (r & 1) * TRACK_WAVES;
      int* we = widx + (r & 1) * TRACK_WAVES;
      if (lane == 0) {
        wc[wave] = bc;
        we[wave] = be;
      }
      __syncthreads();
      bc = wc[0];
      be = we[0];
      for (int w = 1; w < TRACK_WAVES; ++w) {
        const double oc = wc[w];
        const int oe = we[w];
        if (oc < bc || (oc == bc && oe < be)) {
          bc = oc;
          be = oe;
        }
      }
      if (!(bc < inf)) break;                               // (uniform)
      const int t = be / P, p = be - t * P;
      p_taken |= uint64_t(1) << p;
      t_taken |= uint64_t(1) << t;
      if (tid == 0) {
        slot_l[p] = t;
        person_l[t] = p;
        mcost[t] = bc;
      }
    }
    __syncthreads();

    // 4. births and the per-slot bookkeeping (wave 0: lane = person, then lane = slot)
    if (wave == 0) {
      const uint64_t unmatched = present & ~p_taken, free0 = ~alive & t_mask;
      const int n_un = __popcll(unmatched), n_free = __popcll(free0);
      const int n_born = min(n_un, n_free);
      if (lane < P && a.slot_of) {
        int so = -1;
        if (present >> lane & 1) {
          if (p_taken >> lane & 1) so = slot_l[lane];
          else {
            const int k = __popcll(unmatched & below(lane));
            so = k < n_free ? kth_bit(free0, k) : -2;
          }
        }
        a.slot_of[fs * P + lane] = so;
      }
      int q = -1, uid_new = -1, missed_new = 0, fl = 0;
      double mc = qnan;
      if (lane < T) {
        q = person_l[lane];
        mc = mcost[lane];
        const int uid_old = uid_l[lane], missed_old = missed_l[lane];
        uid_new = uid_old;
        missed_new = missed_old;
        bool born = false;
        if (free0 >> lane & 1) {
          const int k = __popcll(free0 & below(lane));
          if (k < n_un) {
            q = kth_bit(unmatched, k);
            uid_new = next_uid + k;
            born = true;
          }
        }
        if (q >= 0) {
          missed_new = 0;
          fl = 1 | 2 | (born ? 4 : 0) | (born || missed_old > 0 ? 8 : 0);
        } else if (uid_old >= 0) {
          missed_new = missed_old + 1;
          if (missed_new > a.max_missed) {
            uid_new = -1;
            fl = 16;
          } else {
            fl = 1;
          }
        }
      }
      if (lane < T) {
        person_l[lane] = q;
        uid_l[lane] = uid_new;
        missed_l[lane] = missed_new;
        const size_t o = fs * T + lane;
        if (a.person_of) a.person_of[o] = q;
        if (a.uid) a.uid[o] = uid_new;
        if (a.flags) a.flags[o] = (uint8_t)fl;
        if (a.cost) a.cost[o] = mc;
      }
      next_uid += n_born;
      if (lane == 0 && a.dropped) a.dropped[fs] = n_un - n_born;
    }
    __syncthreads();

    // 5. a slot with a person takes that person's values bit for bit; the frame's output shows NaN in every other slot
    float* out = a.joints ? a.joints + fs * T * pose_sz : nullptr;
    const int n_val = T * (int)pose_sz;
    for (int e = tid; e < n_val; e += TRACK_THREADS) {
      const int t = e / (int)pose_sz, k = e - t * (int)pose_sz;
      const int q = person_l[t];
      float v = fnan;
      if (q >= 0) {
        v = people[(size_t)q * pose_sz + k];
        st_pose[e] = v;
      }
      if (out) out[e] = v;
    }
    __syncthreads();          // the next frame stages the poses just written and overwrites the LDS image
  }

  if (tid < T) {
    a.st_uid[(size_t)s * T + tid] = uid_l[tid];
    a.st_missed[(size_t)s * T + tid] = missed_l[tid];
  }
  if (tid == 0) a.st_next[s] = next_uid;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-device attribute of a kernel; two host threads may get here at
// once.  A mutex-guarded bitmap over the devices of the process (as chebtile.hip's).
static int track_lds_opt_in(size_t bytes) {
  static std::mutex mu;
  static uint64_t done[4] = {0, 0, 0, 0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 256) {
    set_error("p2m_pose_track: no current device");
    return P2M_ERR_HIP;
  }
  std::lock_guard<std::mutex> lock(mu);
  if (done[dev >> 6] >> (dev & 63) & 1) return P2M_OK;
  const hipError_t e = hipFuncSetAttribute((const void*)k_pose_track, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) {
    set_error("p2m_pose_track: %zu bytes of LDS refused: %s", bytes, hipGetErrorString(e));
    return P2M_ERR_HIP;
  }
  done[dev >> 6] |= uint64_t(1) << (dev & 63);
  return P2M_OK;
}

}  // namespace p2m

using namespace p2m;

static inline bool finite64(double v) { return v - v == 0.0; }

extern "C" int p2m_pose_track(const float* people, int32_t F, int32_t S, int32_t P, int32_t T, int32_t Jo, double pose_thr,
                              double gate, int32_t min_common, int32_t max_missed, float* st_pose, int32_t* st_uid,
                              int32_t* st_missed, int32_t* st_next_uid, float* joints, int32_t* slot_of, int32_t* person_of,
                              int32_t* uid, uint8_t* flags, double* cost, int32_t* dropped, void* stream) {
  P2M_CHECK_ARG(people && st_pose && st_uid && st_missed && st_next_uid, "null pointer");
  P2M_CHECK_ARG(F >= 1 && F <= (1 << 24), "F outside [1, 2^24]");
  P2M_CHECK_ARG(S >= 1 && S <= (1 << 24), "S outside [1, 2^24]");
  P2M_CHECK_ARG(P >= 1 && P <= TRACK_MAX, "P outside [1, 64]");
  P2M_CHECK_ARG(T >= 1 && T <= TRACK_MAX, "T outside [1, 64]");
  P2M_CHECK_ARG(Jo >= 1 && Jo <= TRACK_MAX, "Jo outside [1, 64]");
  P2M_CHECK_ARG(min_common >= 1 && min_common <= Jo, "min_common outside [1, Jo]");
  P2M_CHECK_ARG(max_missed >= 0, "max_missed < 0");
  P2M_CHECK_ARG(finite64(pose_thr) && finite64(gate), "a threshold is not finite");
  P2M_CHECK_ARG((uintptr_t)cost % 8 == 0, "misaligned cost");
  TrackArgs a;
  a.people = people;
  a.F = F;
  a.S = S;
  a.P = P;
  a.T = T;
  a.Jo = Jo;
  a.pose_thr = pose_thr;
  a.gate = gate;
  a.min_common = min_common;
  a.max_missed = max_missed;
  a.st_pose = st_pose;
  a.st_uid = st_uid;
  a.st_missed = st_missed;
  a.st_next = st_next_uid;
  a.joints = joints;
  a.slot_of = slot_of;
  a.person_of = person_of;
  a.uid = uid;
  a.flags = flags;
  a.cost = cost;
  a.dropped = dropped;
  // 10,336 B for 16 people, 16 slots and 19 joints; 102,752 B at the caps, beyond the 64 KB a kernel gets unasked: the kernel is
  // opted in to its cap size once per device (no stream operation; the launch itself asks for what the shapes need)
  const TrackLds L = track_lds(P, T, Jo);
  if (const int rc = track_lds_opt_in(track_lds(TRACK_MAX, TRACK_MAX, TRACK_MAX).bytes)) return rc;
  hipLaunchKernelGGL(k_pose_track, dim3(S), dim3(TRACK_THREADS), L.bytes, (hipStream_t)stream, a);
  return check_launch("p2m_pose_track");
}
