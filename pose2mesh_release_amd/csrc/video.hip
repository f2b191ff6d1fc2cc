// The video half of the 3DPW protocol on the GPU (gfx950): the One-Euro filter over ragged batches of sequences
// (p2m_one_euro) and the per-video acceleration error, MPJPE and PA-MPJPE (p2m_video_eval).
//
// Reference arithmetic (numpy on the host there, one frame at a time):
//   OneEuroFilter.__call__, smooth_pose                                        lib/smooth_utils.py:5-72
//   compute_error_accel                                                        lib/coord_utils.py:194-222
//   the smoothed block of evaluate()                                           data/PW3D/dataset.py:383-417
// The filter is plain fp32, every operation rounded once and none fused (this unit is built with -ffp-contract=off):
// on float32 input numpy computes exactly that, so the output equals the reference's bit for bit (include/p2m.h has
// the formula).  The metrics are accumulated in fp64 from the fp32 inputs, as in eval.hip, in fixed orders and without
// atomics: bitwise reproducible, and a sequence's results depend on that sequence alone.  No allocation or
// synchronisation in the launch path (capturable).
#include <cmath>

#include "p2m_eval.h"

namespace p2m {

// ---- (a) the One-Euro filter ---------------------------------------------------------------------------------------------
// One lane per (sequence, VEC consecutive coordinates): a wave reads 64 * VEC consecutive floats of a frame.  The recurrence
// is serial in time; the loads do not depend on it, so frame f + OE_LOOKAHEAD is requested while frame f is filtered, from a
// ring of registers (every ring index is a compile-time constant after unrolling).  In place (y == x, no row table) a lane
// reads and writes only its own coordinates, and a frame is always loaded before the same lane stores it.
// The recurrence is a chain of a few dozen dependent fp32 instructions per frame, two correctly rounded divisions among them
// (one when te == 1, the reference's case: d / 1 == d bitwise, so UNIT_DT drops that division).  A wave therefore spends
// its time waiting on itself, and what hides that is MORE WAVES, not wider accesses: 8- and 16-byte lane accesses divide the
// lane count by 2 and 4, so they are used only once the narrower width already has OE_FILL_LANES lanes in flight
// (p2m_one_euro below).
constexpr int OE_NT = 256;
constexpr int OE_LOOKAHEAD = 16;
constexpr long OE_FILL_LANES = 1024L * 64 * 8;           // 8 waves on each of the chip's 1024 SIMDs

struct OneEuroArgs {
  const float* x;
  const int* seq_ptr;
  const int* rows;
  float* y;
  int N, C, cblocks;
  float mc, b, te, k2, kd;
  float* state_x;
  float* state_dx;
  const int* started;
};

template <int VEC>
__device__ __forceinline__ void oe_load(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else if constexpr (VEC == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  } else {
    v[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void oe_store(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else if constexpr (VEC == 2) *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  else *p = v[0];
}
template <int VEC>
__device__ __forceinline__ void oe_frame(const OneEuroArgs& a, int f, int c0, float (&v)[VEC]) {
  const size_t row = a.rows ? (size_t)a.rows[f] : (size_t)f;
  oe_load<VEC>(a.x + row * (size_t)a.C + c0, v);
}

// one step of the recurrence on the VEC coordinates of a lane (include/p2m.h has the formula)
template <int VEC, bool UNIT_DT>
__device__ __forceinline__ void oe_step(const OneEuroArgs& a, float ad, float ad1, const float (&cur)[VEC], float (&xp)[VEC],
                                        float (&dxp)[VEC]) {
#pragma unroll
  for (int e = 0; e < VEC; e++) {
    const float d = cur[e] - xp[e];
    const float dx = UNIT_DT ? d : d / a.te;
    const float dxh = ad * dx + ad1 * dxp[e];
    const float cut = a.mc + a.b * fabsf(dxh);
    const float r = (a.k2 * cut) * a.te;
    const float al = r / (r + 1.f);
    xp[e] = al * cur[e] + (1.f - al) * xp[e];
    dxp[e] = dxh;
  }
}

template <int VEC, bool UNIT_DT>
__global__ __launch_bounds__(OE_NT) void k_one_euro(OneEuroArgs a) {
  const int s = (int)blockIdx.x / a.cblocks;
  const int c0 = (((int)blockIdx.x - s * a.cblocks) * OE_NT + (int)threadIdx.x) * VEC;
  if (c0 >= a.C) return;
  const int f0 = max(a.seq_ptr[s], 0), f1 = min(a.seq_ptr[s + 1], a.N);
  if (f1 <= f0) return;                                  // an empty sequence: nothing read, nothing written
  float xp[VEC], dxp[VEC];
  int fs = f0;                                           // the first frame that goes through the recurrence
  if (a.started == nullptr || a.started[s] == 0) {       // a fresh sequence: its first frame passes through
    oe_frame<VEC>(a, f0, c0, xp);
#pragma unroll
    for (int e = 0; e < VEC; e++) dxp[e] = 0.f;
    oe_store<VEC>(a.y + (size_t)f0 * a.C + c0, xp);
    fs = f0 + 1;
  } else {
    oe_load<VEC>(a.state_x + (size_t)s * a.C + c0, xp);
    oe_load<VEC>(a.state_dx + (size_t)s * a.C + c0, dxp);
  }
  float ring[OE_LOOKAHEAD][VEC];
#pragma unroll
  for (int k = 0; k < OE_LOOKAHEAD; k++) {
    if (fs + k < f1) oe_frame<VEC>(a, fs + k, c0, ring[k]);
  }
  const float rd = a.kd * a.te;
  const float ad = rd / (rd + 1.f);
  const float ad1 = 1.f - ad;
  // steady state: every frame of the group and every frame it prefetches exists, so the body has no branch and the waits
  // on the ring are counted (a load or store under a branch would turn each of them into a wait for ALL memory traffic)
  int base = fs;
  for (; base + 2 * OE_LOOKAHEAD <= f1; base += OE_LOOKAHEAD) {
#pragma unroll
    for (int k = 0; k < OE_LOOKAHEAD; k++) {
      float cur[VEC];
#pragma unroll
      for (int e = 0; e < VEC; e++) cur[e] = ring[k][e];
      oe_frame<VEC>(a, base + k + OE_LOOKAHEAD, c0, ring[k]);
      oe_step<VEC, UNIT_DT>(a, ad, ad1, cur, xp, dxp);
      oe_store<VEC>(a.y + (size_t)(base + k) * a.C + c0, xp);
    }
  }
  // the last one or two groups: frames and prefetches that may not exist (uniform over the block: scalar branches)
  for (; base < f1; base += OE_LOOKAHEAD) {
#pragma unroll
    for (int k = 0; k < OE_LOOKAHEAD; k++) {
      const int f = base + k;
      if (f < f1) {
        float cur[VEC];
#pragma unroll
        for (int e = 0; e < VEC; e++) cur[e] = ring[k][e];
        if (f + OE_LOOKAHEAD < f1) oe_frame<VEC>(a, f + OE_LOOKAHEAD, c0, ring[k]);
        oe_step<VEC, UNIT_DT>(a, ad, ad1, cur, xp, dxp);
        oe_store<VEC>(a.y + (size_t)f * a.C + c0, xp);
      }
    }
  }
  if (a.state_x) {
    oe_store<VEC>(a.state_x + (size_t)s * a.C + c0, xp);
    oe_store<VEC>(a.state_dx + (size_t)s * a.C + c0, dxp);
  }
}

// The blocks of one k_one_euro launch that cover the same sequence do not run together: none of them may write started[s]
// while another has yet to read it.  This kernel is the later node on the same stream that sets the flags.
__global__ __launch_bounds__(256) void k_one_euro_mark(const int* __restrict__ seq_ptr, int S, int N, int* __restrict__ started) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s < S && min(seq_ptr[s + 1], N) > max(seq_ptr[s], 0)) started[s] = 1;
}

// ---- (b) per-video metrics -----------------------------------------------------------------------------------------------
constexpr int VE_FRAME_COLS = 4;      // frame_sums: accel (0 where undefined), 1 / 0 valid, sum_j mpjpe, sum_j pa_mpjpe
constexpr int VE_SEQ_COLS = 8;
constexpr int VE_TOT_COLS = 8;

// One wave per frame (4 frames per block), lane j = joint j.
__global__ __launch_bounds__(256) void k_video_frames(const float* __restrict__ pred, const float* __restrict__ gt,
                                                      const int* __restrict__ seq_ptr, const unsigned char* __restrict__ vis,
                                                      int N, int S, int J, int want_pa, float* __restrict__ accel,
                                                      unsigned char* __restrict__ accel_valid, float* __restrict__ mpjpe,
                                                      float* __restrict__ pa_mpjpe, double* __restrict__ frame_sums) {
  const int i = blockIdx.x * 4 + (int)threadIdx.x / 64;
  const int lane = (int)threadIdx.x & 63;
  if (i >= N) return;                                    // whole waves leave
  int lo = 0, hi = S;                                    // the last s with seq_ptr[s] <= i: the sequence that owns frame i
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seq_ptr[mid] <= i) lo = mid;
    else hi = mid;
  }
  const int end = min(seq_ptr[lo + 1], N);
  const bool on = lane < J;
  const size_t o = ((size_t)i * J + (on ? lane : 0)) * 3;
  double p[3], g[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    p[k] = on ? (double)pred[o + k] : 0.0;
    g[k] = on ? (double)gt[o + k] : 0.0;
  }
  const double e = dist3(p[0] - g[0], p[1] - g[1], p[2] - g[2]);
  // acceleration error of the triple (i, i + 1, i + 2)
  bool triple = i + 2 < end;
  if (triple && vis) triple = vis[i] != 0 && vis[i + 1] != 0 && vis[i + 2] != 0;
  double an = 0.0;
  if (triple && on) {
    const size_t s1 = (size_t)J * 3;
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double ap = (p[k] - 2.0 * (double)pred[o + s1 + k]) + (double)pred[o + 2 * s1 + k];
      const double ag = (g[k] - 2.0 * (double)gt[o + s1 + k]) + (double)gt[o + 2 * s1 + k];
      d[k] = ap - ag;
    }
    an = dist3(d[0], d[1], d[2]);
  }
  double m[8] = {p[0], p[1], p[2], g[0], g[1], g[2], on ? e : 0.0, an};
  wave_sum<8>(m);
  const double inv = 1.0 / (double)J;
  const double acc = triple ? m[7] * inv : 0.0;
  double pa_sum = 0.0;
  if (want_pa) {                                         // stage E of k_mesh_eval, on the frame's joints as they are
    const double cP[3] = {m[0] * inv, m[1] * inv, m[2] * inv}, cG[3] = {m[3] * inv, m[4] * inv, m[5] * inv};
    double h[10];
    {
      const double u[3] = {on ? p[0] - cP[0] : 0.0, on ? p[1] - cP[1] : 0.0, on ? p[2] - cP[2] : 0.0};
      const double w[3] = {on ? g[0] - cG[0] : 0.0, on ? g[1] - cG[1] : 0.0, on ? g[2] - cG[2] : 0.0};
#pragma unroll
      for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) h[3 * r + c] = u[r] * w[c];
      }
      h[9] = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
    }
    wave_sum<10>(h);
#pragma unroll
    for (int k = 0; k < 10; k++) h[k] *= inv;
    double R[9], c, t[3];
    similarity_solve(h, h[9], cP, cG, R, &c, t);
    double q[3];
#pragma unroll
    for (int r = 0; r < 3; r++) q[r] = c * (R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2]) + t[r];
    const double pe = dist3(q[0] - g[0], q[1] - g[1], q[2] - g[2]);
    if (on) pa_mpjpe[(size_t)i * J + lane] = (float)pe;
    double sp[1] = {on ? pe : 0.0};
    wave_sum<1>(sp);
    pa_sum = sp[0];
  }
  if (on) mpjpe[(size_t)i * J + lane] = (float)e;
  if (lane == 0) {
    accel[i] = (float)acc;
    accel_valid[i] = triple ? 1 : 0;
    double* fs = frame_sums + (size_t)i * VE_FRAME_COLS;
    fs[0] = acc;
    fs[1] = triple ? 1.0 : 0.0;
    fs[2] = m[6];
    fs[3] = pa_sum;
  }
}

// One block per sequence: thread t sums frames t, t + 256, .. of the sequence in order, then the fixed block tree.
__global__ __launch_bounds__(256) void k_video_seq(const double* __restrict__ frame_sums, const int* __restrict__ seq_ptr, int N,
                                                   int J, int want_pa, double* __restrict__ seq_stats) {
  __shared__ double sh[4 * VE_FRAME_COLS];
  const int s = blockIdx.x;
  const int f0 = max(seq_ptr[s], 0), f1 = max(min(seq_ptr[s + 1], N), f0);
  double a[VE_FRAME_COLS] = {0, 0, 0, 0};
  for (int f = f0 + (int)threadIdx.x; f < f1; f += 256) {
#pragma unroll
    for (int k = 0; k < VE_FRAME_COLS; k++) a[k] += frame_sums[(size_t)f * VE_FRAME_COLS + k];
  }
  block_sum<256, VE_FRAME_COLS>(a, sh);
  if (threadIdx.x == 0) {
    const double frames = (double)(f1 - f0), nan = __builtin_nan("");
    double* o = seq_stats + (size_t)s * VE_SEQ_COLS;
    o[0] = frames;
    o[1] = a[1];
    o[2] = a[1] > 0.0 ? a[0] / a[1] : nan;
    o[3] = frames > 0.0 ? a[2] / (frames * (double)J) : nan;
    o[4] = want_pa ? a[3] : 0.0;
    o[5] = want_pa ? frames * (double)J : 0.0;
    o[6] = 0.0;
    o[7] = 0.0;
  }
}

// One wave: lane l sums sequences l, l + 64, .. in order, then the butterfly.
__global__ __launch_bounds__(64) void k_video_totals(const double* __restrict__ seq_stats, int S, double* __restrict__ totals) {
  double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // accel means, videos with one, mpjpe means, non-empty videos, pa sum, pa count, frames
  for (int s = threadIdx.x; s < S; s += 64) {
    const double* q = seq_stats + (size_t)s * VE_SEQ_COLS;
    if (q[1] > 0.0) { a[0] += q[2]; a[1] += 1.0; }
    if (q[0] > 0.0) { a[2] += q[3]; a[3] += 1.0; }
    a[4] += q[4];
    a[5] += q[5];
    a[6] += q[0];
  }
  wave_sum<8>(a);
  if (threadIdx.x == 0) {
    const double nan = __builtin_nan("");
    totals[0] = a[1] > 0.0 ? a[0] / a[1] : nan;
    totals[1] = a[3] > 0.0 ? a[2] / a[3] : nan;
    totals[2] = a[5] > 0.0 ? a[4] / a[5] : nan;
    totals[3] = a[1];
    totals[4] = (double)S - a[1];
    totals[5] = a[3];
    totals[6] = (double)S - a[3];
    totals[7] = a[6];
  }
}

static inline bool aligned_to(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

}  // namespace p2m

using namespace p2m;

extern "C" int32_t p2m_one_euro_lookahead(void) { return OE_LOOKAHEAD; }

extern "C" int p2m_one_euro(const float* x, const int32_t* seq_ptr, const int32_t* rows, int32_t N, int32_t S, int32_t C,
                            double min_cutoff, double beta, double d_cutoff, double dt, float* state_x, float* state_dx,
                            int32_t* started, float* y, void* stream) {
  P2M_CHECK_ARG(x && seq_ptr && y, "null pointer");
  P2M_CHECK_ARG(N >= 0 && S >= 1 && C >= 1, "need N >= 0, S >= 1, C >= 1");
  P2M_CHECK_ARG((long)N * C < (1L << 31) && (long)S * C < (1L << 31), "2^31 or more elements");
  P2M_CHECK_ARG((state_x != nullptr) == (state_dx != nullptr) && (state_x != nullptr) == (started != nullptr),
                "state_x, state_dx and started: all three or none");
  P2M_CHECK_ARG(!(rows && y == x), "y may alias x only without a row table");
  P2M_CHECK_ARG(std::isfinite(min_cutoff) && std::isfinite(beta) && std::isfinite(d_cutoff) && std::isfinite(dt),
                "non-finite parameter");
  P2M_CHECK_ARG(dt > 0.0 && min_cutoff >= 0.0 && d_cutoff >= 0.0, "need dt > 0, min_cutoff >= 0, d_cutoff >= 0");
  OneEuroArgs a;
  a.mc = (float)min_cutoff; a.b = (float)beta; a.te = (float)dt;
  a.k2 = (float)(2.0 * M_PI); a.kd = (float)(2.0 * M_PI * d_cutoff);
  P2M_CHECK_ARG(std::isfinite(a.mc) && std::isfinite(a.b) && std::isfinite(a.te) && std::isfinite(a.kd) && a.te > 0.f,
                "a parameter leaves the fp32 range (dt rounds to 0, or a value to infinity)");
  if (N == 0) return P2M_OK;
  a.x = x; a.seq_ptr = seq_ptr; a.rows = rows; a.y = y; a.N = N; a.C = C;
  a.state_x = state_x; a.state_dx = state_dx; a.started = started;
  // lane access width: the narrowest that leaves at most OE_FILL_LANES lanes, among those every row start allows (rows are C
  // floats apart from the bases x, y, state_x, state_dx)
  int vec = 1;
  for (int v = 2; v <= 4 && (long)S * (C / vec) > OE_FILL_LANES; v <<= 1) {
    const size_t bytes = 4 * (size_t)v;
    if (C % v != 0 || !aligned_to(x, bytes) || !aligned_to(y, bytes) ||
        (state_x && !(aligned_to(state_x, bytes) && aligned_to(state_dx, bytes))))
      break;
    vec = v;
  }
  a.cblocks = cdiv(C / vec, OE_NT);
  P2M_CHECK_ARG((long)S * a.cblocks < (1L << 31), "2^31 or more blocks");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(S * a.cblocks)), block(OE_NT);
  const bool unit = a.te == 1.f;
  if (vec == 4) hipLaunchKernelGGL((unit ? k_one_euro<4, true> : k_one_euro<4, false>), grid, block, 0, st, a);
  else if (vec == 2) hipLaunchKernelGGL((unit ? k_one_euro<2, true> : k_one_euro<2, false>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((unit ? k_one_euro<1, true> : k_one_euro<1, false>), grid, block, 0, st, a);
  if (started) hipLaunchKernelGGL(k_one_euro_mark, dim3(cdiv(S, 256)), dim3(256), 0, st, seq_ptr, S, N, started);
  return check_launch("one_euro");
}

extern "C" int p2m_video_eval(const float* pred, const float* gt, const int32_t* seq_ptr, const uint8_t* vis, int32_t N,
                              int32_t S, int32_t J, int32_t want_pa, float* accel, uint8_t* accel_valid, float* mpjpe,
                              float* pa_mpjpe, double* frame_sums, double* seq_stats, double* totals, void* stream) {
  P2M_CHECK_ARG(pred && gt && seq_ptr && accel && accel_valid && mpjpe && frame_sums && seq_stats && totals, "null pointer");
  P2M_CHECK_ARG(!want_pa || pa_mpjpe, "want_pa without a pa_mpjpe output");
  P2M_CHECK_ARG(N >= 0 && S >= 1, "need N >= 0, S >= 1");
  P2M_CHECK_ARG(J >= 1 && J <= 64, "J outside 1..64");
  P2M_CHECK_ARG((long)N * J * 3 < (1L << 31) && (long)S * VE_SEQ_COLS < (1L << 31), "2^31 or more elements");
  hipStream_t st = (hipStream_t)stream;
  if (N > 0)
    hipLaunchKernelGGL(k_video_frames, dim3(cdiv(N, 4)), dim3(256), 0, st, pred, gt, seq_ptr, vis, N, S, J, want_pa ? 1 : 0,
                       accel, accel_valid, mpjpe, pa_mpjpe, frame_sums);
  hipLaunchKernelGGL(k_video_seq, dim3(S), dim3(256), 0, st, frame_sums, seq_ptr, N, J, want_pa ? 1 : 0, seq_stats);
  hipLaunchKernelGGL(k_video_totals, dim3(1), dim3(64), 0, st, seq_stats, S, totals);
  return check_launch("video_eval");
}
