// Error profiles on the GPU (gfx950): per-point distances between corresponding points of a prediction and a ground truth,
// optionally after the fp64 similarity alignment of p2m_eval.h, binned against an fp64 threshold table and accumulated per
// group and per point: what PCK curves, their AUC, per-joint error tables and a dataset-mean per-vertex error map are derived
// from.  The reference ships no such code (FreiHAND's AUC comes from the challenge server): the definition in include/p2m.h is
// the contract and tests/profile_ref.py its float64 restatement.
//
// Three kernels per call, all on the caller's stream, no allocation, no sync, no float atomics:
//   k_profile_sample       one block per sample, lanes striding over the points: the alignment sums through block_sum and
//                          similarity_solve in every lane (the scheme of k_mesh_eval's pa_mesh), then per point the error in fp64,
//                          its bin by a binary search of the threshold table held in LDS, the per-sample histogram in LDS with
//                          integer atomics, the per-sample sum through the fixed tree
//   k_profile_fold_points  one wave per point: the samples' bins counted in LDS (integer atomics), their errors added in sample
//                          order, then the point's own row of the per-point totals updated, each entry by one lane
//   k_profile_fold_groups  one thread per (group row, column) walks the samples in order
// Integer sums do not depend on the order of evaluation, every floating-point sum runs in a fixed order that starts from the
// running total: results are bitwise reproducible, and two calls leave bitwise the state of one call over both batches.
// This unit is built with -ffp-contract=off (build.py): dx dx + dy dy + dz dz is three products and two sums, left to right.
#include "p2m_eval.h"

namespace p2m {

constexpr int PROF_NT = 256;                      // threads per block
constexpr int PROF_KMAX = 256;                    // thresholds of a table (LDS: 2 KB + the 257 bins)
constexpr unsigned short PROF_SKIP = 0xFFFF;      // bin of a point that is not counted (not valid, or a padding row)

static inline long prof_ws_bytes(int B, int N) { return ((long)B * 12 + (long)B * N * 2 + 15) & ~15L; }

struct ProfArgs {
  const float* pred;                  // [B, N, 3]
  const float* gt;                    // [B, N, 3], read as gt * gs
  const unsigned char* valid;         // [B, N] or NULL (all counted)
  float gs;
  int B_real, N, K, root, align;      // root < 0: none
  const double* th;                   // [K] ascending
  double* err;                        // [B, N]
  double* mean;                       // [B]
  int* hist;                          // [B, K + 1]
  double* s_sum;                      // workspace [B]: the per-sample sums
  int* s_cnt;                         // workspace [B]: the points counted per sample
  unsigned short* bins;               // workspace [B, N]
};

__global__ __launch_bounds__(PROF_NT) void k_profile_sample(ProfArgs a) {
  __shared__ double th[PROF_KMAX];
  __shared__ int hist[PROF_KMAX + 1];
  __shared__ double sh[(PROF_NT / 64) * 10];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = a.N, K = a.K;
  double* err = a.err + (long)b * N;
  unsigned short* bins = a.bins + (long)b * N;
  int* hout = a.hist + (long)b * (K + 1);
  if (b >= a.B_real) {                // padding row: outputs 0, inputs never read, nothing counted
    for (int i = tid; i < N; i += PROF_NT) { err[i] = 0.0; bins[i] = PROF_SKIP; }
    for (int k = tid; k <= K; k += PROF_NT) hout[k] = 0;
    if (tid == 0) { a.mean[b] = 0.0; a.s_sum[b] = 0.0; a.s_cnt[b] = 0; }
    return;
  }
  for (int k = tid; k < K; k += PROF_NT) th[k] = a.th[k];
  for (int k = tid; k <= K; k += PROF_NT) hist[k] = 0;
  const float* pred = a.pred + (long)b * N * 3;
  const float* gt = a.gt + (long)b * N * 3;
  const unsigned char* valid = a.valid ? a.valid + (long)b * N : nullptr;
  const double gs = (double)a.gs;
  double rP[3] = {0.0, 0.0, 0.0}, rG[3] = {0.0, 0.0, 0.0};
  if (a.root >= 0) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      rP[k] = (double)pred[a.root * 3 + k];
      rG[k] = (double)gt[a.root * 3 + k] * gs;
    }
  }
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, c = 1.0, t[3] = {0.0, 0.0, 0.0};
  if (a.align) {                      // the prediction onto the ground truth over the valid points: pa_mpvpe's H, varP, centroids
    double m[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < N; i += PROF_NT) {
      if (valid && valid[i] == 0) continue;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        m[k] += (double)pred[i * 3 + k] - rP[k];
        m[3 + k] += (double)gt[i * 3 + k] * gs - rG[k];
      }
      m[6] += 1.0;
    }
    block_sum<PROF_NT, 7>(m, sh);
    const double inv = 1.0 / m[6];
    const double cP[3] = {m[0] * inv, m[1] * inv, m[2] * inv}, cG[3] = {m[3] * inv, m[4] * inv, m[5] * inv};
    double h[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < N; i += PROF_NT) {
      if (valid && valid[i] == 0) continue;
      double u[3], w[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        u[k] = ((double)pred[i * 3 + k] - rP[k]) - cP[k];
        w[k] = ((double)gt[i * 3 + k] * gs - rG[k]) - cG[k];
      }
#pragma unroll
      for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int s = 0; s < 3; s++) h[3 * r + s] += u[r] * w[s];
      }
      h[9] += u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
    }
    block_sum<PROF_NT, 10>(h, sh);
#pragma unroll
    for (int k = 0; k < 10; k++) h[k] *= inv;
    similarity_solve(h, h[9], cP, cG, R, &c, t);
  }
  __syncthreads();                    // th and the cleared hist
  double s[2] = {0.0, 0.0};           // this lane's points in ascending order: sum of errors, points counted
  for (int i = tid; i < N; i += PROF_NT) {
    double e = 0.0;
    unsigned short bin = PROF_SKIP;
    if (!valid || valid[i] != 0) {
      double p[3], g[3], d[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        p[k] = (double)pred[i * 3 + k] - rP[k];
        g[k] = (double)gt[i * 3 + k] * gs - rG[k];
      }
      if (a.align) {
#pragma unroll
        for (int r = 0; r < 3; r++) d[r] = (c * (R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2]) + t[r]) - g[r];
      } else {
#pragma unroll
        for (int k = 0; k < 3; k++) d[k] = p[k] - g[k];
      }
      e = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      int lo = 0, hi = K;             // the number of thresholds < e: the first k with e <= th[k], K if there is none
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (th[mid] < e) lo = mid + 1;
        else hi = mid;
      }
      if (!(e == e)) lo = K;          // NaN compares false with everything: past the table, as +inf is
      bin = (unsigned short)lo;
      atomicAdd(&hist[lo], 1);
      s[1] += 1.0;
    }
    err[i] = e;
    bins[i] = bin;
    s[0] += e;
  }
  block_sum<PROF_NT, 2>(s, sh);       // (its barriers also complete the histogram)
  for (int k = tid; k <= K; k += PROF_NT) hout[k] = hist[k];
  if (tid == 0) {
    a.mean[b] = s[0] / s[1];          // no point counted: 0 / 0 = NaN, as numpy's mean of nothing
    a.s_sum[b] = s[0];
    a.s_cnt[b] = (int)s[1];
  }
}

// point i (one wave per point, four points per block): sum[i] += its errors over the samples in order, count[i] += the samples
// that count it, hist[i][bin] += the samples in that bin.  Lane l takes the samples l, l + 64, ...: their bins are counted in
// the wave's own LDS row with integer atomics, their errors pass through the lanes in sample order (a sample that does not count
// has error 0: x + 0 is x), and every entry of the point's row is then touched by one lane, once.
// (One thread per point walking the samples, each step a load - add - store on its row: 64 dependent memory round trips per call,
//  0.035 ms of a 0.059 ms call at B = 64 whatever N - DESIGN.md section 8.)
__global__ __launch_bounds__(PROF_NT) void k_profile_fold_points(const double* __restrict__ err,
                                                                const unsigned short* __restrict__ bins, int B_real, int N, int K,
                                                                double* __restrict__ psum, long long* __restrict__ pcnt,
                                                                long long* __restrict__ phist) {
  __shared__ int cnts[PROF_NT / 64][PROF_KMAX + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * (PROF_NT / 64) + w;
  const bool live = i < N;            // (whole waves)
  for (int k = lane; k <= K; k += 64) cnts[w][k] = 0;
  __syncthreads();
  double acc = 0.0;
  int n = 0;
  if (live) {
    acc = psum[i];
    for (int b0 = 0; b0 < B_real; b0 += 64) {
      const int b = b0 + lane;
      unsigned short bin = PROF_SKIP;
      double e = 0.0;
      if (b < B_real) {
        bin = bins[(long)b * N + i];
        e = err[(long)b * N + i];
      }
      if (bin != PROF_SKIP) atomicAdd(&cnts[w][bin], 1);         // bin <= K: k_profile_sample's search ends in [0, K]
      n += __popcll(__ballot(bin != PROF_SKIP));
#pragma unroll
      for (int l = 0; l < 64; l++) acc += __shfl(e, l);
    }
  }
  __syncthreads();
  if (!live) return;
  long long* h = phist + (long)i * (K + 1);
  for (int k = lane; k <= K; k += 64) {
    const int c = cnts[w][k];
    if (c != 0) h[k] += c;
  }
  if (lane == 0) {
    psum[i] = acc;
    pcnt[i] += n;
  }
}

// row r (0: all samples, 1 + g: group g), column 0: the sum of the per-sample sums, 1: the points counted, 2 + k: bin k.
// Every load of a step is unconditional (a sample outside the row adds nothing), so the steps' loads overlap.
__global__ __launch_bounds__(PROF_NT) void k_profile_fold_groups(const double* __restrict__ s_sum, const int* __restrict__ s_cnt,
                                                                const int* __restrict__ shist, const int* __restrict__ group,
                                                                int n_groups, int B_real, int K, double* __restrict__ gsum,
                                                                long long* __restrict__ gcnt, long long* __restrict__ ghist) {
  const int ncol = K + 3;
  const int i = blockIdx.x * PROF_NT + threadIdx.x;
  if (i >= (n_groups + 1) * ncol) return;
  const int r = i / ncol, col = i - r * ncol;
  const int* grp = r > 0 ? group : nullptr;       // row 0 and a call without ids read none
  if (r > 0 && group == nullptr) return;          // no ids: nothing belongs to a group
  if (col == 0) {
    double acc = gsum[r];
#pragma unroll 8
    for (int b = 0; b < B_real; b++) {
      const double s = s_sum[b];
      const bool in = grp == nullptr || grp[b] == r - 1;
      acc = in ? acc + s : acc;
    }
    gsum[r] = acc;
    return;
  }
  const int* src = col == 1 ? s_cnt : shist + (col - 2);
  const long stride = col == 1 ? 1 : K + 1;
  long long acc = 0;
#pragma unroll 8
  for (int b = 0; b < B_real; b++) {
    const int v = src[b * stride];
    const bool in = grp == nullptr || grp[b] == r - 1;
    acc += in ? v : 0;
  }
  if (col == 1) gcnt[r] += acc;
  else ghist[(long)r * (K + 1) + col - 2] += acc;
}

}  // namespace p2m

using namespace p2m;

extern "C" int64_t p2m_error_profile_workspace(int32_t B, int32_t N) {
  if (B < 0 || N < 1) return -1;
  return prof_ws_bytes(B, N);
}

extern "C" int p2m_error_profile(const float* pred, const float* gt, const uint8_t* valid, int32_t B, int32_t B_real, int32_t N,
                                 float gt_scale, int32_t root, int32_t align, const double* thresholds, int32_t K,
                                 void* workspace, int64_t workspace_bytes, double* error, double* sample_mean,
                                 int32_t* sample_pck, const int32_t* group, int32_t n_groups, double* group_sum,
                                 int64_t* group_count, int64_t* group_hist, double* point_sum, int64_t* point_count,
                                 int64_t* point_hist, void* stream) {
  P2M_CHECK_ARG(pred && gt && thresholds && workspace && error && sample_mean && sample_pck, "null pointer");
  P2M_CHECK_ARG(B >= 0 && B_real >= 0 && B_real <= B && N >= 1, "bad batch / point count");
  P2M_CHECK_ARG((long)B * N * 3 < (1L << 31), "more than 2^31 coordinates");
  P2M_CHECK_ARG(K >= 2 && K <= PROF_KMAX, "2..256 thresholds");
  P2M_CHECK_ARG(root >= -1 && root < N, "root: -1 (none) or a point index");
  P2M_CHECK_ARG((group_sum != nullptr) == (group_count != nullptr) && (group_sum != nullptr) == (group_hist != nullptr),
                "group totals: all three or none");
  P2M_CHECK_ARG(group_sum == nullptr || (n_groups >= 0 && n_groups <= 65535), "n_groups outside 0..65535");
  P2M_CHECK_ARG((point_sum != nullptr) == (point_count != nullptr) && (point_sum != nullptr) == (point_hist != nullptr),
                "point totals: all three or none");
  P2M_CHECK_ARG(workspace_bytes >= p2m_error_profile_workspace(B, N), "workspace too small");
  P2M_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  if (B == 0) return P2M_OK;
  hipStream_t s = (hipStream_t)stream;
  ProfArgs a;
  a.pred = pred; a.gt = gt; a.valid = valid; a.gs = gt_scale; a.B_real = B_real; a.N = N; a.K = K; a.root = root;
  a.align = align ? 1 : 0; a.th = thresholds; a.err = error; a.mean = sample_mean; a.hist = sample_pck;
  a.s_sum = (double*)workspace;
  a.s_cnt = (int*)((char*)workspace + (long)B * 8);
  a.bins = (unsigned short*)((char*)workspace + (long)B * 12);
  hipLaunchKernelGGL(k_profile_sample, dim3(B), dim3(PROF_NT), 0, s, a);
  if (point_sum && B_real > 0)
    hipLaunchKernelGGL(k_profile_fold_points, dim3(cdiv(N, PROF_NT / 64)), dim3(PROF_NT), 0, s, error, a.bins, B_real, N, K,
                       point_sum, (long long*)point_count, (long long*)point_hist);
  if (group_sum && B_real > 0)
    hipLaunchKernelGGL(k_profile_fold_groups, dim3(cdiv((long)(n_groups + 1) * (K + 3), PROF_NT)), dim3(PROF_NT), 0, s, a.s_sum,
                       a.s_cnt, sample_pck, group, n_groups, B_real, K, group_sum, (long long*)group_count,
                       (long long*)group_hist);
  return check_launch("error_profile");
}
