// F-scores on the GPU (gfx950): batched nearest-vertex distances between two point sets per sample, the thresholded
// counts, FreiHAND's F@th per sample and running totals.  The reference ships no F-score code (its FreiHAND numbers come
// from the challenge server): the definition in include/p2m.h is the contract and tests/fscore_ref.py its float64 restatement.
//
// Three kernels per call, all on the caller's stream, no allocation, no sync, no float atomics:
//   k_nn_prepare   one block per sample: centre points (fp64 CSR regression, or given, or none), the fp64 similarity
//                  transform of the aligned variant (exactly PA-MPVPE's: p2m_eval.h), and the point sets the search reads,
//                  written fp32 and coordinate-major about ONE per-sample origin (the centred ground truth's centroid),
//                  subtracted in fp64 before the rounding: the rounding scales with the mesh's extent, not its position.
//   k_nn_search    one block per (sample, variant, direction, tile of queries): queries in registers (Q per lane), targets
//                  staged tile by tile in LDS and read by every lane at the same address (a broadcast, conflict-free); one
//                  LDS read serves all Q queries of a lane.  d^2 in the direct form (px-qx)^2 + (py-qy)^2 + (pz-qz)^2 (the
//                  |p|^2 + |q|^2 - 2 p.q form cancels ~0.01 mm at |p| ~ 1000 mm), min per pair, sqrtf at the end.  The tail
//                  of the last target tile is padded with x = +inf (distance +inf: it cannot win).  Integer counts of
//                  d < th per block go to a partial table.
//   k_fscore_fold  one block: partial counts added in tile order, near_pred / near_gt / F in fp64, running fp64 totals per
//                  group in sample order (the scheme of k_eval_fold).
// min and integer sums do not depend on the order of evaluation, everything else runs in fixed orders: results are bitwise
// reproducible and a sample's results do not depend on the batch around it.
#include "p2m_eval.h"

namespace p2m {

constexpr int NN_NT = 256;            // threads per block (prepare and search)
constexpr int NN_TT = 1024;           // targets per LDS tile: 3 x 4 KB
constexpr int NN_Q_SMALL = 2;         // queries per lane up to NN_SMALL_MAX points: a 778-vertex hand at B = 64 is
constexpr int NN_Q_LARGE = 4;         //   2 x 4 x 64 = 512 blocks; above: a 6890-vertex body stages its targets 7 times
constexpr int NN_SMALL_MAX = 2048;
constexpr int NN_MAX_TH = 4;

static inline int nn_q(int n) { return n <= NN_SMALL_MAX ? NN_Q_SMALL : NN_Q_LARGE; }
static inline int nn_stride(int nA, int nB) { return ((nA > nB ? nA : nB) + 3) & ~3; }
static inline int nn_tiles(int nA, int nB) {
  const int n = nA > nB ? nA : nB;
  return cdiv(n, NN_NT * nn_q(n));
}
static inline long nn_float_bytes(int B, int nA, int nB) { return (long)B * 9 * nn_stride(nA, nB) * 4; }   // a multiple of 16

template <typename T>
__device__ __forceinline__ T pick4(const T (&v)[4], int i) {          // (selects: no runtime index into the argument block)
  return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3]));
}

// ---- prepare ---------------------------------------------------------------------------------------------------------
struct PrepArgs {
  const float* P;                     // [B, nP, 3]  prediction (point set A)
  const float* G;                     // [B, nG, 3]  ground truth (point set B), read as G * gs
  float gs;
  int B_real, nP, nG, S;
  const int* r_ptr; const int* r_idx; const float* r_val; int root;      // CSR regressor (r_ptr == NULL: none)
  const float* cen_P; const float* cen_G;                                // [B, 3] given centres (NULL: none)
  int aligned;                        // write set 1 (the aligned prediction)
  float* ws;                          // [B][3 sets][3][S]: 0 centred prediction, 1 aligned prediction, 2 centred ground truth
  float* dist[4];                     // per (variant, direction) or NULL: zeroed here for the padding rows
};

__global__ __launch_bounds__(NN_NT) void k_nn_prepare(PrepArgs a) {
  __shared__ double cen[2][3];
  __shared__ double sh[(NN_NT / 64) * 10];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nP = a.nP, nG = a.nG;
  if (b >= a.B_real) {                // padding row: outputs 0, inputs never read
#pragma unroll
    for (int c = 0; c < 4; c++) {
      float* d = a.dist[c];
      const int n = (c & 1) ? nG : nP;
      if (d)
        for (int i = tid; i < n; i += NN_NT) d[(long)b * n + i] = 0.f;
    }
    return;
  }
  const float* pred = a.P + (long)b * nP * 3;
  const float* gt = a.G + (long)b * nG * 3;
  if (tid < 6) {
    const int which = tid / 3, k = tid - which * 3;
    double v = 0.0;
    if (a.cen_P) v = (double)(which == 0 ? a.cen_P : a.cen_G)[b * 3 + k];
    else if (a.r_ptr) v = which == 0 ? regress(a.r_ptr, a.r_idx, a.r_val, pred, 1.f, a.root, k, 0.0)
                                     : regress(a.r_ptr, a.r_idx, a.r_val, gt, a.gs, a.root, k, 0.0);
    cen[which][k] = v;
  }
  __syncthreads();
  const double rP[3] = {cen[0][0], cen[0][1], cen[0][2]}, rG[3] = {cen[1][0], cen[1][1], cen[1][2]};
  const double gs = (double)a.gs;
  // centroids of the centred sets
  double m1[6] = {0, 0, 0, 0, 0, 0};
  for (int i = tid; i < nP; i += NN_NT) {
#pragma unroll
    for (int k = 0; k < 3; k++) m1[k] += (double)pred[i * 3 + k] - rP[k];
  }
  for (int i = tid; i < nG; i += NN_NT) {
#pragma unroll
    for (int k = 0; k < 3; k++) m1[3 + k] += (double)gt[i * 3 + k] * gs - rG[k];
  }
  block_sum<NN_NT, 6>(m1, sh);
  const double inv_P = 1.0 / (double)nP, inv_G = 1.0 / (double)nG;
  const double cP[3] = {m1[0] * inv_P, m1[1] * inv_P, m1[2] * inv_P};
  const double cG[3] = {m1[3] * inv_G, m1[4] * inv_G, m1[5] * inv_G};     // the per-sample origin of every staged set
  float* w0 = a.ws + (long)b * 9 * a.S;
  const int S = a.S;
  for (int i = tid; i < nG; i += NN_NT) {
#pragma unroll
    for (int k = 0; k < 3; k++) w0[(6 + k) * S + i] = (float)(((double)gt[i * 3 + k] * gs - rG[k]) - cG[k]);
  }
  for (int i = tid; i < nP; i += NN_NT) {
#pragma unroll
    for (int k = 0; k < 3; k++) w0[k * S + i] = (float)(((double)pred[i * 3 + k] - rP[k]) - cG[k]);
  }
  if (!a.aligned) return;
  // the centred prediction aligned onto the centred ground truth over all vertices: PA-MPVPE's transform (nP == nG)
  double h[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < nP; i += NN_NT) {
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
  block_sum<NN_NT, 10>(h, sh);
#pragma unroll
  for (int k = 0; k < 10; k++) h[k] *= inv_P;
  double R[9], c, t[3];
  similarity_solve(h, h[9], cP, cG, R, &c, t);
  for (int i = tid; i < nP; i += NN_NT) {
    double p[3];
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = (double)pred[i * 3 + k] - rP[k];
#pragma unroll
    for (int r = 0; r < 3; r++)
      w0[(3 + r) * S + i] = (float)((c * (R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2]) + t[r]) - cG[r]);
  }
}

// ---- search ----------------------------------------------------------------------------------------------------------
struct SearchArgs {
  const float* ws;
  int S, nP, nG;
  int ncombo;                         // (variant, direction) pairs of the call
  int qset[4], tset[4];               // staged set of the queries / of the targets (set 2 holds nG points, 0 and 1 nP)
  float* dist[4];                     // [B, nq] or NULL
  int nth;
  float th[NN_MAX_TH];
  int* partial;                       // [B][4][ntmax][NN_MAX_TH] or NULL (nth == 0)
  int ntmax;
};

template <int Q>
__global__ __launch_bounds__(NN_NT) void k_nn_search(SearchArgs a) {
  constexpr int QT = NN_NT * Q;
  __shared__ __align__(16) float tx[NN_TT];
  __shared__ __align__(16) float ty[NN_TT];
  __shared__ __align__(16) float tz[NN_TT];
  __shared__ int red[NN_NT / 64][NN_MAX_TH];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % a.ntmax;
  const int c = (blockIdx.x / a.ntmax) % a.ncombo;
  const int b = blockIdx.x / (a.ntmax * a.ncombo);
  const int qset = pick4(a.qset, c), tset = pick4(a.tset, c);
  const int nq = qset == 2 ? a.nG : a.nP, nt = tset == 2 ? a.nG : a.nP;
  if (tile * QT >= nq) return;        // (the whole block: nA != nB gives the two directions different tile counts)
  float* dist = pick4(a.dist, c);
  if (dist == nullptr && a.nth == 0) return;             // a direction nobody asked for
  const int S = a.S;
  const float* qs = a.ws + ((long)b * 3 + qset) * 3 * S;
  const float* ts = a.ws + ((long)b * 3 + tset) * 3 * S;
  const float inf = __builtin_inff();
  float qx[Q], qy[Q], qz[Q], m[Q];
#pragma unroll
  for (int j = 0; j < Q; j++) {
    const int i = tile * QT + j * NN_NT + tid;
    const int ic = i < nq ? i : nq - 1;                  // lanes past the end repeat the last query and store nothing
    qx[j] = qs[ic];
    qy[j] = qs[S + ic];
    qz[j] = qs[2 * S + ic];
    m[j] = inf;
  }
  for (int t0 = 0; t0 < nt; t0 += NN_TT) {
    const int left = nt - t0;
    const int n4 = left >= NN_TT ? NN_TT : ((left + 3) & ~3);
    __syncthreads();                                     // the previous tile has been read by every wave
    for (int k = tid; k < n4; k += NN_NT) {
      const bool on = k < left;
      tx[k] = on ? ts[t0 + k] : inf;                     // padding: distance +inf from every (finite) query
      ty[k] = on ? ts[S + t0 + k] : 0.f;
      tz[k] = on ? ts[2 * S + t0 + k] : 0.f;
    }
    __syncthreads();
    for (int k = 0; k < n4; k += 4) {
      const float4 X = *reinterpret_cast<const float4*>(&tx[k]);
      const float4 Y = *reinterpret_cast<const float4*>(&ty[k]);
      const float4 Z = *reinterpret_cast<const float4*>(&tz[k]);
      const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
      for (int u = 0; u < 4; u++) {
#pragma unroll
        for (int j = 0; j < Q; j++) {
          const float dx = xs[u] - qx[j], dy = ys[u] - qy[j], dz = zs[u] - qz[j];
          m[j] = fminf(m[j], dx * dx + dy * dy + dz * dz);
        }
      }
    }
  }
  int cnt[NN_MAX_TH] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < Q; j++) {
    const int i = tile * QT + j * NN_NT + tid;
    if (i < nq) {
      const float d = sqrtf(m[j]);
      if (dist) dist[(long)b * nq + i] = d;
#pragma unroll
      for (int t = 0; t < NN_MAX_TH; t++) cnt[t] += (t < a.nth && d < a.th[t]) ? 1 : 0;
    }
  }
  if (a.nth == 0) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int t = 0; t < NN_MAX_TH; t++) cnt[t] += __shfl_xor(cnt[t], o);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int t = 0; t < NN_MAX_TH; t++) red[tid >> 6][t] = cnt[t];
  }
  __syncthreads();
  if (tid < NN_MAX_TH) {
    int s = 0;
    for (int w = 0; w < NN_NT / 64; w++) s += red[w][tid];
    a.partial[(((long)b * 4 + c) * a.ntmax + tile) * NN_MAX_TH + tid] = s;
  }
}

// ---- counts, scores, running totals ------------------------------------------------------------------------------------
// counts [B][nvar][2][nth] (direction 0: prediction -> ground truth, 1: ground truth -> prediction), scores [B][nvar][3][nth]
// (near_pred, near_gt, F).  totals[r][0] += samples of row r, totals[r][1 + k] += sum of scores[:, k] (k over [nvar][3][nth]).
__global__ __launch_bounds__(256) void k_fscore_fold(const int* __restrict__ partial, int ntmax, int QT, int B, int B_real,
                                                     int nv, int nvar, int nth, int* __restrict__ counts,
                                                     double* __restrict__ scores, const int* __restrict__ group, int n_groups,
                                                     double* __restrict__ totals) {
  const int ntq = cdiv_dev(nv, QT);
  for (int i = threadIdx.x; i < B * nvar * nth; i += 256) {
    const int b = i / (nvar * nth), r = i - b * nvar * nth, v = r / nth, t = r - v * nth;
    int cp = 0, cg = 0;
    if (b < B_real) {
      for (int k = 0; k < ntq; k++) {
        cp += partial[(((long)b * 4 + 2 * v) * ntmax + k) * NN_MAX_TH + t];
        cg += partial[(((long)b * 4 + 2 * v + 1) * ntmax + k) * NN_MAX_TH + t];
      }
    }
    if (counts) {
      counts[((b * nvar + v) * 2 + 0) * nth + t] = cp;
      counts[((b * nvar + v) * 2 + 1) * nth + t] = cg;
    }
    if (scores) {
      const double np = (double)cp / (double)nv, ng = (double)cg / (double)nv;
      double* s = scores + ((long)b * nvar + v) * 3 * nth;
      s[t] = np;
      s[nth + t] = ng;
      s[2 * nth + t] = np + ng > 0.0 ? 2.0 * np * ng / (np + ng) : 0.0;
    }
  }
  if (totals == nullptr) return;
  __syncthreads();                    // the scores of this block's own writes
  const int ncol = 1 + nvar * 3 * nth;
  for (int i = threadIdx.x; i < (n_groups + 1) * ncol; i += 256) {
    const int r = i / ncol, col = i - r * ncol;
    double s = 0.0;
    for (int b = 0; b < B_real; b++) {
      if (r > 0 && (group == nullptr || group[b] != r - 1)) continue;
      s += col == 0 ? 1.0 : scores[(long)b * (ncol - 1) + col - 1];
    }
    totals[i] += s;
  }
}

static void launch_search(const SearchArgs& a, int n_max, int B_real, hipStream_t s) {
  const int grid = B_real * a.ncombo * a.ntmax;
  if (nn_q(n_max) == NN_Q_SMALL) hipLaunchKernelGGL(k_nn_search<NN_Q_SMALL>, dim3(grid), dim3(NN_NT), 0, s, a);
  else hipLaunchKernelGGL(k_nn_search<NN_Q_LARGE>, dim3(grid), dim3(NN_NT), 0, s, a);
}

}  // namespace p2m

using namespace p2m;

extern "C" int32_t p2m_nn_target_tile(void) { return NN_TT; }
extern "C" int32_t p2m_nn_query_tile(int32_t n) { return NN_NT * nn_q(n); }

extern "C" int64_t p2m_nn_workspace(int32_t B, int32_t nA, int32_t nB) {
  if (B < 0 || nA < 1 || nB < 1) return -1;
  return nn_float_bytes(B, nA, nB) + (int64_t)B * 4 * nn_tiles(nA, nB) * NN_MAX_TH * 4;
}

extern "C" int p2m_mesh_fscore(const float* pred_mesh, const float* gt_mesh, int32_t B, int32_t B_real, int32_t nv,
                               float gt_mesh_scale, const int32_t* r_ptr, const int32_t* r_idx, const float* r_val, int32_t J,
                               int32_t root, const float* pred_centre, const float* gt_centre, int32_t variants,
                               const float* thresholds, int32_t n_thresholds, void* workspace, int64_t workspace_bytes,
                               float* d_pred, float* d_gt, float* pa_d_pred, float* pa_d_gt, int32_t* counts, double* scores,
                               const int32_t* group, int32_t n_groups, double* totals, void* stream) {
  P2M_CHECK_ARG(pred_mesh && gt_mesh && thresholds && workspace, "null pointer");
  P2M_CHECK_ARG(B >= 0 && B_real >= 0 && B_real <= B && nv >= 1, "bad batch / vertex count");
  P2M_CHECK_ARG((long)B * nv * 3 < (1L << 31), "more than 2^31 coordinates");
  P2M_CHECK_ARG(n_thresholds >= 1 && n_thresholds <= NN_MAX_TH, "1..4 thresholds");
  for (int t = 0; t < n_thresholds; t++)
    P2M_CHECK_ARG(thresholds[t] > 0.f && thresholds[t] < __builtin_inff(), "thresholds must be positive and finite");
  P2M_CHECK_ARG(variants >= 1 && variants <= 3, "variants: bit 0 centred, bit 1 aligned, at least one");
  P2M_CHECK_ARG((r_ptr != nullptr) == (r_idx != nullptr) && (r_ptr != nullptr) == (r_val != nullptr), "incomplete regressor");
  P2M_CHECK_ARG(r_ptr == nullptr || (J >= 1 && root >= 0 && root < J), "regressor: need 0 <= root < J");
  P2M_CHECK_ARG((pred_centre != nullptr) == (gt_centre != nullptr), "centres: both or neither");
  P2M_CHECK_ARG(totals == nullptr || (scores && n_groups >= 0), "totals need scores");
  P2M_CHECK_ARG(workspace_bytes >= p2m_nn_workspace(B, nv, nv), "workspace too small");
  P2M_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  if (B == 0) return P2M_OK;
  hipStream_t s = (hipStream_t)stream;
  const int nvar = (variants & 1) + ((variants >> 1) & 1);
  PrepArgs p;
  p.P = pred_mesh; p.G = gt_mesh; p.gs = gt_mesh_scale; p.B_real = B_real; p.nP = nv; p.nG = nv; p.S = nn_stride(nv, nv);
  p.r_ptr = r_ptr; p.r_idx = r_idx; p.r_val = r_val; p.root = root; p.cen_P = pred_centre; p.cen_G = gt_centre;
  p.aligned = (variants & 2) ? 1 : 0;
  p.ws = (float*)workspace;
  SearchArgs a;
  a.ws = p.ws; a.S = p.S; a.nP = nv; a.nG = nv; a.ncombo = 2 * nvar; a.nth = n_thresholds;
  for (int t = 0; t < NN_MAX_TH; t++) a.th[t] = t < n_thresholds ? thresholds[t] : 0.f;
  a.partial = (int*)((char*)workspace + nn_float_bytes(B, nv, nv));
  a.ntmax = nn_tiles(nv, nv);
  int c = 0;
  for (int v = 0; v < 2; v++) {
    if (!((variants >> v) & 1)) continue;
    a.qset[c] = v; a.tset[c] = 2; a.dist[c] = v == 0 ? d_pred : pa_d_pred; c++;      // prediction -> ground truth
    a.qset[c] = 2; a.tset[c] = v; a.dist[c] = v == 0 ? d_gt : pa_d_gt; c++;          // ground truth -> prediction
  }
  for (; c < 4; c++) { a.qset[c] = 0; a.tset[c] = 0; a.dist[c] = nullptr; }
  for (c = 0; c < 4; c++) p.dist[c] = a.dist[c];
  hipLaunchKernelGGL(k_nn_prepare, dim3(B), dim3(NN_NT), 0, s, p);
  if (B_real > 0) launch_search(a, nv, B_real, s);
  if (counts || scores)
    hipLaunchKernelGGL(k_fscore_fold, dim3(1), dim3(256), 0, s, a.partial, a.ntmax, NN_NT * nn_q(nv), B, B_real, nv, nvar,
                       n_thresholds, counts, scores, group, n_groups, totals);
  return check_launch("mesh_fscore");
}

extern "C" int p2m_point_nn(const float* A, const float* B, int32_t nb, int32_t nA, int32_t nB, float* dAB, float* dBA,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  P2M_CHECK_ARG(A && B && workspace && (dAB || dBA), "null pointer");
  P2M_CHECK_ARG(nb >= 0 && nA >= 1 && nB >= 1, "bad shape");
  P2M_CHECK_ARG((long)nb * (nA > nB ? nA : nB) * 3 < (1L << 31), "more than 2^31 coordinates");
  P2M_CHECK_ARG(workspace_bytes >= p2m_nn_workspace(nb, nA, nB), "workspace too small");
  P2M_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  if (nb == 0) return P2M_OK;
  hipStream_t s = (hipStream_t)stream;
  PrepArgs p;
  p.P = A; p.G = B; p.gs = 1.f; p.B_real = nb; p.nP = nA; p.nG = nB; p.S = nn_stride(nA, nB);
  p.r_ptr = nullptr; p.r_idx = nullptr; p.r_val = nullptr; p.root = 0; p.cen_P = nullptr; p.cen_G = nullptr;
  p.aligned = 0;
  p.ws = (float*)workspace;
  SearchArgs a;
  a.ws = p.ws; a.S = p.S; a.nP = nA; a.nG = nB; a.ncombo = 2; a.nth = 0;
  for (int t = 0; t < NN_MAX_TH; t++) a.th[t] = 0.f;
  a.partial = nullptr;
  a.ntmax = nn_tiles(nA, nB);
  for (int c = 0; c < 4; c++) { a.qset[c] = 0; a.tset[c] = 0; a.dist[c] = nullptr; }
  a.qset[0] = 0; a.tset[0] = 2; a.dist[0] = dAB;
  a.qset[1] = 2; a.tset[1] = 0; a.dist[1] = dBA;
  for (int c = 0; c < 4; c++) p.dist[c] = a.dist[c];
  hipLaunchKernelGGL(k_nn_prepare, dim3(nb), dim3(NN_NT), 0, s, p);
  launch_search(a, nA > nB ? nA : nB, nb, s);
  return check_launch("point_nn");
}
