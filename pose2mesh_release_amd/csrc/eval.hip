// Evaluation of the Tester / dataset.evaluate() on the GPU (gfx950): batched similarity (Procrustes) alignment and the
// per-sample MPJPE / PA-MPJPE / MPVPE / PA-MPVPE of a batch in one launch.
//
// Reference arithmetic (numpy on the host there, one sample at a time):
//   rigid_transform_3D / rigid_align                                          lib/coord_utils.py:127-149
//   compute_both_err (root-centred joint + vertex errors of one batch)        data/PW3D/dataset.py:273-286
//   evaluate: regress, root-align, MPJPE, MPVPE, H36M joints, PA-MPJPE        data/PW3D/dataset.py:322-375,
//                                                                             data/Human36M/dataset.py:514-572
// Everything is accumulated in fp64 from the fp32 inputs (a product of two fp32 values is exact in fp64), and the 3x3
// solve runs in fp64: the fp32 outputs are the fp64 results rounded once.  Fixed thread -> point maps and fixed reduction
// trees, no atomics: bitwise reproducible.  No allocation or synchronisation in the launch path (capturable).
#include "p2m_eval.h"

namespace p2m {

// (the similarity solve, the reductions and the CSR regression: p2m_eval.h, shared with fscore.hip)
// ---- (a) batched rigid_transform_3D / rigid_align -----------------------------------------------------------------------
// TPS threads per set: 64 (one wave per set, 4 sets per block; the joints of a pose) or 256 (one block per set; a mesh).
template <int TPS>
__global__ __launch_bounds__(256) void k_rigid_align(const float* __restrict__ A, const float* __restrict__ B, int nb, int N,
                                                     float* __restrict__ c_out, float* __restrict__ R_out,
                                                     float* __restrict__ t_out, float* __restrict__ A2) {
  __shared__ double sh[(TPS / 64) * 10];
  const int set = blockIdx.x * (256 / TPS) + (int)threadIdx.x / TPS;
  const int lane = (int)threadIdx.x % TPS;
  if (TPS == 64 && set >= nb) return;                    // whole waves leave; (TPS == 256: the grid is exactly nb)
  const float* a = A + (long)set * N * 3;
  const float* b = B + (long)set * N * 3;
  double m[6] = {0, 0, 0, 0, 0, 0};
  for (int i = lane; i < N; i += TPS) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      m[k] += (double)a[i * 3 + k];
      m[3 + k] += (double)b[i * 3 + k];
    }
  }
  if (TPS == 64) wave_sum<6>(m);
  else block_sum<TPS, 6>(m, sh);
  const double inv = 1.0 / (double)N;
  const double cA[3] = {m[0] * inv, m[1] * inv, m[2] * inv}, cB[3] = {m[3] * inv, m[4] * inv, m[5] * inv};
  double h[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = lane; i < N; i += TPS) {
    const double p[3] = {(double)a[i * 3] - cA[0], (double)a[i * 3 + 1] - cA[1], (double)a[i * 3 + 2] - cA[2]};
    const double q[3] = {(double)b[i * 3] - cB[0], (double)b[i * 3 + 1] - cB[1], (double)b[i * 3 + 2] - cB[2]};
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
      for (int s = 0; s < 3; s++) h[3 * r + s] += p[r] * q[s];
    }
    h[9] += p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
  }
  if (TPS == 64) wave_sum<10>(h);
  else block_sum<TPS, 10>(h, sh);
#pragma unroll
  for (int k = 0; k < 10; k++) h[k] *= inv;
  double R[9], c, t[3];
  similarity_solve(h, h[9], cA, cB, R, &c, t);
  if (lane == 0) {
    c_out[set] = (float)c;
#pragma unroll
    for (int k = 0; k < 9; k++) R_out[set * 9 + k] = (float)R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t_out[set * 3 + k] = (float)t[k];
  }
  if (A2 == nullptr) return;
  float* o = A2 + (long)set * N * 3;
  for (int i = lane; i < N; i += TPS) {
    const double p[3] = {(double)a[i * 3], (double)a[i * 3 + 1], (double)a[i * 3 + 2]};
#pragma unroll
    for (int r = 0; r < 3; r++) o[i * 3 + r] = (float)(c * (R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2]) + t[r]);
  }
}

// ---- (b) per-batch evaluation ---------------------------------------------------------------------------------------------
constexpr int EVAL_NT = 256;          // threads per sample
constexpr int EVAL_JMAX = 64;         // joints of a regressor / of a subset (LDS tables)

struct EvalArgs {
  const float* pred;                  // [B, nv, 3]  mesh-model order
  const float* gt;                    // [B, nv, 3]  read as gt * gt_scale
  float gt_scale;
  int B, B_real, nv;
  const int* ra_ptr; const int* ra_idx; const float* ra_val;  int JA, root_A;   // stage A regressor (CSR)
  const int* sub_A; int nsub_A;                              // NULL: all JA joints
  const float* pred_joints_A;                                // [B, JA, 3] or NULL (regressed from pred)
  const float* gt_joints_A;                                  // [B, JA, 3] or NULL (regressed from gt)
  const int* re_ptr; const int* re_idx; const float* re_val; int JE, root_E;    // stage E regressor, JE == 0: no stage E
  const int* sub_E; int nsub_E;
  const float* gt_joints_E;                                  // [B, JE, 3] or NULL
  int pa_mesh;
  float* mpjpe_A;                     // [B, nsub_A]
  float* mpvpe;                       // [B]
  float* mpjpe_E;                     // [B, nsub_E]
  float* pa_mpjpe_E;                  // [B, nsub_E]
  float* pa_mpvpe;                    // [B]
  double* means;                      // [B, 5] or NULL: fp64 per-sample means (mpjpe_E, pa_mpjpe_E, mpjpe_A, mpvpe, pa_mpvpe)
};

__global__ __launch_bounds__(EVAL_NT) void k_mesh_eval(EvalArgs a) {
  __shared__ double jA[2][EVAL_JMAX][3];      // stage-A joints: [0] prediction, [1] ground truth
  __shared__ double jE[2][EVAL_JMAX][3];      // stage-E joints of the A-centred meshes
  __shared__ double sh[(EVAL_NT / 64) * 10];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nsA = a.sub_A ? a.nsub_A : a.JA, nsE = a.sub_E ? a.nsub_E : a.JE;
  if (b >= a.B_real) {                        // padding row: outputs 0, inputs never read
    for (int k = tid; k < nsA; k += EVAL_NT) a.mpjpe_A[b * nsA + k] = 0.f;
    for (int k = tid; k < nsE && a.JE > 0; k += EVAL_NT) { a.mpjpe_E[b * nsE + k] = 0.f; a.pa_mpjpe_E[b * nsE + k] = 0.f; }
    if (tid == 0) {
      a.mpvpe[b] = 0.f;
      if (a.pa_mesh) a.pa_mpvpe[b] = 0.f;
      if (a.means)
        for (int k = 0; k < 5; k++) a.means[b * 5 + k] = 0.0;
    }
    return;
  }
  const float* pred = a.pred + (long)b * a.nv * 3;
  const float* gt = a.gt + (long)b * a.nv * 3;
  const int nv = a.nv;
  // -- stage A: joints of both meshes (the ground truth's may be given)
  for (int i = tid; i < 2 * a.JA * 3; i += EVAL_NT) {
    const int which = i / (a.JA * 3), r = i - which * a.JA * 3, j = r / 3, k = r - j * 3;
    double v;
    if (which == 0) v = a.pred_joints_A ? (double)a.pred_joints_A[((long)b * a.JA + j) * 3 + k]
                                        : regress(a.ra_ptr, a.ra_idx, a.ra_val, pred, 1.f, j, k, 0.0);
    else if (a.gt_joints_A) v = (double)a.gt_joints_A[((long)b * a.JA + j) * 3 + k];
    else v = regress(a.ra_ptr, a.ra_idx, a.ra_val, gt, a.gt_scale, j, k, 0.0);
    jA[which][j][k] = v;
  }
  __syncthreads();
  const double rP[3] = {jA[0][a.root_A][0], jA[0][a.root_A][1], jA[0][a.root_A][2]};
  const double rG[3] = {jA[1][a.root_A][0], jA[1][a.root_A][1], jA[1][a.root_A][2]};
  double sumA = 0.0;                          // (per-joint values are written by their thread; the mean is a fixed-order loop)
  for (int k = tid; k < nsA; k += EVAL_NT) {
    const int j = a.sub_A ? a.sub_A[k] : k;
    const double e = dist3((jA[0][j][0] - rP[0]) - (jA[1][j][0] - rG[0]), (jA[0][j][1] - rP[1]) - (jA[1][j][1] - rG[1]),
                           (jA[0][j][2] - rP[2]) - (jA[1][j][2] - rG[2]));
    a.mpjpe_A[b * nsA + k] = (float)e;
  }
  // -- stage E joints of the A-centred meshes (threads of the upper half; the mesh pass below runs on all)
  if (a.JE > 0) {
    for (int i = tid; i < 2 * a.JE * 3; i += EVAL_NT) {
      const int which = i / (a.JE * 3), r = i - which * a.JE * 3, j = r / 3, k = r - j * 3;
      double v;
      const double rk = which == 0 ? (k == 0 ? rP[0] : (k == 1 ? rP[1] : rP[2]))      // (selects: no runtime index into
                                   : (k == 0 ? rG[0] : (k == 1 ? rG[1] : rG[2]));     //  a register array)
      if (which == 0) v = regress(a.re_ptr, a.re_idx, a.re_val, pred, 1.f, j, k, rk);
      else if (a.gt_joints_E) v = (double)a.gt_joints_E[((long)b * a.JE + j) * 3 + k];
      else v = regress(a.re_ptr, a.re_idx, a.re_val, gt, a.gt_scale, j, k, rk);
      jE[which][j][k] = v;
    }
  }
  // -- mesh pass 1: MPVPE of the A-centred meshes, and their centroids (PA-MPVPE)
  const double gs = (double)a.gt_scale;
  double m1[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < nv; i += EVAL_NT) {
    double p[3], g[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      p[k] = (double)pred[i * 3 + k] - rP[k];
      g[k] = (double)gt[i * 3 + k] * gs - rG[k];
      m1[k] += p[k];
      m1[3 + k] += g[k];
    }
    m1[6] += dist3(p[0] - g[0], p[1] - g[1], p[2] - g[2]);
  }
  block_sum<EVAL_NT, 7>(m1, sh);              // (its barrier also publishes jE)
  const double inv_nv = 1.0 / (double)nv;
  const double mpvpe = m1[6] * inv_nv;
  // fixed-order means of the per-joint values (thread 0; the sets are a few dozen joints)
  if (tid == 0) {
    for (int k = 0; k < nsA; k++) {
      const int j = a.sub_A ? a.sub_A[k] : k;
      sumA += dist3((jA[0][j][0] - rP[0]) - (jA[1][j][0] - rG[0]), (jA[0][j][1] - rP[1]) - (jA[1][j][1] - rG[1]),
                    (jA[0][j][2] - rP[2]) - (jA[1][j][2] - rG[2]));
    }
    a.mpvpe[b] = (float)mpvpe;
    if (a.means) {
      a.means[b * 5 + 2] = sumA / (double)nsA;
      a.means[b * 5 + 3] = mpvpe;
    }
  }
  // -- stage E: re-centre on root_E, subset, MPJPE and PA-MPJPE (wave 0: one lane per subset joint)
  if (a.JE > 0 && tid < 64) {
    const int lane = tid;
    const double eP[3] = {jE[0][a.root_E][0], jE[0][a.root_E][1], jE[0][a.root_E][2]};
    const double eG[3] = {jE[1][a.root_E][0], jE[1][a.root_E][1], jE[1][a.root_E][2]};
    const bool on = lane < nsE;
    const int j = on ? (a.sub_E ? a.sub_E[lane] : lane) : 0;
    double p[3], g[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      p[k] = on ? jE[0][j][k] - eP[k] : 0.0;
      g[k] = on ? jE[1][j][k] - eG[k] : 0.0;
    }
    const double e = dist3(p[0] - g[0], p[1] - g[1], p[2] - g[2]);
    double m[7] = {p[0], p[1], p[2], g[0], g[1], g[2], on ? e : 0.0};
    wave_sum<7>(m);
    const double inv = 1.0 / (double)nsE;
    const double cP[3] = {m[0] * inv, m[1] * inv, m[2] * inv}, cG[3] = {m[3] * inv, m[4] * inv, m[5] * inv};
    double h[10];
    {
      const double u[3] = {on ? p[0] - cP[0] : 0.0, on ? p[1] - cP[1] : 0.0, on ? p[2] - cP[2] : 0.0};
      const double w[3] = {on ? g[0] - cG[0] : 0.0, on ? g[1] - cG[1] : 0.0, on ? g[2] - cG[2] : 0.0};
#pragma unroll
      for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int s = 0; s < 3; s++) h[3 * r + s] = u[r] * w[s];
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
    if (on) {
      a.mpjpe_E[b * nsE + lane] = (float)e;
      a.pa_mpjpe_E[b * nsE + lane] = (float)pe;
    }
    if (a.means) {
      double s[1] = {on ? pe : 0.0};
      wave_sum<1>(s);
      if (lane == 0) {
        a.means[b * 5 + 0] = m[6] * inv;
        a.means[b * 5 + 1] = s[0] * inv;
      }
    }
  } else if (a.JE == 0 && a.means && tid == 0) {
    a.means[b * 5 + 0] = 0.0;
    a.means[b * 5 + 1] = 0.0;
  }
  // -- PA-MPVPE: the A-centred prediction aligned onto the A-centred ground truth (two more passes over the meshes)
  if (!a.pa_mesh) {
    if (a.means && tid == 0) a.means[b * 5 + 4] = 0.0;
    return;
  }
  const double cP[3] = {m1[0] * inv_nv, m1[1] * inv_nv, m1[2] * inv_nv};
  const double cG[3] = {m1[3] * inv_nv, m1[4] * inv_nv, m1[5] * inv_nv};
  double h[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < nv; i += EVAL_NT) {
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
  block_sum<EVAL_NT, 10>(h, sh);
#pragma unroll
  for (int k = 0; k < 10; k++) h[k] *= inv_nv;
  double R[9], c, t[3];
  similarity_solve(h, h[9], cP, cG, R, &c, t);
  double e3[1] = {0.0};
  for (int i = tid; i < nv; i += EVAL_NT) {
    double p[3], g[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      p[k] = (double)pred[i * 3 + k] - rP[k];
      g[k] = (double)gt[i * 3 + k] * gs - rG[k];
    }
    double q[3];
#pragma unroll
    for (int r = 0; r < 3; r++) q[r] = c * (R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2]) + t[r];
    e3[0] += dist3(q[0] - g[0], q[1] - g[1], q[2] - g[2]);
  }
  block_sum<EVAL_NT, 1>(e3, sh);
  if (tid == 0) {
    a.pa_mpvpe[b] = (float)(e3[0] * inv_nv);
    if (a.means) a.means[b * 5 + 4] = e3[0] * inv_nv;
  }
}

// running totals: totals[r][0] += samples, totals[r][1 + m] += sum of means[:, m] over the samples of row r
// (r = 0: all samples, r = 1 + g: group g; samples whose group id is outside [0, n_groups) count in row 0 only).
// One block, one thread per (row, column), samples in order: deterministic.
__global__ __launch_bounds__(256) void k_eval_fold(const double* __restrict__ means, const int* __restrict__ group, int n_groups,
                                                   int B_real, double* __restrict__ totals) {
  for (int i = threadIdx.x; i < (n_groups + 1) * 6; i += 256) {
    const int r = i / 6, col = i - r * 6;
    double s = 0.0;
    for (int b = 0; b < B_real; b++) {
      if (r > 0 && (group == nullptr || group[b] != r - 1)) continue;
      s += col == 0 ? 1.0 : means[b * 5 + col - 1];
    }
    totals[i] += s;
  }
}

}  // namespace p2m

using namespace p2m;

extern "C" int p2m_rigid_align(const float* A, const float* B, int32_t nb, int32_t N, float* c, float* R, float* t, float* A2,
                               void* stream) {
  P2M_CHECK_ARG(A && B && c && R && t, "null pointer");
  P2M_CHECK_ARG(N >= 1 && nb >= 0, "bad shape");
  P2M_CHECK_ARG((long)nb * N * 3 < (1L << 31), "more than 2^31 coordinates");
  if (nb == 0) return P2M_OK;
  hipStream_t s = (hipStream_t)stream;
  if (N <= 256)
    hipLaunchKernelGGL(k_rigid_align<64>, dim3(cdiv(nb, 4)), dim3(256), 0, s, A, B, nb, N, c, R, t, A2);
  else
    hipLaunchKernelGGL(k_rigid_align<256>, dim3(nb), dim3(256), 0, s, A, B, nb, N, c, R, t, A2);
  return check_launch("rigid_align");
}

extern "C" int p2m_mesh_eval(const float* pred_mesh, const float* gt_mesh, int32_t B, int32_t B_real, int32_t nv,
                             float gt_mesh_scale, const int32_t* ra_ptr, const int32_t* ra_idx, const float* ra_val, int32_t JA,
                             int32_t root_A, const int32_t* sub_A, int32_t nsub_A, const float* pred_joints_A,
                             const float* gt_joints_A, const int32_t* re_ptr, const int32_t* re_idx, const float* re_val, int32_t JE, int32_t root_E,
                             const int32_t* sub_E, int32_t nsub_E, const float* gt_joints_E, int32_t pa_mesh, float* mpjpe_A,
                             float* mpvpe, float* mpjpe_E, float* pa_mpjpe_E, float* pa_mpvpe, double* sample_means,
                             const int32_t* group, int32_t n_groups, double* totals, void* stream) {
  P2M_CHECK_ARG(pred_mesh && gt_mesh && mpjpe_A && mpvpe, "null pointer");
  P2M_CHECK_ARG((ra_ptr && ra_idx && ra_val) || (pred_joints_A && gt_joints_A), "stage A: no regressor and no joints");
  P2M_CHECK_ARG(B >= 0 && B_real >= 0 && B_real <= B && nv >= 1, "bad batch / vertex count");
  P2M_CHECK_ARG((long)B * nv * 3 < (1L << 31), "more than 2^31 coordinates");
  P2M_CHECK_ARG(JA >= 1 && JA <= EVAL_JMAX && root_A >= 0 && root_A < JA, "stage A: need 1 <= JA <= 64, 0 <= root_A < JA");
  P2M_CHECK_ARG(sub_A == nullptr || (nsub_A >= 1 && nsub_A <= EVAL_JMAX), "stage A: subset of 1..64 joints");
  P2M_CHECK_ARG(JE >= 0 && JE <= EVAL_JMAX, "stage E: at most 64 joints");
  if (JE > 0) {
    P2M_CHECK_ARG(re_ptr && re_idx && re_val && mpjpe_E && pa_mpjpe_E, "stage E: null regressor or output");
    P2M_CHECK_ARG(root_E >= 0 && root_E < JE, "stage E: 0 <= root_E < JE");
    P2M_CHECK_ARG(sub_E == nullptr || (nsub_E >= 1 && nsub_E <= EVAL_JMAX), "stage E: subset of 1..64 joints");
  }
  P2M_CHECK_ARG(!pa_mesh || pa_mpvpe, "pa_mesh without a pa_mpvpe output");
  P2M_CHECK_ARG(totals == nullptr || (sample_means && n_groups >= 0), "totals need sample_means");
  if (B == 0) return P2M_OK;
  EvalArgs a;
  a.pred = pred_mesh; a.gt = gt_mesh; a.gt_scale = gt_mesh_scale; a.B = B; a.B_real = B_real; a.nv = nv;
  a.ra_ptr = ra_ptr; a.ra_idx = ra_idx; a.ra_val = ra_val; a.JA = JA; a.root_A = root_A; a.sub_A = sub_A; a.nsub_A = nsub_A;
  a.pred_joints_A = pred_joints_A; a.gt_joints_A = gt_joints_A;
  a.re_ptr = re_ptr; a.re_idx = re_idx; a.re_val = re_val; a.JE = JE; a.root_E = root_E; a.sub_E = sub_E; a.nsub_E = nsub_E;
  a.gt_joints_E = gt_joints_E; a.pa_mesh = pa_mesh ? 1 : 0;
  a.mpjpe_A = mpjpe_A; a.mpvpe = mpvpe; a.mpjpe_E = mpjpe_E; a.pa_mpjpe_E = pa_mpjpe_E; a.pa_mpvpe = pa_mpvpe;
  a.means = sample_means;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mesh_eval, dim3(B), dim3(EVAL_NT), 0, s, a);
  if (totals) hipLaunchKernelGGL(k_eval_fold, dim3(1), dim3(256), 0, s, sample_means, group, n_groups, B_real, totals);
  return check_launch("mesh_eval");
}
