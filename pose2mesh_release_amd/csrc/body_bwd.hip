// Body-model layer on the GPU (gfx950): the backward of body.hip - gradients of a loss with respect to pose, betas and
// trans, given the gradients with respect to verts, joints and extra (any of which may be absent).
//
// Two launches on one stream, no atomics, no allocation, no synchronisation (capturable):
//   k_body_bwd_vertex  the forward's tile, 64 vertices x BODY_TB samples, thread = one vertex COMPONENT.  Gathers the
//                      upstream gradient of its component (g_verts, + g_joints of the tips that name the vertex, + the
//                      column of the extra regressor, CSC), recomputes v_posed with the forward's own loop from the saved
//                      coefficient rows, forms g_x = T_v.R^T gv, and reduces the tile's 64 vertices into
//                        g_A_j[r][d] = sum_v w_vj gv[r] [x; 1][d]   (and g_off = sum_v gv as pseudo-joint J, weight 1)
//                        g_coef[k]   = sum_g dirs[k][g] g_x[g]      over the tile's 192 components, from the vertex-major
//                                      copy of the direction table [3V][Kpad] (thread = k, coalesced over k, g_x as LDS
//                                      broadcasts)
//                      written as per-block partials [block][sample][12 (J + 1) float64 | K fp32] into the backward
//                      workspace.
//   k_body_bwd_pose    one block per sample, in float64: 1024 threads fold the partials in block order (one element each, twelve
//                      loads in flight: with one wave the fold alone took 0.28 ms at SMPL size), then the first wave
//                      recomputes R, the rest joints and the chain, then the joint pre-pass, the reverse chain, Rodrigues backward (differentiating
//                      batch_rodrigues' exact sequence, its + 1e-8 included: no special case at theta = 0), g_betas, g_trans.
// Every output element is accumulated in one fixed order by one thread whose instruction sequence does not depend on the
// batch size or on the sample's slot in its tile: a sample's gradient is bitwise the same in any batch.
#include "p2m_body.h"

namespace p2m {

struct BodyBwdArgs {
  // what the forward saw
  const float* pose;         // [B, 3 J]
  const float* pose_mean;    // [3 J] or NULL
  const float* betas;        // [B, nb], or [nb] with betas_stride == 0
  int betas_stride;
  int has_trans;             // the forward added trans (else: subtracted chain joint `center`, if >= 0)
  int center;
  float scale;
  int B, V, J, nb, K;
  const float* tmpl;         // [3 V]
  const float* dirs;         // [K][3 V]
  const float* dirs_t;       // [3 V][kpad]  vertex-major copy, rows padded with zeros to kpad = K rounded up to 4
  const float* wt;           // [J][V]
  const float* jt;           // [J, 3]
  const float* js;           // [J, 3, nb]
  const int* parents;        // [J]
  const int* jslot;          // [J]
  int NJ;
  const int* tip_vert;       // [ntip]
  const int* tip_slot;       // [ntip]
  int ntip;
  const int* xc_ptr;         // [V + 1]  extra regressor by COLUMN (vertex): entries of vertex v, joints ascending
  const int* xc_idx;         // joint of an entry
  const float* xc_val;
  int JX;
  const float* ws;           // the forward's workspace of this call: coefficient rows, A matrices, offsets
  int ws_stride;
  // upstream gradients (NULL: none)
  const float* g_verts;      // [B, V, 3]
  const float* g_joints;     // [B, NJ, 3]
  const float* g_extra;      // [B, JX, 3]
  // per-block partials [nblk][B][part_stride floats]: 12 (J + 1) DOUBLES of g_A (joint J: g_off in column 3), then K floats
  // of g_coef
  float* part;
  int part_stride;
  int nblk;                  // vertex blocks whose partials exist (0: no gradient reaches a vertex)
  int need_coef;             // g_pose or g_betas is wanted
  // outputs (NULL: not wanted)
  float* g_pose;             // [B, 3 J]
  float* g_betas;            // [B, nb]
  float* g_trans;            // [B, 3]
};

// row length of a sample's v_posed / gv in LDS: padded so that the g_A threads, which differ in the sample, hit other banks
constexpr int BODY_BWD_SROW = BODY_NT + 4;
__host__ __device__ inline int body_bwd_jp8(int J) { return ((J + 8) / 8) * 8; }              // J + 1 rows, padded to 8
__host__ __device__ inline int body_bwd_part_floats(int J, int K) { return 24 * (J + 1) + ((K + 3) / 4) * 4; }
// LDS regions of k_body_bwd_vertex, in floats: region 1 holds the coefficient rows, then the weight tile; region 2 the A
// matrices, then g_x; then v_posed (float64) and gv of the tile.  At J = 64, K = 640 it is 62.4 KB, under the 64 KB a block
// may have
__host__ __device__ inline int body_bwd_r1(int J, int K) {
  const int cf = ((K + 3) / 4) * 4 * BODY_TB, w = BODY_VT * (body_bwd_jp8(J) + 4);
  return cf > w ? cf : w;
}
__host__ __device__ inline int body_bwd_r2(int J) {
  const int as = BODY_TB * 12 * J, gx = BODY_NT * BODY_TB;
  return as > gx ? as : gx;
}
static inline size_t body_bwd_lds(int J, int K) {
  return sizeof(float) * ((size_t)body_bwd_r1(J, K) + body_bwd_r2(J) + 3 * BODY_TB * BODY_BWD_SROW);
}

// ---- vertex stage -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BODY_NT) void k_body_bwd_vertex(BodyBwdArgs a) {
  extern __shared__ float4 body_bwd_lds_mem[];
  const int tid = threadIdx.x;
  const int s0 = blockIdx.y * BODY_TB;
  const int K = a.K, J = a.J, V3 = a.V * 3;
  const int kpad = ((K + 3) / 4) * 4;
  const int WS = body_bwd_jp8(J) + 4;                      // row stride of the weight tile
  float* r1 = reinterpret_cast<float*>(body_bwd_lds_mem);
  float* r2 = r1 + body_bwd_r1(J, K);
  double* xch = reinterpret_cast<double*>(r2 + body_bwd_r2(J));              // [BODY_TB][BODY_BWD_SROW]  v_posed, float64
  float* gvs = reinterpret_cast<float*>(xch + BODY_TB * BODY_BWD_SROW);      // [BODY_TB][BODY_BWD_SROW]  scale * upstream gradient
  float (*cf)[BODY_TB] = reinterpret_cast<float (*)[BODY_TB]>(r1);
  float* As = r2;
  // stage the sample tile as the forward does (slots past the batch: zeros - computed like any other, never stored)
  for (int i = tid; i < K * BODY_TB; i += BODY_NT) {
    const int s = i / K, k = i - s * K;
    cf[k][s] = s0 + s < a.B ? a.ws[(long)(s0 + s) * a.ws_stride + k] : 0.f;
  }
  for (int i = tid; i < J * 12 * BODY_TB; i += BODY_NT) {
    const int s = i / (J * 12), e = i - s * (J * 12);
    As[s * 12 * J + e] = s0 + s < a.B ? a.ws[(long)(s0 + s) * a.ws_stride + kpad + e] : 0.f;
  }
  __syncthreads();
  const int g0 = blockIdx.x * BODY_NT;
  const int g = g0 + tid;                                  // component index into [3 V]
  const bool on = g < V3;
  const int vl = tid / 3, c = tid - vl * 3;
  const int v = on ? g / 3 : 0;
  // v_posed, recomputed with the forward's loop, except that the template and the nb shape terms are summed in float64 and
  // the result stays float64: g_G_j.R = sum_v w gv (x) (x_v - J_j) cancels where g_A meets the rest joints (float64 in the
  // pose stage), and a shaped vertex rounded to fp32 would cost |x| / |x - J_j| there.  The pose terms cancel with nothing
  {
    float acc[BODY_TB];
    double sacc[BODY_TB];
#pragma unroll
    for (int s = 0; s < BODY_TB; s++) { acc[s] = 0.f; sacc[s] = 0.0; }
    const float* d = a.dirs + (on ? g : 0);
    for (int k = 0; k < a.nb; k++) {
      const double dv = on ? (double)d[(long)k * V3] : 0.0;
#pragma unroll
      for (int s = 0; s < BODY_TB; s++) sacc[s] = fma((double)cf[k][s], dv, sacc[s]);
    }
#pragma unroll 8
    for (int k = a.nb; k < K; k++) {
      const float dv = on ? d[(long)k * V3] : 0.f;
      const float4 c0 = *reinterpret_cast<const float4*>(&cf[k][0]);
      const float4 c1 = *reinterpret_cast<const float4*>(&cf[k][4]);
      acc[0] = fmaf(c0.x, dv, acc[0]);
      acc[1] = fmaf(c0.y, dv, acc[1]);
      acc[2] = fmaf(c0.z, dv, acc[2]);
      acc[3] = fmaf(c0.w, dv, acc[3]);
      acc[4] = fmaf(c1.x, dv, acc[4]);
      acc[5] = fmaf(c1.y, dv, acc[5]);
      acc[6] = fmaf(c1.z, dv, acc[6]);
      acc[7] = fmaf(c1.w, dv, acc[7]);
    }
    const double t = on ? (double)a.tmpl[g] : 0.0;
#pragma unroll
    for (int s = 0; s < BODY_TB; s++) xch[s * BODY_BWD_SROW + tid] = (t + sacc[s]) + (double)acc[s];
  }
  // upstream gradient of this component: g_verts, then the tips that name the vertex (ascending), then the regressor
  // column (joints ascending); times scale
  {
    float gt[BODY_TB];
#pragma unroll
    for (int s = 0; s < BODY_TB; s++) gt[s] = (on && s0 + s < a.B && a.g_verts) ? a.g_verts[(long)(s0 + s) * V3 + g] : 0.f;
    if (on && a.g_joints) {
      for (int t = 0; t < a.ntip; t++) {
        if (a.tip_vert[t] != v) continue;
        const int slot = a.tip_slot[t];
#pragma unroll
        for (int s = 0; s < BODY_TB; s++)
          if (s0 + s < a.B) gt[s] += a.g_joints[((long)(s0 + s) * a.NJ + slot) * 3 + c];
      }
    }
    if (on && a.g_extra) {
      for (int e = a.xc_ptr[v]; e < a.xc_ptr[v + 1]; e++) {
        const float xv = a.xc_val[e];
        const int j = a.xc_idx[e];
#pragma unroll
        for (int s = 0; s < BODY_TB; s++)
          if (s0 + s < a.B) gt[s] = fmaf(xv, a.g_extra[((long)(s0 + s) * a.JX + j) * 3 + c], gt[s]);
      }
    }
#pragma unroll
    for (int s = 0; s < BODY_TB; s++) gvs[s * BODY_BWD_SROW + tid] = gt[s] * a.scale;
  }
  __syncthreads();                                         // the coefficient rows are dead: region 1 takes the weight tile
  // weight tile [64 vertices][J + 1 rows, padded]: row J is 1 (its "A" gradient is g_off), vertices past V weigh 0
  for (int i = tid; i < body_bwd_jp8(J) * BODY_VT; i += BODY_NT) {
    const int j = i / BODY_VT, vv = i - j * BODY_VT;
    const int gv = blockIdx.x * BODY_VT + vv;
    float w = 0.f;
    if (j < J) w = gv < a.V ? a.wt[(long)j * a.V + gv] : 0.f;
    else if (j == J) w = 1.f;
    r1[vv * WS + j] = w;
  }
  __syncthreads();
  // g_x[v][c] = sum_r T_v[r][c] gv[r]: column c of T_v = sum_j w[v, j] A_j (j ascending)
  float gx[BODY_TB];
  {
    float T[BODY_TB][3];
#pragma unroll
    for (int s = 0; s < BODY_TB; s++) T[s][0] = T[s][1] = T[s][2] = 0.f;
    for (int j = 0; j < J; j++) {
      const float w = r1[vl * WS + j];
#pragma unroll
      for (int s = 0; s < BODY_TB; s++) {
        const float* m = &As[(s * J + j) * 12 + c];
        T[s][0] = fmaf(w, m[0], T[s][0]);
        T[s][1] = fmaf(w, m[4], T[s][1]);
        T[s][2] = fmaf(w, m[8], T[s][2]);
      }
    }
#pragma unroll
    for (int s = 0; s < BODY_TB; s++) {
      const float* gv = &gvs[s * BODY_BWD_SROW + vl * 3];
      gx[s] = fmaf(T[s][2], gv[2], fmaf(T[s][1], gv[1], T[s][0] * gv[0]));
    }
  }
  __syncthreads();                                         // the A matrices are dead: region 2 takes g_x
#pragma unroll
  for (int s = 0; s < BODY_TB; s++) r2[tid * BODY_TB + s] = gx[s];
  // g_A: thread = (entry e of the 3 x 4 matrix, sample s), joints in chunks of 8 (even chunks: threads 0..95, odd: 96..191).
  // Each output is one thread's sum over the 64 vertices, as two float64 halves added once, and stays float64 in the partials
  {
    const int half = tid / 96, rem = tid - half * 96;
    const int s = rem / 12, e = rem - s * 12, r = e >> 2, d = e & 3;
    const float* gvp = &gvs[s * BODY_BWD_SROW + r];
    const double* xp = &xch[s * BODY_BWD_SROW + (d < 3 ? d : 0)];
    const int nch = body_bwd_jp8(J) / 8;
    for (int ch = half; ch < nch; ch += 2) {
      double acc0[8], acc1[8];
#pragma unroll
      for (int i = 0; i < 8; i++) acc0[i] = acc1[i] = 0.0;
      for (int vv = 0; vv < BODY_VT / 2; vv++) {
        const int v1 = vv + BODY_VT / 2;
        const double p0 = (double)gvp[vv * 3] * (d < 3 ? xp[vv * 3] : 1.0);
        const double p1 = (double)gvp[v1 * 3] * (d < 3 ? xp[v1 * 3] : 1.0);
        const float4 w0a = *reinterpret_cast<const float4*>(&r1[vv * WS + ch * 8]);
        const float4 w0b = *reinterpret_cast<const float4*>(&r1[vv * WS + ch * 8 + 4]);
        const float4 w1a = *reinterpret_cast<const float4*>(&r1[v1 * WS + ch * 8]);
        const float4 w1b = *reinterpret_cast<const float4*>(&r1[v1 * WS + ch * 8 + 4]);
        acc0[0] = fma((double)w0a.x, p0, acc0[0]);
        acc0[1] = fma((double)w0a.y, p0, acc0[1]);
        acc0[2] = fma((double)w0a.z, p0, acc0[2]);
        acc0[3] = fma((double)w0a.w, p0, acc0[3]);
        acc0[4] = fma((double)w0b.x, p0, acc0[4]);
        acc0[5] = fma((double)w0b.y, p0, acc0[5]);
        acc0[6] = fma((double)w0b.z, p0, acc0[6]);
        acc0[7] = fma((double)w0b.w, p0, acc0[7]);
        acc1[0] = fma((double)w1a.x, p1, acc1[0]);
        acc1[1] = fma((double)w1a.y, p1, acc1[1]);
        acc1[2] = fma((double)w1a.z, p1, acc1[2]);
        acc1[3] = fma((double)w1a.w, p1, acc1[3]);
        acc1[4] = fma((double)w1b.x, p1, acc1[4]);
        acc1[5] = fma((double)w1b.y, p1, acc1[5]);
        acc1[6] = fma((double)w1b.z, p1, acc1[6]);
        acc1[7] = fma((double)w1b.w, p1, acc1[7]);
      }
      if (s0 + s < a.B) {
        double* out = reinterpret_cast<double*>(a.part + ((long)blockIdx.x * a.B + s0 + s) * a.part_stride);
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const int j = ch * 8 + i;
          if (j <= J) out[j * 12 + e] = acc0[i] + acc1[i];
        }
      }
    }
  }
  if (!a.need_coef) return;                                // uniform over the launch
  __syncthreads();
  // g_coef partial of the tile: thread = k, the table row of component g0 + gg read coalesced over k (rows past 3 V: the
  // last row, against a zero g_x), two halves of 96 components added once
  for (int k = tid; k < K; k += BODY_NT) {
    float b0[BODY_TB], b1[BODY_TB];
#pragma unroll
    for (int s = 0; s < BODY_TB; s++) b0[s] = b1[s] = 0.f;
    const float* T = a.dirs_t + k;
#pragma unroll 4
    for (int gg = 0; gg < BODY_NT / 2; gg++) {
      const int g1 = gg + BODY_NT / 2;
      const int row0 = min(g0 + gg, V3 - 1), row1 = min(g0 + g1, V3 - 1);
      const float d0 = T[(long)row0 * kpad], d1 = T[(long)row1 * kpad];
      const float4 x0 = *reinterpret_cast<const float4*>(&r2[gg * BODY_TB]);
      const float4 x1 = *reinterpret_cast<const float4*>(&r2[gg * BODY_TB + 4]);
      const float4 y0 = *reinterpret_cast<const float4*>(&r2[g1 * BODY_TB]);
      const float4 y1 = *reinterpret_cast<const float4*>(&r2[g1 * BODY_TB + 4]);
      b0[0] = fmaf(d0, x0.x, b0[0]);
      b0[1] = fmaf(d0, x0.y, b0[1]);
      b0[2] = fmaf(d0, x0.z, b0[2]);
      b0[3] = fmaf(d0, x0.w, b0[3]);
      b0[4] = fmaf(d0, x1.x, b0[4]);
      b0[5] = fmaf(d0, x1.y, b0[5]);
      b0[6] = fmaf(d0, x1.z, b0[6]);
      b0[7] = fmaf(d0, x1.w, b0[7]);
      b1[0] = fmaf(d1, y0.x, b1[0]);
      b1[1] = fmaf(d1, y0.y, b1[1]);
      b1[2] = fmaf(d1, y0.z, b1[2]);
      b1[3] = fmaf(d1, y0.w, b1[3]);
      b1[4] = fmaf(d1, y1.x, b1[4]);
      b1[5] = fmaf(d1, y1.y, b1[5]);
      b1[6] = fmaf(d1, y1.z, b1[6]);
      b1[7] = fmaf(d1, y1.w, b1[7]);
    }
#pragma unroll
    for (int s = 0; s < BODY_TB; s++)
      if (s0 + s < a.B) a.part[((long)blockIdx.x * a.B + s0 + s) * a.part_stride + 24 * (J + 1) + k] = b0[s] + b1[s];
  }
}

// ---- pose stage -----------------------------------------------------------------------------------------------------------
constexpr int BODY_BWD_PT = 1024;           // threads of k_body_bwd_pose: they fold; joint-per-lane work is the first wave's
constexpr int BODY_BWD_UNROLL = 12;         // loads in flight per thread of the fold

__global__ __launch_bounds__(BODY_BWD_PT) void k_body_bwd_pose(BodyBwdArgs a) {
  __shared__ double R[BODY_JMAX][9];          // local rotations
  __shared__ double G[BODY_JMAX][12];         // global transforms [R | t]
  __shared__ double Jr[BODY_JMAX][3];         // rest joints
  __shared__ double gR[BODY_JMAX][9], gG[BODY_JMAX][12], gJr[BODY_JMAX][3];
  __shared__ double gA[(BODY_JMAX + 1) * 12];
  __shared__ double gcoef[BODY_KMAX];
  __shared__ double goff[3];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int J = a.J, nb = a.nb, K = a.K;
  const double scale = (double)a.scale;
  const float* beta = a.betas + (long)b * a.betas_stride;
  // fold the per-block partials, in block order
  const int nA = 12 * (J + 1);
  const int nfold = a.need_coef ? nA + K : nA;
  for (int i = tid; i < nfold; i += BODY_BWD_PT) {
    double acc = 0.0;
    const float* p = a.part + (long)b * a.part_stride;
    const long step = (long)a.B * a.part_stride;
    const bool isA = i < nA;
    int blk = 0;
    for (; blk + BODY_BWD_UNROLL <= a.nblk; blk += BODY_BWD_UNROLL) {
      double v[BODY_BWD_UNROLL];
#pragma unroll
      for (int u = 0; u < BODY_BWD_UNROLL; u++)
        v[u] = isA ? reinterpret_cast<const double*>(p + (blk + u) * step)[i] : (double)p[(blk + u) * step + nA + i];
#pragma unroll
      for (int u = 0; u < BODY_BWD_UNROLL; u++) acc += v[u];
    }
    for (; blk < a.nblk; blk++)
      acc += isA ? reinterpret_cast<const double*>(p + blk * step)[i] : (double)p[blk * step + nA + i];
    if (isA) gA[i] = acc; else gcoef[i - nA] = acc;
  }
  // Rodrigues forward, joint per lane (J <= 64): everything the backward needs stays in this lane's registers
  double th[3] = {0, 0, 0}, ang = 1, n[3] = {0, 0, 0}, ch = 1, sh = 0, qn = 1, q[4] = {1, 0, 0, 0};
  if (tid < J) {
    const int j = tid;
    float x = a.pose[((long)b * J + j) * 3], y = a.pose[((long)b * J + j) * 3 + 1], z = a.pose[((long)b * J + j) * 3 + 2];
    if (a.pose_mean) { x += a.pose_mean[j * 3]; y += a.pose_mean[j * 3 + 1]; z += a.pose_mean[j * 3 + 2]; }
    th[0] = x; th[1] = y; th[2] = z;
    const double ex = th[0] + 1e-8, ey = th[1] + 1e-8, ez = th[2] + 1e-8;
    ang = sqrt(ex * ex + ey * ey + ez * ez);
    n[0] = th[0] / ang; n[1] = th[1] / ang; n[2] = th[2] / ang;
    const double h = ang * 0.5;
    ch = cos(h); sh = sin(h);
    const double qt[4] = {ch, sh * n[0], sh * n[1], sh * n[2]};
    qn = sqrt(qt[0] * qt[0] + qt[1] * qt[1] + qt[2] * qt[2] + qt[3] * qt[3]);
    q[0] = qt[0] / qn; q[1] = qt[1] / qn; q[2] = qt[2] / qn; q[3] = qt[3] / qn;
    const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
    const double w2 = qw * qw, x2 = qx * qx, y2 = qy * qy, z2 = qz * qz;
    const double wx = qw * qx, wy = qw * qy, wz = qw * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz;
    R[j][0] = w2 + x2 - y2 - z2; R[j][1] = 2 * xy - 2 * wz; R[j][2] = 2 * wy + 2 * xz;
    R[j][3] = 2 * wz + 2 * xy; R[j][4] = w2 - x2 + y2 - z2; R[j][5] = 2 * yz - 2 * wx;
    R[j][6] = 2 * xz - 2 * wy; R[j][7] = 2 * wx + 2 * yz; R[j][8] = w2 - x2 - y2 + z2;
  }
  for (int i = tid; i < 3 * J; i += BODY_BWD_PT) {
    double acc = (double)a.jt[i];
    for (int m = 0; m < nb; m++) acc += (double)a.js[i * nb + m] * (double)beta[m];
    Jr[i / 3][i % 3] = acc;
  }
  __syncthreads();
  // chain forward: G_0 = [R_0 | J_0], G_j = G_parent [R_j | J_j - J_parent]; 12 lanes, one entry each
  const int r = (tid >> 2) % 3, c = tid & 3;
  if (tid < 12) G[0][tid] = c < 3 ? R[0][r * 3 + c] : Jr[0][r];
  __syncthreads();
  for (int j = 1; j < J; j++) {
    const int p = a.parents[j];
    if (tid < 12) {
      double v;
      if (c < 3) v = G[p][r * 4] * R[j][c] + G[p][r * 4 + 1] * R[j][3 + c] + G[p][r * 4 + 2] * R[j][6 + c];
      else v = G[p][r * 4] * (Jr[j][0] - Jr[p][0]) + G[p][r * 4 + 1] * (Jr[j][1] - Jr[p][1]) +
               G[p][r * 4 + 2] * (Jr[j][2] - Jr[p][2]) + G[p][r * 4 + 3];
      G[j][tid] = v;
    }
    __syncthreads();
  }
  // g_off = sum_v gv (pseudo-joint J of the partials) + scale * sum over the chain joints of the output, j ascending
  if (tid < 3) {
    double go = gA[J * 12 + tid * 4 + 3];
    if (a.g_joints)
      for (int j = 0; j < J; j++) {
        const int slot = a.jslot[j];
        if (slot >= 0) go += scale * (double)a.g_joints[((long)b * a.NJ + slot) * 3 + tid];
      }
    goff[tid] = go;
  }
  __syncthreads();
  // joint pre-pass, joint per lane: A_j = [G_j.R | G_j.t - G_j.R J_j], joints_j = (G_j.t + off) scale, off = -G_center.t
  if (tid < J) {
    const int j = tid, slot = a.jslot[j];
#pragma unroll
    for (int rr = 0; rr < 3; rr++) {
      const double gt = gA[j * 12 + rr * 4 + 3];
#pragma unroll
      for (int cc = 0; cc < 3; cc++) gG[j][rr * 4 + cc] = gA[j * 12 + rr * 4 + cc] - gt * Jr[j][cc];
      double t = gt;
      if (slot >= 0 && a.g_joints) t += scale * (double)a.g_joints[((long)b * a.NJ + slot) * 3 + rr];
      if (!a.has_trans && a.center == j) t -= goff[rr];
      gG[j][rr * 4 + 3] = t;
    }
#pragma unroll
    for (int cc = 0; cc < 3; cc++)
      gJr[j][cc] = -(G[j][cc] * gA[j * 12 + 3] + G[j][4 + cc] * gA[j * 12 + 7] + G[j][8 + cc] * gA[j * 12 + 11]);
#pragma unroll
    for (int e = 0; e < 9; e++) gR[j][e] = 0.0;
  }
  __syncthreads();
  // reverse chain: lanes 0..8 g_R_j, 9..17 g_G_p.R, 18..20 g_G_p.t, 21..23 the rest joints.  A step reads g_G_j and writes
  // g_G_p, p < j
  for (int j = J - 1; j >= 1; j--) {
    const int p = a.parents[j];
    if (tid < 9) {
      const int aa = tid / 3, cc = tid - aa * 3;
      gR[j][tid] = G[p][aa] * gG[j][cc] + G[p][4 + aa] * gG[j][4 + cc] + G[p][8 + aa] * gG[j][8 + cc];
    } else if (tid < 18) {
      const int l = tid - 9, rr = l / 3, aa = l - rr * 3;
      gG[p][rr * 4 + aa] += gG[j][rr * 4] * R[j][aa * 3] + gG[j][rr * 4 + 1] * R[j][aa * 3 + 1] +
                            gG[j][rr * 4 + 2] * R[j][aa * 3 + 2] + gG[j][rr * 4 + 3] * (Jr[j][aa] - Jr[p][aa]);
    } else if (tid < 21) {
      const int rr = tid - 18;
      gG[p][rr * 4 + 3] += gG[j][rr * 4 + 3];
    } else if (tid < 24) {
      const int aa = tid - 21;
      const double u = G[p][aa] * gG[j][3] + G[p][4 + aa] * gG[j][7] + G[p][8 + aa] * gG[j][11];
      gJr[j][aa] += u;
      gJr[p][aa] -= u;
    }
    __syncthreads();
  }
  if (tid < 9) gR[0][tid] = gG[0][(tid / 3) * 4 + tid % 3];
  else if (tid < 12) gJr[0][tid - 9] += gG[0][(tid - 9) * 4 + 3];
  __syncthreads();
  if (a.g_trans && tid < 3) a.g_trans[(long)b * 3 + tid] = (float)goff[tid];
  if (a.g_betas) {
    for (int m = tid; m < nb; m += BODY_BWD_PT) {
      double acc = gcoef[m];
      for (int i = 0; i < 3 * J; i++) acc += (double)a.js[i * nb + m] * gJr[i / 3][i % 3];
      a.g_betas[(long)b * nb + m] = (float)acc;
    }
  }
  // Rodrigues backward: R(q), q = qt / |qt|, qt = (cos h, sin h n), h = a / 2, n = theta / a, a = |theta + 1e-8|
  if (a.g_pose && tid < J) {
    const int j = tid;
    double Gm[9];
#pragma unroll
    for (int e = 0; e < 9; e++) Gm[e] = gR[j][e] + (j >= 1 ? gcoef[nb + (j - 1) * 9 + e] : 0.0);
    const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
    const double tr = Gm[0] + Gm[4] + Gm[8];
    const double ax = Gm[7] - Gm[5], ay = Gm[2] - Gm[6], az = Gm[3] - Gm[1];
    const double s01 = Gm[1] + Gm[3], s02 = Gm[2] + Gm[6], s12 = Gm[5] + Gm[7];
    double gq[4];
    gq[0] = 2 * (qw * tr + qx * ax + qy * ay + qz * az);
    gq[1] = 2 * (qx * (Gm[0] - Gm[4] - Gm[8]) + qy * s01 + qz * s02 + qw * ax);
    gq[2] = 2 * (qy * (-Gm[0] + Gm[4] - Gm[8]) + qx * s01 + qz * s12 + qw * ay);
    gq[3] = 2 * (qz * (-Gm[0] - Gm[4] + Gm[8]) + qx * s02 + qy * s12 + qw * az);
    const double dot = q[0] * gq[0] + q[1] * gq[1] + q[2] * gq[2] + q[3] * gq[3];
    double gt[4];
#pragma unroll
    for (int e = 0; e < 4; e++) gt[e] = (gq[e] - q[e] * dot) / qn;
    const double gh = -sh * gt[0] + ch * (n[0] * gt[1] + n[1] * gt[2] + n[2] * gt[3]);
    const double gn[3] = {sh * gt[1], sh * gt[2], sh * gt[3]};
    const double ga = -(th[0] * gn[0] + th[1] * gn[1] + th[2] * gn[2]) / (ang * ang) + 0.5 * gh;
#pragma unroll
    for (int e = 0; e < 3; e++)
      a.g_pose[((long)b * J + j) * 3 + e] = (float)(gn[e] / ang + ga * (th[e] + 1e-8) / ang);
  }
}

static inline bool al(const void* p, size_t n) { return ((uintptr_t)p % n) == 0; }

}  // namespace p2m

using namespace p2m;

extern "C" int64_t p2m_body_backward_workspace(int32_t B, int32_t V, int32_t J, int32_t nb) {
  if (B < 1 || V < 1 || J < 1 || J > BODY_JMAX || nb < 0 || nb + 9 * (J - 1) < 1 || nb + 9 * (J - 1) > BODY_KMAX) return -1;
  return (int64_t)cdiv((long)V, BODY_VT) * B * body_bwd_part_floats(J, nb + 9 * (J - 1)) * (int64_t)sizeof(float);
}

extern "C" int p2m_body_backward(const float* pose, const float* pose_mean, const float* betas, int32_t betas_per_sample,
                                 int32_t has_trans, int32_t center_joint, float scale, int32_t B, int32_t V, int32_t J,
                                 int32_t nb, const float* v_template, const float* dirs, const float* dirs_t,
                                 const float* weights_t, const float* joint_template, const float* joint_shapedirs,
                                 const int32_t* parents, const int32_t* joint_slot, int32_t n_joints_out,
                                 const int32_t* tip_vert, const int32_t* tip_slot, int32_t n_tips, const int32_t* xc_ptr,
                                 const int32_t* xc_idx, const float* xc_val, int32_t n_extra, const void* fwd_workspace,
                                 int64_t fwd_workspace_bytes, const float* g_verts, const float* g_joints,
                                 const float* g_extra, void* workspace, int64_t workspace_bytes, float* g_pose,
                                 float* g_betas, float* g_trans, void* stream) {
  P2M_CHECK_ARG(pose && betas && v_template && dirs && weights_t && joint_template && joint_shapedirs && parents &&
                joint_slot && fwd_workspace && workspace, "null pointer");
  P2M_CHECK_ARG(B >= 1 && V >= 1 && J >= 1, "B, V and J must be >= 1");
  P2M_CHECK_ARG(J <= BODY_JMAX, "at most 64 chain joints");
  const int K = nb + 9 * (J - 1);
  P2M_CHECK_ARG(nb >= 0 && K >= 1 && K <= BODY_KMAX, "nb + 9 (J - 1) must be in [1, 640]");
  P2M_CHECK_ARG((long)B * V * 3 < (1L << 31) && (long)(K + 3) * V * 3 < (1L << 31) && cdiv(B, BODY_TB) <= 65535,
                "more than 2^31 coordinates or table entries, or more than 65535 sample tiles");
  P2M_CHECK_ARG(center_joint >= -1 && center_joint < J, "center_joint outside [-1, J)");
  P2M_CHECK_ARG(n_tips >= 0 && n_tips <= BODY_JMAX && (n_tips == 0 || (tip_vert && tip_slot)), "tips: 0..64, with tables");
  P2M_CHECK_ARG(n_joints_out >= 1 && n_joints_out <= J + n_tips, "n_joints_out outside [1, J + n_tips]");
  P2M_CHECK_ARG(n_extra >= 0 && n_extra <= BODY_JMAX && (n_extra == 0 || !g_extra || (xc_ptr && xc_idx && xc_val)),
                "extra regressor: 0..64 joints; g_extra needs the column tables");
  P2M_CHECK_ARG(g_extra == nullptr || n_extra > 0, "g_extra without an extra regressor");
  P2M_CHECK_ARG(g_pose || g_betas || g_trans, "no gradient output");
  P2M_CHECK_ARG(g_verts || g_joints || g_extra, "no upstream gradient");
  P2M_CHECK_ARG(!g_trans || has_trans, "g_trans: the forward had no trans");
  P2M_CHECK_ARG(!g_betas || betas_per_sample, "g_betas: the forward used the stored betas");
  P2M_CHECK_ARG(!(g_pose || g_betas) || dirs_t, "g_pose / g_betas need the vertex-major table dirs_t");
  P2M_CHECK_ARG(al(pose, 4) && al(pose_mean, 4) && al(betas, 4) && al(v_template, 4) && al(dirs, 4) && al(dirs_t, 4) &&
                al(weights_t, 4) && al(joint_template, 4) && al(joint_shapedirs, 4) && al(parents, 4) && al(joint_slot, 4) &&
                al(tip_vert, 4) && al(tip_slot, 4) && al(xc_ptr, 4) && al(xc_idx, 4) && al(xc_val, 4) && al(g_verts, 4) &&
                al(g_joints, 4) && al(g_extra, 4) && al(g_pose, 4) && al(g_betas, 4) && al(g_trans, 4) &&
                al(fwd_workspace, 16) && al(workspace, 16), "misaligned buffer (4 bytes; workspaces: 16)");
  P2M_CHECK_ARG(fwd_workspace_bytes >= (int64_t)B * body_ws_floats(J, K) * (int64_t)sizeof(float),
                "forward workspace smaller than p2m_body_workspace()");
  P2M_CHECK_ARG(workspace_bytes >= p2m_body_backward_workspace(B, V, J, nb), "workspace smaller than p2m_body_backward_workspace()");
  BodyBwdArgs a;
  a.pose = pose; a.pose_mean = pose_mean; a.betas = betas; a.betas_stride = betas_per_sample ? nb : 0;
  a.has_trans = has_trans != 0; a.center = center_joint; a.scale = scale; a.B = B; a.V = V; a.J = J; a.nb = nb; a.K = K;
  a.tmpl = v_template; a.dirs = dirs; a.dirs_t = dirs_t; a.wt = weights_t; a.jt = joint_template; a.js = joint_shapedirs;
  a.parents = parents; a.jslot = joint_slot; a.NJ = n_joints_out;
  a.tip_vert = tip_vert; a.tip_slot = tip_slot; a.ntip = n_tips;
  a.xc_ptr = xc_ptr; a.xc_idx = xc_idx; a.xc_val = xc_val; a.JX = n_extra;
  a.ws = (const float*)fwd_workspace; a.ws_stride = body_ws_floats(J, K);
  a.g_verts = g_verts; a.g_joints = g_joints; a.g_extra = g_extra;
  a.part = (float*)workspace; a.part_stride = body_bwd_part_floats(J, K);
  a.need_coef = (g_pose || g_betas) ? 1 : 0;
  a.g_pose = g_pose; a.g_betas = g_betas; a.g_trans = g_trans;
  // a gradient reaches a vertex through g_verts, g_extra, or g_joints of a tip
  a.nblk = (g_verts || g_extra || (g_joints && n_tips > 0)) ? cdiv((long)V, BODY_VT) : 0;
  hipStream_t s = (hipStream_t)stream;
  if (a.nblk > 0)
    hipLaunchKernelGGL(k_body_bwd_vertex, dim3(a.nblk, cdiv(B, BODY_TB)), dim3(BODY_NT), body_bwd_lds(J, K), s, a);
  hipLaunchKernelGGL(k_body_bwd_pose, dim3(B), dim3(BODY_BWD_PT), 0, s, a);
  return check_launch("body_backward");
}
