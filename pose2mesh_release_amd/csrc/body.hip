// Body-model layer on the GPU (gfx950): the forward of the SMPL / MANO layers the datasets call once per sample on a
// dataloader worker to make a target mesh - parameters in, vertices and joints out, for a whole batch.
//
// Reference arithmetic (PyTorch on the host there):
//   batch_rodrigues / quat2mat (through the quaternion, with its + 1e-8)      smplpytorch/pytorch/rodrigues_layer.py:15-52
//   SMPL_Layer.forward                                                        smplpytorch/pytorch/smpl_layer.py:65-158
//   ManoLayer.forward (use_pca=False, axis-angle root)                        manopth/manolayer.py:109-273
//
// Three launches on one stream, no atomics, no allocation, no synchronisation (capturable):
//   k_body_pose   one wave per sample: Rodrigues per joint, the coefficient row [beta | R_j - I, j >= 1], the rest
//                 joints (from J_regressor . template and J_regressor . shapedirs, folded on the host), the kinematic
//                 chain, the skinning matrices A_j = [R_j | t_j - R_j J_j], the offset and the chain joints
//   k_body_skin   64 vertices x BODY_TB samples per block: thread = one vertex COMPONENT, the direction table is read
//                 coefficient-major [K][3V] (a wave reads 64 consecutive floats per coefficient), the sample tile's
//                 coefficient rows and A matrices sit in LDS and are read as broadcasts; the three components of a vertex
//                 meet through LDS for the skinning; rows of [B, V, 3] are stored coalesced
//   k_body_tail   the appended tip vertices of the joint set and the optional extra_regressor @ verts
// Plain fp32 fmaf on the VALU, every output element accumulated in one fixed order by one thread whose instruction
// sequence does not depend on the batch size or on the sample's slot in its tile: a sample's result is bitwise the same
// in any batch.
#include "p2m_body.h"

namespace p2m {

struct BodyArgs {
  // inputs
  const float* pose;         // [B, 3 J]  axis-angle
  const float* pose_mean;    // [3 J] added to pose (MANO: 0 for the root, hands_mean after) or NULL
  const float* betas;        // [B, nb], or [nb] with betas_stride == 0 (the model's stored betas)
  int betas_stride;
  const float* trans;        // [B, 3] or NULL
  int center;                // chain joint subtracted when trans == NULL; -1: none
  float scale;
  int B, V, J, nb, K;
  // model tables
  const float* tmpl;         // [3 V]
  const float* dirs;         // [K][3 V]   shapedirs then posedirs, coefficient-major
  const float* wt;           // [J][V]     skinning weights, joint-major
  const float* jt;           // [J, 3]     J_regressor . template
  const float* js;           // [J, 3, nb] J_regressor . shapedirs
  const int* parents;        // [J]
  const int* jslot;          // [J]  output slot of chain joint j in joints (-1: not an output)
  int NJ;                    // joints per sample of the output
  // workspace (floats per sample: see body_ws_floats)
  float* ws;
  int ws_stride;
  // outputs
  float* verts;              // [B, V, 3]
  float* joints;             // [B, NJ, 3]
};

// dynamic LDS of k_body_skin in bytes: at J = 64, K = 640 it is 51.3 KB, under the 64 KB a block may have
static inline size_t body_skin_lds(int J, int K) {
  return sizeof(float) * ((size_t)((K + 3) / 4) * 4 * BODY_TB + (size_t)BODY_TB * 12 * J + BODY_TB * BODY_NT + BODY_TB * 4);
}

// ---- pose kernel ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_body_pose(BodyArgs a) {
  __shared__ float R[BODY_JMAX][9];         // local rotations
  __shared__ float G[BODY_JMAX][12];        // global transforms [R | t], row-major 3 x 4
  __shared__ float Jr[BODY_JMAX][3];        // rest joints
  __shared__ float off[3];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int J = a.J, nb = a.nb;
  float* ws = a.ws + (long)b * a.ws_stride;
  float* coef = ws;
  float* A = ws + ((a.K + 3) / 4) * 4;
  float* woff = A + 12 * J;
  const float* beta = a.betas + (long)b * a.betas_stride;
  // Rodrigues, joint per lane (rodrigues_layer.py:41-52, 15-38)
  for (int j = tid; j < J; j += 64) {
    float x = a.pose[((long)b * J + j) * 3], y = a.pose[((long)b * J + j) * 3 + 1], z = a.pose[((long)b * J + j) * 3 + 2];
    if (a.pose_mean) { x += a.pose_mean[j * 3]; y += a.pose_mean[j * 3 + 1]; z += a.pose_mean[j * 3 + 2]; }
    const float ex = x + 1e-8f, ey = y + 1e-8f, ez = z + 1e-8f;
    const float angle = sqrtf(fmaf(ez, ez, fmaf(ey, ey, ex * ex)));
    const float nx = x / angle, ny = y / angle, nz = z / angle;
    const float h = angle * 0.5f;
    const float c = cosf(h), s = sinf(h);
    float qw = c, qx = s * nx, qy = s * ny, qz = s * nz;
    const float qn = sqrtf(fmaf(qz, qz, fmaf(qy, qy, fmaf(qx, qx, qw * qw))));
    qw /= qn; qx /= qn; qy /= qn; qz /= qn;
    const float w2 = qw * qw, x2 = qx * qx, y2 = qy * qy, z2 = qz * qz;
    const float wx = qw * qx, wy = qw * qy, wz = qw * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz;
    const float r[9] = {w2 + x2 - y2 - z2, 2.f * xy - 2.f * wz, 2.f * wy + 2.f * xz,
                        2.f * wz + 2.f * xy, w2 - x2 + y2 - z2, 2.f * yz - 2.f * wx,
                        2.f * xz - 2.f * wy, 2.f * wx + 2.f * yz, w2 - x2 - y2 + z2};
#pragma unroll
    for (int e = 0; e < 9; e++) {
      R[j][e] = r[e];
      if (j >= 1) coef[nb + (j - 1) * 9 + e] = r[e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
    }
  }
  for (int n = tid; n < nb; n += 64) coef[n] = beta[n];
  // rest joints: J_regressor . (template + shapedirs beta), folded
  for (int i = tid; i < 3 * J; i += 64) {
    float acc = a.jt[i];
    for (int n = 0; n < nb; n++) acc = fmaf(a.js[i * nb + n], beta[n], acc);
    Jr[i / 3][i % 3] = acc;
  }
  __syncthreads();
  // chain (smpl_layer.py:103-118): G_0 = [R_0 | J_0], G_j = G_parent [R_j | J_j - J_parent]; 12 lanes, one entry each
  const int r = (tid >> 2) % 3, c = tid & 3;
  if (tid < 12) G[0][tid] = c < 3 ? R[0][r * 3 + c] : Jr[0][r];
  __syncthreads();
  for (int j = 1; j < J; j++) {
    const int p = a.parents[j];
    if (tid < 12) {
      float v;
      if (c < 3) {
        v = G[p][r * 4] * R[j][c];
        v = fmaf(G[p][r * 4 + 1], R[j][3 + c], v);
        v = fmaf(G[p][r * 4 + 2], R[j][6 + c], v);
      } else {
        v = G[p][r * 4] * (Jr[j][0] - Jr[p][0]);
        v = fmaf(G[p][r * 4 + 1], Jr[j][1] - Jr[p][1], v);
        v = fmaf(G[p][r * 4 + 2], Jr[j][2] - Jr[p][2], v);
        v += G[p][r * 4 + 3];
      }
      G[j][tid] = v;
    }
    __syncthreads();
  }
  // offset: the translation, or minus the centre joint (smpl_layer.py:146-154)
  if (tid < 3) {
    float o = 0.f;
    if (a.trans) o = a.trans[(long)b * 3 + tid];
    else if (a.center >= 0) o = -G[a.center][tid * 4 + 3];
    off[tid] = o;
    woff[tid] = o;
  }
  if (tid == 3) woff[3] = 0.f;
  __syncthreads();
  // skinning matrices A_j = G_j - pack(G_j [J_j; 0]) (smpl_layer.py:121-132) and the chain joints of the output
  for (int i = tid; i < 12 * J; i += 64) {
    const int j = i / 12, e = i - j * 12, rr = e >> 2, cc = e & 3;
    float v = G[j][e];
    if (cc == 3) {
      float t = G[j][rr * 4] * Jr[j][0];
      t = fmaf(G[j][rr * 4 + 1], Jr[j][1], t);
      t = fmaf(G[j][rr * 4 + 2], Jr[j][2], t);
      const float g = v;
      v = g - t;
      const int slot = a.jslot[j];
      if (slot >= 0) a.joints[((long)b * a.NJ + slot) * 3 + rr] = (g + off[rr]) * a.scale;
    }
    A[i] = v;
  }
}

// ---- skin kernel ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BODY_NT) void k_body_skin(BodyArgs a) {
  extern __shared__ float4 body_lds[];                 // sized by the launch to K and J (body_skin_lds)
  const int tid = threadIdx.x;
  const int s0 = blockIdx.y * BODY_TB;
  const int K = a.K, J = a.J, V3 = a.V * 3;
  const int kpad = ((K + 3) / 4) * 4;
  float (*cf)[BODY_TB] = reinterpret_cast<float (*)[BODY_TB]>(body_lds);          // [K]  coefficient k of the tile's samples
  float* As = &cf[kpad][0];                                                       // [BODY_TB][12 J]  skinning matrices
  float (*xch)[BODY_NT] = reinterpret_cast<float (*)[BODY_NT]>(As + BODY_TB * 12 * J);   // v_posed of the tile
  float (*offs)[4] = reinterpret_cast<float (*)[4]>(&xch[BODY_TB][0]);
  // stage the sample tile (slots past the batch: zeros - computed like any other, never stored)
  for (int i = tid; i < K * BODY_TB; i += BODY_NT) {
    const int s = i / K, k = i - s * K;
    cf[k][s] = s0 + s < a.B ? a.ws[(long)(s0 + s) * a.ws_stride + k] : 0.f;
  }
  for (int i = tid; i < J * 12 * BODY_TB; i += BODY_NT) {
    const int s = i / (J * 12), e = i - s * (J * 12);
    As[s * 12 * J + e] = s0 + s < a.B ? a.ws[(long)(s0 + s) * a.ws_stride + kpad + e] : 0.f;
  }
  if (tid < BODY_TB * 4) {
    const int s = tid >> 2, e = tid & 3;
    offs[s][e] = s0 + s < a.B ? a.ws[(long)(s0 + s) * a.ws_stride + kpad + 12 * J + e] : 0.f;
  }
  __syncthreads();
  const int g = blockIdx.x * BODY_NT + tid;           // component index into [3 V]
  const bool on = g < V3;
  // blend: v_posed = template + (sum_k coef[k] dirs[k], k ascending).  The offsets are summed on their own and the
  // template added last: 217 roundings at the size of the offsets (centimetres), not at the size of the template - summed
  // into the template one by one they cost 2.5 x the error of the reference's fp32 run
  float acc[BODY_TB];
#pragma unroll
  for (int s = 0; s < BODY_TB; s++) acc[s] = 0.f;
  const float* d = a.dirs + (on ? g : 0);
#pragma unroll 4
  for (int k = 0; k < K; k++) {
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
  {
    const float t = on ? a.tmpl[g] : 0.f;
#pragma unroll
    for (int s = 0; s < BODY_TB; s++) xch[s][tid] = t + acc[s];
  }
  __syncthreads();
  // skin: row c of T_v = sum_j w[v, j] A_j (j ascending), applied to [v_posed, 1]
  const int vl = tid / 3, c = tid - vl * 3;
  const int v = on ? g / 3 : 0;
  float T[BODY_TB][4];
#pragma unroll
  for (int s = 0; s < BODY_TB; s++) T[s][0] = T[s][1] = T[s][2] = T[s][3] = 0.f;
  for (int j = 0; j < J; j++) {
    const float w = on ? a.wt[(long)j * a.V + v] : 0.f;
#pragma unroll
    for (int s = 0; s < BODY_TB; s++) {
      const float4 m = *reinterpret_cast<const float4*>(&As[(s * J + j) * 12 + c * 4]);
      T[s][0] = fmaf(w, m.x, T[s][0]);
      T[s][1] = fmaf(w, m.y, T[s][1]);
      T[s][2] = fmaf(w, m.z, T[s][2]);
      T[s][3] = fmaf(w, m.w, T[s][3]);
    }
  }
#pragma unroll
  for (int s = 0; s < BODY_TB; s++) {
    const float x = xch[s][vl * 3], y = xch[s][vl * 3 + 1], z = xch[s][vl * 3 + 2];
    float o = fmaf(T[s][2], z, fmaf(T[s][1], y, fmaf(T[s][0], x, T[s][3])));
    o = (o + offs[s][c]) * a.scale;
    if (on && s0 + s < a.B) a.verts[(long)(s0 + s) * V3 + g] = o;
  }
}

// ---- tail: tip vertices of the joint set and the extra regressor ---------------------------------------------------------------
__global__ __launch_bounds__(64) void k_body_tail(const float* __restrict__ verts, int V, float* __restrict__ joints, int NJ,
                                                  const int* __restrict__ tip_vert, const int* __restrict__ tip_slot, int ntip,
                                                  const int* __restrict__ xr_ptr, const int* __restrict__ xr_idx,
                                                  const float* __restrict__ xr_val, int JX, float* __restrict__ extra) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* m = verts + (long)b * V * 3;
  for (int i = tid; i < ntip * 3; i += 64) {
    const int t = i / 3, k = i - t * 3;
    joints[((long)b * NJ + tip_slot[t]) * 3 + k] = m[tip_vert[t] * 3 + k];
  }
  for (int i = tid; i < JX * 3; i += 64) {          // fp64 over the CSR row, in its order, rounded once
    const int j = i / 3, k = i - j * 3;
    double acc = 0.0;
    for (int e = xr_ptr[j]; e < xr_ptr[j + 1]; e++) acc += (double)xr_val[e] * (double)m[xr_idx[e] * 3 + k];
    extra[((long)b * JX + j) * 3 + k] = (float)acc;
  }
}

static inline bool al(const void* p, size_t n) { return ((uintptr_t)p % n) == 0; }

}  // namespace p2m

using namespace p2m;

extern "C" int32_t p2m_body_sample_tile(void) { return BODY_TB; }
extern "C" int32_t p2m_body_vertex_tile(void) { return BODY_VT; }

extern "C" int64_t p2m_body_workspace(int32_t B, int32_t J, int32_t nb) {
  if (B < 1 || J < 1 || J > BODY_JMAX || nb < 0) return -1;
  return (int64_t)B * body_ws_floats(J, nb + 9 * (J - 1)) * (int64_t)sizeof(float);
}

extern "C" int p2m_body_forward(const float* pose, const float* pose_mean, const float* betas, int32_t betas_per_sample,
                                const float* trans, int32_t center_joint, float scale, int32_t B, int32_t V, int32_t J,
                                int32_t nb, const float* v_template, const float* dirs, const float* weights_t,
                                const float* joint_template, const float* joint_shapedirs, const int32_t* parents,
                                const int32_t* joint_slot, int32_t n_joints_out, const int32_t* tip_vert,
                                const int32_t* tip_slot, int32_t n_tips, const int32_t* xr_ptr, const int32_t* xr_idx,
                                const float* xr_val, int32_t n_extra, void* workspace, int64_t workspace_bytes, float* verts,
                                float* joints, float* extra, void* stream) {
  P2M_CHECK_ARG(pose && betas && v_template && dirs && weights_t && joint_template && joint_shapedirs && parents &&
                joint_slot && workspace && verts && joints, "null pointer");
  P2M_CHECK_ARG(B >= 1 && V >= 1 && J >= 1, "B, V and J must be >= 1");
  P2M_CHECK_ARG(J <= BODY_JMAX, "at most 64 chain joints");
  const int K = nb + 9 * (J - 1);
  P2M_CHECK_ARG(nb >= 0 && K >= 1 && K <= BODY_KMAX, "nb + 9 (J - 1) must be in [1, 640]");
  P2M_CHECK_ARG((long)B * V * 3 < (1L << 31) && (long)K * V * 3 < (1L << 31) && cdiv(B, BODY_TB) <= 65535,
                "more than 2^31 coordinates or table entries, or more than 65535 sample tiles");
  P2M_CHECK_ARG(center_joint >= -1 && center_joint < J, "center_joint outside [-1, J)");
  P2M_CHECK_ARG(n_tips >= 0 && n_tips <= BODY_JMAX && (n_tips == 0 || (tip_vert && tip_slot)), "tips: 0..64, with tables");
  P2M_CHECK_ARG(n_joints_out >= 1 && n_joints_out <= J + n_tips, "n_joints_out outside [1, J + n_tips]");
  P2M_CHECK_ARG(n_extra >= 0 && n_extra <= BODY_JMAX && (n_extra == 0 || (xr_ptr && xr_idx && xr_val && extra)),
                "extra regressor: 0..64 joints, with tables and an output");
  P2M_CHECK_ARG(al(pose, 4) && al(pose_mean, 4) && al(betas, 4) && al(trans, 4) && al(v_template, 4) && al(dirs, 4) &&
                al(weights_t, 4) && al(joint_template, 4) && al(joint_shapedirs, 4) && al(parents, 4) && al(joint_slot, 4) &&
                al(tip_vert, 4) && al(tip_slot, 4) && al(xr_ptr, 4) && al(xr_idx, 4) && al(xr_val, 4) && al(verts, 4) &&
                al(joints, 4) && al(extra, 4) && al(workspace, 16), "misaligned buffer (4 bytes; workspace: 16)");
  P2M_CHECK_ARG(workspace_bytes >= p2m_body_workspace(B, J, nb), "workspace smaller than p2m_body_workspace()");
  BodyArgs a;
  a.pose = pose; a.pose_mean = pose_mean; a.betas = betas; a.betas_stride = betas_per_sample ? nb : 0; a.trans = trans;
  a.center = center_joint; a.scale = scale; a.B = B; a.V = V; a.J = J; a.nb = nb; a.K = K;
  a.tmpl = v_template; a.dirs = dirs; a.wt = weights_t; a.jt = joint_template; a.js = joint_shapedirs; a.parents = parents;
  a.jslot = joint_slot; a.NJ = n_joints_out;
  a.ws = (float*)workspace; a.ws_stride = body_ws_floats(J, K);
  a.verts = verts; a.joints = joints;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_body_pose, dim3(B), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_body_skin, dim3(cdiv((long)V * 3, BODY_NT), cdiv(B, BODY_TB)), dim3(BODY_NT), body_skin_lds(J, K), s, a);
  if (n_tips > 0 || n_extra > 0)
    hipLaunchKernelGGL(k_body_tail, dim3(B), dim3(64), 0, s, (const float*)verts, V, joints, n_joints_out, tip_vert, tip_slot,
                       n_tips, xr_ptr, xr_idx, xr_val, n_extra, extra);
  return check_launch("body_forward");
}
