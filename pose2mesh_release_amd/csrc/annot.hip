// Dataset annotations to camera-frame body parameters on the GPU (gfx950), and the per-sample choice between the meshes of a
// gender bank: the device counterpart of get_smpl_coord / get_mano_coord in the reference's datasets (data/Human36M/
// dataset.py:253-299, data/AMASS/dataset.py:182-213, data/FreiHAND/dataset.py:110-134 and the simpler variants), which run
// per sample in numpy and transforms3d on a dataloader worker.  The comments of p2m_annot_gather and p2m_body_select in
// include/p2m.h are the contract; tests/annot_ref.py restates them in float64 numpy.
//
// One kernel per entry on the caller's stream; no allocation, no memset, no sync, no atomics:
//   k_annot_gather  one wave per sample b, row r = idx[b].  The glue (exp of the root, R . exp, the quaternion logarithm, the
//                   folded root joint, the translation) is a few hundred float64 operations on values that are uniform over
//                   the wave, so every lane computes them and lane 0 stores; the beta reset is one ballot with lane k on
//                   beta k; the row copies (3 J + nb + 5 Jr + 4 words) are spread over the 64 lanes.  An index outside [0, N)
//                   is decided before any table address is formed from it.
//   k_body_select   a streaming copy over the flat output buffers of verts, joints and extra, one 16-byte store per lane.  A
//                   vector may straddle two samples (3 V floats is not a multiple of 4 for odd V): the source pointer is
//                   chosen per element from the element's own sample, and a 16-byte load is taken only when the four
//                   elements share a source whose address is 16-byte aligned.  The elements before the first and after the
//                   last aligned vector of a buffer (3 each at most) go one by one.
#include "p2m_common.h"

namespace p2m {

constexpr int A_MAX_J = 64, A_MAX_NB = 64, A_MAX_G = 4, A_MAX_JR = 32;
constexpr int A_WAVES = 4;            // samples per block of k_annot_gather
constexpr int S_NT = 256;

struct AnnotArgs {
  const float *pose, *betas, *trans, *cam_R, *cam_t, *focal, *princpt, *given_cam, *given_img, *root_tmpl, *root_dirs;
  const unsigned char* gender;
  const void* idx;
  long long N;
  int idx64, B, J, nb, Jr, G, rotate_root, beta_reset, compensate_root;
  double beta_limit, t_scale;
  float *pose_out, *betas_out, *trans_out, *focal_out, *princpt_out, *given_cam_out, *given_img_out;
  int *gender_out, *status;
};

// exp of an axis-angle vector by the exact Rodrigues formula, as transforms3d's axangle2mat(v / |v|, |v|); |v| = 0: identity
__device__ __forceinline__ void annot_exp(const double v[3], double E[9]) {
  const double angle = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (!(angle > 0.0)) {
    E[0] = E[4] = E[8] = 1.0;
    E[1] = E[2] = E[3] = E[5] = E[6] = E[7] = 0.0;
    return;
  }
  const double x = v[0] / angle, y = v[1] / angle, z = v[2] / angle;
  const double c = cos(angle), s = sin(angle), C = 1.0 - c;
  const double xs = x * s, ys = y * s, zs = z * s, xC = x * C, yC = y * C, zC = z * C;
  const double xyC = x * yC, yzC = y * zC, zxC = z * xC;
  E[0] = x * xC + c, E[1] = xyC - zs, E[2] = zxC + ys;
  E[3] = xyC + zs, E[4] = y * yC + c, E[5] = yzC - xs;
  E[6] = zxC - ys, E[7] = yzC + xs, E[8] = z * zC + c;
}

// principal logarithm of a (near-)rotation matrix through its quaternion: Shepperd's choice of the largest of the trace and
// the three diagonal entries, w >= 0, rotvec = 2 atan2(|v|, w) v / |v| (zero when |v| = 0)
__device__ __forceinline__ void annot_log(const double M[9], double out[3]) {
  const double tr = M[0] + M[4] + M[8];
  double w, x, y, z;
  if (tr >= M[0] && tr >= M[4] && tr >= M[8]) {
    const double s = 2.0 * sqrt(1.0 + tr);
    w = 0.25 * s, x = (M[7] - M[5]) / s, y = (M[2] - M[6]) / s, z = (M[3] - M[1]) / s;
  } else if (M[0] >= M[4] && M[0] >= M[8]) {
    const double s = 2.0 * sqrt(1.0 + M[0] - M[4] - M[8]);
    w = (M[7] - M[5]) / s, x = 0.25 * s, y = (M[1] + M[3]) / s, z = (M[2] + M[6]) / s;
  } else if (M[4] >= M[8]) {
    const double s = 2.0 * sqrt(1.0 + M[4] - M[0] - M[8]);
    w = (M[2] - M[6]) / s, x = (M[1] + M[3]) / s, y = 0.25 * s, z = (M[5] + M[7]) / s;
  } else {
    const double s = 2.0 * sqrt(1.0 + M[8] - M[0] - M[4]);
    w = (M[3] - M[1]) / s, x = (M[2] + M[6]) / s, y = (M[5] + M[7]) / s, z = 0.25 * s;
  }
  if (w < 0.0) w = -w, x = -x, y = -y, z = -z;
  const double n = sqrt(x * x + y * y + z * z);
  if (!(n > 0.0)) {
    out[0] = out[1] = out[2] = 0.0;
    return;
  }
  const double k = 2.0 * atan2(n, w) / n;
  out[0] = k * x, out[1] = k * y, out[2] = k * z;
}

__device__ __forceinline__ bool annot_finite(double v) { return fabs(v) < __builtin_inf(); }

__global__ __launch_bounds__(A_WAVES * 64) void k_annot_gather(const AnnotArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * A_WAVES + (threadIdx.x >> 6)));
  if (b >= a.B) return;
  const int nP = 3 * a.J, nb = a.nb, nC = a.given_cam ? a.Jr * 3 : 0, nI = a.given_img ? a.Jr * 2 : 0;
  float* po = a.pose_out + (size_t)b * nP;
  float* bo = a.betas_out + (size_t)b * nb;             // never dereferenced when nb = 0
  float* co = a.given_cam_out + (size_t)b * nC;
  float* io = a.given_img_out + (size_t)b * nI;
  const long long r = a.idx64 ? ((const long long*)a.idx)[b] : (long long)((const int*)a.idx)[b];
  if (r < 0 || r >= a.N) {                              // status bit 0: all zero, and no table is read at this index
    for (int i = lane; i < nP; i += 64) po[i] = 0.f;
    if (lane < nb) bo[lane] = 0.f;
    for (int i = lane; i < nC; i += 64) co[i] = 0.f;
    for (int i = lane; i < nI; i += 64) io[i] = 0.f;
    if (lane < 3) a.trans_out[(size_t)b * 3 + lane] = 0.f;
    if (lane < 2) a.focal_out[(size_t)b * 2 + lane] = 0.f, a.princpt_out[(size_t)b * 2 + lane] = 0.f;
    if (lane == 0) a.gender_out[b] = 0, a.status[b] = 1;
    return;
  }
  const size_t row = (size_t)r;
  int st = 0;
  int g = a.gender ? (int)a.gender[row] : 0;
  if (g >= a.G) g = 0, st |= 2;
  // betas: lane k holds beta k (nb <= 64); the reset is decided by one ballot.  A NaN compares false and is kept.
  float beta = 0.f;
  if (lane < nb) beta = a.betas[row * nb + lane];
  if (a.beta_reset && __ballot(lane < nb && fabs((double)beta) > a.beta_limit) != 0ull) beta = 0.f, st |= 4;
  if (lane < nb) bo[lane] = beta;
  // the glue, uniform over the wave, in float64
  const float* prow = a.pose + row * nP;
  double root[3] = {(double)prow[0], (double)prow[1], (double)prow[2]};
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  bool finite = annot_finite(root[0]) && annot_finite(root[1]) && annot_finite(root[2]);
  if (a.cam_R)
    for (int i = 0; i < 9; ++i) {
      R[i] = (double)a.cam_R[row * 9 + i];
      finite = finite && annot_finite(R[i]);
    }
  if (!finite) st |= 8;
  float new_root[3] = {prow[0], prow[1], prow[2]};
  if (a.rotate_root && finite) {
    double E[9], M[9], lg[3];
    annot_exp(root, E);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) M[i * 3 + j] = R[i * 3] * E[j] + R[i * 3 + 1] * E[3 + j] + R[i * 3 + 2] * E[6 + j];
    annot_log(M, lg);
    for (int c = 0; c < 3; ++c) new_root[c] = (float)lg[c];
  }
  double tw[3] = {0.0, 0.0, 0.0}, tc[3] = {0.0, 0.0, 0.0}, T[3];
  if (a.trans)
    for (int c = 0; c < 3; ++c) tw[c] = (double)a.trans[row * 3 + c];
  if (a.cam_t)
    for (int c = 0; c < 3; ++c) tc[c] = (double)a.cam_t[row * 3 + c];
  for (int c = 0; c < 3; ++c) T[c] = R[c * 3] * tw[0] + R[c * 3 + 1] * tw[1] + R[c * 3 + 2] * tw[2] + a.t_scale * tc[c];
  if (a.compensate_root) {                              // + R J0 - J0 with the folded rest root of model g at betas_out
    double J0[3];
    for (int c = 0; c < 3; ++c) J0[c] = (double)a.root_tmpl[g * 3 + c];
    for (int k = 0; k < nb; ++k) {
      const double bk = (double)__shfl(beta, k);
      for (int c = 0; c < 3; ++c) J0[c] += (double)a.root_dirs[((size_t)g * 3 + c) * nb + k] * bk;
    }
    for (int c = 0; c < 3; ++c) T[c] += R[c * 3] * J0[0] + R[c * 3 + 1] * J0[1] + R[c * 3 + 2] * J0[2] - J0[c];
  }
  if (lane == 0) {
    for (int c = 0; c < 3; ++c) a.trans_out[(size_t)b * 3 + c] = (float)T[c];
    a.gender_out[b] = g;
    a.status[b] = st;
  }
  // the row copies
  for (int i = lane; i < nP; i += 64) {
    float v = prow[i];
    if (i < 3) v = i == 0 ? new_root[0] : i == 1 ? new_root[1] : new_root[2];
    po[i] = v;
  }
  for (int i = lane; i < nC; i += 64) co[i] = a.given_cam[row * nC + i];
  for (int i = lane; i < nI; i += 64) io[i] = a.given_img[row * nI + i];
  if (lane < 2) {
    a.focal_out[(size_t)b * 2 + lane] = a.focal[row * 2 + lane];
    a.princpt_out[(size_t)b * 2 + lane] = a.princpt[row * 2 + lane];
  }
}

struct SelectSeg {
  const float* src[A_MAX_G];
  float* out;
  unsigned n, per, head, nvec;        // floats in all and per sample; scalar floats before the first vector; 16-byte vectors
  unsigned first_block;
};
struct SelectArgs {
  SelectSeg seg[3];
  const int* gender;
  int nseg, G;
};

__device__ __forceinline__ const float* select_src(const SelectSeg& s, const int* gender, int G, unsigned i) {
  const int g = gender[i / s.per];
  return s.src[(unsigned)g < (unsigned)G ? g : 0];
}

// unit u < nvec of a segment: the aligned vector out[head + 4 u ..]; unit nvec: the head and tail floats one by one
__global__ __launch_bounds__(S_NT) void k_body_select(const SelectArgs a) {
  int k = 0;
  if (a.nseg > 1 && blockIdx.x >= a.seg[1].first_block) k = 1;
  if (a.nseg > 2 && blockIdx.x >= a.seg[2].first_block) k = 2;
  const SelectSeg& s = a.seg[k];
  const unsigned u = (blockIdx.x - s.first_block) * S_NT + threadIdx.x;
  if (u < s.nvec) {
    const unsigned i = s.head + 4u * u;
    const float* p0 = select_src(s, a.gender, a.G, i);
    const float* p3 = select_src(s, a.gender, a.G, i + 3);
    float4 v;
    if (p0 == p3 && (((uintptr_t)(p0 + i)) & 15) == 0) {
      v = *reinterpret_cast<const float4*>(p0 + i);
    } else {
      v.x = p0[i];
      v.y = select_src(s, a.gender, a.G, i + 1)[i + 1];
      v.z = select_src(s, a.gender, a.G, i + 2)[i + 2];
      v.w = p3[i + 3];
    }
    *reinterpret_cast<float4*>(s.out + i) = v;
  } else if (u == s.nvec) {
    for (unsigned i = 0; i < s.head; ++i) s.out[i] = select_src(s, a.gender, a.G, i)[i];
    for (unsigned i = s.head + 4u * s.nvec; i < s.n; ++i) s.out[i] = select_src(s, a.gender, a.G, i)[i];
  }
}

}  // namespace p2m

using namespace p2m;

extern "C" int p2m_annot_gather(const float* pose, const float* betas, const float* trans, const float* cam_R,
                                const float* cam_t, const float* focal, const float* princpt, const uint8_t* gender,
                                const float* given_cam, const float* given_img, int64_t N, int32_t J, int32_t nb, int32_t Jr,
                                const void* idx, int32_t idx_is_int64, int32_t B, const float* root_template,
                                const float* root_shapedirs, int32_t G, int32_t rotate_root, int32_t beta_reset,
                                int32_t compensate_root, double beta_limit, double t_scale, float* pose_out, float* betas_out,
                                float* trans_out, float* focal_out, float* princpt_out, int32_t* gender_out,
                                float* given_cam_out, float* given_img_out, int32_t* status, void* stream) {
  P2M_CHECK_ARG(B >= 1 && B <= (1 << 24), "B outside [1, 2^24]");
  P2M_CHECK_ARG(N >= 1, "N < 1");
  P2M_CHECK_ARG(J >= 1 && J <= A_MAX_J, "J outside [1, 64]");
  P2M_CHECK_ARG(nb >= 0 && nb <= A_MAX_NB, "nb outside [0, 64]");
  P2M_CHECK_ARG(G >= 1 && G <= A_MAX_G, "G outside [1, 4]");
  P2M_CHECK_ARG(Jr >= 0 && Jr <= A_MAX_JR, "Jr outside [0, 32]");
  P2M_CHECK_ARG(pose && focal && princpt && idx && (nb == 0 || betas), "null input pointer");
  P2M_CHECK_ARG(pose_out && trans_out && focal_out && princpt_out && gender_out && status && (nb == 0 || betas_out),
                "null output pointer");
  const bool gc = given_cam && Jr > 0, gi = given_img && Jr > 0;
  P2M_CHECK_ARG((!gc || given_cam_out) && (!gi || given_img_out), "given joints without their output");
  P2M_CHECK_ARG(!compensate_root || (root_template && (nb == 0 || root_shapedirs)), "compensate_root without the root tables");
  P2M_CHECK_ARG(beta_limit == beta_limit && t_scale == t_scale, "beta_limit or t_scale is NaN");
  const void* f4[] = {pose, betas, trans, cam_R, cam_t, focal, princpt, given_cam, given_img, root_template, root_shapedirs,
                      pose_out, betas_out, trans_out, focal_out, princpt_out, gender_out, given_cam_out, given_img_out, status};
  for (const void* p : f4) P2M_CHECK_ARG((uintptr_t)p % 4 == 0, "misaligned buffer");
  P2M_CHECK_ARG((uintptr_t)idx % (idx_is_int64 ? 8 : 4) == 0, "misaligned idx");
  AnnotArgs a{};
  a.pose = pose, a.betas = betas, a.trans = trans, a.cam_R = cam_R, a.cam_t = cam_t, a.focal = focal, a.princpt = princpt;
  a.given_cam = gc ? given_cam : nullptr, a.given_img = gi ? given_img : nullptr;
  a.root_tmpl = root_template, a.root_dirs = root_shapedirs, a.gender = gender, a.idx = idx, a.N = N;
  a.idx64 = idx_is_int64 != 0, a.B = B, a.J = J, a.nb = nb, a.Jr = Jr, a.G = G;
  a.rotate_root = rotate_root != 0, a.beta_reset = beta_reset != 0, a.compensate_root = compensate_root != 0;
  a.beta_limit = beta_limit, a.t_scale = t_scale;
  a.pose_out = pose_out, a.betas_out = betas_out, a.trans_out = trans_out, a.focal_out = focal_out;
  a.princpt_out = princpt_out, a.given_cam_out = given_cam_out, a.given_img_out = given_img_out;
  a.gender_out = gender_out, a.status = status;
  hipLaunchKernelGGL(k_annot_gather, dim3(cdiv(B, A_WAVES)), dim3(A_WAVES * 64), 0, (hipStream_t)stream, a);
  return check_launch("annot_gather");
}

extern "C" int p2m_body_select(const float* const* verts_src, const float* const* joints_src, const float* const* extra_src,
                               int32_t G, const int32_t* gender, int32_t B, int32_t V, int32_t NJ, int32_t JX, float* verts,
                               float* joints, float* extra, void* stream) {
  P2M_CHECK_ARG(G >= 1 && G <= A_MAX_G, "G outside [1, 4]");
  P2M_CHECK_ARG(B >= 1 && V >= 1 && NJ >= 1 && JX >= 0, "B, V or NJ < 1, or JX < 0");
  P2M_CHECK_ARG((long)B * 3 * V < (1L << 31) && (long)B * 3 * NJ < (1L << 31) && (long)B * 3 * JX < (1L << 31),
                "an output of 2^31 floats or more");
  P2M_CHECK_ARG(verts_src && joints_src && gender && verts && joints && (JX == 0 || (extra_src && extra)), "null pointer");
  P2M_CHECK_ARG((uintptr_t)gender % 4 == 0, "misaligned gender");
  const float* const* srcs[3] = {verts_src, joints_src, extra_src};
  float* outs[3] = {verts, joints, extra};
  const int per[3] = {3 * V, 3 * NJ, 3 * JX};
  SelectArgs a{};
  a.gender = gender, a.G = G;
  unsigned blocks = 0;
  for (int k = 0; k < 3; ++k) {
    if (per[k] == 0) continue;
    SelectSeg& s = a.seg[a.nseg++];
    s.out = outs[k], s.per = (unsigned)per[k], s.n = (unsigned)B * (unsigned)per[k];
    P2M_CHECK_ARG((uintptr_t)s.out % 4 == 0, "misaligned output");
    const uintptr_t ob = (uintptr_t)s.out, oe = ob + (uintptr_t)s.n * 4;
    for (int g = 0; g < A_MAX_G; ++g) {
      s.src[g] = srcs[k][g < G ? g : 0];
      P2M_CHECK_ARG(s.src[g] && (uintptr_t)s.src[g] % 4 == 0, "null or misaligned source");
      const uintptr_t sb = (uintptr_t)s.src[g];
      P2M_CHECK_ARG(oe <= sb || sb + (uintptr_t)s.n * 4 <= ob, "an output overlaps a source");
    }
    const unsigned head = (unsigned)(((16 - (ob & 15)) & 15) >> 2);
    s.head = head < s.n ? head : s.n;
    s.nvec = (s.n - s.head) >> 2;
    s.first_block = blocks;
    blocks += (unsigned)cdiv((long)s.nvec + 1, S_NT);
  }
  hipLaunchKernelGGL(k_body_select, dim3(blocks), dim3(S_NT), 0, (hipStream_t)stream, a);
  return check_launch("body_select");
}
