// The demo's camera on the device (include/p2m.h, "The demo's camera"): p2m_pose_prepare - get_bbox, two process_bbox, two
// j2d_processing and the standardisation of demo/run.py:150-159 for a batch - and p2m_camera_fit - OptimzeCamLayer + L1Loss +
// Adam with the reference's rate steps, one wave per person.  The fit is 1500 strictly dependent steps on three scalars: a
// latency chain, so the wave keeps everything in registers (no LDS, no atomics, no global traffic inside the loop) and the
// only cross-lane work per step is three butterfly sums.  The first four butterfly stages are DPP row operations (a few
// cycles each, no LDS crossbar); lanes l ^ 16 and l ^ 32 lie in other rows and go through ds_bpermute (__shfl_xor).
// This file is compiled with -ffp-contract=off (build.py): the header defines every operation as rounded once, unfused.
#include "p2m_common.h"
#include "p2m_philox.h"

#pragma STDC FP_CONTRACT OFF

namespace p2m {

constexpr int FIT_WAVES = 4;       // waves (samples) per block
constexpr uint32_t ST_CAM_START = 10;

// DPP controls: quad_perm [1, 0, 3, 2], quad_perm [2, 3, 0, 1], row_half_mirror (lane i <-> 7 - i of its 8), row_mirror (i <->
// 15 - i of its 16).  After the two quad stages a quad's lanes hold equal values, after the half-mirror stage each 8 lanes do:
// the mirrors then pair the same partial sums as l ^ 4 and l ^ 8, and a + b = b + a bitwise - the header's butterfly exactly.
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// Every lane of the wave must get here (DPP and bpermute read inactive lanes as garbage / zero).
__device__ __forceinline__ float wave_sum(float v) {
  v = v + dpp_move<0xB1>(v);
  v = v + dpp_move<0x4E>(v);
  v = v + dpp_move<0x141>(v);
  v = v + dpp_move<0x140>(v);
  v = v + __shfl_xor(v, 16);
  v = v + __shfl_xor(v, 32);
  return v;
}
__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < __builtin_inff(); }
__device__ __forceinline__ float signf(float v) { return (float)((v > 0.f) - (v < 0.f)); }

// ---- p2m_pose_prepare ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FIT_WAVES * 64) void k_pose_prepare(const float* __restrict__ joints, int B, int J, float in_W,
                                                                 float in_H, float crop, float* __restrict__ pose2d,
                                                                 float* __restrict__ target, float* __restrict__ bbox,
                                                                 int* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * FIT_WAVES + (threadIdx.x >> 6)));
  if (b >= B) return;
  const bool on = lane < J;
  const size_t base = ((size_t)b * J + (on ? lane : 0)) * 2;
  const float x = joints[base], y = joints[base + 1];
  const float inf = __builtin_inff();
  float xmin = on ? x : inf, xmax = on ? x : -inf, ymin = on ? y : inf, ymax = on ? y : -inf;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    xmin = fminf(xmin, __shfl_xor(xmin, o));
    xmax = fmaxf(xmax, __shfl_xor(xmax, o));
    ymin = fminf(ymin, __shfl_xor(ymin, o));
    ymax = fmaxf(ymax, __shfl_xor(ymax, o));
  }
  bool ok = __all(!on || (finitef(x) && finitef(y)));
  const float tw = xmax - xmin, th = ymax - ymin;
  const float w = tw - 1.0f, h = th - 1.0f;
  ok = ok && tw * th > 0.f && w >= 0.f && h >= 0.f;
  const float cx = xmin + w / 2.0f, cy = ymin + h / 2.0f;
  const float aspect = in_W / in_H;
  float w2 = w, h2 = h, w1 = w, h1 = h;
  if (w2 > aspect * h2) h2 = w2 / aspect;
  else if (w2 < aspect * h2) w2 = h2 * aspect;
  if (w1 > h1) h1 = w1;
  else if (w1 < h1) w1 = h1;
  w1 = w1 * 1.25f;
  h1 = h1 * 1.25f;
  ok = ok && w2 > 0.f && w1 > 0.f;
  const float s2 = in_W / w2, s1 = crop / w1;
  const float dx = x - cx, dy = y - cy;
  const float tx = s1 * dx + crop / 2.0f, ty = s1 * dy + crop / 2.0f;
  float px = (s2 * dx + in_W / 2.0f) / in_W, py = (s2 * dy + in_H / 2.0f) / in_H;
  if (!on || !ok) px = py = 0.f;
  const float fj = (float)J;
  const float mx = wave_sum(px) / fj, my = wave_sum(py) / fj;
  const float ex = on ? px - mx : 0.f, ey = on ? py - my : 0.f;
  const float sdx = sqrtf(wave_sum(ex * ex) / fj), sdy = sqrtf(wave_sum(ey * ey) / fj);
  ok = ok && sdx > 0.f && sdy > 0.f && sdx < inf && sdy < inf;
  if (on) {
    pose2d[base] = ok ? ex / sdx : 0.f;
    pose2d[base + 1] = ok ? ey / sdy : 0.f;
    target[base] = ok ? tx : 0.f;
    target[base + 1] = ok ? ty : 0.f;
  }
  if (lane == 0) {
    bbox[(size_t)b * 4] = ok ? cx - w1 / 2.0f : 0.f;
    bbox[(size_t)b * 4 + 1] = ok ? cy - h1 / 2.0f : 0.f;
    bbox[(size_t)b * 4 + 2] = ok ? w1 : 0.f;
    bbox[(size_t)b * 4 + 3] = ok ? h1 : 0.f;
    status[b] = ok ? 0 : 1;
  }
}

// ---- p2m_camera_fit -----------------------------------------------------------------------------------------------------
struct FitArgs {
  const float* joints3d;
  const float* target;
  const float* weight;
  const float* cam0;
  const uint64_t* state;
  int B, J, steps;
  float r;
  double beta1, beta2;
  float om1, b2f, om2, epsf;     // (float)(1 - beta1), (float)beta2, (float)(1 - beta2), (float)eps
  p2m_fit_schedule sched;
  float* cam;
  float* loss;
  int* status;
};

__global__ __launch_bounds__(FIT_WAVES * 64) void k_camera_fit(const FitArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * FIT_WAVES + (threadIdx.x >> 6)));
  if (b >= a.B) return;
  const int J = a.J;
  const bool on = lane < J;
  const size_t jb = (size_t)b * J + (on ? lane : 0);
  const float r = a.r;
  const float x = on ? a.joints3d[jb * 3] : 0.f, y = on ? a.joints3d[jb * 3 + 1] : 0.f;
  const float t_x = on ? a.target[jb * 2] : r, t_y = on ? a.target[jb * 2 + 1] : r;
  const float w = on ? (a.weight ? a.weight[jb] : 1.0f) : 0.f;
  float s, tx, ty;
  if (a.cam0) {
    s = a.cam0[(size_t)b * 3];
    tx = a.cam0[(size_t)b * 3 + 1];
    ty = a.cam0[(size_t)b * 3 + 2];
  } else {
    const Philox4 d = philox_draw(a.state[0], a.state[1] + (uint64_t)b, 0, ST_CAM_START, 0);
    s = philox_uniform(d.w[0]);
    tx = philox_uniform(d.w[1]);
    ty = philox_uniform(d.w[2]);
  }
  const float W = wave_sum(w);
  const bool ok = __all(finitef(x) && finitef(y) && finitef(t_x) && finitef(t_y) && finitef(w)) && finitef(s) && finitef(tx) &&
                  finitef(ty) && W > 0.f;
  if (!ok) {                       // wave-uniform: the whole wave leaves
    if (lane == 0) {
      a.cam[(size_t)b * 3] = a.cam[(size_t)b * 3 + 1] = a.cam[(size_t)b * 3 + 2] = 0.f;
      a.loss[b] = 0.f;
      a.status[b] = 1;
    }
    return;
  }
  const float c = (w / (2.0f * W)) * r;
  float m0 = 0.f, m1 = 0.f, m2 = 0.f, v0 = 0.f, v1 = 0.f, v2 = 0.f;
  double p1 = 1.0, p2 = 1.0;
  int k = 0;
  double lr = a.sched.lr[0];
  for (int i = 0; i < a.steps; ++i) {
    if (k + 1 < a.sched.n && a.sched.first_step[k + 1] <= i) lr = a.sched.lr[++k];
    p1 *= a.beta1;
    p2 *= a.beta2;
    const float step_size = (float)(lr / (1.0 - p1));
    const float c2 = (float)sqrt(1.0 - p2);
    const float qx = x + tx, qy = y + ty;
    const float ex = ((qx * s) * r + r) - t_x, ey = ((qy * s) * r + r) - t_y;
    const float gx = signf(ex) * c, gy = signf(ey) * c;
    const float g0 = wave_sum(gx * qx + gy * qy), g1 = wave_sum(gx * s), g2 = wave_sum(gy * s);
    m0 = m0 + (g0 - m0) * a.om1;
    m1 = m1 + (g1 - m1) * a.om1;
    m2 = m2 + (g2 - m2) * a.om1;
    v0 = v0 * a.b2f + (a.om2 * g0) * g0;
    v1 = v1 * a.b2f + (a.om2 * g1) * g1;
    v2 = v2 * a.b2f + (a.om2 * g2) * g2;
    s = s - (step_size * m0) / (sqrtf(v0) / c2 + a.epsf);
    tx = tx - (step_size * m1) / (sqrtf(v1) / c2 + a.epsf);
    ty = ty - (step_size * m2) / (sqrtf(v2) / c2 + a.epsf);
  }
  const float qx = x + tx, qy = y + ty;
  const float ex = ((qx * s) * r + r) - t_x, ey = ((qy * s) * r + r) - t_y;
  const float L = wave_sum(w * (fabsf(ex) + fabsf(ey))) / (2.0f * W);
  if (lane == 0) {
    a.cam[(size_t)b * 3] = s;
    a.cam[(size_t)b * 3 + 1] = tx;
    a.cam[(size_t)b * 3 + 2] = ty;
    a.loss[b] = L;
    a.status[b] = s <= 0.f ? 2 : 0;
  }
}

}  // namespace p2m

using namespace p2m;

extern "C" int p2m_pose_prepare(const float* joints, int32_t B, int32_t J, float in_W, float in_H, float crop, float* pose2d,
                                float* target, float* bbox, int32_t* status, void* stream) {
  P2M_CHECK_ARG(joints && pose2d && target && bbox && status, "null pointer");
  P2M_CHECK_ARG(B >= 1 && B <= (1 << 24), "B outside [1, 2^24]");
  P2M_CHECK_ARG(J >= 1 && J <= 64, "J outside [1, 64]");
  P2M_CHECK_ARG(in_W > 0.f && in_H > 0.f && crop > 0.f && in_W < 1e6f && in_H < 1e6f && crop < 1e6f,
                "in_W, in_H, crop outside (0, 1e6)");
  hipLaunchKernelGGL(k_pose_prepare, dim3(cdiv(B, FIT_WAVES)), dim3(FIT_WAVES * 64), 0, (hipStream_t)stream, joints, B, J, in_W,
                     in_H, crop, pose2d, target, bbox, status);
  return check_launch("p2m_pose_prepare");
}

extern "C" int p2m_camera_fit(const float* joints3d, const float* target, const float* weight, const float* cam0,
                              const uint64_t* state, int32_t B, int32_t J, p2m_fit_schedule sched, int32_t steps, float img_res,
                              double beta1, double beta2, double eps, float* cam, float* loss, int32_t* status, void* stream) {
  P2M_CHECK_ARG(joints3d && target && cam && loss && status, "null pointer");
  P2M_CHECK_ARG(cam0 || state, "cam0 and state are both NULL: give a start or the stream to draw it from");
  P2M_CHECK_ARG((uintptr_t)state % 8 == 0, "misaligned state");
  P2M_CHECK_ARG(B >= 1 && B <= (1 << 24), "B outside [1, 2^24]");
  P2M_CHECK_ARG(J >= 1 && J <= 64, "J outside [1, 64]");
  P2M_CHECK_ARG(steps >= 0 && steps <= 65535, "steps outside [0, 65535]");
  P2M_CHECK_ARG(sched.n >= 1 && sched.n <= 8, "schedule: 1 to 8 (first_step, lr) pairs");
  P2M_CHECK_ARG(sched.first_step[0] == 0, "schedule: the first entry must start at step 0");
  for (int k = 0; k < sched.n; ++k) {
    P2M_CHECK_ARG(k == 0 || sched.first_step[k] > sched.first_step[k - 1], "schedule: first_step must ascend strictly");
    P2M_CHECK_ARG(sched.lr[k] - sched.lr[k] == 0.0, "schedule: lr is not finite");
  }
  P2M_CHECK_ARG(img_res > 0.f && img_res < __builtin_inff(), "img_res must be positive and finite");
  P2M_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && eps < 1e30, "betas / eps");
  FitArgs a;
  a.joints3d = joints3d;
  a.target = target;
  a.weight = weight;
  a.cam0 = cam0;
  a.state = state;
  a.B = B;
  a.J = J;
  a.steps = steps;
  a.r = img_res;
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.om1 = (float)(1.0 - beta1);
  a.b2f = (float)beta2;
  a.om2 = (float)(1.0 - beta2);
  a.epsf = (float)eps;
  a.sched = sched;
  a.cam = cam;
  a.loss = loss;
  a.status = status;
  hipLaunchKernelGGL(k_camera_fit, dim3(cdiv(B, FIT_WAVES)), dim3(FIT_WAVES * 64), 0, (hipStream_t)stream, a);
  return check_launch("p2m_camera_fit");
}
