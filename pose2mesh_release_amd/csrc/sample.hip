// Training-sample noise on the GPU (include/p2m.h, "training-sample noise"): the synthetic 2D detector errors every released
// recipe of the reference puts in place of the clean input joints (use_gt_input: False) -
//   p2m_pose_noise_coco    synthesize_pose(joints, area, num_overlap = 0), lib/noise_utils.py:17-285, for the COCO joint set
//   p2m_pose_noise_table   generate_syn_error and its use, data/AMASS/dataset.py:77-89, 327-329
// on the one counter-based stream of csrc/p2m_philox.h.  tests/sample_ref.py is the float64 restatement: stage numbering,
// draw order and operation sequence below are mirrored there line by line; change both or neither.
#include "p2m_common.h"
#include "p2m_philox.h"

namespace p2m {

// stages: counter word 2 = joint | stage << 8
enum { ST_JITTER = 0, ST_MISS_COUNT0 = 1, ST_MISS_COUNT1 = 2, ST_MISS_PICK0 = 3, ST_MISS_PICK1 = 4, ST_INV = 5, ST_GOOD = 6,
       ST_SELECT = 7, ST_TABLE = 8, ST_AUG = 9 };
constexpr int N_JITTER = 500, N_MISS = 2000, N_INV = 500, N_GOOD = 125;
constexpr int NOISE_WAVES = 4;                 // (sample, unit) pairs per block, one wave each
constexpr int COCO_J = 17, COCO_UNITS = 9;     // the nose, and eight left / right pairs of two sequential steps
// sqrt(-2 ln ks) for ks = 0.10, 0.50, 0.85 (get_dist_wrt_ks, noise_utils.py:18-24: sqrt(-2 area (2 sigma)^2 ln ks))
constexpr float C10 = 2.1459660262893472f, C50 = 1.1774100225154747f, C85 = 0.5701209161182826f;
constexpr float FAR = 1.0f + 0x1p-10f;

struct Source {       // one candidate source and the other one, if any (wave-uniform)
  float cx, cy, ox, oy;
  bool has;
};
struct Pick {
  bool found;
  float x, y;
};

// One candidate: angle / radius uniforms -> point (x, y) around (cx, cy); passes when its squared distance to the other
// source exceeds thr2 (>= 0), or r^2 when thr2 < 0.  Every operation is one fp32 rounding; the band of sample_ref.py is
// derived from exactly this sequence.
__device__ __forceinline__ bool candidate(uint32_t wa, uint32_t wr, float lo, float hi, const Source& s, float thr2, float& x,
                                          float& y) {
  const float ua = philox_uniform(wa), ur = philox_uniform(wr);
  const float r = fmaf(hi - lo, ur, lo);
  float sn, cs;
  sincospif(2.0f * ua, &sn, &cs);
  x = fmaf(r, cs, s.cx);
  y = fmaf(r, sn, s.cy);
  const float dx = s.ox - x, dy = s.oy - y;
  const float d2 = fmaf(dx, dx, dy * dy);
  return d2 > (thr2 < 0.f ? r * r : thr2);
}

// First passing candidate of a stage: 128 candidates per step across the wave (lane l draws block c0 / 2 + l, which holds
// candidates c0 + 2 l and c0 + 2 l + 1), the lowest index picked from the two ballots.  Without a second source nothing is
// compared and candidate 0 is the result.
__device__ __forceinline__ Pick first_pass(uint64_t seed, uint64_t index, int j, int stage, int N, float lo, float hi,
                                           const Source& s, float thr2, int lane) {
  Pick p{false, 0.f, 0.f};
  if (!s.has) {
    const Philox4 d = philox_draw(seed, index, j, stage, 0);
    candidate(d.w[0], d.w[1], lo, hi, s, thr2, p.x, p.y);
    p.found = true;
    return p;
  }
  for (int c0 = 0; c0 < N; c0 += 128) {
    const Philox4 d = philox_draw(seed, index, j, stage, (c0 >> 1) + lane);
    float xa, ya, xb, yb;
    const bool oka = candidate(d.w[0], d.w[1], lo, hi, s, thr2, xa, ya) && c0 + 2 * lane < N;
    const bool okb = candidate(d.w[2], d.w[3], lo, hi, s, thr2, xb, yb) && c0 + 2 * lane + 1 < N;
    const unsigned long long ma = __ballot(oka), mb = __ballot(okb);
    if (ma | mb) {
      const int l = __ffsll((long long)(ma | mb)) - 1;
      const bool a = (ma >> l) & 1ull;
      p.x = __shfl(a ? xa : xb, l);
      p.y = __shfl(a ? ya : yb, l);
      p.found = true;
      return p;
    }
  }
  return p;
}

// Passing candidates among the N_MISS of a counting stage (only called with a second source).
__device__ __forceinline__ int count_pass(uint64_t seed, uint64_t index, int j, int stage, float lo, float hi, const Source& s,
                                          float thr2, int lane) {
  int n = 0;
  for (int c0 = 0; c0 < N_MISS; c0 += 128) {
    const Philox4 d = philox_draw(seed, index, j, stage, (c0 >> 1) + lane);
    float x, y;
    const bool oka = candidate(d.w[0], d.w[1], lo, hi, s, thr2, x, y) && c0 + 2 * lane < N_MISS;
    const bool okb = candidate(d.w[2], d.w[3], lo, hi, s, thr2, x, y) && c0 + 2 * lane + 1 < N_MISS;
    n += __popcll(__ballot(oka)) + __popcll(__ballot(okb));
  }
  return n;
}

// [jitter, miss, inversion] by joint and by the number of valid joints (noise_utils.py:70-83, 105-125, 161-166); swap is 0
// (:231) and good the remainder
__device__ __forceinline__ void probabilities(int j, int num_valid, float& pj, float& pm, float& pi) {
  const bool leg = j == 0 || (j >= 13 && j <= 16), up = j >= 1 && j <= 10;
  if (num_valid <= 10) pj = leg ? 0.15f : up ? 0.20f : 0.25f;
  else pj = leg ? 0.10f : up ? 0.15f : 0.20f;
  const bool face = j <= 4, sa = j == 5 || j == 6 || j == 15 || j == 16;
  if (num_valid <= 5) pm = face ? 0.15f : sa ? 0.20f : 0.25f;
  else if (num_valid <= 10) pm = face ? 0.10f : sa ? 0.13f : 0.15f;
  else pm = face ? 0.02f : sa ? 0.05f : 0.10f;
  pi = j <= 4 ? 0.01f : j <= 10 ? 0.03f : 0.06f;
}

// One joint: own source (x, y), the partner's current coordinates (ox, oy) when `has`.  Returns the kind; x, y updated
// (0, 0 when the joint is zeroed).  Wave-uniform in, wave-uniform out.
__device__ __forceinline__ int noise_joint(uint64_t seed, uint64_t index, int j, int num_valid, float root, float sigma,
                                           float& x, float& y, float ox, float oy, bool has, int lane) {
  const float base = root * (2.0f * sigma);
  const float ks10 = base * C10, ks50 = base * C50, ks85 = base * C85;
  const float thr50 = ks50 * ks50;
  const Source own{x, y, has ? ox : x, has ? oy : y, has};
  const Source oth{own.ox, own.oy, x, y, has};
  const Pick jit = first_pass(seed, index, j, ST_JITTER, N_JITTER, ks85, ks50, own, -1.f, lane);
  const Pick good = first_pass(seed, index, j, ST_GOOD, N_GOOD, 0.f, ks85, own, -1.f, lane);
  Pick inv{false, 0.f, 0.f};
  if (has) inv = first_pass(seed, index, j, ST_INV, N_INV, 0.f, ks50, oth, -1.f, lane);
  // miss: the pool of noise_utils.py:143-151 is n0 points of source 0 and n1 / 4 of source 1; the point itself is the first
  // passing candidate of a separate stage of the chosen source
  int n0 = N_MISS, n1 = 0;
  if (has) {
    const float ddx = x - ox, ddy = y - oy;
    if (sqrtf(fmaf(ddx, ddx, ddy * ddy)) > (ks10 + ks50) * FAR) {
      n1 = N_MISS;                                   // too far apart to fail: every candidate of both sources passes
    } else {
      n0 = count_pass(seed, index, j, ST_MISS_COUNT0, ks50, ks10, own, thr50, lane);
      n1 = count_pass(seed, index, j, ST_MISS_COUNT1, ks50, ks10, oth, thr50, lane);
    }
  }
  const Philox4 sel = philox_draw(seed, index, j, ST_SELECT, 0);
  const uint64_t pool = (uint64_t)n0 + (uint64_t)(n1 / 4);
  Pick miss{false, 0.f, 0.f};
  if (pool > 0) {
    const bool src0 = (uint64_t)(sel.w[0] >> 8) * pool < ((uint64_t)n0 << 24);
    miss = src0 ? first_pass(seed, index, j, ST_MISS_PICK0, N_MISS, ks50, ks10, own, thr50, lane)
                : first_pass(seed, index, j, ST_MISS_PICK1, N_MISS, ks50, ks10, oth, thr50, lane);
  }
  // category: availability zeroing and renormalisation (:256-276), then one uniform against the cumulative weights
  float pj, pm, pi;
  probabilities(j, num_valid, pj, pm, pi);
  const float pg = 1.0f - ((pj + pm) + pi);
  const float w0 = jit.found ? pj : 0.f, w1 = miss.found ? pm : 0.f, w2 = inv.found ? pi : 0.f, w3 = good.found ? pg : 0.f;
  const float c1 = w0, c2 = c1 + w1, c3 = c2 + w2, norm = c3 + w3;
  if (!(jit.found || miss.found || inv.found || good.found)) {
    x = 0.f;
    y = 0.f;
    return -1;
  }
  const float t = philox_uniform(sel.w[1]) * norm;
  int pick = t < c1 ? 0 : t < c2 ? 1 : t < c3 ? 2 : 3;
  const bool avail[4] = {jit.found, miss.found, inv.found, good.found};
  if (!avail[pick]) pick = good.found ? 3 : inv.found ? 2 : miss.found ? 1 : 0;        // the last available type
  const Pick& p = pick == 0 ? jit : pick == 1 ? miss : pick == 2 ? inv : good;
  x = p.x;
  y = p.y;
  return pick == 3 ? 4 : pick;
}

// One wave per (sample, unit): unit 0 the nose, unit p the joints 2 p - 1 and 2 p in that order - the higher joint sees the
// already synthesised lower one ((0, 0) if that was zeroed), as noise_utils.py:31-36 does by updating synth_joints in place.
// Layout: joint j of sample b at joints[b * sb + j * sj] (x, y and, when sj == 3, the validity flag); area[b * sa].  The
// chain (p2m_train_sample) runs it IN PLACE on pose2d [B, J, 2] (sj = 2: every joint valid, no flag stored) - a wave reads
// the coordinates of its own unit only, and before it stores them - and skips samples whose status bit 0 is set.
__global__ __launch_bounds__(NOISE_WAVES * 64) void k_noise_coco(const float* joints, const float* __restrict__ area,
                                                                 const float* __restrict__ sigmas,
                                                                 const unsigned long long* __restrict__ state, float* out,
                                                                 signed char* __restrict__ kind, int B, int sj, int sb, int sa,
                                                                 const int* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * NOISE_WAVES + (threadIdx.x >> 6)));
  if (wave >= B * COCO_UNITS) return;
  const int b = wave / COCO_UNITS, unit = wave - b * COCO_UNITS;
  if (status && (status[b] & 1)) return;
  const float* jb = joints + (size_t)b * sb;
  int num_valid = COCO_J;
  if (sj == 3) {
    num_valid = 0;
    for (int k = 0; k < COCO_J; ++k) num_valid += jb[k * 3 + 2] > 0.f;
  }
  const uint64_t seed = state[0], index = state[1] + (uint64_t)b;
  const float root = sqrtf(fmaxf(area[(size_t)b * sa], 0.f));
  const int j0 = unit == 0 ? 0 : 2 * unit - 1, nj = unit == 0 ? 1 : 2;
  const int j1 = j0 + nj - 1;                    // the unit's second joint (the nose: itself, never used as a partner)
  float x0 = jb[j0 * sj], y0 = jb[j0 * sj + 1], x1 = jb[j1 * sj], y1 = jb[j1 * sj + 1];
  const bool valid0 = sj != 3 || jb[j0 * 3 + 2] > 0.f, valid1 = sj != 3 || jb[j1 * 3 + 2] > 0.f;
  auto store = [&](int j, float x, float y, int kd) {
    if (lane == 0) {
      float* o = out + (size_t)b * sb + j * sj;
      o[0] = x;
      o[1] = y;
      if (sj == 3) o[2] = kd < 0 ? 0.f : 1.f;
      if (kind) kind[(size_t)b * COCO_J + j] = (signed char)kd;
    }
  };
  const int kd0 = noise_joint(seed, index, j0, num_valid, root, sigmas[j0], x0, y0, x1, y1, nj == 2 && valid1, lane);
  store(j0, x0, y0, kd0);
  if (nj == 2) {
    const int kd1 = noise_joint(seed, index, j1, num_valid, root, sigmas[j1], x1, y1, x0, y0, valid0, lane);
    store(j1, x1, y1, kd1);
  }
}

// out[b, j, :] = in[b, j, :] + [weight_j > u] * (mean_j + std_j * n) * (sx, sy); one draw block per (sample, joint): word 0
// the Bernoulli uniform, words 1 and 2 the Box-Muller pair on (1 - u0, u1): n_x = R cos 2 pi u1, n_y = R sin 2 pi u1.
// (pose is not __restrict__: out may be pose itself)
__global__ __launch_bounds__(256) void k_noise_table(const float* pose, const float* __restrict__ mean,
                                                     const float* __restrict__ sd, const float* __restrict__ weight, int J,
                                                     float sx, float sy, const unsigned long long* __restrict__ state,
                                                     float* out, int n, const int* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = i / J, j = i - b * J;
  if (status && (status[b] & 1)) return;
  const Philox4 d = philox_draw(state[0], state[1] + (uint64_t)b, j, ST_TABLE, 0);
  float ox = pose[2 * (size_t)i], oy = pose[2 * (size_t)i + 1];
  if (weight[j] > philox_uniform(d.w[0])) {
    const float R = sqrtf(-2.0f * logf(1.0f - philox_uniform(d.w[1])));
    float sn, cs;
    sincospif(2.0f * philox_uniform(d.w[2]), &sn, &cs);
    ox += fmaf(sd[2 * j], R * cs, mean[2 * j]) * sx;
    oy += fmaf(sd[2 * j + 1], R * sn, mean[2 * j + 1]) * sy;
  }
  out[2 * (size_t)i] = ox;
  out[2 * (size_t)i + 1] = oy;
}

// ---- the chain (p2m_train_sample) ---------------------------------------------------------------------------------------
constexpr int MAX_SJ = 32, MAX_MID = 4, MAX_PAIRS = 16;
constexpr int WORK_FLOATS = 8;     // per sample: root x, y, z, area, flip, unused x 3

struct SampleArgs {
  const float *verts, *trans, *focal, *princpt;
  const int *rr_ptr, *rr_idx;
  const float* rr_val;
  const int *ir_ptr, *ir_idx;      // NULL: the input set is the reg set
  const float* ir_val;
  const float *given_cam, *given_img, *rot;
  const int* flip;
  const unsigned long long* state;
  float *pose2d, *mesh, *lift, *reg, *mesh_valid, *lift_valid, *reg_valid, *fit_err, *rot_flip, *work;
  int* status;
  int B, nv, Jr, reg_root, Ji, n_mid, input_root, J, n_pairs, flip_enabled;
  int mid[2 * MAX_MID], pairs[2 * MAX_PAIRS];
  float mesh_scale, fit_thr, rot_factor, W, H;
};

// One block per sample.  Waves regress the joints (fp64 accumulation over the CSR rows); thread 0 walks the <= 32 joints
// through projection, bbox, affine and the 3D processing; then the whole block streams the sample's mesh.
__global__ __launch_bounds__(256) void k_sample_main(const SampleArgs a) {
  __shared__ float jr[MAX_SJ][3], ji[MAX_SJ][3], px[MAX_SJ], py[MAX_SJ];
  __shared__ float sh_root[3];
  __shared__ int sh_st;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* vb = a.verts + (size_t)b * a.nv * 3;
  float t[3] = {0.f, 0.f, 0.f};
  if (a.trans)
    for (int c = 0; c < 3; ++c) t[c] = a.trans[(size_t)b * 3 + c];
  const float scale = a.mesh_scale;
  const int nrows = a.Jr + (a.ir_ptr ? a.Ji : 0);
  for (int r = wv; r < nrows; r += 4) {
    const bool in = r >= a.Jr;
    const int row = in ? r - a.Jr : r;
    const int* ptr = in ? a.ir_ptr : a.rr_ptr;
    const int* idx = in ? a.ir_idx : a.rr_idx;
    const float* val = in ? a.ir_val : a.rr_val;
    double s[3] = {0.0, 0.0, 0.0};
    for (int e = ptr[row] + lane; e < ptr[row + 1]; e += 64) {
      const float* v = vb + (size_t)idx[e] * 3;
      const double w = (double)val[e];
      for (int c = 0; c < 3; ++c) s[c] += w * (double)((v[c] + t[c]) * scale);
    }
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s[c] += __shfl_xor(s[c], o);
      if (lane == 0) (in ? ji : jr)[row][c] = (float)s[c];
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int Jr = a.Jr, J = a.J;
    const float W = a.W, H = a.H;
    int st = 0;
    float fit = 0.f;
    if (a.given_cam) {
      // get_fitting_error (data/Human36M/dataset.py:301-308): mean distance after aligning the two joint sets' means
      const float* g = a.given_cam + (size_t)b * Jr * 3;
      float mg[3] = {0.f, 0.f, 0.f}, mr[3] = {0.f, 0.f, 0.f};
      for (int j = 0; j < Jr; ++j)
        for (int c = 0; c < 3; ++c) {
          mg[c] += g[j * 3 + c];
          mr[c] += jr[j][c];
        }
      for (int c = 0; c < 3; ++c) {
        mg[c] /= (float)Jr;
        mr[c] /= (float)Jr;
      }
      for (int j = 0; j < Jr; ++j) {
        float d2 = 0.f;
        for (int c = 0; c < 3; ++c) {
          const float d = (g[j * 3 + c] - mg[c]) - (jr[j][c] - mr[c]);
          d2 = fmaf(d, d, d2);
        }
        fit += sqrtf(d2);
      }
      fit /= (float)Jr;
      for (int j = 0; j < Jr; ++j)
        for (int c = 0; c < 3; ++c) jr[j][c] = g[j * 3 + c];
      if (a.fit_thr > 0.f && fit > a.fit_thr) st |= 2;
    }
    if (a.fit_err) a.fit_err[b] = fit;
    const bool own_set = a.ir_ptr != nullptr;
    if (!own_set) {
      for (int j = 0; j < Jr; ++j)
        for (int c = 0; c < 3; ++c) ji[j][c] = jr[j][c];
    } else {
      for (int m = 0; m < a.n_mid; ++m)          // add_pelvis_and_neck
        for (int c = 0; c < 3; ++c) ji[a.Ji + m][c] = (ji[a.mid[2 * m]][c] + ji[a.mid[2 * m + 1]][c]) * 0.5f;
    }
    // cam2pixel of joint_cam / 1000 (given 2D joints of the reg set are taken as they are)
    const float f0 = a.focal[b * 2], f1 = a.focal[b * 2 + 1], c0 = a.princpt[b * 2], c1 = a.princpt[b * 2 + 1];
    for (int j = 0; j < J; ++j) {
      if (!own_set && a.given_img) {
        px[j] = a.given_img[((size_t)b * Jr + j) * 2];
        py[j] = a.given_img[((size_t)b * Jr + j) * 2 + 1];
      } else {
        const float z = ji[j][2] / 1000.0f;
        px[j] = fmaf((ji[j][0] / 1000.0f) / z, f0, c0);
        py[j] = fmaf((ji[j][1] / 1000.0f) / z, f1, c1);
      }
    }
    // get_bbox, process_bbox at aspect W / H, get_center_scale (lib/coord_utils.py:7-66)
    float xmin = px[0], xmax = px[0], ymin = py[0], ymax = py[0];
    for (int j = 1; j < J; ++j) {
      xmin = fminf(xmin, px[j]);
      xmax = fmaxf(xmax, px[j]);
      ymin = fminf(ymin, py[j]);
      ymax = fmaxf(ymax, py[j]);
    }
    bool finite = true;
    for (int j = 0; j < J; ++j) finite = finite && fabsf(px[j]) < __builtin_inff() && fabsf(py[j]) < __builtin_inff();
    const float tw = xmax - xmin, th = ymax - ymin;
    float w = tw - 1.0f, h = th - 1.0f;
    if (!(finite && tw * th > 0.f && w >= 0.f && h >= 0.f)) st |= 1;
    const float cx = xmin + w * 0.5f, cy = ymin + h * 0.5f, aspect = W / H;
    if (w > aspect * h) h = w / aspect;
    else if (w < aspect * h) w = h * aspect;
    if (!(w > 0.f)) st |= 1;
    // augmentation parameters: given, or drawn (augm_params, lib/aug_utils.py:98-117)
    const Philox4 d = philox_draw(a.state[0], a.state[1] + (uint64_t)b, 0, ST_AUG, 0);
    int flip = a.flip ? (a.flip[b] != 0) : (a.flip_enabled && philox_uniform(d.w[0]) < 0.5f);
    float rot;
    if (a.rot) {
      rot = a.rot[b];
    } else {
      const float R = sqrtf(-2.0f * logf(1.0f - philox_uniform(d.w[1])));
      float sn, cs;
      sincospif(2.0f * philox_uniform(d.w[2]), &sn, &cs);
      const float lim = 2.0f * a.rot_factor;
      rot = fminf(lim, fmaxf(-lim, (R * cs) * a.rot_factor));
      if (philox_uniform(d.w[3]) < 0.5f) rot = 0.f;
    }
    if (a.rot_flip) {
      a.rot_flip[b * 2] = rot;
      a.rot_flip[b * 2 + 1] = (float)flip;
    }
    // get_affine_transform is a similarity: scale W / bbox_w, rotation by -rot about the bbox centre onto the crop centre
    const float s = W / w;
    float sn, cs;
    sincospif(rot / 180.0f, &sn, &cs);
    float* p2 = a.pose2d + (size_t)b * J * 2;
    float* lo = a.lift + (size_t)b * J * 3;
    float* ro = a.reg + (size_t)b * Jr * 3;
    const bool dead = st & 1;
    for (int j = 0; j < J; ++j) {
      const float dx = px[j] - cx, dy = py[j] - cy;
      p2[j * 2] = dead ? 0.f : fmaf(s, fmaf(cs, dx, sn * dy), W * 0.5f);
      p2[j * 2 + 1] = dead ? 0.f : fmaf(s, fmaf(cs, dy, -(sn * dx)), H * 0.5f);
    }
    // root-relative targets; j3d_processing of the lift target only (rotation by -rot about z, pair swaps, x = -x)
    const int iroot = a.input_root;
    const float r0 = ji[iroot][0], r1 = ji[iroot][1], r2 = ji[iroot][2];
    for (int j = 0; j < J; ++j) {
      int src = j;
      if (flip)
        for (int p = 0; p < a.n_pairs; ++p) {
          if (a.pairs[2 * p] == j) src = a.pairs[2 * p + 1];
          else if (a.pairs[2 * p + 1] == j) src = a.pairs[2 * p];
        }
      const float x = ji[src][0] - r0, y = ji[src][1] - r1, z = ji[src][2] - r2;
      float xr = x, yr = y;
      if (rot != 0.f) {                // sin(-r) = -sn, cos(-r) = cs
        xr = fmaf(cs, x, sn * y);
        yr = fmaf(cs, y, -(sn * x));
      }
      lo[j * 3] = dead ? 0.f : (flip ? -xr : xr);
      lo[j * 3 + 1] = dead ? 0.f : yr;
      lo[j * 3 + 2] = dead ? 0.f : z;
      a.lift_valid[(size_t)b * J + j] = (dead || ((st & 2) && own_set)) ? 0.f : 1.f;
    }
    for (int c = 0; c < 3; ++c) sh_root[c] = jr[a.reg_root][c];
    for (int j = 0; j < Jr; ++j) {
      for (int c = 0; c < 3; ++c) ro[j * 3 + c] = dead ? 0.f : jr[j][c] - sh_root[c];
      a.reg_valid[(size_t)b * Jr + j] = dead ? 0.f : 1.f;
    }
    float* wk = a.work + (size_t)b * WORK_FLOATS;
    wk[3] = (s * tw) * (s * th);       // the tight box's transformed sides (:315-320)
    wk[4] = (float)flip;
    a.status[b] = st;
    sh_st = st;
  }
  __syncthreads();
  // the mesh: ((v + trans) * scale - root) / 1000, 16 bytes per lane where input and output are aligned alike
  const int st = sh_st;
  const float root[3] = {sh_root[0], sh_root[1], sh_root[2]};
  const int n = a.nv * 3;
  float* mo = a.mesh + (size_t)b * n;
  const bool dead = st & 1;
  auto elem = [&](float v, int c) { return dead ? 0.f : ((v + t[c]) * scale - root[c]) / 1000.0f; };
  const bool vec = ((((uintptr_t)vb) ^ ((uintptr_t)mo)) & 15) == 0;
  const int head = vec ? min(n, (int)(((16 - ((uintptr_t)vb & 15)) & 15) >> 2)) : n;
  for (int i = tid; i < head; i += 256) mo[i] = elem(vb[i], i % 3);
  if (vec) {
    const int n4 = (n - head) >> 2;
    for (int k = tid; k < n4; k += 256) {
      const int i = head + 4 * k, c = i % 3;
      const float4 v = *reinterpret_cast<const float4*>(vb + i);
      float4 o;
      o.x = elem(v.x, c);
      o.y = elem(v.y, c == 2 ? 0 : c + 1);
      o.z = elem(v.z, c == 0 ? 2 : c - 1);
      o.w = elem(v.w, c);
      *reinterpret_cast<float4*>(mo + i) = o;
    }
    for (int i = head + 4 * n4 + tid; i < n; i += 256) mo[i] = elem(vb[i], i % 3);
  }
  const float mv = (st & 3) ? 0.f : 1.f;
  for (int i = tid; i < a.nv; i += 256) a.mesh_valid[(size_t)b * a.nv + i] = mv;
}

// One wave per sample, lane j = joint j: the 2D flip (x = W - x - 1, pair swaps), / (W, H), per-sample standardisation with
// the population std.  A zero (or NaN) std sets status bit 0 and zeroes the sample - its mesh included, a path no sane
// sample takes.
__global__ __launch_bounds__(256) void k_sample_finish(const SampleArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (b >= a.B) return;
  const int J = a.J, st = a.status[b];
  if (st & 1) return;
  float* p2 = a.pose2d + (size_t)b * J * 2;
  int src = lane;
  const bool flip = a.work[(size_t)b * WORK_FLOATS + 4] != 0.f;
  if (flip)
    for (int p = 0; p < a.n_pairs; ++p) {
      if (a.pairs[2 * p] == lane) src = a.pairs[2 * p + 1];
      else if (a.pairs[2 * p + 1] == lane) src = a.pairs[2 * p];
    }
  const bool on = lane < J;
  float x = on ? p2[src * 2] : 0.f, y = on ? p2[src * 2 + 1] : 0.f;
  if (flip) x = a.W - x - 1.0f;
  x /= a.W;
  y /= a.H;
  if (!on) x = y = 0.f;
  float sx = x, sy = y;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sx += __shfl_xor(sx, o);
    sy += __shfl_xor(sy, o);
  }
  const float mx = sx / (float)J, my = sy / (float)J;
  const float dx = on ? x - mx : 0.f, dy = on ? y - my : 0.f;
  float vx = dx * dx, vy = dy * dy;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    vx += __shfl_xor(vx, o);
    vy += __shfl_xor(vy, o);
  }
  const float sdx = sqrtf(vx / (float)J), sdy = sqrtf(vy / (float)J);
  const bool ok = sdx > 0.f && sdy > 0.f && sdx < __builtin_inff() && sdy < __builtin_inff();
  if (ok) {
    if (on) {
      p2[lane * 2] = dx / sdx;
      p2[lane * 2 + 1] = dy / sdy;
    }
    return;
  }
  if (lane == 0) a.status[b] = st | 1;
  for (int i = lane; i < J * 2; i += 64) p2[i] = 0.f;
  for (int i = lane; i < J * 3; i += 64) a.lift[(size_t)b * J * 3 + i] = 0.f;
  for (int i = lane; i < J; i += 64) a.lift_valid[(size_t)b * J + i] = 0.f;
  for (int i = lane; i < a.Jr * 3; i += 64) a.reg[(size_t)b * a.Jr * 3 + i] = 0.f;
  for (int i = lane; i < a.Jr; i += 64) a.reg_valid[(size_t)b * a.Jr + i] = 0.f;
  for (int i = lane; i < a.nv * 3; i += 64) a.mesh[(size_t)b * a.nv * 3 + i] = 0.f;
  for (int i = lane; i < a.nv; i += 64) a.mesh_valid[(size_t)b * a.nv + i] = 0.f;
}

}  // namespace p2m

using namespace p2m;

extern "C" int64_t p2m_train_sample_workspace(int32_t B) { return B < 1 ? 0 : (int64_t)B * WORK_FLOATS * (int64_t)sizeof(float); }

extern "C" int p2m_train_sample(const float* verts, const float* trans, float mesh_scale, const float* focal, const float* princpt,
                                int32_t B, int32_t nv, const int32_t* rr_ptr, const int32_t* rr_idx, const float* rr_val,
                                int32_t Jr, int32_t reg_root, const int32_t* ir_ptr, const int32_t* ir_idx, const float* ir_val,
                                int32_t Ji, const int32_t* midpoints, int32_t n_mid, int32_t input_root,
                                const float* given_reg_cam, const float* given_reg_img, float fit_thr, const float* rot,
                                const int32_t* flip, float rot_factor, int32_t flip_enabled, int32_t noise_mode,
                                const float* sigmas, const float* tab_mean, const float* tab_std, const float* tab_weight,
                                const int32_t* flip_pairs, int32_t n_pairs, float W, float H, const uint64_t* state,
                                void* workspace, int64_t workspace_bytes, float* pose2d, float* mesh, float* lift_pose3d,
                                float* reg_pose3d, float* mesh_valid, float* lift_valid, float* reg_valid, int32_t* status,
                                float* fit_err, int8_t* kind, float* rot_flip, void* stream) {
  P2M_CHECK_ARG(verts && focal && princpt && rr_ptr && rr_idx && rr_val, "null input pointer");
  P2M_CHECK_ARG(pose2d && mesh && lift_pose3d && reg_pose3d && mesh_valid && lift_valid && reg_valid && status,
                "null output pointer");
  P2M_CHECK_ARG(state, "state is NULL (two uint64 words in device memory: seed, first sample index)");
  P2M_CHECK_ARG((uintptr_t)state % 8 == 0, "misaligned state");
  P2M_CHECK_ARG(B >= 1 && B <= (1 << 20), "B outside [1, 2^20]");
  P2M_CHECK_ARG(nv >= 1 && nv <= (1 << 20) && (long)B * nv * 3 < (1L << 40), "nv outside [1, 2^20]");
  P2M_CHECK_ARG(Jr >= 1 && Jr <= MAX_SJ, "Jr outside [1, 32]");
  P2M_CHECK_ARG(reg_root >= 0 && reg_root < Jr, "reg_root outside [0, Jr)");
  const bool own_set = ir_ptr != nullptr;
  if (own_set) {
    P2M_CHECK_ARG(ir_idx && ir_val, "input regressor: null idx / val");
    P2M_CHECK_ARG(n_mid >= 0 && n_mid <= MAX_MID, "midpoints outside [0, 4]");
    P2M_CHECK_ARG(Ji >= 1 && Ji + n_mid <= MAX_SJ, "J = Ji + midpoints outside [1, 32]");
    P2M_CHECK_ARG(n_mid == 0 || midpoints, "midpoints is NULL");
    for (int m = 0; m < 2 * n_mid; ++m) P2M_CHECK_ARG(midpoints[m] >= 0 && midpoints[m] < Ji, "midpoint joint outside [0, Ji)");
  } else {
    P2M_CHECK_ARG(n_mid == 0, "midpoints need an input regressor");
  }
  const int J = own_set ? Ji + n_mid : Jr;
  P2M_CHECK_ARG(input_root >= 0 && input_root < J, "input_root outside [0, J)");
  P2M_CHECK_ARG(!given_reg_img || given_reg_cam, "given_reg_img without given_reg_cam");
  P2M_CHECK_ARG(n_pairs >= 0 && n_pairs <= MAX_PAIRS && (n_pairs == 0 || flip_pairs), "flip pairs outside [0, 16]");
  unsigned used = 0;
  for (int p = 0; p < 2 * n_pairs; ++p) {
    P2M_CHECK_ARG(flip_pairs[p] >= 0 && flip_pairs[p] < J, "flip pair joint outside [0, J)");
    P2M_CHECK_ARG(!(used >> flip_pairs[p] & 1u), "flip pairs must be disjoint");
    used |= 1u << flip_pairs[p];
  }
  P2M_CHECK_ARG(noise_mode == P2M_SAMPLE_NOISE_NONE || noise_mode == P2M_SAMPLE_NOISE_COCO ||
                noise_mode == P2M_SAMPLE_NOISE_TABLE, "unknown noise_mode");
  P2M_CHECK_ARG(noise_mode != P2M_SAMPLE_NOISE_COCO || (sigmas && J >= COCO_J), "coco noise needs sigmas and J >= 17");
  P2M_CHECK_ARG(noise_mode != P2M_SAMPLE_NOISE_TABLE || (tab_mean && tab_std && tab_weight), "table noise needs the table");
  P2M_CHECK_ARG(W > 0.f && H > 0.f && W < 1e6f && H < 1e6f, "W, H outside (0, 1e6)");
  P2M_CHECK_ARG(mesh_scale == mesh_scale && rot_factor >= 0.f && fit_thr == fit_thr, "mesh_scale / rot_factor / fit_thr");
  P2M_CHECK_ARG(workspace && workspace_bytes >= p2m_train_sample_workspace(B) && (uintptr_t)workspace % 4 == 0,
                "workspace too small (p2m_train_sample_workspace) or misaligned");
  P2M_CHECK_ARG((uintptr_t)verts % 4 == 0 && (uintptr_t)mesh % 4 == 0 && (uintptr_t)pose2d % 4 == 0, "misaligned buffer");
  SampleArgs a{};
  a.verts = verts, a.trans = trans, a.focal = focal, a.princpt = princpt;
  a.rr_ptr = rr_ptr, a.rr_idx = rr_idx, a.rr_val = rr_val, a.ir_ptr = ir_ptr, a.ir_idx = ir_idx, a.ir_val = ir_val;
  a.given_cam = given_reg_cam, a.given_img = given_reg_img, a.rot = rot, a.flip = flip;
  a.state = (const unsigned long long*)state;
  a.pose2d = pose2d, a.mesh = mesh, a.lift = lift_pose3d, a.reg = reg_pose3d, a.mesh_valid = mesh_valid;
  a.lift_valid = lift_valid, a.reg_valid = reg_valid, a.fit_err = fit_err, a.rot_flip = rot_flip, a.work = (float*)workspace;
  a.status = status;
  a.B = B, a.nv = nv, a.Jr = Jr, a.reg_root = reg_root, a.Ji = own_set ? Ji : Jr, a.n_mid = n_mid, a.input_root = input_root;
  a.J = J, a.n_pairs = n_pairs, a.flip_enabled = flip_enabled;
  for (int m = 0; m < 2 * n_mid; ++m) a.mid[m] = midpoints[m];
  for (int p = 0; p < 2 * n_pairs; ++p) a.pairs[p] = flip_pairs[p];
  a.mesh_scale = mesh_scale, a.fit_thr = fit_thr, a.rot_factor = rot_factor, a.W = W, a.H = H;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sample_main, dim3(B), dim3(256), 0, s, a);
  if (noise_mode == P2M_SAMPLE_NOISE_COCO)       // the first 17 joints, in place; pelvis and neck keep their clean values
    hipLaunchKernelGGL(k_noise_coco, dim3(cdiv((long)B * COCO_UNITS, NOISE_WAVES)), dim3(NOISE_WAVES * 64), 0, s, pose2d,
                       a.work + 3, sigmas, a.state, pose2d, (signed char*)kind, B, 2, J * 2, WORK_FLOATS, status);
  else if (noise_mode == P2M_SAMPLE_NOISE_TABLE)
    hipLaunchKernelGGL(k_noise_table, dim3(cdiv((long)B * J, 256)), dim3(256), 0, s, pose2d, tab_mean, tab_std, tab_weight, J,
                       W / 256.0f, H / 256.0f, a.state, pose2d, B * J, status);
  hipLaunchKernelGGL(k_sample_finish, dim3(cdiv(B, 4)), dim3(256), 0, s, a);
  return check_launch("train_sample");
}

extern "C" int p2m_pose_noise_coco(const float* joints, const float* area, const float* sigmas, const uint64_t* state,
                                   float* out, int8_t* kind, int32_t B, void* stream) {
  P2M_CHECK_ARG(joints && area && sigmas && out, "null pointer");
  P2M_CHECK_ARG(state, "state is NULL (two uint64 words in device memory: seed, first sample index)");
  P2M_CHECK_ARG(B >= 1 && (long)B * COCO_UNITS * 64 < (1L << 31), "B outside [1, 2^31 / 576)");
  const uintptr_t jb0 = (uintptr_t)joints, ob0 = (uintptr_t)out, nbytes = (uintptr_t)B * COCO_J * 3 * sizeof(float);
  P2M_CHECK_ARG(ob0 + nbytes <= jb0 || jb0 + nbytes <= ob0,
                "out must not alias or overlap joints (a wave reads all 17 validity flags)");
  P2M_CHECK_ARG((uintptr_t)state % 8 == 0 && (uintptr_t)joints % 4 == 0 && (uintptr_t)area % 4 == 0 &&
                (uintptr_t)sigmas % 4 == 0 && (uintptr_t)out % 4 == 0, "misaligned buffer");
  hipLaunchKernelGGL(k_noise_coco, dim3(cdiv((long)B * COCO_UNITS, NOISE_WAVES)), dim3(NOISE_WAVES * 64), 0,
                     (hipStream_t)stream, joints, area, sigmas, (const unsigned long long*)state, out, (signed char*)kind, B, 3,
                     COCO_J * 3, 1, (const int*)nullptr);
  return check_launch("pose_noise_coco");
}

extern "C" int p2m_pose_noise_table(const float* pose, const float* mean, const float* std, const float* weight, int32_t J,
                                    float W, float H, const uint64_t* state, float* out, int32_t B, void* stream) {
  P2M_CHECK_ARG(pose && mean && std && weight && out, "null pointer");
  P2M_CHECK_ARG(state, "state is NULL (two uint64 words in device memory: seed, first sample index)");
  P2M_CHECK_ARG(J >= 1 && J <= 32, "J outside [1, 32]");
  P2M_CHECK_ARG(B >= 1 && (long)B * J * 2 < (1L << 31), "B * J * 2 outside [2, 2^31)");
  P2M_CHECK_ARG(W == W && H == H, "W or H is NaN");
  P2M_CHECK_ARG((uintptr_t)state % 8 == 0 && (uintptr_t)pose % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)mean % 4 == 0 &&
                (uintptr_t)std % 4 == 0 && (uintptr_t)weight % 4 == 0, "misaligned buffer");
  hipLaunchKernelGGL(k_noise_table, dim3(cdiv((long)B * J, 256)), dim3(256), 0, (hipStream_t)stream, pose, mean, std, weight, J,
                     W / 256.0f, H / 256.0f, (const unsigned long long*)state, out, B * J, (const int*)nullptr);
  return check_launch("pose_noise_table");
}
