// 2D pose overlay on the GPU (gfx950): batched anti-aliased lines, discs and rings blended into uint8 images, the device
// counterpart of the reference's lib/vis.py (vis_2d_keypoints, vis_coco_skeleton; there OpenCV's LINE_AA).  OpenCV is not a
// dependency of this project, so the comment of p2m_pose_overlay in include/p2m.h is the contract and tests/overlay_ref.py its
// exact-integer restatement.  Geometry, paint order and blending semantics follow the reference; the pixel arithmetic is ours.
//
// Two kernels per call on the caller's stream, no memset, no allocation, no sync, no data-dependent grid, no atomics in global
// memory:
//   k_overlay_setup  one block per (image, person): thread j snaps joint j and decides its visibility, thread s writes the
//                    record of primitive slot s at the slot's paint index - an 8-byte pixel bbox (inflated by the reach of the
//                    primitive, clipped to the image; empty: draws nothing) and 16 bytes of endpoints, style and colour - and
//                    thread 0 the status word (bits collected with an integer atomicOr in LDS).
//   k_overlay_tile   one block per 32 x 32-pixel tile of an image, a lane holds 4 neighbouring pixels of a row in registers.
//                    The image's records are scanned in paint order, 256 at a time; the ones whose bbox meets the tile are
//                    compacted in order (a ballot per wave, a prefix over the waves) into an LDS queue of 256 entries - the
//                    chunk's size, so it cannot overflow - together with their 16-byte records, and then applied one after the
//                    other: the record is read from LDS at an address that is uniform over the block (a broadcast).  A tile no
//                    record meets is never loaded; it is left alone in place and copied out of place.
#include "p2m_common.h"

namespace p2m {

constexpr int O_NT = 256;             // threads per block, and records per scan chunk
constexpr int O_TILE = 32;            // tile edge in pixels: 8 lanes x 4 pixels per row, 32 rows
constexpr int O_MAX_DIM = 8192;
constexpr int O_MAX_J = 64, O_MAX_P = 64, O_MAX_L = 64;
constexpr int O_COORD = 16384;        // a coordinate is usable when |v| < 16384
constexpr int O_MAX_H2 = 64, O_MAX_R16 = 1024;
constexpr int O_FAR_C = 1 << 26;      // |cross| from which a pixel is more than 1400 px from the segment's line
constexpr int O_FAR_D = 2048;         // an estimate of D from which cov = 0 whatever the fix-up gives (D matters below 1544)
constexpr int O_STATUS_JOINT = 1, O_STATUS_BOX = 2;

struct OverlaySetupArgs {
  const float* poses; const int* bones; const unsigned char* colours; const float* boxes;
  int B, P, J, C, L, S, H, W, colour_mode, has_boxes;
  unsigned box_rgb;
  float thr;
  int line_h2, mark_h2, mark_r16, box_h2;
  short4* pbox;                       // [B][P * S]  pixel bbox (x0, y0, x1, y1), inclusive, clipped; empty: x0 > x1
  int4* prec;                         // [B][P * S]  (ax | ay << 16, bx | by << 16, h2 | r16 << 16, rgb), for non-empty boxes
  int* status;                        // [B][P] or NULL
};

__device__ __forceinline__ bool snap_px(float v, int& out) {            // (int)v, usable iff finite and |v| < 16384
  const bool ok = fabsf(v) < (float)O_COORD;                            // (NaN and infinity compare false)
  out = ok ? (int)v : 0;
  return ok;
}

__device__ __forceinline__ int pack2(int lo, int hi) { return (int)(((unsigned)lo & 0xffffu) | ((unsigned)hi << 16)); }
__device__ __forceinline__ int lo16(int v) { return (int)(short)(v & 0xffff); }
__device__ __forceinline__ int hi16(int v) { return v >> 16; }

__global__ __launch_bounds__(O_NT) void k_overlay_setup(OverlaySetupArgs a) {
  __shared__ int jx[O_MAX_J], jy[O_MAX_J], jvis[O_MAX_J];
  __shared__ int cx[4], cy[4];
  __shared__ int st;
  const int tid = threadIdx.x;
  const long bp = blockIdx.x;                                            // (image, person)
  if (tid == 0) st = 0;
  __syncthreads();
  if (tid < a.J) {
    const float* q = a.poses + (bp * a.J + tid) * a.C;
    int x, y;
    const bool okx = snap_px(q[0], x), oky = snap_px(q[1], y);
    const bool usable = okx && oky;
    bool vis = usable;
    if (a.C == 3) vis = vis && (q[2] > a.thr);                            // strict; a NaN confidence is invisible
    jx[tid] = x; jy[tid] = y; jvis[tid] = vis ? 1 : 0;
    if (!usable) atomicOr(&st, O_STATUS_JOINT);
  } else if (a.has_boxes && tid >= O_MAX_J && tid < O_MAX_J + 4) {
    const int k = tid - O_MAX_J;
    const float* q = a.boxes + (bp * 4 + k) * 2;
    int x, y;
    const bool okx = snap_px(q[0], x), oky = snap_px(q[1], y);
    cx[k] = x; cy[k] = y;
    if (!(okx && oky)) atomicOr(&st, O_STATUS_BOX);
  }
  __syncthreads();
  if (tid == 0 && a.status) a.status[bp] = st;
  if (tid >= a.S) return;
  // slot -> primitive
  int ax = 0, ay = 0, bx = 0, by = 0, h2 = 0, r16 = -1;
  unsigned rgb = 0;
  bool draw = false;
  const int nbox = a.has_boxes ? 4 : 0;
  if (tid < nbox) {
    const int k = tid, k1 = (tid + 1) & 3;
    draw = !(st & O_STATUS_BOX);
    ax = cx[k]; ay = cy[k]; bx = cx[k1]; by = cy[k1];
    h2 = a.box_h2; rgb = a.box_rgb & 0xffffffu;
  } else {
    const int s = tid - nbox, l = s / 3, kind = s - 3 * l;
    const unsigned i1 = (unsigned)a.bones[2 * l], i2 = (unsigned)a.bones[2 * l + 1];
    // (an index outside [0, J) is refused on the host where the host can see the bones; here it only must not be followed)
    if (i1 < (unsigned)a.J && i2 < (unsigned)a.J) {
      const bool v1 = jvis[i1] != 0, v2 = jvis[i2] != 0;
      if (kind == 0) {
        draw = v1 && v2;
        ax = jx[i1]; ay = jy[i1]; bx = jx[i2]; by = jy[i2];
        h2 = a.line_h2;
      } else {
        const unsigned i = kind == 1 ? i1 : i2;
        draw = kind == 1 ? v1 : v2;
        ax = bx = jx[i]; ay = by = jy[i];
        h2 = a.mark_h2; r16 = a.mark_r16;
      }
      const unsigned char* c = a.colours + 3 * (a.colour_mode == 0 ? (long)l : bp);
      rgb = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
    }
  }
  int x0 = 32767, y0 = 32767, x1 = -1, y1 = -1;
  if (draw) {
    // cov > 0 needs D < T = 8 h2 + 8 + max(r16, 0) sixteenths, i.e. an integer offset of at most (T - 1) >> 4 from the bbox
    const int reach = (8 * h2 + 8 + max(r16, 0) - 1) >> 4;
    const int qx0 = max(min(ax, bx) - reach, 0), qx1 = min(max(ax, bx) + reach, a.W - 1);
    const int qy0 = max(min(ay, by) - reach, 0), qy1 = min(max(ay, by) + reach, a.H - 1);
    if (qx0 <= qx1 && qy0 <= qy1) { x0 = qx0; y0 = qy0; x1 = qx1; y1 = qy1; }
  }
  const long o = bp * a.S + tid;                                         // = image * (P S) + the slot's paint index
  a.pbox[o] = make_short4((short)x0, (short)y0, (short)x1, (short)y1);
  if (x0 <= x1) a.prec[o] = make_int4(pack2(ax, ay), pack2(bx, by), pack2(h2, r16), (int)rgb);
}

// ---- tiles -------------------------------------------------------------------------------------------------------------
struct OverlayTileArgs {
  const short4* pbox; const int4* prec;
  int n_rec;                          // records per image: P * S
  int H, W, tiles_x, tiles_y, alpha256;
  const unsigned char* src; unsigned char* dst;
};

// Coverage of pixel (px, py) by the primitive in sixteenths, 0 .. 16: include/p2m.h.  dx, dy, L2 and inv_len = 1 / sqrt(L2) are
// uniform over the block.  Pixels lie in [0, 8191] and snapped coordinates in [-16383, 16383], so |w| <= 24574 and |d| <= 32766
// per axis: w.d, the cross product c and w.w stay below 2 x 24574 x 32766 < 2^31 and are taken in 32 bits.
// D = isqrt(floor(256 num / den)) comes from an fp32 estimate of 16 sqrt(num / den) = 16 |c| / |d| (or 16 |w|): six roundings
// of 2^-24 each, so below O_FAR_D = 2048 the estimate is within 1e-3 of the real value.  Its floor IS D unless it lies
// within 2e-3 of an integer; only there, and only where D - 1, D and D + 1 do not all give the same coverage, the two exact
// 64-bit comparisons D^2 den <= 256 num < (D + 1)^2 den settle it.  (A wave pays for its slowest lane; settling every pixel
// near a shape measured 10 % slower on the 1080p legs, and this loop is where the kernel's time goes: DESIGN.md section 8e.)
__device__ __forceinline__ int cov_of(int D, int full, int r16) {
  const int d = r16 >= 0 ? abs(D - r16) : D;
  return min(max(full - d, 0), 16);
}

__device__ __forceinline__ int coverage(int px, int py, int ax, int ay, int bx, int by, int dx, int dy, long L2, float inv_len,
                                        int h2, int r16) {
  const int wx = px - ax, wy = py - ay;
  const int t = wx * dx + wy * dy;
  int n32 = 0, c = 0;
  bool mid = false;
  if (L2 == 0 || t <= 0) {
    n32 = wx * wx + wy * wy;
  } else if ((long)t >= L2) {
    const int ex = px - bx, ey = py - by;
    n32 = ex * ex + ey * ey;
  } else {
    c = wx * dy - wy * dx;
    if (c >= O_FAR_C || c <= -O_FAR_C) return 0;
    mid = true;
  }
  const float est = mid ? 16.f * fabsf((float)c) * inv_len : 16.f * sqrtf((float)n32);
  if (!(est < (float)O_FAR_D)) return 0;
  const int full = 8 * h2 + 8;                                           // cov = clamp(full - D', 0, 16)
  if (r16 < 0 ? est >= (float)(full + 1) : (est >= (float)(r16 + full + 1) || est <= (float)(r16 - full - 1))) return 0;
  int D = (int)est;
  const float frac = est - (float)D;
  if (frac < 2e-3f || frac > 1.f - 2e-3f) {
    const int c0 = cov_of(D, full, r16);
    if (cov_of(D - 1, full, r16) != c0 || cov_of(D + 1, full, r16) != c0) {
      const long num = mid ? (long)c * c : (long)n32, den = mid ? L2 : 1L;
      const long n256 = num << 8;                                        // (num < 2^52)
      long E = D;
      while (E * E * den > n256) E--;
      while ((E + 1) * (E + 1) * den <= n256) E++;
      D = (int)E;
    }
  }
  return cov_of(D, full, r16);
}

__global__ __launch_bounds__(O_NT) void k_overlay_tile(OverlayTileArgs a) {
  __shared__ int4 q_rec[O_NT];
  __shared__ short4 q_box[O_NT];
  __shared__ int wcnt[2][O_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int tiles = a.tiles_x * a.tiles_y;
  const int img = blockIdx.x / tiles, tl = blockIdx.x - img * tiles;
  const int tyi = tl / a.tiles_x, txi = tl - tyi * a.tiles_x;
  const int tx0 = txi * O_TILE, ty0 = tyi * O_TILE;
  const int tx1 = min(tx0 + O_TILE, a.W) - 1, ty1 = min(ty0 + O_TILE, a.H) - 1;
  // this lane's pixels: row y, columns x .. x + nx - 1
  const int y = ty0 + (tid >> 3), x = tx0 + (tid & 7) * 4;
  const int nx = (y <= ty1 && x <= tx1) ? min(4, tx1 - x + 1) : 0;
  const long off = (((long)img * a.H + y) * a.W + x) * 3;               // (only used when nx > 0)
  const bool wide_in = nx == 4 && (((uintptr_t)(a.src + off)) & 3) == 0;
  const bool wide_out = nx == 4 && (((uintptr_t)(a.dst + off)) & 3) == 0;
  unsigned sp[4] = {0, 0, 0, 0};                                        // the source pixels, packed
  int m[4][3] = {};
  bool loaded = false;

  const short4* pbox = a.pbox + (long)img * a.n_rec;
  const int4* prec = a.prec + (long)img * a.n_rec;
  for (int c0 = 0, step = 0; c0 < a.n_rec; c0 += O_NT, step++) {
    const int r = c0 + tid;
    bool hit = false;
    short4 bb = make_short4(0, 0, 0, 0);
    if (r < a.n_rec) {
      bb = pbox[r];
      hit = bb.x <= tx1 && bb.z >= tx0 && bb.y <= ty1 && bb.w >= ty0;     // (an empty box has x0 = 32767: never a hit)
    }
    // compaction in paint order: a ballot per wave, the waves' counts through LDS (two buffers: the next chunk's writes
    // cannot overtake this chunk's reads)
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) wcnt[step & 1][tid >> 6] = __popcll(bal);
    __syncthreads();                                                     // (also: the previous chunk's queue has been read)
    int base = 0, n = 0;
#pragma unroll
    for (int w = 0; w < O_NT / 64; w++) {
      const int c = wcnt[step & 1][w];
      base += w < (tid >> 6) ? c : 0;
      n += c;
    }
    if (hit) {
      const int e = base + __popcll(bal & ((1ull << lane) - 1ull));
      q_box[e] = bb;
      q_rec[e] = prec[r];
    }
    if (n == 0) continue;                                                // (uniform)
    __syncthreads();
    if (!loaded) {
      loaded = true;
      if (wide_in) {
        const unsigned* w = reinterpret_cast<const unsigned*>(a.src + off);
        const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
        sp[0] = w0 & 0xffffffu; sp[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
        sp[2] = (w1 >> 16) | ((w2 & 0xffu) << 16); sp[3] = w2 >> 8;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (j < nx) {
            const unsigned char* p = a.src + off + 3 * j;
            sp[j] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
          }
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        m[j][0] = (int)(sp[j] & 0xffu); m[j][1] = (int)((sp[j] >> 8) & 0xffu); m[j][2] = (int)(sp[j] >> 16);
      }
    }
    for (int e = 0; e < n; e++) {
      const short4 eb = q_box[e];                                        // (uniform address: one LDS broadcast each)
      const int4 rec = q_rec[e];
      if (nx == 0 || y < eb.y || y > eb.w || x > eb.z || x + nx - 1 < eb.x) continue;
      const int ax = lo16(rec.x), ay = hi16(rec.x), bx = lo16(rec.y), by = hi16(rec.y);
      const int h2 = lo16(rec.z), r16 = hi16(rec.z);
      const int col[3] = {rec.w & 0xff, (rec.w >> 8) & 0xff, (rec.w >> 16) & 0xff};
      const int dx = bx - ax, dy = by - ay;
      const long L2 = (long)dx * dx + (long)dy * dy;
      const float inv_len = L2 > 0 ? 1.f / sqrtf((float)L2) : 0.f;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int px = x + j;
        if (j >= nx || px < eb.x || px > eb.z) continue;
        const int cov = coverage(px, y, ax, ay, bx, by, dx, dy, L2, inv_len, h2, r16);
        if (cov > 0) {
#pragma unroll
          for (int k = 0; k < 3; k++) m[j][k] += ((col[k] - m[j][k]) * cov + 8) >> 4;
        }
      }
    }
  }
  if (nx == 0) return;
  if (!loaded) {                                                         // nothing met the tile
    if (a.src == a.dst) return;
    if (wide_in && wide_out) {
      const unsigned* w = reinterpret_cast<const unsigned*>(a.src + off);
      unsigned* o = reinterpret_cast<unsigned*>(a.dst + off);
      const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
      o[0] = w0; o[1] = w1; o[2] = w2;
    } else {
      unsigned char v[12];
#pragma unroll
      for (int j = 0; j < 12; j++) v[j] = j < 3 * nx ? a.src[off + j] : (unsigned char)0;
#pragma unroll
      for (int j = 0; j < 12; j++)
        if (j < 3 * nx) a.dst[off + j] = v[j];
    }
    return;
  }
  // dst = (src (256 - alpha) + m alpha + 128) >> 8
  unsigned op[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int s = (int)((sp[j] >> (8 * k)) & 0xffu);
      v |= (unsigned)((s * (256 - a.alpha256) + m[j][k] * a.alpha256 + 128) >> 8) << (8 * k);
    }
    op[j] = v;
  }
  if (wide_out) {
    unsigned* o = reinterpret_cast<unsigned*>(a.dst + off);
    o[0] = op[0] | (op[1] << 24);
    o[1] = (op[1] >> 8) | (op[2] << 16);
    o[2] = (op[2] >> 16) | (op[3] << 8);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (j < nx) {
        unsigned char* p = a.dst + off + 3 * j;
        p[0] = (unsigned char)(op[j] & 0xffu); p[1] = (unsigned char)((op[j] >> 8) & 0xffu); p[2] = (unsigned char)(op[j] >> 16);
      }
  }
}

static inline long overlay_box_bytes(long n) { return (n * 8 + 15) & ~15L; }

}  // namespace p2m

using namespace p2m;

static int overlay_shape_ok(int32_t B, int32_t P, int32_t L, int32_t with_boxes, const char* fn) {
  if (B < 0) { set_error("%s: bad batch", fn); return 0; }
  if (P < 1 || P > O_MAX_P) { set_error("%s: P must lie in [1, 64]", fn); return 0; }
  if (L < 0 || L > O_MAX_L) { set_error("%s: L must lie in [0, 64]", fn); return 0; }
  if (L == 0 && !with_boxes) { set_error("%s: no bones and no boxes: nothing to draw", fn); return 0; }
  if ((long)B * P * (3L * L + 4) >= (1L << 31)) { set_error("%s: B * P * (3 L + 4) >= 2^31", fn); return 0; }
  return 1;
}

extern "C" int p2m_pose_overlay_workspace(int32_t B, int32_t P, int32_t L, int32_t with_boxes, int64_t* bytes_out) {
  P2M_CHECK_ARG(bytes_out, "null pointer");
  if (!overlay_shape_ok(B, P, L, with_boxes, __func__)) return P2M_ERR_INVALID;
  const long n = (long)B * P * (3L * L + (with_boxes ? 4 : 0));
  *bytes_out = overlay_box_bytes(n) + n * (int64_t)sizeof(int4) + 16;
  return P2M_OK;
}

extern "C" int p2m_pose_overlay(const float* poses, int32_t B, int32_t P, int32_t J, int32_t C, const int32_t* bones, int32_t L,
                                const uint8_t* colours, int32_t colour_mode, const float* boxes, uint32_t box_rgb,
                                const uint8_t* src, uint8_t* dst, int32_t H, int32_t W, float thr, int32_t line_h2,
                                int32_t mark_h2, int32_t mark_r16, int32_t box_h2, int32_t alpha256, int32_t* status,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  P2M_CHECK_ARG(poses && src && dst && workspace, "null pointer");
  P2M_CHECK_ARG(L <= 0 || (bones && colours), "null pointer");
  if (!overlay_shape_ok(B, P, L, boxes != nullptr, __func__)) return P2M_ERR_INVALID;
  P2M_CHECK_ARG(H >= 1 && H <= O_MAX_DIM && W >= 1 && W <= O_MAX_DIM, "H, W must lie in [1, 8192]");
  P2M_CHECK_ARG(J >= 1 && J <= O_MAX_J, "J must lie in [1, 64]");
  P2M_CHECK_ARG(C == 2 || C == 3, "C must be 2 or 3");
  P2M_CHECK_ARG(colour_mode == 0 || colour_mode == 1, "colour_mode: 0 per bone, 1 per person");
  P2M_CHECK_ARG(line_h2 >= 0 && line_h2 <= O_MAX_H2 && mark_h2 >= 0 && mark_h2 <= O_MAX_H2 && box_h2 >= 0 && box_h2 <= O_MAX_H2,
                "a thickness (half pixels) must lie in [0, 64]");
  P2M_CHECK_ARG(mark_r16 >= -1 && mark_r16 <= O_MAX_R16, "mark_r16: -1 (disc) or a ring radius in [0, 1024] sixteenths");
  P2M_CHECK_ARG(alpha256 >= 0 && alpha256 <= 256, "alpha256 must lie in [0, 256]");
  const int S = 3 * L + (boxes ? 4 : 0);
  const long n = (long)B * P * S;
  const int tiles_x = cdiv(W, O_TILE), tiles_y = cdiv(H, O_TILE);
  P2M_CHECK_ARG((long)B * tiles_x * tiles_y < (1L << 31), "image batch too large");
  P2M_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  P2M_CHECK_ARG(workspace_bytes >= overlay_box_bytes(n) + n * (int64_t)sizeof(int4) + 16, "workspace too small");
  if (B == 0) return P2M_OK;
  hipStream_t s = (hipStream_t)stream;
  OverlaySetupArgs sa;
  sa.poses = poses; sa.bones = bones; sa.colours = colours; sa.boxes = boxes;
  sa.B = B; sa.P = P; sa.J = J; sa.C = C; sa.L = L; sa.S = S; sa.H = H; sa.W = W; sa.colour_mode = colour_mode;
  sa.has_boxes = boxes ? 1 : 0; sa.box_rgb = box_rgb; sa.thr = thr;
  sa.line_h2 = line_h2; sa.mark_h2 = mark_h2; sa.mark_r16 = mark_r16; sa.box_h2 = box_h2;
  char* w = (char*)workspace;
  sa.pbox = (short4*)w;
  sa.prec = (int4*)(w + overlay_box_bytes(n));
  sa.status = status;
  hipLaunchKernelGGL(k_overlay_setup, dim3(B * P), dim3(O_NT), 0, s, sa);
  OverlayTileArgs ta;
  ta.pbox = sa.pbox; ta.prec = sa.prec; ta.n_rec = P * S; ta.H = H; ta.W = W; ta.tiles_x = tiles_x; ta.tiles_y = tiles_y;
  ta.alpha256 = alpha256; ta.src = src; ta.dst = dst;
  hipLaunchKernelGGL(k_overlay_tile, dim3(B * tiles_x * tiles_y), dim3(O_NT), 0, s, ta);
  return check_launch("pose_overlay");
}
