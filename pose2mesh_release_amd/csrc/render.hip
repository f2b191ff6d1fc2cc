// Mesh rendering on the GPU (gfx950): a batched z-buffer rasteriser with flat shading and image overlay, the device
// counterpart of the reference's demo/renderer.py (trimesh + pyrender + OpenGL).  The reference's rendering code is not
// runnable without an OpenGL context, so the comment of p2m_mesh_render in include/p2m.h is the contract and
// tests/render_ref.py its float64 / exact-integer restatement.  Geometry follows the reference, shading is this project's.
//
// One memset node and two kernels per call, all on the caller's stream, no allocation, no sync, no data-dependent grid:
//   k_render_setup  one thread per (mesh, face): the fp64 projection of its three vertices (one fma per coordinate) snapped
//                   to 1/256 pixel, orientation and culling from the exact integer area, the clipped pixel bbox as 4 x int16,
//                   the fp64 face normal -> intensity -> packed RGB, a 48-byte record per kept face, the per-mesh pixel bbox
//                   (wave-reduced, one integer atomicMin per wave and component) and the status bits.
//   k_render_tile   one block per 64 x 64-pixel tile of an image: 32 KB of 64-bit keys in LDS.  It scans the 8-byte bbox
//                   records of every mesh whose bbox meets the tile (a plain scan: capacity-free, never drops a face),
//                   compacts the hits per wave with a ballot into a block queue, and rasterises a full queue with one lane
//                   per face (faces whose clipped bbox is larger go to the whole block, pixel by pixel).  Edge functions are
//                   exact int64; the visible fragment is the 64-bit atomicMin IN LDS of a packed key (order-preserving bits
//                   of the fp32 depth, mesh rank, face id): no float atomics, no global atomics, and min does not depend on
//                   the order of arrival, so the result is reproducible bit for bit.  The tile is then resolved to the
//                   outputs row by row.
//   k_render_project  (p2m_mesh_project) one thread per (mesh, vertex): the same projection and snap, for callers and tests.
#include "p2m_render.h"

namespace p2m {

constexpr int R_NT = 256;             // threads per block
constexpr int R_TILE = 64;            // tile edge in pixels: 4096 keys x 8 B = 32 KB of LDS
constexpr int R_QCAP = 2 * R_NT;      // queue of hit faces: flushed as soon as a scan step could overflow it
constexpr int R_BIG = 256;            // clipped bbox pixels above which a face is rasterised by the whole block

struct FaceRec {                      // 48 bytes: three 16-byte loads
  int x0, y0, x1, y1;
  int x2, y2; float z0, z1;
  float z2; unsigned rgb; int pad0, pad1;
};

// ---- projection and snap: cam_coef / snap of p2m_render.h (shared with shade.hip: bitwise the same) -----------------------
__global__ __launch_bounds__(R_NT) void k_render_project(const float* __restrict__ verts, const float* __restrict__ cam, int B,
                                                         int nv, int H, int W, int* __restrict__ xy_fix,
                                                         int* __restrict__ status) {
  const long i = (long)blockIdx.x * R_NT + threadIdx.x;
  bool clamped = false;
  int m = 0;
  if (i < (long)B * nv) {
    m = (int)(i / nv);
    const CamCoef c = cam_coef(cam + 4 * m, H, W);
    xy_fix[2 * i] = snap(c.ax, (double)verts[3 * i], c.bx, clamped);
    xy_fix[2 * i + 1] = snap(c.ay, (double)verts[3 * i + 1], c.by, clamped);
  }
  if (status && clamped) atomicOr(&status[m], R_STATUS_CLAMPED);         // (rare: a vertex 32 768 pixels off the image)
}

// ---- per-face setup --------------------------------------------------------------------------------------------------
struct SetupArgs {
  const float* verts; const int* faces; const float* cam; const float* colours;
  int B, nv, nf, H, W, cull;
  Lights L;
  short4* fbox;                       // [B][nf]  pixel bbox (x0, y0, x1, y1), inclusive, clipped to the image; empty: x0 > x1
  FaceRec* frec;                      // [B][nf]  written for kept faces only
  int* mbox;                          // [B][4]   min x0, min y0, min -x1, min -y1 over the kept faces (memset to 0x7f bytes)
  int* status;                        // [B] or NULL
};

__global__ __launch_bounds__(R_NT) void k_render_setup(SetupArgs a) {
  const int m = blockIdx.y;
  const int f = blockIdx.x * R_NT + threadIdx.x;
  int bx0 = 32767, by0 = 32767, bx1 = -1, by1 = -1, st = 0;
  if (f < a.nf) {
    const int* fi = a.faces + 3 * (long)f;
    const unsigned i0 = (unsigned)fi[0], i1 = (unsigned)fi[1], i2 = (unsigned)fi[2];
    if (i0 >= (unsigned)a.nv || i1 >= (unsigned)a.nv || i2 >= (unsigned)a.nv) {
      st = R_STATUS_BAD_INDEX;                                           // never read: the face covers nothing
    } else {
      const float* v = a.verts + (long)m * a.nv * 3;
      const float p[3][3] = {{v[3 * i0], v[3 * i0 + 1], v[3 * i0 + 2]}, {v[3 * i1], v[3 * i1 + 1], v[3 * i1 + 2]},
                             {v[3 * i2], v[3 * i2 + 1], v[3 * i2 + 2]}};
      const CamCoef c = cam_coef(a.cam + 4 * m, a.H, a.W);
      bool clamped = false;
      int x[3], y[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        x[k] = snap(c.ax, (double)p[k][0], c.bx, clamped);
        y[k] = snap(c.ay, (double)p[k][1], c.by, clamped);
      }
      if (clamped) st = R_STATUS_CLAMPED;
      const long area2 = (long)(x[1] - x[0]) * (y[2] - y[0]) - (long)(x[2] - x[0]) * (y[1] - y[0]);
      // screen area = ax ay n_z: front (normal towards -z in mesh coordinates) <=> area2 sgn(ax ay) < 0
      const bool mirror = (c.ax < 0.0) != (c.ay < 0.0);
      const bool front = mirror ? area2 > 0 : area2 < 0;
      if (area2 != 0 && (front || !a.cull)) {
        const int xmin = min(x[0], min(x[1], x[2])), xmax = max(x[0], max(x[1], x[2]));
        const int ymin = min(y[0], min(y[1], y[2])), ymax = max(y[0], max(y[1], y[2]));
        // pixels whose centre 256 j + 128 lies in [min, max] (>> of a negative int is arithmetic: floor)
        const int jx0 = max((xmin - R_FIX / 2 + R_FIX - 1) >> 8, 0), jx1 = min((xmax - R_FIX / 2) >> 8, a.W - 1);
        const int jy0 = max((ymin - R_FIX / 2 + R_FIX - 1) >> 8, 0), jy1 = min((ymax - R_FIX / 2) >> 8, a.H - 1);
        if (jx0 <= jx1 && jy0 <= jy1) {
          bx0 = jx0; by0 = jy0; bx1 = jx1; by1 = jy1;
          const double I = face_intensity(p, a.L);                      // flat shading (p2m_render.h)
          const float* col = a.colours + 3 * m;
          FaceRec r;
          r.x0 = x[0]; r.y0 = y[0]; r.x1 = x[1]; r.y1 = y[1]; r.x2 = x[2]; r.y2 = y[2];
          r.z0 = p[0][2]; r.z1 = p[1][2]; r.z2 = p[2][2];
          r.rgb = to_u8((double)col[0] * I) | (to_u8((double)col[1] * I) << 8) | (to_u8((double)col[2] * I) << 16);
          r.pad0 = 0; r.pad1 = 0;
          a.frec[(long)m * a.nf + f] = r;
        }
      }
    }
    a.fbox[(long)m * a.nf + f] = make_short4((short)bx0, (short)by0, (short)bx1, (short)by1);
  }
  // per-mesh bbox and status: reduced over the wave first, then one atomic per wave and component
  int q[4] = {bx0, by0, -bx1, -by1};
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = min(q[k], __shfl_xor(q[k], o));
    st |= __shfl_xor(st, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (q[0] <= -q[2]) {
#pragma unroll
      for (int k = 0; k < 4; k++) atomicMin(&a.mbox[4 * m + k], q[k]);
    }
    if (st && a.status) atomicOr(&a.status[m], st);
  }
}

// ---- tiles -------------------------------------------------------------------------------------------------------------
struct TileArgs {
  const short4* fbox; const FaceRec* frec; const int* mbox;
  int B, nf, H, W, scene, list_order, vec;
  float zmin, zmax;
  const unsigned char* bg; int bg_per_mesh;
  unsigned char* image; int* face_id; int* mesh_id; float* depth;
};

__device__ __forceinline__ FaceRec load_rec(const FaceRec* p) {
  const int4* q = reinterpret_cast<const int4*>(p);
  const int4 a = q[0], b = q[1], c = q[2];
  FaceRec r;
  r.x0 = a.x; r.y0 = a.y; r.x1 = a.z; r.y1 = a.w;
  r.x2 = b.x; r.y2 = b.y; r.z0 = __int_as_float(b.z); r.z1 = __int_as_float(b.w);
  r.z2 = __int_as_float(c.x); r.rgb = (unsigned)c.y; r.pad0 = 0; r.pad1 = 0;
  return r;
}

// The three edge functions of a face, oriented so that the interior is E > 0:  E_k(p) = A_k (px - xa_k) + B_k (py - ya_k) for
// the edge a_k -> b_k (k = 0: v0 -> v1, 1: v1 -> v2, 2: v2 -> v0), A_k = -s (yb - ya), B_k = s (xb - xa), s = sgn(area2).
// Top-left rule: a centre with E_k = 0 belongs to the face only on a left edge (A_k > 0) or a top edge (A_k = 0, B_k > 0);
// bias_k = 0 for those and -1 for the others, and the pixel is covered iff E_k + bias_k >= 0 for all k.
struct Edges {
  long A[3], Bc[3], C[3];             // E_k(px, py) = A px + Bc py + C   (bias not included)
  long bias[3];
  float area;                         // (float)|area2|
  float z0, d1, d2;                   // z0, z1 - z0, z2 - z0 (fp32)
};

__device__ __forceinline__ Edges make_edges(const FaceRec& r) {
  const long xs[3] = {r.x0, r.x1, r.x2}, ys[3] = {r.y0, r.y1, r.y2};
  const long area2 = (xs[1] - xs[0]) * (ys[2] - ys[0]) - (xs[2] - xs[0]) * (ys[1] - ys[0]);
  const long s = area2 < 0 ? -1 : 1;
  Edges e;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int kb = k == 2 ? 0 : k + 1;
    e.A[k] = -s * (ys[kb] - ys[k]);
    e.Bc[k] = s * (xs[kb] - xs[k]);
    e.C[k] = -(e.A[k] * xs[k] + e.Bc[k] * ys[k]);
    e.bias[k] = (e.A[k] > 0 || (e.A[k] == 0 && e.Bc[k] > 0)) ? 0 : -1;
  }
  e.area = (float)(s * area2);
  e.z0 = r.z0; e.d1 = r.z1 - r.z0; e.d2 = r.z2 - r.z0;
  return e;
}

__device__ __forceinline__ unsigned depth_bits(float d) {                // order-preserving: smaller float <=> smaller unsigned
  const unsigned u = __float_as_uint(d);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bits_depth(unsigned b) {
  return __uint_as_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b);
}

// One covered pixel: E0, E2 are the unbiased edge values (the weights of v2 and v1).  depth = fma(l2, z2 - z0, fma(l1, z1 - z0,
// z0)) with l1 = (float)E2 / (float)|area2|, l2 = (float)E0 / (float)|area2|, every operation in fp32.
__device__ __forceinline__ void emit(unsigned long long* keys, int li, const Edges& e, long E0, long E2, float zmin, float zmax,
                                     unsigned long long key_lo, int list_order) {
  const float l1 = (float)E2 / e.area, l2 = (float)E0 / e.area;
  const float d = fmaf(l2, e.d2, fmaf(l1, e.d1, e.z0));
  if (d >= zmin && d <= zmax) {
    const unsigned long long db = depth_bits(d);
    const unsigned long long key = list_order ? (key_lo | (db << 24)) : (key_lo | (db << 32));
    atomicMin(&keys[li], key);
  }
}

__global__ __launch_bounds__(R_NT) void k_render_tile(TileArgs a) {
  __shared__ unsigned long long keys[R_TILE * R_TILE];
  __shared__ int queue[R_QCAP];
  __shared__ int big[R_QCAP];
  __shared__ int wcnt[2][R_NT / 64];
  __shared__ int bn;
  const int tid = threadIdx.x, lane = tid & 63;
  const int img = blockIdx.z;
  const int tx0 = blockIdx.x * R_TILE, ty0 = blockIdx.y * R_TILE;
  const int tx1 = min(tx0 + R_TILE, a.W) - 1, ty1 = min(ty0 + R_TILE, a.H) - 1;
  for (int i = tid; i < R_TILE * R_TILE; i += R_NT) keys[i] = ~0ull;
  if (tid == 0) bn = 0;
  __syncthreads();
  const int m_begin = a.scene ? 0 : img, m_end = a.scene ? a.B : img + 1;
  for (int m = m_begin; m < m_end; m++) {
    const int* mb = a.mbox + 4 * m;
    if (mb[0] > tx1 || -mb[2] < tx0 || mb[1] > ty1 || -mb[3] < ty0) continue;     // (uniform over the block)
    const short4* fbox = a.fbox + (long)m * a.nf;
    const FaceRec* frec = a.frec + (long)m * a.nf;
    const unsigned rank = a.scene ? (unsigned)m : 0u;
    // list order: the later mesh wins, then the nearer fragment, then the lower face id; depth order: nearer, rank, face id
    const unsigned long long key_m = a.list_order ? ((unsigned long long)(255u - rank) << 56) : ((unsigned long long)rank << 24);
    int nq = 0;                                                          // entries in the queue (the same in every thread)
    for (int f0 = 0, step = 0; f0 < a.nf; f0 += R_NT, step++) {
      {
        const int f = f0 + tid;
        bool hit = false;
        if (f < a.nf) {
          const short4 bb = fbox[f];
          hit = bb.x <= tx1 && bb.z >= tx0 && bb.y <= ty1 && bb.w >= ty0;
        }
        // compaction: a ballot per wave, the waves' counts through LDS (two buffers: the next step's writes cannot
        // overtake this step's reads), a fixed order of the entries
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) wcnt[step & 1][tid >> 6] = __popcll(bal);
        __syncthreads();
        int base = nq, total = 0;
#pragma unroll
        for (int w = 0; w < R_NT / 64; w++) {
          const int c = wcnt[step & 1][w];
          base += w < (tid >> 6) ? c : 0;
          total += c;
        }
        if (hit) queue[base + __popcll(bal & ((1ull << lane) - 1ull))] = f;
        nq += total;
        if (nq <= R_QCAP - R_NT && f0 + R_NT < a.nf) continue;          // room for another step, and faces left to scan
        __syncthreads();
      }
      // ---- rasterise the queue: one lane per face, large faces handed to the whole block ----
      const int n = nq;
      for (int e = tid; e < n; e += R_NT) {
        const int f = queue[e];
        const short4 bb = fbox[f];
        const int xa = max((int)bb.x, tx0), xb = min((int)bb.z, tx1), ya = max((int)bb.y, ty0), yb = min((int)bb.w, ty1);
        if ((xb - xa + 1) * (yb - ya + 1) > R_BIG) {
          big[atomicAdd(&bn, 1)] = f;
          continue;
        }
        const Edges ed = make_edges(load_rec(frec + f));
        const unsigned long long key_lo = key_m | (unsigned long long)f;
        const long px0 = (long)xa * R_FIX + R_FIX / 2;
        for (int y = ya; y <= yb; y++) {
          const long py = (long)y * R_FIX + R_FIX / 2;
          long E0 = ed.A[0] * px0 + ed.Bc[0] * py + ed.C[0];
          long E1 = ed.A[1] * px0 + ed.Bc[1] * py + ed.C[1];
          long E2 = ed.A[2] * px0 + ed.Bc[2] * py + ed.C[2];
          for (int x = xa; x <= xb; x++) {
            if (((E0 + ed.bias[0]) | (E1 + ed.bias[1]) | (E2 + ed.bias[2])) >= 0)
              emit(keys, (y - ty0) * R_TILE + (x - tx0), ed, E0, E2, a.zmin, a.zmax, key_lo, a.list_order);
            E0 += ed.A[0] * R_FIX; E1 += ed.A[1] * R_FIX; E2 += ed.A[2] * R_FIX;
          }
        }
      }
      __syncthreads();
      const int nb = bn;
      for (int e = 0; e < nb; e++) {
        const int f = big[e];
        const short4 bb = fbox[f];
        const int xa = max((int)bb.x, tx0), xb = min((int)bb.z, tx1), ya = max((int)bb.y, ty0), yb = min((int)bb.w, ty1);
        const int w = xb - xa + 1, npx = w * (yb - ya + 1);
        const Edges ed = make_edges(load_rec(frec + f));
        const unsigned long long key_lo = key_m | (unsigned long long)f;
        for (int i = tid; i < npx; i += R_NT) {
          const int y = ya + i / w, x = xa + i % w;
          const long px = (long)x * R_FIX + R_FIX / 2, py = (long)y * R_FIX + R_FIX / 2;
          const long E0 = ed.A[0] * px + ed.Bc[0] * py + ed.C[0];
          const long E1 = ed.A[1] * px + ed.Bc[1] * py + ed.C[1];
          const long E2 = ed.A[2] * px + ed.Bc[2] * py + ed.C[2];
          if (((E0 + ed.bias[0]) | (E1 + ed.bias[1]) | (E2 + ed.bias[2])) >= 0)
            emit(keys, (y - ty0) * R_TILE + (x - tx0), ed, E0, E2, a.zmin, a.zmax, key_lo, a.list_order);
        }
      }
      __syncthreads();
      nq = 0;
      if (tid == 0) bn = 0;                                              // (next touched behind the next step's barrier)
    }
  }
  __syncthreads();
  // ---- resolve: a lane takes 4 neighbouring pixels of a row (16 lanes per 64-pixel row segment, 16 rows per pass); every
  // load of a pass is issued before its stores.  vec (W % 4 = 0 and aligned planes): 16-byte stores per plane and three
  // dwords of image per lane; otherwise pixel by pixel ----
  const long img_px = (long)img * a.H * a.W;
  const unsigned char* bg = a.bg ? a.bg + (a.bg_per_mesh ? img_px * 3 : 0) : nullptr;
  for (int pass = 0; pass < R_TILE / 16; pass++) {
    const int ly = pass * 16 + (tid >> 4), lx = (tid & 15) * 4;
    const int x = tx0 + lx, y = ty0 + ly;
    if (x > tx1 || y > ty1) continue;
    const int nx = min(4, tx1 - x + 1);                                  // (vec: always 4)
    const long o = (long)y * a.W + x;
    int f4[4], m4[4];
    float d4[4];
    unsigned rgb4[4];
    bool cov[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const unsigned long long key = keys[ly * R_TILE + lx + j];
      cov[j] = key != ~0ull;
      f4[j] = -1; m4[j] = -1; d4[j] = __builtin_inff(); rgb4[j] = 0;
      if (cov[j]) {
        f4[j] = (int)(key & 0xffffffu);
        unsigned rank, db;
        if (a.list_order) { rank = 255u - (unsigned)(key >> 56); db = (unsigned)(key >> 24); }
        else { rank = (unsigned)(key >> 24) & 0xffu; db = (unsigned)(key >> 32); }
        m4[j] = a.scene ? (int)rank : img;
        d4[j] = bits_depth(db);
        rgb4[j] = a.frec[(long)m4[j] * a.nf + f4[j]].rgb;
      }
    }
    if (a.vec) {
      if (bg) {
        const unsigned* bw = reinterpret_cast<const unsigned*>(bg + 3 * o);
        const unsigned b0 = bw[0], b1 = bw[1], b2 = bw[2];
        const unsigned bq[4] = {b0 & 0xffffffu, (b0 >> 24) | ((b1 & 0xffffu) << 8), (b1 >> 16) | ((b2 & 0xffu) << 16), b2 >> 8};
#pragma unroll
        for (int j = 0; j < 4; j++) rgb4[j] = cov[j] ? rgb4[j] : bq[j];
      }
      if (a.image) {
        unsigned* ow = reinterpret_cast<unsigned*>(a.image + (img_px + o) * 3);
        ow[0] = rgb4[0] | (rgb4[1] << 24);
        ow[1] = (rgb4[1] >> 8) | (rgb4[2] << 16);
        ow[2] = (rgb4[2] >> 16) | (rgb4[3] << 8);
      }
      if (a.face_id) *reinterpret_cast<int4*>(a.face_id + img_px + o) = make_int4(f4[0], f4[1], f4[2], f4[3]);
      if (a.mesh_id) *reinterpret_cast<int4*>(a.mesh_id + img_px + o) = make_int4(m4[0], m4[1], m4[2], m4[3]);
      if (a.depth) *reinterpret_cast<float4*>(a.depth + img_px + o) = make_float4(d4[0], d4[1], d4[2], d4[3]);
    } else {
      if (bg) {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (j < nx && !cov[j]) rgb4[j] = bg[3 * (o + j)] | (bg[3 * (o + j) + 1] << 8) | (bg[3 * (o + j) + 2] << 16);
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (j >= nx) continue;
        if (a.image) {
          unsigned char* out = a.image + (img_px + o + j) * 3;
          out[0] = (unsigned char)(rgb4[j] & 0xffu); out[1] = (unsigned char)((rgb4[j] >> 8) & 0xffu);
          out[2] = (unsigned char)(rgb4[j] >> 16);
        }
        if (a.face_id) a.face_id[img_px + o + j] = f4[j];
        if (a.mesh_id) a.mesh_id[img_px + o + j] = m4[j];
        if (a.depth) a.depth[img_px + o + j] = d4[j];
      }
    }
  }
}

static inline long render_rec_bytes(long B, long nf) { return ((B * nf * 8 + 15) & ~15L); }

}  // namespace p2m

using namespace p2m;

static int render_shape_ok(int32_t B, int32_t nf, int32_t H, int32_t W, int32_t mode, const char* fn) {
  if (B < 0 || nf < 1) { set_error("%s: bad batch / face count", fn); return 0; }
  if (nf >= (1 << 24)) { set_error("%s: nf >= 2^24 (the face id has 24 bits of the key)", fn); return 0; }
  if (mode != 0 && mode != 1) { set_error("%s: mode: 0 batch, 1 scene", fn); return 0; }
  if (mode == 1 && B > 255) { set_error("%s: more than 255 meshes in scene mode (the rank has 8 bits of the key)", fn); return 0; }
  if (B > 65535) { set_error("%s: more than 65535 meshes", fn); return 0; }
  if (H < 1 || H > R_MAX_DIM || W < 1 || W > R_MAX_DIM) { set_error("%s: H, W must lie in [1, 8192]", fn); return 0; }
  if ((long)B * nf >= (1L << 31)) { set_error("%s: B * nf >= 2^31", fn); return 0; }
  return 1;
}

extern "C" int p2m_mesh_project(const float* verts, const float* cam, int32_t B, int32_t nv, int32_t H, int32_t W,
                                int32_t* xy_fix, int32_t* status, void* stream) {
  P2M_CHECK_ARG(verts && cam && xy_fix, "null pointer");
  P2M_CHECK_ARG(B >= 0 && nv >= 1, "bad batch / vertex count");
  P2M_CHECK_ARG(H >= 1 && H <= R_MAX_DIM && W >= 1 && W <= R_MAX_DIM, "H, W must lie in [1, 8192]");
  P2M_CHECK_ARG((long)B * nv * 3 < (1L << 31), "more than 2^31 coordinates");
  if (B == 0) return P2M_OK;
  hipStream_t s = (hipStream_t)stream;
  if (status && hipMemsetAsync(status, 0, sizeof(int32_t) * B, s) != hipSuccess) return check_launch("mesh_project");
  hipLaunchKernelGGL(k_render_project, dim3(cdiv((long)B * nv, R_NT)), dim3(R_NT), 0, s, verts, cam, B, nv, H, W, xy_fix,
                     status);
  return check_launch("mesh_project");
}

extern "C" int p2m_mesh_render_workspace(int32_t B, int32_t nf, int32_t H, int32_t W, int32_t mode, int64_t* bytes_out) {
  P2M_CHECK_ARG(bytes_out, "null pointer");
  if (!render_shape_ok(B, nf, H, W, mode, __func__)) return P2M_ERR_INVALID;
  *bytes_out = render_rec_bytes(B, nf) + (int64_t)B * nf * sizeof(FaceRec) + (int64_t)B * 16 + 16;
  return P2M_OK;
}

extern "C" int p2m_mesh_render(const float* verts, const int32_t* faces, int32_t nf, const float* cam, const float* colours,
                               const float* lights, int32_t nl, float ambient, float zmin, float zmax, int32_t flags,
                               const uint8_t* background, int32_t bg_per_mesh, int32_t B, int32_t nv, int32_t H, int32_t W,
                               int32_t mode, uint8_t* image, int32_t* face_id, int32_t* mesh_id, float* depth,
                               int32_t* status, void* workspace, void* stream) {
  P2M_CHECK_ARG(verts && faces && cam && colours && workspace, "null pointer");
  P2M_CHECK_ARG(nl >= 0 && nl <= R_MAX_LIGHTS, "0..4 lights");
  P2M_CHECK_ARG(nl == 0 || lights, "null pointer");
  if (!render_shape_ok(B, nf, H, W, mode, __func__)) return P2M_ERR_INVALID;
  P2M_CHECK_ARG(nv >= 1 && (long)B * nv * 3 < (1L << 31), "bad vertex count");
  P2M_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  P2M_CHECK_ARG(!(mode == 1 && bg_per_mesh), "scene mode has one image: one background");
  P2M_CHECK_ARG((flags & ~3) == 0, "flags: bit 0 cull back faces, bit 1 depth order");
  const int n_img = mode == 1 ? 1 : B;
  P2M_CHECK_ARG((long)n_img * H * W * 3 < (1L << 40), "image batch too large");
  if (B == 0) return P2M_OK;
  hipStream_t s = (hipStream_t)stream;
  SetupArgs sa;
  sa.verts = verts; sa.faces = faces; sa.cam = cam; sa.colours = colours;
  sa.B = B; sa.nv = nv; sa.nf = nf; sa.H = H; sa.W = W; sa.cull = flags & 1;
  P2M_CHECK_ARG(lights_from_host(lights, nl, ambient, sa.L), "a light direction must be non-zero and finite");
  char* w = (char*)workspace;
  sa.fbox = (short4*)w;
  sa.frec = (FaceRec*)(w + render_rec_bytes(B, nf));
  sa.mbox = (int*)(w + render_rec_bytes(B, nf) + (long)B * nf * sizeof(FaceRec));
  sa.status = status;
  if (hipMemsetAsync(sa.mbox, 0x7f, sizeof(int) * 4 * B, s) != hipSuccess) return check_launch("mesh_render");
  if (status && hipMemsetAsync(status, 0, sizeof(int32_t) * B, s) != hipSuccess) return check_launch("mesh_render");
  hipLaunchKernelGGL(k_render_setup, dim3(cdiv(nf, R_NT), B), dim3(R_NT), 0, s, sa);
  if (image || face_id || mesh_id || depth) {
    TileArgs ta;
    ta.fbox = sa.fbox; ta.frec = sa.frec; ta.mbox = sa.mbox;
    ta.B = B; ta.nf = nf; ta.H = H; ta.W = W; ta.scene = mode == 1; ta.list_order = (mode == 1 && !(flags & 2)) ? 1 : 0;
    ta.zmin = zmin; ta.zmax = zmax; ta.bg = background; ta.bg_per_mesh = bg_per_mesh;
    ta.image = image; ta.face_id = face_id; ta.mesh_id = mesh_id; ta.depth = depth;
    ta.vec = (W & 3) == 0 && (((uintptr_t)face_id | (uintptr_t)mesh_id | (uintptr_t)depth) & 15) == 0 &&
             (((uintptr_t)image | (uintptr_t)background) & 3) == 0;
    hipLaunchKernelGGL(k_render_tile, dim3(cdiv(W, R_TILE), cdiv(H, R_TILE), n_img), dim3(R_NT), 0, s, ta);
  }
  return check_launch("mesh_render");
}
