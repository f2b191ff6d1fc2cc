// Deferred shading of a visibility buffer (gfx950): what p2m_mesh_render's face_id / mesh_id are for.  The comments of
// p2m_vertex_normals and p2m_mesh_shade in include/p2m.h are the contract, tests/shade_ref.py their numpy restatement.
// Built with -ffp-contract=off: the contract states the fp64 and fp32 arithmetic one rounding at a time.  The pieces that must
// match the rasteriser bit for bit (projection, snap, flat intensity, byte rounding) come from p2m_render.h.
//
// One memset node and one kernel per call, on the caller's stream, no allocation, no sync, grids from shapes only:
//   k_vertex_normals  one thread per (mesh, vertex): a GATHER over the vertex's incident faces in table order (no float atomics:
//                     the sum has one order, whatever the batch).  The face list and the vertices of a mesh (SMPL: 165 KB +
//                     83 KB) stay in L2 across the block's reads; each face's cross product is recomputed by its three
//                     vertices, which costs fp64 flops the kernel has to spare and saves a workspace and a second launch.
//                     The kernel waits on chains of dependent 4-byte loads (table -> face -> vertices), so it wants threads:
//                     four meshes per thread (indices read once for the four) measured 1.6 to 2.4 times slower.
//   k_mesh_shade      one lane per 4 neighbouring pixels of a row.  The ids come as one 16-byte load per plane where the row
//                     allows; a lane whose four pixels are background leaves after copying the background.  A covered pixel
//                     sets its face up (gathers from L2, fp64 projection and snap, integer edges) unless its left neighbour in
//                     the lane shows the same face, evaluates the integer edge functions at its centre - every factor fits 32
//                     bits, so a term is one v_mad_i64_i32 - and derives barycentrics, attributes, the wire test (128-bit
//                     integers) and the fp64 shading from them, each only where an output needs it.  The lane's 12 image bytes
//                     leave as three dwords where the row's base allows, byte by byte otherwise.
#include "p2m_render.h"

namespace p2m {

constexpr int S_NT = 256;
constexpr int S_MAX_ATTR = 16;
constexpr int S_MAX_WIRE = 1 << 16;
constexpr int S_STATUS_DEGENERATE = 1, S_STATUS_BAD_INDEX = 2;

// ---- vertex normals ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(S_NT) void k_vertex_normals(const float* __restrict__ verts, const int* __restrict__ faces,
                                                         const int* __restrict__ vf_ptr, const int* __restrict__ vf_idx,
                                                         int n_idx, int nv, int nf, float* __restrict__ normals,
                                                         int* __restrict__ status) {
  const int m = blockIdx.y;
  const int v = blockIdx.x * S_NT + threadIdx.x;
  if (v >= nv) return;
  const float* vm = verts + (long)m * nv * 3;
  int st = 0;
  double n0 = 0.0, n1 = 0.0, n2 = 0.0;
  int e0 = vf_ptr[v], e1 = vf_ptr[v + 1];
  if (e0 < 0 || e1 > n_idx || e0 > e1) {                                 // a table that points outside itself: nothing is read
    st |= S_STATUS_BAD_INDEX;
    e0 = e1 = 0;
  }
  for (int e = e0; e < e1; e++) {
    const unsigned f = (unsigned)vf_idx[e];
    if (f >= (unsigned)nf) { st |= S_STATUS_BAD_INDEX; continue; }
    const int* fi = faces + 3 * (long)f;
    const unsigned i0 = (unsigned)fi[0], i1 = (unsigned)fi[1], i2 = (unsigned)fi[2];
    if (i0 >= (unsigned)nv || i1 >= (unsigned)nv || i2 >= (unsigned)nv) { st |= S_STATUS_BAD_INDEX; continue; }
    const double p0[3] = {(double)vm[3 * i0], (double)vm[3 * i0 + 1], (double)vm[3 * i0 + 2]};
    const double a[3] = {(double)vm[3 * i1] - p0[0], (double)vm[3 * i1 + 1] - p0[1], (double)vm[3 * i1 + 2] - p0[2]};
    const double b[3] = {(double)vm[3 * i2] - p0[0], (double)vm[3 * i2 + 1] - p0[1], (double)vm[3 * i2 + 2] - p0[2]};
    n0 += a[1] * b[2] - a[2] * b[1];
    n1 += a[2] * b[0] - a[0] * b[2];
    n2 += a[0] * b[1] - a[1] * b[0];
  }
  const double q = (n0 * n0 + n1 * n1) + n2 * n2;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f;
  if (q > 0.0 && q < __builtin_inf()) {
    const double len = __dsqrt_rn(q);
    o0 = (float)__ddiv_rn(n0, len); o1 = (float)__ddiv_rn(n1, len); o2 = (float)__ddiv_rn(n2, len);
  } else {
    st |= S_STATUS_DEGENERATE;
  }
  float* out = normals + ((long)m * nv + v) * 3;
  out[0] = o0; out[1] = o1; out[2] = o2;
  if (st && status) atomicOr(&status[m], st);                            // (rare: a broken mesh)
}

// ---- the shading pass --------------------------------------------------------------------------------------------------
struct ShadeArgs {
  const int* face_id; const int* mesh_id; const float* verts; const int* faces; const float* cam;
  const float* colours; const float* vcol; const float* normals; const float* attrs; const unsigned char* bg;
  int B, nv, nf, H, W, C, vcol_shared, bg_per_mesh, wire_T, wire_only, vec_ids, vec_img;
  unsigned wire_rgb;
  float attr_fill;
  Lights L;
  unsigned char* image; float* bary; float* attr_out; int* status;
};

struct FaceCtx {                      // one face of one mesh, as the pixels of a lane see it
  bool ok;
  bool back;
  unsigned i0, i1, i2;
  int xs[3], ys[3];                   // the snapped vertices
  int A[3], Bc[3];                    // E_k(P) = A_k (Px - Xa) + B_k (Py - Ya), the edge functions of include/p2m.h: every factor
                                      // fits 32 bits (|X|, |Y| <= 2^23, P < 2^22), so a term is ONE 32 x 32 -> 64-bit multiply-add
  float area;                         // (float)|area2|
  double I_flat;                      // the rasteriser's intensity of the face (flat shading only)
  unsigned rgb_flat;                  // and, with a mesh colour, its packed bytes
};

__device__ __forceinline__ unsigned pack_rgb(double r, double g, double b) {
  return to_u8(r) | (to_u8(g) << 8) | (to_u8(b) << 16);
}

// the rasteriser's flat intensity of face (i0, i1, i2) of mesh m
__device__ __forceinline__ double flat_intensity(const ShadeArgs& a, int m, const FaceCtx& c) {
  const float* v = a.verts + (long)m * a.nv * 3;
  const float p[3][3] = {{v[3 * c.i0], v[3 * c.i0 + 1], v[3 * c.i0 + 2]}, {v[3 * c.i1], v[3 * c.i1 + 1], v[3 * c.i1 + 2]},
                         {v[3 * c.i2], v[3 * c.i2 + 1], v[3 * c.i2 + 2]}};
  return face_intensity(p, a.L);
}

__device__ __forceinline__ void shade_setup(const ShadeArgs& a, int m, int f, FaceCtx& c) {
  c.ok = false;
  const int* fi = a.faces + 3 * (long)f;
  c.i0 = (unsigned)fi[0]; c.i1 = (unsigned)fi[1]; c.i2 = (unsigned)fi[2];
  if (c.i0 >= (unsigned)a.nv || c.i1 >= (unsigned)a.nv || c.i2 >= (unsigned)a.nv) return;
  const float* v = a.verts + (long)m * a.nv * 3;
  const float px[3] = {v[3 * c.i0], v[3 * c.i1], v[3 * c.i2]}, py[3] = {v[3 * c.i0 + 1], v[3 * c.i1 + 1], v[3 * c.i2 + 1]};
  const CamCoef cc = cam_coef(a.cam + 4 * m, a.H, a.W);
  bool clamped = false;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    c.xs[k] = snap(cc.ax, (double)px[k], cc.bx, clamped);
    c.ys[k] = snap(cc.ay, (double)py[k], cc.by, clamped);
  }
  const long area2 = (long)(c.xs[1] - c.xs[0]) * (c.ys[2] - c.ys[0]) - (long)(c.xs[2] - c.xs[0]) * (c.ys[1] - c.ys[0]);
  if (area2 == 0) return;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int kb = k == 2 ? 0 : k + 1;
    const int dy = c.ys[kb] - c.ys[k], dx = c.xs[kb] - c.xs[k];        // (|d| <= 2^24)
    c.A[k] = area2 < 0 ? dy : -dy;                                     // -s dy
    c.Bc[k] = area2 < 0 ? -dx : dx;                                    //  s dx
  }
  c.area = (float)(area2 < 0 ? -area2 : area2);
  const bool mirror = (cc.ax < 0.0) != (cc.ay < 0.0);
  c.back = !(mirror ? area2 > 0 : area2 < 0);
  c.I_flat = 0.0;
  c.rgb_flat = 0;
  if (a.image && !a.normals) {                                         // (with normals the flat value is the rare fall-back)
    c.I_flat = flat_intensity(a, m, c);
    if (a.colours) {
      const float* col = a.colours + 3 * m;
      c.rgb_flat = pack_rgb((double)col[0] * c.I_flat, (double)col[1] * c.I_flat, (double)col[2] * c.I_flat);
    }
  }
  c.ok = true;
}

// E^2 <= T^2 (A^2 + B^2), exactly: |E| < 2^50, the right side < 2^83
__device__ __forceinline__ bool on_wire(long E, int A, int Bc, unsigned long long T2) {
  const unsigned long long e = (unsigned long long)(E < 0 ? -E : E);
  const unsigned __int128 lhs = (unsigned __int128)e * e;
  const unsigned __int128 rhs = (unsigned __int128)T2 * (unsigned long long)((long)A * A + (long)Bc * Bc);
  return lhs <= rhs;
}

__global__ __launch_bounds__(S_NT) void k_mesh_shade(ShadeArgs a) {
  const int img = blockIdx.y;
  const int W4 = (a.W + 3) >> 2;
  const long li = (long)blockIdx.x * S_NT + threadIdx.x;
  if (li >= (long)a.H * W4) return;
  const int y = (int)(li / W4), x = (int)(li % W4) * 4;
  const int nx = min(4, a.W - x);                                        // (vec_ids, vec_img: always 4)
  const long img_px = (long)img * a.H * a.W, o = img_px + (long)y * a.W + x;
  int f4[4] = {-1, -1, -1, -1}, m4[4] = {-1, -1, -1, -1};
  if (a.vec_ids) {
    const int4 fq = *reinterpret_cast<const int4*>(a.face_id + o), mq = *reinterpret_cast<const int4*>(a.mesh_id + o);
    f4[0] = fq.x; f4[1] = fq.y; f4[2] = fq.z; f4[3] = fq.w;
    m4[0] = mq.x; m4[1] = mq.y; m4[2] = mq.z; m4[3] = mq.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (j < nx) { f4[j] = a.face_id[o + j]; m4[j] = a.mesh_id[o + j]; }
  }
  // the background of the lane's pixels, 24 bits each
  unsigned bq[4] = {0u, 0u, 0u, 0u};
  if (a.image && a.bg) {
    const unsigned char* bg = a.bg + 3 * (a.bg_per_mesh ? o : o - img_px);
    if (a.vec_img) {
      const unsigned* bw = reinterpret_cast<const unsigned*>(bg);
      const unsigned b0 = bw[0], b1 = bw[1], b2 = bw[2];
      bq[0] = b0 & 0xffffffu; bq[1] = (b0 >> 24) | ((b1 & 0xffffu) << 8); bq[2] = (b1 >> 16) | ((b2 & 0xffu) << 16); bq[3] = b2 >> 8;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (j < nx) bq[j] = bg[3 * j] | (bg[3 * j + 1] << 8) | (bg[3 * j + 2] << 16);
    }
  }
  unsigned long long lo = 0ull;                                          // the lane's 12 image bytes: pixel j at bit 24 j
  unsigned hi = 0u;
  bool bad = false;
  FaceCtx c;
  c.ok = false;
  int pm = -1, pf = -1;
  const unsigned long long T2 = (unsigned long long)a.wire_T * (unsigned long long)a.wire_T;
  // a flat image with a mesh colour and no wire is the face's packed bytes: no edge value is needed
  const bool need_e = a.bary || a.attr_out || (a.image && (a.vcol || a.normals || a.wire_T > 0));
#pragma unroll 1
  for (int j = 0; j < nx; j++) {
    const int f = j == 0 ? f4[0] : j == 1 ? f4[1] : j == 2 ? f4[2] : f4[3];
    const int m = j == 0 ? m4[0] : j == 1 ? m4[1] : j == 2 ? m4[2] : m4[3];
    unsigned rgb = j == 0 ? bq[0] : j == 1 ? bq[1] : j == 2 ? bq[2] : bq[3];
    bool covered = f >= 0;
    if (covered && (f >= a.nf || (unsigned)m >= (unsigned)a.B)) { covered = false; bad = true; }   // never used as an index
    if (covered) {
      if (m != pm || f != pf) { shade_setup(a, m, f, c); pm = m; pf = f; }
      if (!c.ok) { covered = false; bad = true; }
    }
    float l0 = 0.f, l1 = 0.f, l2 = 0.f;
    if (covered) {
      long E0 = 0, E1 = 0, E2 = 0;
      if (need_e) {
        const int px = (x + j) * R_FIX + R_FIX / 2, py = y * R_FIX + R_FIX / 2;
        E0 = (long)c.A[0] * (px - c.xs[0]) + (long)c.Bc[0] * (py - c.ys[0]);
        E1 = (long)c.A[1] * (px - c.xs[1]) + (long)c.Bc[1] * (py - c.ys[1]);
        E2 = (long)c.A[2] * (px - c.xs[2]) + (long)c.Bc[2] * (py - c.ys[2]);
        l0 = (float)E1 / c.area; l1 = (float)E2 / c.area; l2 = (float)E0 / c.area;
      }
      if (a.image) {
        bool wire = false;
        if (a.wire_T > 0)
          wire = on_wire(E0, c.A[0], c.Bc[0], T2) || on_wire(E1, c.A[1], c.Bc[1], T2) || on_wire(E2, c.A[2], c.Bc[2], T2);
        if (wire) {
          rgb = a.wire_rgb;
        } else if (a.wire_T > 0 && a.wire_only) {
          // the background stays
        } else if (!a.vcol && !a.normals) {
          rgb = c.rgb_flat;
        } else {
          const double d0 = (double)l0, d1 = (double)l1, d2 = (double)l2;
          double I = c.I_flat;
          bool lit = !a.normals;
          if (a.normals) {
            const float* nm = a.normals + (long)m * a.nv * 3;
            const float* q0 = nm + 3 * (long)c.i0; const float* q1 = nm + 3 * (long)c.i1; const float* q2 = nm + 3 * (long)c.i2;
            const double mx = (d0 * (double)q0[0] + d1 * (double)q1[0]) + d2 * (double)q2[0];
            const double my = (d0 * (double)q0[1] + d1 * (double)q1[1]) + d2 * (double)q2[1];
            const double mz = (d0 * (double)q0[2] + d1 * (double)q1[2]) + d2 * (double)q2[2];
            const double q = (mx * mx + my * my) + mz * mz;
            if (q > 0.0 && q < __builtin_inf()) {
              const double len = __dsqrt_rn(q);
              double ux = __ddiv_rn(mx, len), uy = __ddiv_rn(my, len), uz = __ddiv_rn(mz, len);
              if (c.back) { ux = -ux; uy = -uy; uz = -uz; }
              I = a.L.ambient;
              lit = true;
#pragma unroll
              for (int l = 0; l < R_MAX_LIGHTS; l++) {
                if (l < a.L.nl) {
                  const double d = (ux * a.L.dir[l][0] + uy * a.L.dir[l][1]) + uz * a.L.dir[l][2];
                  I += a.L.k[l] * (d > 0.0 ? d : 0.0);
                }
              }
            }
          }
          if (!lit) I = flat_intensity(a, m, c);                        // a vanishing interpolated normal: the face's own
          double cr, cg, cb;
          if (a.vcol) {
            const float* vc = a.vcol + (a.vcol_shared ? 0 : (long)m * a.nv * 3);
            const float* c0 = vc + 3 * (long)c.i0; const float* c1 = vc + 3 * (long)c.i1; const float* c2 = vc + 3 * (long)c.i2;
            cr = (d0 * (double)c0[0] + d1 * (double)c1[0]) + d2 * (double)c2[0];
            cg = (d0 * (double)c0[1] + d1 * (double)c1[1]) + d2 * (double)c2[1];
            cb = (d0 * (double)c0[2] + d1 * (double)c1[2]) + d2 * (double)c2[2];
          } else {
            const float* col = a.colours + 3 * m;
            cr = (double)col[0]; cg = (double)col[1]; cb = (double)col[2];
          }
          rgb = pack_rgb(cr * I, cg * I, cb * I);
        }
      }
    }
    if (a.image) {
      if (a.vec_img) {
        const int sh = 24 * j;
        if (sh < 64) lo |= (unsigned long long)rgb << sh;
        if (sh == 48) hi |= rgb >> 16;
        if (sh == 72) hi |= rgb << 8;
      } else {
        unsigned char* out = a.image + (o + j) * 3;
        out[0] = (unsigned char)(rgb & 0xffu); out[1] = (unsigned char)((rgb >> 8) & 0xffu); out[2] = (unsigned char)(rgb >> 16);
      }
    }
    if (a.bary) {
      float* out = a.bary + (o + j) * 3;
      out[0] = l0; out[1] = l1; out[2] = l2;
    }
    if (a.attr_out) {
      float* out = a.attr_out + (o + j) * a.C;
      if (covered) {
        const float* at = a.attrs + (long)m * a.nv * a.C;
        const float* a0 = at + (long)c.i0 * a.C; const float* a1 = at + (long)c.i1 * a.C; const float* a2 = at + (long)c.i2 * a.C;
        for (int ch = 0; ch < a.C; ch++) out[ch] = fmaf(l2, a2[ch], fmaf(l1, a1[ch], l0 * a0[ch]));
      } else {
        for (int ch = 0; ch < a.C; ch++) out[ch] = a.attr_fill;
      }
    }
  }
  if (a.image && a.vec_img) {
    unsigned* ow = reinterpret_cast<unsigned*>(a.image + o * 3);
    ow[0] = (unsigned)lo; ow[1] = (unsigned)(lo >> 32); ow[2] = hi;
  }
  if (bad && a.status) atomicOr(&a.status[0], S_STATUS_BAD_INDEX);       // (rare: a hand-made buffer)
}

// [p, p + n) and [q, q + k) share a byte
static inline bool overlaps(const void* p, long n, const void* q, long k) {
  if (!p || !q || n <= 0 || k <= 0) return false;
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)k && b < a + (uintptr_t)n;
}

}  // namespace p2m

using namespace p2m;

extern "C" int p2m_vertex_normals(const float* verts, const int32_t* faces, const int32_t* vf_ptr, const int32_t* vf_idx,
                                  int32_t n_idx, int32_t B, int32_t nv, int32_t nf, float* normals, int32_t* status,
                                  void* stream) {
  P2M_CHECK_ARG(verts && faces && vf_ptr && normals, "null pointer");
  P2M_CHECK_ARG(n_idx >= 0 && (n_idx == 0 || vf_idx), "bad table length / null table");
  P2M_CHECK_ARG(B >= 0 && nv >= 1 && nf >= 1, "bad batch / vertex / face count");
  P2M_CHECK_ARG(B <= 65535, "more than 65535 meshes");
  P2M_CHECK_ARG((long)B * nv * 3 < (1L << 31), "more than 2^31 coordinates");
  P2M_CHECK_ARG(((((uintptr_t)verts | (uintptr_t)faces | (uintptr_t)vf_ptr | (uintptr_t)vf_idx | (uintptr_t)normals |
                   (uintptr_t)status) & 3) == 0), "misaligned buffer");
  const long nb = (long)B * nv * 12;
  P2M_CHECK_ARG(!overlaps(normals, nb, verts, nb) && !overlaps(normals, nb, faces, (long)nf * 12) &&
                !overlaps(normals, nb, vf_ptr, ((long)nv + 1) * 4) && !overlaps(normals, nb, vf_idx, (long)n_idx * 4) &&
                !overlaps(status, (long)B * 4, verts, nb) && !overlaps(status, (long)B * 4, faces, (long)nf * 12) &&
                !overlaps(status, (long)B * 4, vf_ptr, ((long)nv + 1) * 4) &&
                !overlaps(status, (long)B * 4, vf_idx, (long)n_idx * 4) && !overlaps(status, (long)B * 4, normals, nb),
                "an output overlaps an input");
  if (B == 0) return P2M_OK;
  hipStream_t s = (hipStream_t)stream;
  if (status && hipMemsetAsync(status, 0, sizeof(int32_t) * B, s) != hipSuccess) return check_launch("vertex_normals");
  hipLaunchKernelGGL(k_vertex_normals, dim3(cdiv(nv, S_NT), B), dim3(S_NT), 0, s, verts, faces, vf_ptr, vf_idx, n_idx, nv, nf,
                     normals, status);
  return check_launch("vertex_normals");
}

extern "C" int p2m_mesh_shade(const int32_t* face_id, const int32_t* mesh_id, const float* verts, const int32_t* faces,
                              int32_t nf, const float* cam, const float* colours, const float* vertex_colours,
                              int32_t vertex_colours_shared, const float* normals, const float* lights, int32_t nl,
                              float ambient, const float* attrs, int32_t C, int32_t wire_T, const uint8_t* wire_rgb,
                              int32_t wire_only, const uint8_t* background, int32_t bg_per_mesh, float attr_fill, int32_t B,
                              int32_t nv, int32_t H, int32_t W, int32_t mode, uint8_t* image, float* bary, float* attr_out,
                              int32_t* status, void* stream) {
  P2M_CHECK_ARG(face_id && mesh_id && verts && faces && cam, "null pointer");
  P2M_CHECK_ARG(nl >= 0 && nl <= R_MAX_LIGHTS, "0..4 lights");
  P2M_CHECK_ARG(nl == 0 || lights, "null pointer");
  P2M_CHECK_ARG(B >= 0 && nf >= 1 && nf < (1 << 24), "bad batch / face count");
  P2M_CHECK_ARG(mode == 0 || mode == 1, "mode: 0 batch, 1 scene");
  P2M_CHECK_ARG(!(mode == 1 && B > 255), "more than 255 meshes in scene mode");
  P2M_CHECK_ARG(B <= 65535, "more than 65535 meshes");
  P2M_CHECK_ARG(H >= 1 && H <= R_MAX_DIM && W >= 1 && W <= R_MAX_DIM, "H, W must lie in [1, 8192]");
  P2M_CHECK_ARG((long)B * nf < (1L << 31), "B * nf >= 2^31");
  P2M_CHECK_ARG(nv >= 1 && (long)B * nv * 3 < (1L << 31), "bad vertex count");
  P2M_CHECK_ARG(!(mode == 1 && bg_per_mesh), "scene mode has one image: one background");
  const int n_img = mode == 1 ? 1 : B;
  P2M_CHECK_ARG((long)n_img * H * W * 3 < (1L << 40), "image batch too large");
  P2M_CHECK_ARG(!attrs || (C >= 1 && C <= S_MAX_ATTR), "1..16 attribute channels");
  P2M_CHECK_ARG(!attr_out || attrs, "attr_out without attrs");
  P2M_CHECK_ARG(!attrs || (long)B * nv * C < (1L << 31), "more than 2^31 attribute values");
  P2M_CHECK_ARG(wire_T >= 0 && wire_T <= S_MAX_WIRE, "wire_T must lie in [0, 2^16]");
  P2M_CHECK_ARG(wire_T == 0 || wire_rgb, "null pointer");
  P2M_CHECK_ARG(!image || ((colours != nullptr) != (vertex_colours != nullptr)), "an image takes colours or vertex_colours, not both");
  P2M_CHECK_ARG((((uintptr_t)face_id | (uintptr_t)mesh_id | (uintptr_t)verts | (uintptr_t)faces | (uintptr_t)cam |
                  (uintptr_t)colours | (uintptr_t)vertex_colours | (uintptr_t)normals | (uintptr_t)attrs | (uintptr_t)bary |
                  (uintptr_t)attr_out | (uintptr_t)status) & 3) == 0, "misaligned buffer");
  ShadeArgs sa;
  P2M_CHECK_ARG(lights_from_host(lights, nl, ambient, sa.L), "a light direction must be non-zero and finite");
  {
    const long px = (long)n_img * H * W, vb = (long)B * nv * 12;
    const void* in[10] = {face_id, mesh_id, verts, faces, cam, colours, vertex_colours, normals, attrs, background};
    const long in_n[10] = {px * 4, px * 4, vb, (long)nf * 12, (long)B * 16, (long)B * 12,
                           vertex_colours_shared ? (long)nv * 12 : vb, vb, attrs ? (long)B * nv * C * 4 : 0,
                           (bg_per_mesh ? px : (long)H * W) * 3};
    const void* out[4] = {image, bary, attr_out, status};
    const long out_n[4] = {px * 3, px * 12, attrs ? px * C * 4 : 0, (long)B * 4};
    for (int i = 0; i < 4; i++) {
      for (int k = 0; k < 10; k++) P2M_CHECK_ARG(!overlaps(out[i], out_n[i], in[k], in_n[k]), "an output overlaps an input");
      for (int k = i + 1; k < 4; k++) P2M_CHECK_ARG(!overlaps(out[i], out_n[i], out[k], out_n[k]), "two outputs overlap");
    }
  }
  if (B == 0) return P2M_OK;
  hipStream_t s = (hipStream_t)stream;
  sa.face_id = face_id; sa.mesh_id = mesh_id; sa.verts = verts; sa.faces = faces; sa.cam = cam;
  sa.colours = colours; sa.vcol = vertex_colours; sa.normals = normals; sa.attrs = attrs; sa.bg = background;
  sa.B = B; sa.nv = nv; sa.nf = nf; sa.H = H; sa.W = W; sa.C = attrs ? C : 0; sa.vcol_shared = vertex_colours_shared ? 1 : 0;
  sa.bg_per_mesh = bg_per_mesh ? 1 : 0; sa.wire_T = wire_T; sa.wire_only = wire_only ? 1 : 0;
  sa.vec_ids = (W & 3) == 0 && (((uintptr_t)face_id | (uintptr_t)mesh_id) & 15) == 0;
  sa.vec_img = (W & 3) == 0 && (((uintptr_t)image | (uintptr_t)background) & 3) == 0;
  sa.wire_rgb = wire_T > 0 ? ((unsigned)wire_rgb[0] | ((unsigned)wire_rgb[1] << 8) | ((unsigned)wire_rgb[2] << 16)) : 0u;
  sa.attr_fill = attr_fill;
  sa.image = image; sa.bary = bary; sa.attr_out = attr_out; sa.status = status;
  if (status && hipMemsetAsync(status, 0, sizeof(int32_t) * B, s) != hipSuccess) return check_launch("mesh_shade");
  if (image || bary || attr_out)
    hipLaunchKernelGGL(k_mesh_shade, dim3(cdiv((long)H * cdiv(W, 4), S_NT), n_img), dim3(S_NT), 0, s, sa);
  return check_launch("mesh_shade");
}
