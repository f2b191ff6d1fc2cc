// What the rasteriser (render.hip) and the deferred shading pass (shade.hip) must compute bit for bit alike: the projection and
// snap of include/p2m.h, the lights, the flat face intensity and the rounding to a byte.  One definition, included by both.
#pragma once
#include "p2m_common.h"

namespace p2m {

constexpr int R_FIX = 256;            // sub-pixel units per pixel
constexpr int R_CLAMP = 1 << 23;      // snapped coordinates are clamped to +-2^23
constexpr int R_MAX_LIGHTS = 4;
constexpr int R_MAX_DIM = 8192;
constexpr int R_STATUS_CLAMPED = 1, R_STATUS_BAD_INDEX = 2;

// ---- projection and snap (shared by setup, project and shade: bitwise the same) ------------------------------------------
struct CamCoef { double ax, bx, ay, by; };

__device__ __forceinline__ CamCoef cam_coef(const float* cam, int H, int W) {
  const double sx = (double)cam[0], sy = (double)cam[1], tx = (double)cam[2], ty = (double)cam[3];
  const double hw = 0.5 * (double)W, hh = 0.5 * (double)H;
  CamCoef c;                          // (each operation rounded once: no contraction)
  c.ax = __dmul_rn(hw, sx);
  c.bx = __dmul_rn(hw, __dadd_rn(1.0, __dmul_rn(sx, tx)));
  c.ay = __dmul_rn(hh, sy);
  c.by = __dmul_rn(hh, __dadd_rn(1.0, __dmul_rn(sy, ty)));
  return c;
}

__device__ __forceinline__ int snap(double a, double v, double b, bool& clamped) {
  const double t = rint(__dmul_rn((double)R_FIX, __fma_rn(a, v, b)));    // ties to even
  if (!(t <= (double)R_CLAMP)) { clamped = true; return R_CLAMP; }      // (NaN lands here)
  if (t < -(double)R_CLAMP) { clamped = true; return -R_CLAMP; }
  return (int)t;
}

struct Lights {
  int nl;
  double ambient;
  double dir[R_MAX_LIGHTS][3];        // unit vectors towards the lights
  double k[R_MAX_LIGHTS];
};

// lights: HOST array [nl][4] -> the kernel argument, directions normalised in fp64.  False: a zero or non-finite direction.
static inline bool lights_from_host(const float* lights, int nl, float ambient, Lights& L) {
  L.nl = nl; L.ambient = (double)ambient;
  for (int l = 0; l < R_MAX_LIGHTS; l++) {
    double d[3] = {0.0, 0.0, 0.0}, k = 0.0;
    if (l < nl) {
      for (int c = 0; c < 3; c++) d[c] = (double)lights[4 * l + c];
      k = (double)lights[4 * l + 3];
      const double len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      if (!(len > 0.0 && len < __builtin_inf())) return false;
      for (int c = 0; c < 3; c++) d[c] /= len;
    }
    for (int c = 0; c < 3; c++) L.dir[l][c] = d[c];
    L.k[l] = k;
  }
  return true;
}

// The two functions below are the rasteriser's flat shading as it has always been compiled: with the compiler free to contract
// a product and a sum into one fma.  The pragma keeps that form in a translation unit built with -ffp-contract=off (shade.hip),
// so that both units round the same values at the same places.
__device__ __forceinline__ unsigned to_u8(double v) {                    // floor(255 min(1, v) + 0.5), negative and NaN -> 0
#pragma clang fp contract(fast)
  const double c = v < 1.0 ? v : 1.0;
  const double r = floor(255.0 * c + 0.5);
  return r > 0.0 ? (unsigned)r : 0u;
}

// flat shading: the fp64 unit normal of the face p turned towards the viewer (n_z <= 0), I = ambient + sum k max(0, n.l)
__device__ __forceinline__ double face_intensity(const float (&p)[3][3], const Lights& L) {
#pragma clang fp contract(fast)
  const double e1[3] = {(double)p[1][0] - (double)p[0][0], (double)p[1][1] - (double)p[0][1], (double)p[1][2] - (double)p[0][2]};
  const double e2[3] = {(double)p[2][0] - (double)p[0][0], (double)p[2][1] - (double)p[0][1], (double)p[2][2] - (double)p[0][2]};
  double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  double I = L.ambient;
  if (len > 0.0) {
    const double s = (n[2] > 0.0 ? -1.0 : 1.0) / len;
#pragma unroll
    for (int l = 0; l < R_MAX_LIGHTS; l++) {
      if (l < L.nl) {
        const double d = s * (n[0] * L.dir[l][0] + n[1] * L.dir[l][1] + n[2] * L.dir[l][2]);
        I += L.k[l] * (d > 0.0 ? d : 0.0);
      }
    }
  }
  return I;
}

}  // namespace p2m
