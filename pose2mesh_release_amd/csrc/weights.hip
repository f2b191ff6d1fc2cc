// Weight kernels of the dense contractions: what a parameter goes through on its way to and from the matrix cores.
//
//   k_weight_split              : the pre-split weight operand of the slice arithmetics (three bf16 or two scaled fp16 slices)
//   k_weight_pack               : nn.Linear / graph-conv weight -> the [K, N] operands of the forward and dX contractions
//   k_transpose_tiled           : the K = 1 form of the above, a plain transpose through LDS
//   k_weight_eff                : the K = Fin weight W0 + a W1 + b W2 seen by fake vertices
//   k_conv_weights_amax/_images : every slice image of a network's conv weights in two launches (_images_tiled: through LDS)
//   k_weight_grad_unpack        : per-chunk partial weight gradients (gemm_tn.hip) -> dW, db in the parameter's layout
#include "p2m_gemm.h"

namespace p2m {

// Bx[k / 16][s][n][k % 16] = s-th bf16 slice of Bm[k][n] (zero for N <= n < Npad): the pre-split weight operand,
// chunk-major so that the [BN x 16] slice a block stages per chunk is one contiguous run
// NS = 2: fp16 slices of Bm 2^sb, sb from the bound 2^bits * (*amax_in) - the word trailing the image itself (bits = 0,
// written by k_amax_one_block just before) or the word of the tensor Bm was derived from; the trailer then receives
// that bound, so every consumer re-derives the same sb from the image alone
template <int NS>
__global__ void k_weight_split(const float* __restrict__ Bm, unsigned short* __restrict__ Bx, int K, int N, int Npad,
                               const unsigned* __restrict__ amax_in, int bits) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)Npad * K) return;
  const int k = (int)(i / Npad), n = (int)(i - (long)k * Npad);      // n fastest: coalesced reads of Bm
  const long sl = (long)Npad * 16;
  unsigned short* d = Bx + (long)(k >> 4) * NS * sl + (long)n * 16 + (k & 15);
  if constexpr (NS == 3) {
    unsigned h = 0, m = 0, l = 0;
    if (n < N) split3(Bm[(long)k * N + n], h, m, l);
    d[0] = (unsigned short)(h >> 16);
    d[sl] = (unsigned short)(m >> 16);
    d[2 * sl] = (unsigned short)(l >> 16);
  } else {
    unsigned* trailer = reinterpret_cast<unsigned*>(Bx + (long)NS * Npad * K);
    const unsigned word = *amax_in;
    if (i == 0 && amax_in != trailer) *trailer = word == 0u ? 0u : __float_as_uint(__builtin_ldexpf(__uint_as_float(word), bits));
    const float y = n < N ? Bm[(long)k * N + n] * exp2_int(slice_scale_exp(word, bits)) : 0.f;
    const _Float16 h = (_Float16)y;
    const _Float16 l = (_Float16)(y - (float)h);
    d[0] = __builtin_bit_cast(unsigned short, h);
    d[sl] = __builtin_bit_cast(unsigned short, l);
  }
}

// ---------------------------------------------------------------------------------------------
// weight pack / gradient unpack
// ---------------------------------------------------------------------------------------------
__global__ void k_weight_pack(const float* __restrict__ W, float* __restrict__ Wt, float* __restrict__ W2,
                              float* __restrict__ W3, int Fout, int Fin, int K) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long tot = (long)Fout * Fin * K;
  if (idx >= tot) return;
  // idx enumerates Wt: [(k*Fin+fin)][fout]
  int fout = (int)(idx % Fout);
  long kk = idx / Fout;
  int k = (int)(kk / Fin), fin = (int)(kk % Fin);
  float v = W[(long)fout * Fin * K + (long)fin * K + k];
  Wt[idx] = v;
  if (W2) W2[(long)fout * Fin * K + kk] = v;
  if (W3) W3[((long)k * Fout + fout) * Fin + fin] = v;     // [k*Fout + fout][fin]: B operand of dX = [g|Lg|L2g] W3
}

// K = 1, Wt only: a plain transpose Wt[fin][fout] = W[fout][fin] (the fc lift of meshnet.py:105 and, round 5, the four
// 4096 x 4096 Linears of PoseNet: 67 MB each per optimizer step).  k_weight_pack reads W at a stride of Fin floats per lane:
// 100 us for 4096 x 4096 (1.3 TB/s) in the round-5 step trace.  64 x 64 tiles through LDS, 16-byte accesses on both sides.
__global__ __launch_bounds__(256) void k_transpose_tiled(const float* __restrict__ W, float* __restrict__ Wt, int R, int C) {
  __shared__ float tile[64][65];
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int tq = threadIdx.x & 15, ty = threadIdx.x >> 4;           // 16 column quads x 16 rows per pass
  const bool vec = (C & 3) == 0 && (R & 3) == 0;
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int r = r0 + ty + 16 * p, c = c0 + 4 * tq;
    if (r < R) {
      if (vec && c + 3 < C) {
        const float4 v = *reinterpret_cast<const float4*>(W + (long)r * C + c);
        tile[ty + 16 * p][4 * tq] = v.x; tile[ty + 16 * p][4 * tq + 1] = v.y;
        tile[ty + 16 * p][4 * tq + 2] = v.z; tile[ty + 16 * p][4 * tq + 3] = v.w;
      } else {
        for (int e = 0; e < 4; e++)
          if (c + e < C) tile[ty + 16 * p][4 * tq + e] = W[(long)r * C + c + e];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int c = c0 + ty + 16 * p, r = r0 + 4 * tq;               // output row c, columns r .. r + 3
    if (c < C) {
      if (vec && r + 3 < R) {
        float4 v;
        v.x = tile[4 * tq][ty + 16 * p]; v.y = tile[4 * tq + 1][ty + 16 * p];
        v.z = tile[4 * tq + 2][ty + 16 * p]; v.w = tile[4 * tq + 3][ty + 16 * p];
        *reinterpret_cast<float4*>(Wt + (long)c * R + r) = v;
      } else {
        for (int e = 0; e < 4; e++)
          if (r + e < R) Wt[(long)c * R + r + e] = tile[4 * tq + e][ty + 16 * p];
      }
    }
  }
}

// Weff[k][n] = Wt[k][n] + a * Wt[Ka + k][n] + b * Wt[2 Ka + k][n]: the K = Fin weight seen by fake vertices
__global__ void k_weight_eff(const float* __restrict__ Wt, float* __restrict__ We, int Ka, int N, float a, float b) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)Ka * N) return;
  const long plane = (long)Ka * N;
  We[idx] = Wt[idx] + a * Wt[plane + idx] + b * Wt[2 * plane + idx];
}

// ---- every slice image of a network's conv weights in two launches ----------------------------------------------------
// A split conv needs four pre-split operands of its weight W[Fout][Fin * 3 + k] per optimizer step: [3 Fin, Fout] (forward,
// real rows), its effective K = Fin form W0 + a W1 + b W2 (forward, padding rows), [3 Fout, Fin] (backward dX, real rows)
// and that one's effective form.  Through p2m_weight_pack / _eff / _split / p2m_amax that is 8 launches per layer, ~150
// per step, each a few microseconds long with a pipeline drain on either side - 1.5 ms of a 38 ms step.  Here: one block per
// layer for the parameters' amax words, then ONE launch that writes all images straight from W (blockIdx.y = layer).
struct ConvWeights {            // == p2m_conv_weights of include/p2m.h
  const float* W;
  int Fout, Fin;
  float fake_a, fake_b;
  int eff_bits, reserved;
  unsigned short *Bx_f, *Bx_ef, *Bx_b, *Bx_eb;
  unsigned* amax;
};
static_assert(sizeof(ConvWeights) == 72, "layout shared with the callers (include/p2m.h, ops.py)");

__global__ __launch_bounds__(1024) void k_conv_weights_amax(const ConvWeights* __restrict__ d) {
  __shared__ float red[16];
  const ConvWeights c = d[blockIdx.x];
  const long n = (long)c.Fout * c.Fin * 3;
  float m = 0.f;
  const long n4 = (reinterpret_cast<uintptr_t>(c.W) & 15) == 0 ? n >> 2 : 0;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(c.W);
  for (long i = threadIdx.x; i < n4; i += 1024) {
    const f32x4 v = x4[i];
    m = fmaxf(fmaxf(m, fmaxf(amax_abs(v[0]), amax_abs(v[1]))), fmaxf(amax_abs(v[2]), amax_abs(v[3])));
  }
  for (long j = n4 * 4 + threadIdx.x; j < n; j += 1024) m = fmaxf(m, amax_abs(c.W[j]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; w++) m = fmaxf(m, red[w]);
    *c.amax = __float_as_uint(m);
  }
}

// one image: Bx[k / 16][slice][n][k % 16] of value(k, n), n < Npad (zero beyond N), + the trailing amax word (NS = 2)
template <int NS, typename F>
__device__ __forceinline__ void write_weight_image(unsigned short* __restrict__ Bx, int K, int N, unsigned word, int bits,
                                                   F value) {
  if (Bx == nullptr) return;
  const int Npad = cdiv_dev(N, 128) * 128;
  const long sl = (long)Npad * 16, tot = (long)Npad * K;
  float sc = 1.f;
  if constexpr (NS == 2) {
    sc = exp2_int(slice_scale_exp(word, bits));
    if (blockIdx.x == 0 && threadIdx.x == 0)
      *reinterpret_cast<unsigned*>(Bx + (long)NS * Npad * K) =
          word == 0u ? 0u : __float_as_uint(__builtin_ldexpf(__uint_as_float(word), bits));
  }
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (long)gridDim.x * blockDim.x) {
    const int k = (int)(i / Npad), n = (int)(i - (long)k * Npad);
    const float v = n < N ? value(k, n) : 0.f;
    unsigned short* dst = Bx + (long)(k >> 4) * NS * sl + (long)n * 16 + (k & 15);
    if constexpr (NS == 3) {
      unsigned h, m, l;
      split3(v, h, m, l);
      dst[0] = (unsigned short)(h >> 16);
      dst[sl] = (unsigned short)(m >> 16);
      dst[2 * sl] = (unsigned short)(l >> 16);
    } else {
      const float y = v * sc;
      const _Float16 h = (_Float16)y;
      const _Float16 l = (_Float16)(y - (float)h);
      dst[0] = __builtin_bit_cast(unsigned short, h);
      dst[sl] = __builtin_bit_cast(unsigned short, l);
    }
  }
}

template <int NS>
__global__ __launch_bounds__(256) void k_conv_weights_images(const ConvWeights* __restrict__ d) {
  const ConvWeights c = d[blockIdx.y];
  const float* __restrict__ W = c.W;
  const int Fout = c.Fout, Fin = c.Fin, ld = 3 * c.Fin;
  const float a = c.fake_a, b = c.fake_b;
  const unsigned word = NS == 2 ? *c.amax : 0u;
  // forward, real rows: Wt[kk * Fin + fin][fo] = W[fo][fin * 3 + kk]
  write_weight_image<NS>(c.Bx_f, 3 * Fin, Fout, word, 0, [&](int k, int n) {
    const int kk = k / Fin, fin = k - kk * Fin;
    return W[(long)n * ld + fin * 3 + kk];
  });
  // forward, padding rows: (W0 + a W1 + b W2)[fin][fo]   (the expression of k_weight_eff)
  write_weight_image<NS>(c.Bx_ef, Fin, Fout, word, c.eff_bits, [&](int k, int n) {
    const float* w = W + (long)n * ld + k * 3;
    return w[0] + a * w[1] + b * w[2];
  });
  // backward dX, real rows: W3[kk * Fout + fo][fin] = W[fo][fin * 3 + kk]
  write_weight_image<NS>(c.Bx_b, 3 * Fout, Fin, word, 0, [&](int k, int n) {
    const int kk = k / Fout, fo = k - kk * Fout;
    return W[(long)fo * ld + n * 3 + kk];
  });
  // backward dX, padding rows: (W3_0 + a W3_1 + b W3_2)[fo][fin]
  write_weight_image<NS>(c.Bx_eb, Fout, Fin, word, c.eff_bits, [&](int k, int n) {
    const float* w = W + (long)k * ld + n * 3;
    return w[0] + a * w[1] + b * w[2];
  });
}

// ---- the same four images, tiled through LDS (P2M_NARROW_ROWS = 1) -------------------------------------------------------
// A block takes a 32 (fo) x 32 (fin) tile of W - 32 runs of 96 contiguous floats, read once along W's fast axis - and emits the
// tile's part of all four images from LDS: an item is 8 consecutive k of one n, i.e. one 16-byte store per slice, and the 64
// lanes of a wave cover (n, half) pairs that are contiguous in the image (1 KB per slice and store).  The tile grid spans
// Npad in both directions, so the zero columns n >= N come out of the same stores.  Values, split and trailer word are those
// of write_weight_image.  An image whose K is not cut into 16-groups along the tile (Fin or Fout not a multiple of 16) or
// that is not 16-byte aligned is written by write_weight_image.
constexpr int WI_T = 32;                  // tile edge
constexpr int WI_LD = 3 * WI_T + 1;       // LDS row: 96 floats + 1 (a column walk then touches 32 different banks)

__device__ __forceinline__ float weight_eff_value(const float* w, float a, float b) { return w[0] + a * w[1] + b * w[2]; }

template <int NS>
__device__ __forceinline__ void store_k8(unsigned short* __restrict__ dst, long sl, const float (&v)[8], float sc) {
  unsigned short s[NS][8];
#pragma unroll
  for (int e = 0; e < 8; e++) {
    if constexpr (NS == 3) {
      unsigned h, m, l;
      split3(v[e], h, m, l);
      s[0][e] = (unsigned short)(h >> 16);
      s[1][e] = (unsigned short)(m >> 16);
      s[2][e] = (unsigned short)(l >> 16);
    } else {
      const float y = v[e] * sc;
      const _Float16 h = (_Float16)y;
      const _Float16 l = (_Float16)(y - (float)h);
      s[0][e] = __builtin_bit_cast(unsigned short, h);
      s[1][e] = __builtin_bit_cast(unsigned short, l);
    }
  }
#pragma unroll
  for (int q = 0; q < NS; q++) {
    u32x4 p;
#pragma unroll
    for (int i = 0; i < 4; i++) p[i] = (unsigned)s[q][2 * i] | ((unsigned)s[q][2 * i + 1] << 16);
    *reinterpret_cast<u32x4*>(dst + q * sl) = p;
  }
}

// the trailing amax word of a two-slice image and its scale (write_weight_image)
template <int NS>
__device__ __forceinline__ float weight_image_scale(unsigned short* Bx, int K, int Npad, unsigned word, int bits) {
  if constexpr (NS == 2) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      *reinterpret_cast<unsigned*>(Bx + (long)NS * Npad * K) =
          word == 0u ? 0u : __float_as_uint(__builtin_ldexpf(__uint_as_float(word), bits));
    return exp2_int(slice_scale_exp(word, bits));
  }
  return 1.f;
}

template <int NS>
__global__ __launch_bounds__(256) void k_conv_weights_images_tiled(const ConvWeights* __restrict__ d) {
  __shared__ float tile[WI_T][WI_LD];
  const ConvWeights c = d[blockIdx.y];
  const float* __restrict__ W = c.W;
  const int Fout = c.Fout, Fin = c.Fin, ld = 3 * c.Fin;
  const float a = c.fake_a, b = c.fake_b;
  const unsigned word = NS == 2 ? *c.amax : 0u;
  const int t = threadIdx.x;
  const auto tiled = [](const unsigned short* Bx, int kdim) {
    return Bx != nullptr && kdim % 16 == 0 && (reinterpret_cast<uintptr_t>(Bx) & 15) == 0;
  };
  const bool tf = tiled(c.Bx_f, Fin), tef = tiled(c.Bx_ef, Fin), tb = tiled(c.Bx_b, Fout), teb = tiled(c.Bx_eb, Fout);
  // images that cannot take the tiled form: the element walk, all blocks of the layer
  if (!tf)
    write_weight_image<NS>(c.Bx_f, 3 * Fin, Fout, word, 0, [&](int k, int n) {
      const int kk = k / Fin, fin = k - kk * Fin;
      return W[(long)n * ld + fin * 3 + kk];
    });
  if (!tef)
    write_weight_image<NS>(c.Bx_ef, Fin, Fout, word, c.eff_bits, [&](int k, int n) {
      return weight_eff_value(W + (long)n * ld + k * 3, a, b);
    });
  if (!tb)
    write_weight_image<NS>(c.Bx_b, 3 * Fout, Fin, word, 0, [&](int k, int n) {
      const int kk = k / Fout, fo = k - kk * Fout;
      return W[(long)fo * ld + n * 3 + kk];
    });
  if (!teb)
    write_weight_image<NS>(c.Bx_eb, Fout, Fin, word, c.eff_bits, [&](int k, int n) {
      return weight_eff_value(W + (long)k * ld + n * 3, a, b);
    });
  if (!(tf || tef || tb || teb)) return;
  const int FoP = cdiv_dev(Fout, 128) * 128, FiP = cdiv_dev(Fin, 128) * 128;     // Npad of f / ef and of b / eb
  const long sl_o = (long)FoP * 16, sl_i = (long)FiP * 16;                        // slice strides
  float sc_f = 1.f, sc_ef = 1.f, sc_b = 1.f, sc_eb = 1.f;
  if (tf) sc_f = weight_image_scale<NS>(c.Bx_f, 3 * Fin, FoP, word, 0);
  if (tef) sc_ef = weight_image_scale<NS>(c.Bx_ef, Fin, FoP, word, c.eff_bits);
  if (tb) sc_b = weight_image_scale<NS>(c.Bx_b, 3 * Fout, FiP, word, 0);
  if (teb) sc_eb = weight_image_scale<NS>(c.Bx_eb, Fout, FiP, word, c.eff_bits);
  const int nti = FiP / WI_T, nt = (FoP / WI_T) * nti;
  for (int tl = blockIdx.x; tl < nt; tl += gridDim.x) {
    const int fo0 = (tl / nti) * WI_T, fin0 = (tl - (tl / nti) * nti) * WI_T;
    const bool has_o = fo0 < Fout, has_i = fin0 < Fin;       // the tile holds rows / columns of W
    if (!has_o && !has_i) continue;                          // (block-uniform)
    __syncthreads();                                         // the previous tile's readers are done
    for (int e = t; e < WI_T * 3 * WI_T; e += 256) {
      const int r = e / (3 * WI_T), cc = e - r * (3 * WI_T);
      const int fo = fo0 + r, col = 3 * fin0 + cc;
      tile[r][cc] = (fo < Fout && col < ld) ? W[(long)fo * ld + col] : 0.f;
    }
    __syncthreads();
    // item j = half + 2 * nl + 64 * (g + 2 * kk): 8 values k = kbase + 16 g + 8 half + 0 .. 7 of column n = n0 + nl
    if (has_i && (tf || tef)) {          // f, ef: k runs along fin, n = fo
      for (int j = t; j < 64 * 2 * 4; j += 256) {
        const int half = j & 1, nl = (j >> 1) & 31, g = (j >> 6) & 1, kk = j >> 7;      // kk == 3: the effective image
        const int fl = 16 * g + 8 * half, fin = fin0 + fl, n = fo0 + nl;
        if (fin >= Fin) continue;
        float v[8];
        if (kk < 3) {
          if (!tf) continue;
#pragma unroll
          for (int e = 0; e < 8; e++) v[e] = n < Fout ? tile[nl][(fl + e) * 3 + kk] : 0.f;
          const int k = kk * Fin + fin;
          store_k8<NS>(c.Bx_f + (long)(k >> 4) * NS * sl_o + (long)n * 16 + (k & 15), sl_o, v, sc_f);
        } else {
          if (!tef) continue;
#pragma unroll
          for (int e = 0; e < 8; e++) v[e] = n < Fout ? weight_eff_value(&tile[nl][(fl + e) * 3], a, b) : 0.f;
          store_k8<NS>(c.Bx_ef + (long)(fin >> 4) * NS * sl_o + (long)n * 16 + (fin & 15), sl_o, v, sc_ef);
        }
      }
    }
    if (has_o && (tb || teb)) {          // b, eb: k runs along fo, n = fin
      for (int j = t; j < 64 * 2 * 4; j += 256) {
        const int half = j & 1, nl = (j >> 1) & 31, g = (j >> 6) & 1, kk = j >> 7;
        const int rl = 16 * g + 8 * half, fo = fo0 + rl, n = fin0 + nl;
        if (fo >= Fout) continue;
        float v[8];
        if (kk < 3) {
          if (!tb) continue;
#pragma unroll
          for (int e = 0; e < 8; e++) v[e] = n < Fin ? tile[rl + e][nl * 3 + kk] : 0.f;
          const int k = kk * Fout + fo;
          store_k8<NS>(c.Bx_b + (long)(k >> 4) * NS * sl_i + (long)n * 16 + (k & 15), sl_i, v, sc_b);
        } else {
          if (!teb) continue;
#pragma unroll
          for (int e = 0; e < 8; e++) v[e] = n < Fin ? weight_eff_value(&tile[rl + e][nl * 3], a, b) : 0.f;
          store_k8<NS>(c.Bx_eb + (long)(fo >> 4) * NS * sl_i + (long)n * 16 + (fo & 15), sl_i, v, sc_eb);
        }
      }
    }
  }
}

// Block = 32 consecutive output elements x UNP_CG chunk groups: the partial buffers hold hundreds of chunks (one per
// sample in row-set mode), so the chunk loop is split UNP_CG ways (4 loads in flight each) and reduced through LDS.
// 8 groups (256 threads): alone on the GPU 32 groups are faster, but this kernel runs on the side stream next to the
// GEMM blocks that own most of the CUs' registers and LDS, and small blocks find a slot sooner (whole step, meshes/s:
// 2 groups 4213, 4: 4222-4230, 8: 4206-4253, 16: 4209, 32: 4174-4189).
constexpr int UNP_CG = 8;
__global__ __launch_bounds__(32 * UNP_CG) void k_weight_grad_unpack(
    const float* __restrict__ P, const float* __restrict__ Pdb, int nchunks, float* __restrict__ dW,
    float* __restrict__ db, int Fout, int Fin, int K, int accumulate, int layout, int pdb_stride,
    const float* __restrict__ P2, const float* __restrict__ Pdb2, int nchunks2, float fake_a, float fake_b) {
  __shared__ double red[UNP_CG][32];
  const int e = threadIdx.x & 31, cg = threadIdx.x >> 5;
  const long idx = (long)blockIdx.x * 32 + e;
  const long tot = (long)Fout * Fin * K;
  int fout = 0, k = 0, fin = 0;
  double s = 0.0;
  if (idx < tot) {
    if (layout == 0) {            // P[chunk][k*Fin + fin][fout]
      fout = (int)(idx % Fout);
      long kk = idx / Fout;
      k = (int)(kk / Fin); fin = (int)(kk % Fin);
    } else if (layout == 2) {     // P[chunk][fout][fin], K = 1: already the nn.Linear layout (a plain Linear's gradient
      fout = (int)(idx / Fin);    // taken as G^T X with the roles of the two operands swapped): reads AND writes coalesced
      fin = (int)(idx - (long)fout * Fin);
    } else {                      // P[chunk][fin][k*Fout + fout]   (weight gradient taken as X^T [g|Lg|L2g])
      long nn = idx % ((long)K * Fout);
      fin = (int)(idx / ((long)K * Fout));
      k = (int)(nn / Fout); fout = (int)(nn % Fout);
    }
    float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
    int c = cg;
    for (; c + 3 * UNP_CG < nchunks; c += 4 * UNP_CG) {
      t0 += P[(long)c * tot + idx];
      t1 += P[(long)(c + UNP_CG) * tot + idx];
      t2 += P[(long)(c + 2 * UNP_CG) * tot + idx];
      t3 += P[(long)(c + 3 * UNP_CG) * tot + idx];
    }
    for (; c < nchunks; c += UNP_CG) t0 += P[(long)c * tot + idx];
    s = ((double)t0 + (double)t1) + ((double)t2 + (double)t3);
    if (P2 != nullptr) {          // fake-vertex partials P2[chunk][fin][fout] enter plane k scaled by (1, a, b)[k]
      const long o2 = (long)fin * Fout + fout, st2 = (long)Fin * Fout;
      float q0 = 0.f, q1 = 0.f;
      int c2 = cg;
      for (; c2 + UNP_CG < nchunks2; c2 += 2 * UNP_CG) {
        q0 += P2[(long)c2 * st2 + o2];
        q1 += P2[(long)(c2 + UNP_CG) * st2 + o2];
      }
      for (; c2 < nchunks2; c2 += UNP_CG) q0 += P2[(long)c2 * st2 + o2];
      s += ((double)q0 + (double)q1) * (k == 0 ? 1.0 : (k == 1 ? (double)fake_a : (double)fake_b));
    }
  }
  red[cg][e] = s;
  __syncthreads();
  if (cg == 0 && idx < tot) {
    double r = 0.0;
#pragma unroll
    for (int q = 0; q < UNP_CG; q++) r += red[q][e];
    const long o = (long)fout * Fin * K + (long)fin * K + k;
    dW[o] = accumulate ? dW[o] + (float)r : (float)r;
  }
  // bias gradient: the first blocks also reduce Pdb (one output feature per lane, the chunks spread over the UNP_CG
  // lane groups and merged through LDS: a single thread walking all chunks was the kernel's long pole)
  if (db != nullptr && Pdb != nullptr && (long)blockIdx.x * 32 < Fout) {      // block-uniform
    __syncthreads();
    double r = 0.0;
    if (idx < Fout) {
      for (int c = cg; c < nchunks; c += UNP_CG) r += (double)Pdb[(long)c * pdb_stride + idx];
      if (Pdb2 != nullptr)
        for (int c2 = cg; c2 < nchunks2; c2 += UNP_CG) r += (double)Pdb2[(long)c2 * Fout + idx];
    }
    red[cg][e] = r;
    __syncthreads();
    if (cg == 0 && idx < Fout) {
      double t = 0.0;
#pragma unroll
      for (int q = 0; q < UNP_CG; q++) t += red[q][e];
      db[idx] = accumulate ? db[idx] + (float)t : (float)t;
    }
  }
}

}  // namespace p2m

using namespace p2m;

extern "C" int64_t p2m_weight_split_elems(int32_t K, int32_t N, int32_t arith) {
  if (K <= 0 || N <= 0 || K % 16 != 0 || (arith != P2M_ARITH_BF16X3 && arith != P2M_ARITH_F16X2)) return 0;
  return (long)slices_of(arith) * (cdiv(N, 128) * 128ll) * K + (arith == P2M_ARITH_F16X2 ? 8 : 0);
}

extern "C" int p2m_weight_split(const float* Bm, int32_t K, int32_t N, int32_t arith, const void* amax_in,
                                int32_t amax_bits, void* Bx, void* stream) {
  P2M_CHECK_ARG(Bm && Bx && K > 0 && N > 0, "null pointer or empty shape");
  P2M_CHECK_ARG(K % 16 == 0, "K must be a multiple of 16");
  P2M_CHECK_ARG(arith == P2M_ARITH_BF16X3 || arith == P2M_ARITH_F16X2, "arith must be P2M_ARITH_BF16X3 or P2M_ARITH_F16X2");
  const int Npad = cdiv(N, 128) * 128;
  const dim3 grid(cdiv((long)Npad * K, 256));
  unsigned short* bx = static_cast<unsigned short*>(Bx);
  if (arith == P2M_ARITH_F16X2) {
    const unsigned* word = static_cast<const unsigned*>(amax_in);
    P2M_CHECK_ARG(amax_bits >= 0 && amax_bits <= 30, "amax_bits out of range");
    if (word == nullptr) {              // no bound from the caller: the weight's own maximum (one small extra launch)
      unsigned* trailer = const_cast<unsigned*>(weight_amax_word(Bx, arith, Npad, K));
      amax_one_block(Bm, (long)K * N, trailer, (hipStream_t)stream);
      word = trailer;
      amax_bits = 0;
    }
    hipLaunchKernelGGL(k_weight_split<2>, grid, dim3(256), 0, (hipStream_t)stream, Bm, bx, K, N, Npad, word, amax_bits);
  } else {
    hipLaunchKernelGGL(k_weight_split<3>, grid, dim3(256), 0, (hipStream_t)stream, Bm, bx, K, N, Npad, nullptr, 0);
  }
  return check_launch("weight_split");
}

extern "C" int p2m_conv_weights_prepare(const p2m_conv_weights* dev_desc, int32_t n, int32_t arith, void* stream) {
  static_assert(sizeof(p2m_conv_weights) == sizeof(ConvWeights), "descriptor layout");
  P2M_CHECK_ARG(dev_desc != nullptr && n > 0, "null descriptor array or no layers");
  P2M_CHECK_ARG(arith == P2M_ARITH_BF16X3 || arith == P2M_ARITH_F16X2, "arith must be P2M_ARITH_BF16X3 or P2M_ARITH_F16X2");
  const ConvWeights* d = reinterpret_cast<const ConvWeights*>(dev_desc);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(96, n);                    // grid-stride over each image: the largest (768 x 256) is 768 elements per thread
  const bool tiled = narrow_rows();          // the LDS-tiled form: the largest layer (256 x 256) is 64 tiles
  if (arith == P2M_ARITH_F16X2) {
    hipLaunchKernelGGL(k_conv_weights_amax, dim3(n), dim3(1024), 0, s, d);
    if (tiled) hipLaunchKernelGGL(k_conv_weights_images_tiled<2>, grid, dim3(256), 0, s, d);
    else hipLaunchKernelGGL(k_conv_weights_images<2>, grid, dim3(256), 0, s, d);
  } else {
    if (tiled) hipLaunchKernelGGL(k_conv_weights_images_tiled<3>, grid, dim3(256), 0, s, d);
    else hipLaunchKernelGGL(k_conv_weights_images<3>, grid, dim3(256), 0, s, d);
  }
  return check_launch("conv_weights_prepare");
}

extern "C" int p2m_weight_pack(const float* W, float* Wt, float* W2, float* W3, int32_t Fout, int32_t Fin, int32_t K,
                               void* stream) {
  P2M_CHECK_ARG(W && Wt && Fout > 0 && Fin > 0 && K > 0, "null pointer or empty shape");
  long tot = (long)Fout * Fin * K;
  if (K == 1 && W2 == nullptr && W3 == nullptr && aligned16(W) && aligned16(Wt)) {
    hipLaunchKernelGGL(k_transpose_tiled, dim3(cdiv(Fin, 64), cdiv(Fout, 64)), dim3(256), 0, (hipStream_t)stream, W, Wt, Fout,
                       Fin);
    return check_launch("weight_pack(transpose)");
  }
  hipLaunchKernelGGL(k_weight_pack, dim3(cdiv(tot, 256)), dim3(256), 0, (hipStream_t)stream, W, Wt, W2, W3, Fout, Fin, K);
  return check_launch("weight_pack");
}

extern "C" int p2m_weight_eff(const float* Wt, float* We, int32_t Ka, int32_t N, float a, float b, void* stream) {
  P2M_CHECK_ARG(Wt && We && Ka > 0 && N > 0, "null pointer or empty shape");
  hipLaunchKernelGGL(k_weight_eff, dim3(cdiv((long)Ka * N, 256)), dim3(256), 0, (hipStream_t)stream, Wt, We, Ka, N, a, b);
  return check_launch("weight_eff");
}

extern "C" int p2m_weight_grad_unpack2(const float* P, const float* Pdb, int32_t nchunks, const float* P2,
                                       const float* Pdb2, int32_t nchunks2, float s1, float s2, float* dW, float* db,
                                       int32_t Fout, int32_t Fin, int32_t K, int32_t accumulate, void* stream) {
  P2M_CHECK_ARG(P && P2 && dW && Fout > 0 && Fin > 0 && K == 3 && nchunks > 0 && nchunks2 > 0, "null pointer or bad shape");
  long tot = (long)Fout * Fin * K;
  hipLaunchKernelGGL(k_weight_grad_unpack, dim3(cdiv(tot, 32)), dim3(32 * UNP_CG), 0, (hipStream_t)stream, P, Pdb, nchunks,
                     dW, db, Fout, Fin, K, accumulate, 1, K * Fout, P2, Pdb2, nchunks2, s1, s2);
  return check_launch("weight_grad_unpack2");
}

extern "C" int p2m_weight_grad_unpack(const float* P, const float* Pdb, int32_t nchunks, float* dW, float* db,
                                      int32_t Fout, int32_t Fin, int32_t K, int32_t accumulate, int32_t layout,
                                      int32_t pdb_stride, void* stream) {
  P2M_CHECK_ARG(P && dW && Fout > 0 && Fin > 0 && K > 0 && nchunks > 0, "null pointer or empty shape");
  P2M_CHECK_ARG(layout >= 0 && layout <= 2 && (layout != 2 || K == 1), "layout must be 0, 1 or (K = 1 only) 2");
  long tot = (long)Fout * Fin * K;
  hipLaunchKernelGGL(k_weight_grad_unpack, dim3(cdiv(tot, 32)), dim3(32 * UNP_CG), 0, (hipStream_t)stream, P, Pdb, nchunks,
                     dW, db, Fout, Fin, K, accumulate, layout, pdb_stride, nullptr, nullptr, 0, 0.f, 0.f);
  return check_launch("weight_grad_unpack");
}
