// Operand amax kernels of the two-fp16-slice arithmetic (P2M_ARITH_F16X2, p2m_split.h): the bits of max |x| over a tensor, or over
// the rows of a row set, in a device word - the bound from which every consumer of the tensor derives its power-of-two scale.
//
//   k_amax_one_block : one block, overwrites the word (weights: p2m_weight_split, weights.hip)
//   k_amax           : any size and alignment, atomic max into a word the caller has zeroed
//   k_amax_rows      : the rows of a row set only
#include "p2m_gemm.h"

namespace p2m {

// amax words (p2m_split.h).  One block, overwrites the word: for small tensors (weights) - no zeroing, no atomics.
__global__ __launch_bounds__(1024) void k_amax_one_block(const float* __restrict__ x, long n, unsigned* __restrict__ word) {
  __shared__ float red[16];
  float m = 0.f;
  const long n4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? n >> 2 : 0;      // float4 body, 8 loads in flight per thread
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  long i = threadIdx.x;
  for (; i + 7 * 1024 < n4; i += 8 * 1024) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = x4[i + u * 1024];
#pragma unroll
    for (int u = 0; u < 8; u++)
      m = fmaxf(fmaxf(m, fmaxf(amax_abs(v[u][0]), amax_abs(v[u][1]))), fmaxf(amax_abs(v[u][2]), amax_abs(v[u][3])));
  }
  for (; i < n4; i += 1024) {
    const f32x4 v = x4[i];
    m = fmaxf(fmaxf(m, fmaxf(amax_abs(v[0]), amax_abs(v[1]))), fmaxf(amax_abs(v[2]), amax_abs(v[3])));
  }
  for (long j = n4 * 4 + threadIdx.x; j < n; j += 1024) m = fmaxf(m, amax_abs(x[j]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; w++) m = fmaxf(m, red[w]);
    *word = __float_as_uint(m);
  }
}
// Any size and alignment: atomic max into a word the caller has zeroed.  `head` scalars up to the first 16-byte boundary,
// n4 float4, `tail` scalars (block 0 takes the scalars).
// ONE commit per block (the block's maximum through LDS): the word starts at zero, so the first wave of every block sees a
// value it can raise - with a commit per wave a 6 MB tensor issued ~6 000 same-address atomics and took 95 us (round 4 trace:
// 64 GB/s); four loads in flight per thread.
__device__ __forceinline__ void amax_commit_block(unsigned* word, float m) {
  __shared__ float wmax[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    if (m > 0.f) {
      const unsigned bits = __float_as_uint(m);
      if (bits > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, bits);
    }
  }
}
__global__ __launch_bounds__(256) void k_amax(const float* __restrict__ x, int head, long n4, int tail,
                                              unsigned* __restrict__ word) {
  float m = 0.f;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x + head);
  const long stride = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const f32x4 v0 = x4[i], v1 = x4[i + stride], v2 = x4[i + 2 * stride], v3 = x4[i + 3 * stride];
    auto mx = [](const f32x4& v) {
      return fmaxf(fmaxf(amax_abs(v[0]), amax_abs(v[1])), fmaxf(amax_abs(v[2]), amax_abs(v[3])));
    };
    m = fmaxf(m, fmaxf(fmaxf(mx(v0), mx(v1)), fmaxf(mx(v2), mx(v3))));
  }
  for (; i < n4; i += stride) {
    const f32x4 v = x4[i];
    m = fmaxf(fmaxf(m, fmaxf(amax_abs(v[0]), amax_abs(v[1]))), fmaxf(amax_abs(v[2]), amax_abs(v[3])));
  }
  if (blockIdx.x == 0) {
    if ((int)threadIdx.x < head) m = fmaxf(m, amax_abs(x[threadIdx.x]));
    if ((int)threadIdx.x < tail) m = fmaxf(m, amax_abs(x[head + n4 * 4 + threadIdx.x]));
  }
  amax_commit_block(word, m);
}
// The rows of a row set only (the others may hold no data): row (b, i) -> b * V + ids[i], F % 4 == 0
__global__ __launch_bounds__(256) void k_amax_rows(const float* __restrict__ x, RowSet rs, int B, int F,
                                                   unsigned* __restrict__ word) {
  const int f4 = F >> 2;
  const long tot = (long)B * rs.n * f4;
  float m = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < tot; i += (long)gridDim.x * 256) {
    const long row = i / f4;
    const int c = (int)(i - row * f4);
    const int b = (int)(row / rs.n), r = (int)(row - (long)b * rs.n);
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((long)b * rs.V + (rs.ids ? rs.ids[r] : r)) * F + c * 4);
    m = fmaxf(fmaxf(m, fmaxf(amax_abs(v[0]), amax_abs(v[1]))), fmaxf(amax_abs(v[2]), amax_abs(v[3])));
  }
  amax_commit_block(word, m);
}

void amax_one_block(const float* x, long n, unsigned* word, hipStream_t stream) {
  hipLaunchKernelGGL(k_amax_one_block, dim3(1), dim3(1024), 0, stream, x, n, word);
}

}  // namespace p2m

using namespace p2m;

extern "C" int p2m_amax(const float* x, int64_t n, void* word, void* stream) {
  P2M_CHECK_ARG(x && word && n >= 0, "null pointer");
  P2M_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3) == 0, "x must be 4-byte aligned");
  if (n == 0) return P2M_OK;
  long head = (long)((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) / 4;
  if (head > n) head = n;
  const long n4 = (n - head) / 4;
  const int tail = (int)(n - head - 4 * n4);
  const int grid = (int)(n4 < 256l * 4 * 1024 ? (n4 > 0 ? cdiv(n4, 256 * 4) : 1) : 1024);    // >= 4 float4 per thread
  hipLaunchKernelGGL(k_amax, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (int)head, n4, tail,
                     static_cast<unsigned*>(word));
  return check_launch("amax");
}

extern "C" int p2m_amax_rows(p2m_graph_t gh, int32_t row_set, const float* x, int32_t B, int32_t F, void* word,
                             void* stream) {
  P2M_CHECK_ARG(gh && x && word, "null pointer");
  P2M_CHECK_ARG(row_set >= 0 && row_set <= 4, "row_set must be 0 (live rows) or 1..4");
  P2M_CHECK_ARG(F > 0 && F % 4 == 0, "F must be a positive multiple of 4");
  const Graph& gr = *reinterpret_cast<const Graph*>(gh);
  RowSet rs;
  if (row_set == 0) {                       // every row that holds data: all of them, or the live ones under classes
    rs.V = gr.V;
    rs.ids = gr.live_ids;
    rs.n = gr.live_ids ? gr.n_live : gr.V;
  } else {
    rs = row_set_of(gr, row_set);
  }
  if (B <= 0 || rs.n == 0) return P2M_OK;
  const long tot = (long)B * rs.n * (F / 4);
  const int grid = (int)(tot < 256l * 2048 ? cdiv(tot, 256) : 2048);       // (one load per thread and iteration: keep the grid wide)
  hipLaunchKernelGGL(k_amax_rows, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, rs, B, F, static_cast<unsigned*>(word));
  return check_launch("amax_rows");
}
