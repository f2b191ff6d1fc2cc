// Weight-gradient contractions of the Pose2Mesh Chebyshev GCN on gfx950 matrix cores.
//
//   k_gemm_tn[_ws]  : P[chunk] = [A0|A1|A2]^T * G  over a chunk of rows (weight gradient)
//   k_naive_gemm_tn : scalar fall-back for the odd shapes (Fin=5 first conv, Fout=3 last conv)
//
// The autograd backward of nn.Linear inside graph_conv_cheby (lib/models/backbones/cheby_graph_conv.py:37) and of the fc lift
// (lib/models/meshnet.py:105).  The three arithmetics (include/p2m.h, P2M_ARITH_*), the block and wave tiling and the
// wave-specialised staging are those of the plane contractions: gemm_planes.hip.
#include "p2m_gemm.h"
#include "p2m_probe.h"

namespace p2m {

// ---------------------------------------------------------------------------------------------
// weight gradient: P[chunk][kk][n] = sum_{r in chunk} Z[r][kk] * G[r][n]
// ---------------------------------------------------------------------------------------------
struct TnArgs {
  const float* A[3] = {};
  const float* G[3] = {};   // nplanesG column planes of width Gc (N = nplanesG * Gc)
  int Gc = 0;
  float* P = nullptr;
  float* Pdb = nullptr;
  long M = 0, chunk_rows = 0;
  int nplanesA = 0, Ka = 0, a0_shift = 0, Ktot = 0, N = 0;
  int nkt = 0, ntn = 0;
  // row-set mode: chunk = (sample b, split s) over logical rows i < nset; A and G plane 0 are read at the actual row
  // b*V + ids[i], G planes 1,2 at the compact row b*nset + i when `compact`
  const int* ids = nullptr;
  int nset = 0, V = 0, splits = 0, compact = 0;
  // k_gemm_tn_ws, row-set mode, splits = 1: a chunk is `spc` consecutive WHOLE samples (the last chunk: what is left of the B
  // samples) - fewer partials for the unpack to read where a sample has few rows and the gradient many tiles
  int spc = 1, B = 0;
  // two-fp16-slice mode: amax words of the A planes and of the G planes (+ binades of headroom), p2m_split.h
  const unsigned* a_amax = nullptr;
  const unsigned* g_amax = nullptr;
  int a_bits = 0, g_bits = 0;
  // activation on load of A plane 0 (k_gemm_tn_ws): the operand is max(fma(A, a_scale[k], a_shift[k]), 0); or null
  const float* a_scale = nullptr;
  const float* a_shift = nullptr;
  int nchunks = 0;       // k_gemm_tn_ws: one-dimensional grid of ceil(nchunks / 8) * 8 * nkt * ntn blocks (XCD-aware mapping)
  int accum = 0;         // P += result instead of P = result (single chunk only: a plain Linear's weight gradient added
                         // straight into the parameter's .grad, p2m_gemm_tn_acc)
};

template <int BN, bool ROWS = false>
__global__ __launch_bounds__(256) void k_gemm_tn(TnArgs g) {
  constexpr int WTN = BN / 2;
  constexpr int TN = WTN / 32;
  constexpr int TM = 2;
  constexpr int RK = 32;                 // rows (reduction) per LDS stage
  constexpr int GPASS = BN / 32;         // float4 loads of G per thread per stage
  constexpr int GROWS = 256 / (BN / 4);
  __shared__ float smem[2 * RK * BM + 2 * RK * BN];
  float* As = smem;                      // [buf][r][kk]  (kk contiguous)
  float* Gs = smem + 2 * RK * BM;        // [buf][r][n]

  const int tile = blockIdx.x;
  const int kt = tile / g.ntn, nt = tile % g.ntn;
  const int chunk = blockIdx.y;
  const int kk0 = kt * BM, n0 = nt * BN;
  // flat mode: rows [r_begin, r_end) of the flattened (B*V) dimension; ROWS mode: logical rows of one sample
  const int rs_b = ROWS ? chunk / g.splits : 0;
  const long r_begin = ROWS ? (long)(chunk - rs_b * g.splits) * g.chunk_rows : (long)chunk * g.chunk_rows;
  long r_end = r_begin + g.chunk_rows;
  if (r_end > (ROWS ? (long)g.nset : g.M)) r_end = ROWS ? (long)g.nset : g.M;

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lhi = lane >> 5;

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

  // this thread's column of the A tile: fixed plane / offset for the whole kernel
  const int a_r = t >> 5, a_c4 = (t & 31) * 4;
  const int kk = kk0 + a_c4;
  const bool a_ok = kk < g.Ktot;
  const int ap = a_ok ? kk / g.Ka : 0;
  const int ak = kk - ap * g.Ka;
  const float* Ap = g.A[ap];
  const int ash = (ap == 0) ? g.a0_shift : 0;
  const int g_r = t / (BN / 4), g_c4 = (t % (BN / 4)) * 4;
  const bool g_ok = (n0 + g_c4) < g.N;
  const int gq = g_ok ? (n0 + g_c4) / g.Gc : 0;
  const int gcol = (n0 + g_c4) - gq * g.Gc;
  const float* Gp = g.G[gq];

  float4 ra[4], rg[GPASS];
  float4 dbs = make_float4(0.f, 0.f, 0.f, 0.f);
  // ROWS: vertex ids of the rows this thread loads, fetched ONE STAGE AHEAD of the data loads that depend on them
  int ida[ROWS ? 4 : 1], idg[ROWS ? GPASS : 1];
  auto load_ids = [&](long r0) {
    if (!ROWS) return;
#pragma unroll
    for (int ps = 0; ps < 4; ps++) {
      const long r = r0 + ps * 8 + a_r;
      ida[ps] = (r < r_end) ? g.ids[r] : 0;
    }
#pragma unroll
    for (int ps = 0; ps < GPASS; ps++) {
      const long r = r0 + ps * GROWS + g_r;
      idg[ps] = (r < r_end) ? g.ids[r] : 0;
    }
  };
  auto load_stage = [&](long r0) {
#pragma unroll
    for (int ps = 0; ps < 4; ps++) {
      long r = r0 + ps * 8 + a_r;
      if (a_ok && r < r_end) {
        if (ROWS) r = (long)rs_b * g.V + ida[ps];
        ra[ps] = *reinterpret_cast<const float4*>(Ap + (r >> ash) * g.Ka + ak);
      } else {
        ra[ps] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int ps = 0; ps < GPASS; ps++) {
      long r = r0 + ps * GROWS + g_r;
      if (g_ok && r < r_end) {
        if (ROWS) r = (gq == 0 || !g.compact) ? (long)rs_b * g.V + idg[ps] : (long)rs_b * g.nset + r;
        rg[ps] = *reinterpret_cast<const float4*>(Gp + r * g.Gc + gcol);
      } else {
        rg[ps] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      dbs.x += rg[ps].x; dbs.y += rg[ps].y; dbs.z += rg[ps].z; dbs.w += rg[ps].w;
    }
    load_ids(r0 + RK);
  };
  auto store_stage = [&](int buf) {
    float* as = As + buf * RK * BM;
#pragma unroll
    for (int ps = 0; ps < 4; ps++)
      *reinterpret_cast<float4*>(as + (ps * 8 + a_r) * BM + a_c4) = ra[ps];
    float* gs = Gs + buf * RK * BN;
#pragma unroll
    for (int ps = 0; ps < GPASS; ps++)
      *reinterpret_cast<float4*>(gs + (ps * GROWS + g_r) * BN + g_c4) = rg[ps];
  };

  load_ids(r_begin);
  load_stage(r_begin);
  store_stage(0);
  __syncthreads();
  int it = 0;
  for (long r0 = r_begin; r0 < r_end; r0 += RK, it++) {
    const int cur = it & 1;
    const bool more = (r0 + RK) < r_end;
    if (more) load_stage(r0 + RK);
    const float* as = As + cur * RK * BM + lhi * BM + wm * 64 + l31;
    const float* gs = Gs + cur * RK * BN + lhi * BN + wn * WTN + l31;
#pragma unroll
    for (int ks = 0; ks < RK / 2; ks++) {
      float a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; i++) a[i] = as[2 * ks * BM + i * 32];
#pragma unroll
      for (int j = 0; j < TN; j++) b[j] = gs[2 * ks * BN + j * 32];
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) store_stage(cur ^ 1);
    __syncthreads();
  }

  float* Pc = g.P + (long)chunk * g.Ktot * g.N;
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const int n = n0 + wn * WTN + j * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int krow = kk0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        if (krow < g.Ktot && n < g.N) {
          float* d = Pc + (long)krow * g.N + n;
          *d = g.accum ? *d + acc[i][j][r] : acc[i][j][r];
        }
      }
    }
  if (kt == 0 && g.Pdb != nullptr) {
    // bias gradient: column sums of G over this chunk (reduce the GROWS row groups through LDS)
    float* red = smem;  // [GROWS][BN]
    *reinterpret_cast<float4*>(red + g_r * BN + g_c4) = dbs;
    __syncthreads();
    if (t < BN) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < GROWS; q++) s += red[q * BN + t];
      if (n0 + t < g.N) g.Pdb[(long)chunk * g.N + n0 + t] = s;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Weight gradient on the BF16 matrix pipe (same 3-slice split as k_gemm_planes_ws).
//
// Both operands are activations stored row-major over the REDUCTION index r ([r][kk], [r][n]), while the MFMA wants
// each lane to hold 8 consecutive r of one kk / n.  The transpose happens in registers on the way into LDS: a staging
// thread owns a 4 (r) x 4 (kk) block (four float4 loads, rows r..r+3), cuts it into slices and writes, per kk, the
// four r of a slice as ONE 8-byte store into the kk-major image [slice][kk][16 r + 8 pad].  Staging waves 4,5 stage A,
// waves 6,7 stage G (wave-uniform roles, identical instruction stream); waves 0..3 run the MFMAs.
// Loads are unconditional (rows past the end are clamped and their values zeroed; columns past Ktot / N are clamped
// and never stored), with two register stages of lead and an LDS-only barrier, as in k_gemm_planes_ws.  In ROWS mode
// the vertex ids of a stage are fetched two phases before the data loads that depend on them (g.ids is zero-padded
// by ID_SLACK entries at bake time, so those 16-byte id loads need no bounds).
// ---------------------------------------------------------------------------------------------
typedef int i32x4 __attribute__((ext_vector_type(4)));

#ifdef P2M_TN_TRACE
// Probe build only (tools/tn_trace.sh, tools/probes/tn_trace_probe.py): s_memtime stamps of every wave of one block at the
// phase boundaries of 32 steady-state stages.  [wave][stage - P2M_TN_TRACE_S0][event]; events: 0 past the barrier,
// 1 operands there (staging: global loads landed; MFMA: fragments read), 2 work issued (LDS stores / last MFMA), 3 at the barrier
__device__ unsigned long long g_tn_tr[8][32][4];
#ifndef P2M_TN_TRACE_S0
#define P2M_TN_TRACE_S0 40
#endif
#define P2M_TNT(s, ev)                                                                                          \
  do {                                                                                                          \
    if (tnt_on && (s) >= P2M_TN_TRACE_S0 && (s) < P2M_TN_TRACE_S0 + 32)                                         \
      g_tn_tr[threadIdx.x >> 6][(s) - P2M_TN_TRACE_S0][ev] = __builtin_amdgcn_s_memtime();                      \
  } while (0)
#else
#define P2M_TNT(s, ev) do { } while (0)
#endif

// Wave-specialised (4 MFMA waves + 4 staging waves, one LDS-only barrier per 16-row stage, two register stages of lead);
// see k_gemm_planes_ws.
template <int BN, bool ROWS, int NS>
__global__ __launch_bounds__(512, 2) void k_gemm_tn_ws(TnArgs g) {
  typedef typename SliceFrag<NS>::type frag_t;
  constexpr int RK = 16;                 // rows (reduction) per stage = one bf16 MFMA k-step
  constexpr int LDX = RK + 8;            // bf16 per LDS row: 48-byte stride, conflict-free ds_read_b128
  constexpr int WTN = BN / 2;
  constexpr int TN = WTN / 32;
  constexpr int TM = 2;
  constexpr int A_BUF = NS * BM * LDX;
  constexpr int G_BUF = NS * BN * LDX;
  __shared__ __attribute__((aligned(16))) float smem[(2 * A_BUF + 2 * G_BUF) / 2];
  unsigned short* As = reinterpret_cast<unsigned short*>(smem);
  unsigned short* Gs = As + 2 * A_BUF;

  // The n-tiles of one row chunk read the SAME rows of A: give them consecutive slots of one XCD (observed dispatch: block
  // b runs on XCD b % 8), so that A comes from HBM once and from that XCD's L2 for the others.  With the chunk in
  // blockIdx.y the three n-tiles of a 128 x 384 weight gradient sat on three different XCDs (PMC: 1.9x the algorithmic
  // bytes per launch; 1 408 -> 884 MB on the finest level, 144 -> 131 GB per train step).  +0.4 % on the step.
  // Fewer than 8 chunks (a plain Linear's weight gradient over a batch of rows: ONE chunk, p2m_gemm_tn_acc): that mapping
  // would put every live block on the XCDs 0 .. nchunks - 1 (measured: one chunk of 1024 tiles ran on 32 of the 256 CUs,
  // 740 us for 8.6 GFLOP); consecutive blocks then simply take consecutive tiles.
  const int ntiles = g.nkt * g.ntn;
  int tile, chunk;
  if (g.nchunks >= 8) {
    const int slot = blockIdx.x >> 3;
    tile = slot % ntiles;
    chunk = (slot / ntiles) * 8 + (blockIdx.x & 7);
  } else {
    tile = blockIdx.x % ntiles;
    chunk = blockIdx.x / ntiles;
  }
  if (chunk >= g.nchunks) return;
  const int kt = tile / g.ntn, nt = tile % g.ntn;
  const int kk0 = kt * BM, n0 = nt * BN;
  const int spc = ROWS ? g.spc : 1;
  const int rs_b = ROWS ? (spc > 1 ? chunk * spc : chunk / g.splits) : 0;      // (first) sample of this chunk
  const int nsamp = (ROWS && spc > 1) ? (g.B - rs_b < spc ? g.B - rs_b : spc) : 1;
  const long r_begin = ROWS ? (spc > 1 ? 0L : (long)(chunk - rs_b * g.splits) * g.chunk_rows) : (long)chunk * g.chunk_rows;
  long r_end = r_begin + g.chunk_rows;
  if (r_end > (ROWS ? (long)g.nset : g.M)) r_end = ROWS ? (long)g.nset : g.M;
  const int nst = r_end > r_begin ? (int)((r_end - r_begin + RK - 1) / RK) : 0;

  const int t = threadIdx.x;
  const bool producer = t >= 256;          // waves 4..7 stage, waves 0..3 run the MFMAs (k_gemm_planes_ws)
#ifdef P2M_TN_TRACE
  const bool tnt_on = blockIdx.x == P2M_TN_TRACE && (t & 63) == 0 && BN == 128 && ROWS;
#endif
  const int pt = t & 255;
  const int lane = t & 63, wave = (t >> 6) & 3;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lhi = lane >> 5;

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

  // staging role of this thread: a 4-row x 4-column block of the A tile (pt < 128) or of the G tile.  The role is
  // wave-uniform (waves 4,5 stage A, waves 6,7 stage G): readfirstlane tells the compiler so, and the role-dependent
  // code becomes scalar branches instead of exec-masked ones
  const bool is_a = __builtin_amdgcn_readfirstlane((int)(pt < 128)) != 0;
  const int st = pt & 127;
  const int rq = st & 3;                                   // row quad of the 16-row stage
  const int c4 = is_a ? (st >> 2) : (st >> 2) % (BN / 4);  // column quad (BN = 64: the upper threads duplicate)
  const float* src;       // plane base + column offset
  int pitch, shift;
  bool compact_rows;      // ROWS: read at the compact row b*nset + r instead of b*V + ids[r]
  unsigned short* dst;    // LDS image (buffer 0, slice 0) of this thread's first column, at its row quad
  int slice_stride;
  {
    if (is_a) {
      int kk = kk0 + c4 * 4;
      if (kk >= g.Ktot) kk = 0;                            // clamped: those rows of P are never stored
      const int ap = kk / g.Ka;
      src = g.A[ap] + (kk - ap * g.Ka);
      pitch = g.Ka;
      shift = (ap == 0) ? g.a0_shift : 0;
      compact_rows = false;
      dst = As + (c4 >> 2) * 16 * LDX + (c4 & 3) * 2 * LDX + rq * 4;
      slice_stride = BM * LDX;
    } else {
      int n = n0 + c4 * 4;
      if (n >= g.N) n = 0;
      const int gq = n / g.Gc;
      src = g.G[gq] + (n - gq * g.Gc);
      pitch = g.Gc;
      shift = 0;
      compact_rows = ROWS && gq != 0 && g.compact;
      dst = Gs + (c4 >> 2) * 16 * LDX + (c4 & 3) * 2 * LDX + rq * 4;
      slice_stride = BN * LDX;
    }
  }
  const int buf_stride = is_a ? A_BUF : G_BUF;
  // activation on load (A staging waves only; wave-uniform): the coefficients of this thread's four columns
  const bool a_act = __builtin_amdgcn_readfirstlane((int)(is_a && g.a_scale != nullptr)) != 0;
  f32x4 act_sc = {1.f, 1.f, 1.f, 1.f}, act_sh = {0.f, 0.f, 0.f, 0.f};
  if (a_act) {
    int kk = kk0 + c4 * 4;
    if (kk >= g.Ktot) kk = 0;
    act_sc = *reinterpret_cast<const f32x4*>(g.a_scale + kk);
    act_sh = *reinterpret_cast<const f32x4*>(g.a_shift + kk);
  }
  float my_sc = 1.f;                     // two-fp16-slice mode: this staging wave's operand is staged times 2^s
  int descale = 0;
  if (NS == 2) {
    const int sa = slice_scale_exp(*g.a_amax, g.a_bits), sg = slice_scale_exp(*g.g_amax, g.g_bits);
    my_sc = exp2_int(is_a ? sa : sg);
    descale = -(sa + sg);
  }
  const int* idp = ROWS ? g.ids + r_begin + rq * 4 : nullptr;
  // Addresses: per-thread 64-bit base (plane + column + the first row of this block's sample / chunk), fixed for the
  // whole kernel, plus a 32-bit byte offset per load = (row relative to that base >> shift) * pitch * 4: three 32-bit
  // VALU instructions and one 64-bit add per load instead of the 64-bit multiply-add chain.  base rows are even
  // (V is even whenever shift = 1; chunk_rows is a multiple of 16), so (base + rel) >> shift == (base >> shift) + (rel >> shift).
  const long base_row = ROWS ? (compact_rows ? (long)rs_b * g.nset + r_begin : (long)rs_b * g.V) : r_begin;
  const char* srcb = reinterpret_cast<const char*>(src + (base_row >> shift) * pitch);
  const long samp_bytes = ROWS ? (((long)(compact_rows ? g.nset : g.V) >> shift) * pitch) * 4 : 0;   // sample to sample
  const unsigned pitch4 = (unsigned)pitch * 4u;
  const int nrows_m1 = (int)(r_end - r_begin) - 1;

  f32x4 x0[4], x1[4];       // two register stages (native vector types: no scratch)
  i32x4 id0 = {0, 0, 0, 0}, id1 = {0, 0, 0, 0};
  f32x4 dbs = {0.f, 0.f, 0.f, 0.f};

  // No bounds: the tables end in ID_SLACK (p2m_common.h) zero entries.  The prologue fetches stages 0 .. 4 whatever nst is,
  // so the highest index read is r_begin + 4 * RK + 3 * 4 + 3 = r_begin + 79 <= nset - 1 + 79 < nset + ID_SLACK (r_begin <
  // nset in every chunk that gets here: nst > 0); the loops stay below that (stage nst + 1: r_begin + 16 nst + 31 <=
  // nset + 46).  The matching load_stage is range-checked: ids past the end are never used as rows of the set.
  static_assert(ID_SLACK >= 5 * RK && RK == ID_STAGE_ROWS, "the id prefetch of the prologue reads stages 0 .. 4");
  auto load_ids = [&](int kc, i32x4& id) {
    if (ROWS) id = *reinterpret_cast<const i32x4*>(idp + (long)kc * RK);
  };
  // CLAMP = false: every row of the stage exists (steady state); true: rows past the end are clamped to the last one
  auto load_stage = [&](int kc, f32x4 (&x)[4], const i32x4& id, auto clamp_tag) {
    constexpr bool CLAMP = decltype(clamp_tag)::value;
#pragma unroll
    for (int ps = 0; ps < 4; ps++) {
      int rel = kc * RK + rq * 4 + ps;                     // row relative to r_begin
      if (CLAMP && rel > nrows_m1) rel = nrows_m1;
      if (ROWS && !compact_rows) rel = id[ps];             // vertex id inside the sample (slack entries: vertex 0)
      const unsigned off = __umul24((unsigned)(rel >> shift), pitch4);
#ifdef P2M_TN_ABL_NOLOAD
      x[ps] = f32x4{__uint_as_float(off), 1.f, 2.f, 3.f};
#else                                   // (non-temporal loads - `nt` - of G, or of both operands: +6.5 % / +5 %, round 6)
      x[ps] = *reinterpret_cast<const f32x4*>(srcb + off);
#endif
    }
  };
  // TAIL = true: rows past the end of the chunk are zeroed before they are used
  auto store_stage = [&](int buf, int kc, f32x4 (&x)[4], auto tail_tag) {
    constexpr bool TAIL = decltype(tail_tag)::value;
#pragma unroll
    for (int ps = 0; ps < 4; ps++) asm volatile("" : "+v"(x[ps]));     // see k_gemm_planes_bx
    P2M_TNT(kc, 1);
    if (a_act) {                                                        // (before the tail's zeroing: act(0) != 0)
#pragma unroll
      for (int ps = 0; ps < 4; ps++)
#pragma unroll
        for (int e = 0; e < 4; e++) x[ps][e] = fmaxf(fmaf(x[ps][e], act_sc[e], act_sh[e]), 0.f);
    }
    if (TAIL) {
      const int rlast = nrows_m1 + 1 - (kc * RK + rq * 4);             // rows of this quad that exist
#pragma unroll
      for (int ps = 0; ps < 4; ps++)
        if (ps >= rlast) x[ps] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (!is_a) {                                                        // bias gradient: column sums of G (scalar branch)
#pragma unroll
      for (int ps = 0; ps < 4; ps++) dbs += x[ps];
    }
    unsigned short* d = dst + buf * buf_stride;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      u32x2 sl[NS];
#ifdef P2M_TN_ABL_NOSLICE
      for (int q = 0; q < NS; q++) sl[q] = u32x2{__float_as_uint(x[q & 1][e]), __float_as_uint(x[2 + (q & 1)][e])};
#else
      split_pack4<NS>(x[0][e], x[1][e], x[2][e], x[3][e], my_sc, sl);
#endif
      // LDS rows are PERMUTED inside every block of 16: column 4 c + e of the block lives in row 2 c + (e & 1) + 8 (e >> 1).
      // The 16 lanes of a ds_write_b64 group are 4 column quads x 4 row quads: with the natural order their rows are 4
      // apart = 48 dwords = 16 banks, i.e. 2-way conflicts on every store (PMC: 33 % of the kernel's LDS cycles); rows
      // 2 apart are 24 dwords: four distinct 8-dword windows.  The MFMA waves read a block's 16 rows as a set either way.
#pragma unroll
      for (int q = 0; q < NS; q++)
        *reinterpret_cast<u32x2*>(d + ((e & 1) + 8 * (e >> 1)) * LDX + q * slice_stride) = sl[q];
    }
    P2M_TNT(kc, 2);
  };
  using std::false_type;
  using std::true_type;
  auto compute = [&](int cur, int kc) {
    // (row permutation of the staging stores: logical row j of a 16-block -> 2 (j >> 2) + (j & 1) + 8 ((j & 3) >> 1))
    const int lrow = (l31 & 16) + 2 * ((l31 & 15) >> 2) + (l31 & 1) + 8 * ((l31 & 3) >> 1);
    const unsigned short* as = As + cur * A_BUF + (wm * 64 + lrow) * LDX + lhi * 8;
    const unsigned short* gs = Gs + cur * G_BUF + (wn * WTN + lrow) * LDX + lhi * 8;
    frag_t fa[NS][TM], fb[NS][TN];       // [slice, high first][tile]
#pragma unroll
    for (int sl = 0; sl < NS; sl++) {
#pragma unroll
      for (int i = 0; i < TM; i++)
        fa[sl][i] = __builtin_bit_cast(frag_t, *reinterpret_cast<const u32x4*>(as + (sl * BM + i * 32) * LDX));
#pragma unroll
      for (int j = 0; j < TN; j++)
        fb[sl][j] = __builtin_bit_cast(frag_t, *reinterpret_cast<const u32x4*>(gs + (sl * BN + j * 32) * LDX));
    }
#ifdef P2M_TN_TRACE
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    P2M_TNT(kc, 1);
#endif
#define P2M_PAIR(SA, SB)                                                                       \
  _Pragma("unroll") for (int i = 0; i < TM; i++) _Pragma("unroll") for (int j = 0; j < TN; j++) \
      acc[i][j] = slice_mfma<NS>(fa[SA][i], fb[SB][j], acc[i][j]);
#ifdef P2M_TN_ABL_NOMFMA
    if constexpr (NS == 3) {
      P2M_PAIR(0, 0)
      for (int sl = 1; sl < NS; sl++)
        for (int i = 0; i < TM; i++) for (int j = 0; j < TN; j++) { asm volatile("" :: "v"(fa[sl][i])); asm volatile("" :: "v"(fb[sl][j])); }
    } else
#endif
    if constexpr (NS == 3) {            // smallest products first
      P2M_PAIR(2, 0)
      P2M_PAIR(0, 2)
      P2M_PAIR(1, 1)
      P2M_PAIR(1, 0)
      P2M_PAIR(0, 1)
      P2M_PAIR(0, 0)
    } else {
      P2M_PAIR(1, 0)
      P2M_PAIR(0, 1)
      P2M_PAIR(0, 0)
    }
#undef P2M_PAIR
    P2M_TNT(kc, 2);
    (void)kc;
  };
  auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

  for (int sb = 0; sb < nsamp; sb++) {      // (one pass unless the chunk is several whole samples: same stages, next sample)
  if (nst > 0) {
    if (producer) {
      // stage s lives in register set s & 1 and LDS buffer s & 1; ids of stage s in id set s & 1.  During iteration
      // kc (consumers: MFMAs of stage kc) the producers store stage kc+1 and refill its set with stage kc+3.
      load_ids(0, id0);
      load_ids(1, id1);
      load_stage(0, x0, id0, true_type{});
      load_ids(2, id0);
      load_stage(nst > 1 ? 1 : 0, x1, id1, true_type{});
      load_ids(3, id1);
      store_stage(0, 0, x0, true_type{});
      load_stage(nst > 2 ? 2 : nst - 1, x0, id0, true_type{});
      load_ids(4, id0);
      lds_barrier();
      int kc = 0;
      // steady state: stages up to kc+4 are FULL stages (the possibly partial last stage nst-1 is left to the tail), so
      // neither the loads nor the stores carry clamps, zeroing or conditions
      for (; kc + 5 < nst; kc += 2) {
        P2M_TNT(kc + 1, 0);
        store_stage(1, kc + 1, x1, false_type{});
        load_stage(kc + 3, x1, id1, false_type{});
        load_ids(kc + 5, id1);
        P2M_TNT(kc + 1, 3);
        lds_barrier();
        P2M_TNT(kc + 2, 0);
        store_stage(0, kc + 2, x0, false_type{});
        load_stage(kc + 4, x0, id0, false_type{});
        load_ids(kc + 6, id0);
        P2M_TNT(kc + 2, 3);
        lds_barrier();
      }
      for (; kc < nst; kc += 2) {                // tail: same rotation, range-checked
        if (kc + 1 < nst) store_stage(1, kc + 1, x1, true_type{});
        if (kc + 3 < nst) {
          load_stage(kc + 3, x1, id1, true_type{});
          load_ids(kc + 5, id1);
        }
        lds_barrier();
        if (kc + 1 < nst) {
          if (kc + 2 < nst) store_stage(0, kc + 2, x0, true_type{});
          if (kc + 4 < nst) {
            load_stage(kc + 4, x0, id0, true_type{});
            load_ids(kc + 6, id0);
          }
          lds_barrier();
        }
      }
    } else {
      lds_barrier();                             // stage 0 is in LDS
      for (int kc = 0; kc < nst; kc++) {
        P2M_TNT(kc, 0);
        compute(kc & 1, kc);
        P2M_TNT(kc, 3);
        lds_barrier();
      }
    }
  }
  srcb += samp_bytes;
  }
  __syncthreads();

  float* Pc = g.P + (long)chunk * g.Ktot * g.N;
  if (!producer) {
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TN; j++) {
        const int n = n0 + wn * WTN + j * 32 + l31;
        // accumulate form (p2m_gemm_tn_acc): the 16 old values of the tile first, all loads in flight, then add and store
        // (one load - add - store chain per element waited for every load in turn: 116 us for a 4096 x 4096 gradient)
        // (round 8) `accumulate` is hoisted around the tile: under a per-element condition the loads were branches whose
        // vmcnt(0) stood in the plain form too, where it drained the 16 stores of the tile before - the form every conv's
        // weight gradient runs.  The plain form keeps its `+ 0`: -0 is stored as +0, as before.
        if (g.accum) {
          float old[16];
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int krow = kk0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            old[r] = (krow < g.Ktot && n < g.N) ? Pc[(long)krow * g.N + n] : 0.f;
          }
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int krow = kk0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            if (krow < g.Ktot && n < g.N) Pc[(long)krow * g.N + n] = __builtin_ldexpf(acc[i][j][r], descale) + old[r];
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int krow = kk0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            if (krow < g.Ktot && n < g.N) Pc[(long)krow * g.N + n] = __builtin_ldexpf(acc[i][j][r], descale) + 0.f;
          }
        }
      }
  }
  if (kt == 0 && g.Pdb != nullptr) {
    // bias gradient: column sums of G over this chunk; the four row quads of a column quad meet through LDS
    float* red = smem;  // [4 (rq)][BN]
    if (producer && !is_a && (st >> 2) < BN / 4) *reinterpret_cast<f32x4*>(red + rq * BN + c4 * 4) = dbs;
    __syncthreads();
    if (t < BN) {
      const float sum = red[t] + red[BN + t] + red[2 * BN + t] + red[3 * BN + t];
      if (n0 + t < g.N) g.Pdb[(long)chunk * g.N + n0 + t] = sum;
    }
  }
}

__global__ void k_naive_gemm_tn(TnArgs g) {
  // one thread per output (kk, n), one block row per chunk
  int o = blockIdx.x * blockDim.x + threadIdx.x;
  const int chunk = blockIdx.y;
  const long r_begin = (long)chunk * g.chunk_rows;
  long r_end = r_begin + g.chunk_rows;
  if (r_end > g.M) r_end = g.M;
  const int nout = g.Ktot * g.N;
  if (o < nout) {
    int kk = o / g.N, n = o - kk * g.N;
    int p = kk / g.Ka, k = kk - p * g.Ka;
    const float* Ap = g.A[p];
    int sh = p == 0 ? g.a0_shift : 0;
    float acc = 0.f;
    const int q = n / g.Gc;
    const float* Gq = g.G[q] + (n - q * g.Gc);
    for (long r = r_begin; r < r_end; r++) acc = fmaf(Ap[(r >> sh) * g.Ka + k], Gq[r * g.Gc], acc);
    g.P[(long)chunk * nout + o] = g.accum ? g.P[(long)chunk * nout + o] + acc : acc;
  }
  if (g.Pdb != nullptr && o < g.N) {
    float s = 0.f;
    const int q = o / g.Gc;
    const float* Gq = g.G[q] + (o - q * g.Gc);
    for (long r = r_begin; r < r_end; r++) s += Gq[r * g.Gc];
    g.Pdb[(long)chunk * g.N + o] = s;
  }
}

}  // namespace p2m

using namespace p2m;

// picks the instantiation (tile width from N, the kernel from the arithmetic) and the grid that goes with it
template <bool ROWS>
static void launch_gemm_tn(TnArgs& g, int arith, hipStream_t s) {
  const bool bx = arith != P2M_ARITH_F32;
  g.nkt = cdiv(g.Ktot, BM);
  // N = 192 (three planes of 64): two 128-wide tiles (the second half empty) stage A twice, three 64-wide tiles thrice
  const bool wide = g.N % 128 == 0 || (bx && g.N > 128);
  g.ntn = cdiv(g.N, wide ? 128 : 64);
  const dim3 grid(g.nkt * g.ntn, g.nchunks);
  const dim3 grid_ws((g.nchunks >= 8 ? cdiv(g.nchunks, 8) * 8 : g.nchunks) * g.nkt * g.ntn);
  with_bools([&](auto wide_t) {
    constexpr int BN = decltype(wide_t)::value ? 128 : 64;
    if (arith == P2M_ARITH_F16X2) hipLaunchKernelGGL((k_gemm_tn_ws<BN, ROWS, 2>), grid_ws, dim3(512), 0, s, g);
    else if (bx) hipLaunchKernelGGL((k_gemm_tn_ws<BN, ROWS, 3>), grid_ws, dim3(512), 0, s, g);
    else hipLaunchKernelGGL((k_gemm_tn<BN, ROWS>), grid, dim3(256), 0, s, g);
  }, wide);
}

static int gemm_tn_impl(const float* A0, const float* A1, const float* A2, int32_t nplanesA, int32_t Ka,
                        int32_t a0_shift, const float* G0, const float* G1, const float* G2, int32_t nplanesG,
                        int32_t Gc, int64_t M, int64_t chunk_rows, float* P, float* Pdb, int32_t arith,
                        const void* a_amax, int32_t a_bits, const void* g_amax, int32_t g_bits, int32_t accumulate,
                        void* stream) {
  P2M_CHECK_ARG(nplanesA >= 1 && nplanesA <= 3 && nplanesG >= 1 && nplanesG <= 3, "plane count must be 1..3");
  P2M_CHECK_ARG(arith == P2M_ARITH_F32 || arith == P2M_ARITH_BF16X3 || arith == P2M_ARITH_F16X2, "unknown arithmetic");
  P2M_CHECK_ARG(arith != P2M_ARITH_F16X2 || (a_amax && g_amax), "P2M_ARITH_F16X2 needs the amax words of both operands");
  const int N = nplanesG * Gc;
  P2M_CHECK_ARG(A0 && G0 && P && Ka > 0 && Gc > 0 && chunk_rows > 0, "null pointer or empty shape");
  P2M_CHECK_ARG(a0_shift == 0 || a0_shift == 1, "a0_shift must be 0 or 1");
  if (M <= 0) return P2M_OK;
  TnArgs g;
  g.A[0] = A0; g.A[1] = A1; g.A[2] = A2;
  for (int p = 0; p < nplanesA; p++) P2M_CHECK_ARG(g.A[p] != nullptr, "missing A plane");
  g.G[0] = G0; g.G[1] = G1; g.G[2] = G2; g.Gc = Gc;
  for (int p = 0; p < nplanesG; p++) P2M_CHECK_ARG(g.G[p] != nullptr, "missing G plane");
  g.P = P; g.Pdb = Pdb; g.M = M; g.chunk_rows = chunk_rows;
  g.nplanesA = nplanesA; g.Ka = Ka; g.a0_shift = a0_shift; g.Ktot = nplanesA * Ka; g.N = N;
  g.splits = 1;
  g.a_amax = static_cast<const unsigned*>(a_amax); g.g_amax = static_cast<const unsigned*>(g_amax);
  g.a_bits = a_bits; g.g_bits = g_bits;
  g.nchunks = cdiv(M, chunk_rows);
  g.accum = accumulate;
  P2M_CHECK_ARG(!accumulate || g.nchunks == 1, "accumulation needs the whole reduction in one chunk");
  hipStream_t s = (hipStream_t)stream;
  const bool mfma_ok = (Ka % 4 == 0) && (N % 32 == 0) && (Gc % 4 == 0) && (g.Ktot >= 32);
  if (!mfma_ok) {
    int nout = g.Ktot * N;
    if (nout < N) nout = N;
    hipLaunchKernelGGL(k_naive_gemm_tn, dim3(cdiv(nout, 256), g.nchunks), dim3(256), 0, s, g);
    return check_launch("gemm_tn(naive)");
  }
  launch_gemm_tn<false>(g, arith, s);
  return check_launch("gemm_tn");
}

extern "C" int p2m_gemm_tn(const float* A0, const float* A1, const float* A2, int32_t nplanesA, int32_t Ka,
                           int32_t a0_shift, const float* G0, const float* G1, const float* G2, int32_t nplanesG,
                           int32_t Gc, int64_t M, int64_t chunk_rows, float* P, float* Pdb, int32_t arith,
                           const void* a_amax, int32_t a_bits, const void* g_amax, int32_t g_bits, void* stream) {
  return gemm_tn_impl(A0, A1, A2, nplanesA, Ka, a0_shift, G0, G1, G2, nplanesG, Gc, M, chunk_rows, P, Pdb, arith, a_amax,
                      a_bits, g_amax, g_bits, 0, stream);
}
// P[k][n] += sum_r A[r][k] G[r][n] over ALL M rows in one chunk: the weight gradient of a plain Linear
// (lib/models/posenet.py:19,22,59,68) added straight into the parameter's .grad - no partial buffer, no unpack pass.
extern "C" int p2m_gemm_tn_acc(const float* A, int32_t Ka, const float* G, int32_t N, int64_t M, float* P, int32_t arith,
                               const void* a_amax, const void* g_amax, void* stream) {
  const int64_t chunk_rows = ((M + 31) / 32) * 32;
  return gemm_tn_impl(A, nullptr, nullptr, 1, Ka, 0, G, nullptr, nullptr, 1, N, M, chunk_rows > 0 ? chunk_rows : 32, P,
                      nullptr, arith, a_amax, 0, g_amax, 0, 1, stream);
}

extern "C" int p2m_gemm_tn_rows(p2m_graph_t gh, int32_t row_set, int32_t B, const float* A, int32_t Ka,
                                int32_t a0_shift, const float* G0, const float* G1, const float* G2, int32_t nplanesG,
                                int32_t Gc, int32_t planes_compact, int32_t splits, float* P, float* Pdb,
                                int32_t arith, const void* a_amax, const void* g_amax, int32_t g_bits,
                                const float* a_scale, const float* a_shift, void* stream) {
  P2M_CHECK_ARG(gh && A && G0 && P, "null pointer");
  P2M_CHECK_ARG((a_scale == nullptr) == (a_shift == nullptr), "a_scale / a_shift must both be given or both NULL");
  P2M_CHECK_ARG(a_scale == nullptr || arith != P2M_ARITH_F32, "activation on load exists in the slice arithmetics only");
  P2M_CHECK_ARG(arith == P2M_ARITH_F32 || arith == P2M_ARITH_BF16X3 || arith == P2M_ARITH_F16X2, "unknown arithmetic");
  P2M_CHECK_ARG(arith != P2M_ARITH_F16X2 || (a_amax && g_amax), "P2M_ARITH_F16X2 needs the amax words of both operands");
  P2M_CHECK_ARG(row_set_valid(row_set), "row_set must be 1 (real), 2 (fake), 3 (paired real) or 4 (paired fake)");
  P2M_CHECK_ARG(nplanesG >= 1 && nplanesG <= 3 && (splits >= 1 || splits <= -2),
                "plane count must be 1..3; splits >= 1, or <= -2 (that many whole samples per chunk)");
  P2M_CHECK_ARG(splits >= 1 || arith != P2M_ARITH_F32, "several samples per chunk exist in the slice arithmetics only");
  P2M_CHECK_ARG(Ka % 32 == 0 && Gc % 32 == 0, "Ka and Gc must be multiples of 32");
  P2M_CHECK_ARG(a0_shift == 0 || a0_shift == 1, "a0_shift must be 0 or 1");
  const Graph& gr = *reinterpret_cast<const Graph*>(gh);
  const RowSet rs = row_set_of(gr, row_set);
  if (B <= 0 || rs.n == 0) return P2M_OK;
  TnArgs g;
  g.A[0] = A;
  g.G[0] = G0; g.G[1] = G1; g.G[2] = G2; g.Gc = Gc;
  for (int p = 0; p < nplanesG; p++) P2M_CHECK_ARG(g.G[p] != nullptr, "missing G plane");
  g.P = P; g.Pdb = Pdb; g.M = (long)B * rs.n;
  g.spc = splits < 0 ? -splits : 1;
  g.splits = splits < 0 ? 1 : splits;
  g.chunk_rows = cdiv(rs.n, g.splits);
  if (arith != P2M_ARITH_F32) g.chunk_rows = cdiv(g.chunk_rows, 16) * 16;    // 16-byte aligned id loads; trailing splits may be empty
  g.nplanesA = 1; g.Ka = Ka; g.a0_shift = a0_shift; g.Ktot = Ka; g.N = nplanesG * Gc;
  g.ids = rs.ids; g.nset = rs.n; g.V = rs.V; g.compact = planes_compact;
  g.B = B;
  g.a_amax = static_cast<const unsigned*>(a_amax); g.g_amax = static_cast<const unsigned*>(g_amax);
  g.g_bits = g_bits;
  g.a_scale = a_scale; g.a_shift = a_shift;
  g.nchunks = g.spc > 1 ? cdiv(B, g.spc) : B * g.splits;
  launch_gemm_tn<true>(g, arith, (hipStream_t)stream);
  return check_launch("gemm_tn_rows");
}

#ifdef P2M_TN_TRACE
extern "C" int p2m_tn_trace_dump(unsigned long long* out /* [8][32][4] host */) {
  if (hipDeviceSynchronize() != hipSuccess) return P2M_ERR_HIP;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(p2m::g_tn_tr), sizeof(unsigned long long) * 8 * 32 * 4) == hipSuccess ? P2M_OK
                                                                                                                : P2M_ERR_HIP;
}
#endif
