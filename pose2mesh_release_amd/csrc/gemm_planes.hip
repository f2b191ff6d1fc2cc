// Plane contractions of the Pose2Mesh Chebyshev GCN on gfx950 matrix cores.
//
//   k_gemm_planes[_ws]     : C = [A0|A1|A2] * Bm + bias  (+ addend / un-pool pair-sum, BatchNorm partials in the epilogue)
//   k_gemm_rows_k1         : the row-set form of the above with one A plane and Ka <= 256, slice arithmetics: whole-K tile, no ring
//   k_naive_*              : scalar fall-backs for the odd shapes (Fin=5 first conv, Fout=3 last conv)
//
// Replaces nn.Linear inside graph_conv_cheby (lib/models/backbones/cheby_graph_conv.py:37) and the fc lift
// (lib/models/meshnet.py:105); their autograd backward takes the same kernels for dX and gemm_tn.hip for the weight gradient.
// 1e-4 vertex parity needs fp32 products; gfx950 has no TF32/xf32.  Three arithmetics compute the same fp32 contraction
// (include/p2m.h, P2M_ARITH_*):
//   plain    native f32 MFMA v_mfma_f32_32x32x2_f32 (bitwise an fmaf chain, 157 TFLOP/s peak);
//   _ws<3>   every operand cut exactly into three bf16 slices, six slice products per fp32 product on
//            v_mfma_f32_32x32x16_bf16 (2500 / 6 = 417 TFLOP/s peak), fp32 accumulation;
//   _ws<2>   every operand scaled by a power of two (from its amax word) and cut into two fp16 slices, three slice
//            products on v_mfma_f32_32x32x16_f16 (2500 / 3 = 833 TFLOP/s peak), 22-bit operands (p2m_split.h).
//            _ws = wave-specialised (4 MFMA waves + 4 staging waves per block).
//
// Tiling (64-wide waves), all variants: the MFMA waves are arranged 2(M) x 2(N); block tile 128 x BN (BN = 128 or
// 64); each wave owns 64 x BN/2 = (2 x BN/64) MFMA 32x32 tiles; K chunk 32 (f32) or 16 (bf16 slices) per barrier,
// global -> registers -> LDS staging with register prefetch, two blocks per CU.
#include <cstdlib>

#include "p2m_gemm.h"
#include "p2m_probe.h"

namespace p2m {

struct GemmArgs {
  const float* A[3] = {};
  const float* Bm = nullptr;
  const float* bias = nullptr;
  const float* addend = nullptr;   // optional [M, N] added to the result (single output plane)
  // optional fused activation (eval-mode BatchNorm + ReLU folded into the contraction that produces the tensor):
  //   v = fmaf(acc + bias, act_scale[n], act_shift[n]);  v = max(v, 0) if act_relu   -- the same two roundings as the
  //   separate p2m_bn_act_fwd pass, so the fused result is bitwise the unfused one
  const float* act_scale = nullptr;
  const float* act_shift = nullptr;
  int act_relu = 0;
  int pair_out = 0;      // write C[(row>>1)] = v(row) + v(row^1): backward of the x2 un-pool (single output plane)
  float* C[3] = {};
  float* stats = nullptr;
  long M = 0;
  int nplanesA = 0, Ka = 0, a0_shift = 0;
  int N = 0, Nc = 0;
  int ntm = 0, ntn = 0;
  // row-set mode (ROWS kernels): logical row (b, i), i < nset -> actual row b*V + ids[i]; tiles do not cross samples
  // (tps tiles per sample); planes 1,2 of A are COMPACT ([B*nset, Ka]) when `compact`
  const int* ids = nullptr;
  int nset = 0, V = 0, tps = 0, compact = 0;
  // optional weights of the logical rows (aligned with ids): the BatchNorm partials count row i row_w[i] times (class
  // representatives stand for their whole class); NULL = every row once
  const float* row_w = nullptr;
  // split-bf16 mode (k_gemm_planes_bx): Bx[k / 16][s][n][k % 16], s < 3, n < Npad, k < Ktot = nplanesA * Ka
  const unsigned short* Bx = nullptr;
  int Npad = 0, Ktot = 0;
  // two-fp16-slice mode: amax words (p2m_split.h) of the A planes (+ a_bits binades of headroom) and of the weight
  const unsigned* a_amax = nullptr;
  const unsigned* b_amax = nullptr;
  int a_bits = 0;
  unsigned* amax_out = nullptr;    // optional: receives max |value stored| (atomic max; the caller zeroes it)
  // activation on load of A plane 0 (k_gemm_planes_ws, Ka <= 256): the operand is max(fma(A0, in_scale[k], in_shift[k]), 0)
  const float* in_scale = nullptr;
  const float* in_shift = nullptr;
};

// blockIdx -> (m tile, n tile).  Blocks b, b+8, b+16.. share an XCD (observed dispatch: b % 8);
// give the n-tiles of one m-tile consecutive slots of the SAME XCD so the A tile is re-read
// from that XCD's L2, not from HBM.
__device__ __forceinline__ bool tile_of_block(int bid, int ntm, int ntn, int& mt, int& nt) {
  int xcd = bid & 7;
  int slot = bid >> 3;
  nt = slot % ntn;
  mt = (slot / ntn) * 8 + xcd;
  return mt < ntm;
}

// Epilogue shared by the native-fp32 and the split-bf16 kernels: bias (+ addend), store (or pair-sum store), and the
// ROWS kernels keep, behind the BM row indices, the BM row weights and the two per-wave weight totals (threads 0..BM-1 =
// waves 0, 1 fill them; the k loop's barriers order the fill before the epilogue reads it)
constexpr int ROWTAB_WORDS = 2 * BM + 2;
__device__ __forceinline__ void rows_weights_fill(const GemmArgs& g, int* rowtab, int i, int t) {
  float* wtab = reinterpret_cast<float*>(rowtab + BM);
  const float w = (i < g.nset) ? g.row_w[i] : 0.f;
  wtab[t] = w;
  float s = w;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((t & 63) == 0) wtab[BM + (t >> 6)] = s;
}

// The four tile rows of group gi (accumulator i = gi >> 2, registers 4 * (gi & 3) .. + 3) of a lane: ml0 + 0 .. 3.  ROWS: the
// actual rows come from the row table in one 16-byte LDS read (ml0 is a multiple of four), -1 = no row; flat: m0 + ml0 + e.
template <bool ROWS>
__device__ __forceinline__ void epi_group_rows(const int* rowtab, long m0, long M, int ml0, int (&rl)[4]) {
  if (ROWS) {
    const u32x4 rt = *reinterpret_cast<const u32x4*>(rowtab + ml0);
#pragma unroll
    for (int e = 0; e < 4; e++) rl[e] = (int)rt[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++) rl[e] = (m0 + ml0 + e < M) ? ml0 + e : -1;
  }
}

// per-tile BatchNorm partials (sum, centred M2).  `smem` is block LDS that is free once the k loop is over.
//
// The store path (round 8).  A lane's 32 rows are walked in eight groups of four consecutive tile rows; inside a group the
// columns (j) are the inner loop, so a group's row indices and row weights are read once (one ds_read_b128 each) and serve
// every column.  The walk does not wait for memory with a store in front of it (as compiled: but for the last addend element
// of a lane, and for the spilled values of the statistics walks of the 128-register row-set forms):
//   * the output plane of a wave's 32 columns is chosen among the three kernel-argument pointers by scalar compares and
//     selects (g.C[q] with a per-lane q was a vector load from the argument block and a vmcnt(0) per accumulator tile - on
//     gfx9 that wait also drains every store issued before it);
//   * the addend of group gi + 1 is requested BEFORE the stores of group gi are issued, unconditionally (rows and columns
//     that do not exist read the block's first row / column 0 and the value is dropped by a select: a load under a
//     per-lane condition is a branch and a full wait per element), and `has addend` is hoisted around the whole walk.  The
//     wait for a group's addend is a counted vmcnt that leaves the stores of the group before it in flight;
//   * the amax word is committed after the statistics, so no block barrier waits for a lane's store drain.
// Per accumulator the value chain is unchanged (ldexp, + bias, fma act, max, + addend), each lane's csum[j] / m2[j] are
// accumulated over i then r ascending as before, and the merges keep their operand order: results are bitwise the same.
// Statistics: sums and M2 meet in two disjoint reduction buffers, two block barriers.  A wave whose columns all lie beyond N
// (the upper half of a 64-wide tile at N = 32) skips every element loop and only attends the barriers.
constexpr int EPI_BARRIERS = 2;     // block barriers of the statistics reduction (the staging waves of _ws attend them)
// LDS the epilogue takes from the front of the block's (free) staging buffers: the two reduction buffers, and behind them,
// in the staged forms, two strips of 8 rows x BN / 2 columns for each of the four MFMA waves
#ifndef P2M_EPI_COPYOUT_DEFAULT
#define P2M_EPI_COPYOUT_DEFAULT true   // what P2M_EPI_COPYOUT is when the environment does not set it
#endif
constexpr int EPI_STRIP_ROWS = 8;
constexpr int EPI_RED_WORDS(int BN) { return 4 * BN; }
constexpr int EPI_LDS_WORDS(int BN, bool CO) { return EPI_RED_WORDS(BN) + (CO ? 4 * 2 * EPI_STRIP_ROWS * (BN / 2) : 0); }
template <int BN, bool EXTRA, bool ROWS, bool CO = false, bool CO_STATS = CO>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& g, floatx16 (&acc)[2][BN / 64], float* smem,
                                              const int* rowtab, int mt, long m0, int n0, int rs_i0, int wm, int wn,
                                              int l31, int lhi, int descale = 0) {
  constexpr int WTN = BN / 2;
  constexpr int TN = WTN / 32;
  constexpr int TM = 2;
  constexpr int NG = TM * 4;           // row groups per lane
  // C/D layout of 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
  const int wnu = __builtin_amdgcn_readfirstlane(wn);                      // (wave-uniform, and known to be)
  const bool live = n0 + wnu * WTN < g.N;                                  // wave-uniform
  // CO without CO_STATS: a staged form that is never launched with statistics (k_gemm_planes_ws at its 128-register bound) -
  // no statistics walk, no M2 pass, nothing kept
  const bool has_stats = (!CO || CO_STATS) && g.stats != nullptr;         // block-uniform
  const bool wst = ROWS && g.row_w != nullptr && has_stats;               // weighted partials (block-uniform)
  const float* wtab = reinterpret_cast<const float*>(rowtab + BM);
  const int mlw = wm * 64 + 4 * lhi;   // first tile row of the lane; group gi adds (gi >> 2) * 32 + (gi & 3) * 8
  float csum[TN];
  float vmax = 0.f;
#pragma unroll
  for (int j = 0; j < TN; j++) csum[j] = 0.f;
  // the 64 values of the lane one by one from here on: written back into the 16-register accumulator tuples, every element
  // assembles a second copy of its tuple (two tiles in flight: 32 registers the row-set forms at 128 do not have)
  float val[TM][TN][16];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) val[i][j][r] = acc[i][j][r];

  if (live) {
    // Addresses = wave-uniform 64-bit base (output plane + first row of the block's sample / tile: SALU) + a 32-bit byte
    // offset per lane (row inside the sample / tile times the row pitch, + column): the stores and the addend loads take the
    // `global_store v_off, v, s[base]` form, no 64-bit vector address per element (16 registers a group otherwise).
    float bias_v[TN], sc_v[TN], sh_v[TN];
    bool cok[TN];
    unsigned c4[TN];                   // byte offset of the column inside its output plane
    char* Cb[TN];                      // uniform: output plane of the wave's 32 columns, at the block's first row
    const bool pair = !CO && EXTRA && !ROWS && g.pair_out;            // (the pair sums are launched with CO off)
    const long rowbase = ROWS ? (long)(mt / g.tps) * g.V : m0;            // uniform: the rows of this block start here
    const int rowbase32 = (int)rowbase;                                   // (ROWS: the row table holds ints)
    const unsigned pitch = (unsigned)g.Nc * 4u;
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const int nu = n0 + wnu * WTN + j * 32;                              // uniform: first of the wave's 32 columns
      const int n = nu + l31;
      cok[j] = n < g.N;
      bias_v[j] = (g.bias != nullptr && cok[j]) ? g.bias[n] : 0.f;
      sc_v[j] = (g.act_scale != nullptr && cok[j]) ? g.act_scale[n] : 1.f;
      sh_v[j] = (g.act_scale != nullptr && cok[j]) ? g.act_shift[n] : 0.f;
      // the plane is n / Nc (n < N <= 3 Nc) without the division and without the per-lane read of the argument block.  The
      // 32 columns of an MFMA tile lie in ONE plane: the MFMA entries admit Nc % 32 == 0 only (any other Nc runs k_naive_*)
      const int q = (nu >= g.Nc ? 1 : 0) + (nu >= 2 * g.Nc ? 1 : 0);
      float* const Cq = q == 0 ? g.C[0] : (q == 1 ? g.C[1] : g.C[2]);
      Cb[j] = reinterpret_cast<char*>(Cq + (pair ? rowbase >> 1 : rowbase) * g.Nc);
      c4[j] = (unsigned)(n - q * g.Nc) * 4u;
    }
    const char* const Ab = reinterpret_cast<const char*>(g.addend + (EXTRA && g.addend != nullptr ? rowbase * g.Nc : 0));
    constexpr unsigned NOROW = 0xFFFFFFFFu;                                // (no byte offset of a row: those are multiples of 4)

    // byte offsets of the four rows of group gi from the block's first row, or NOROW
    auto row_offsets = [&](int gi, unsigned (&ro)[4]) {
      int rl[4];
      epi_group_rows<ROWS>(rowtab, m0, g.M, mlw + (gi >> 2) * 32 + (gi & 3) * 8, rl);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        ro[e] = rl[e] >= 0 ? (unsigned)(ROWS ? rl[e] - rowbase32 : rl[e]) * pitch : NOROW;
        // (opaque from here on: knowing where `no row` comes from, the compiler threads the whole element - value chain, select,
        // sums - into a branch per row, and the waits it then places at the joins are full ones)
        asm volatile("" : "+v"(ro[e]));
      }
    };
    // ADD: there is an addend.  KEEP: there are statistics - the values stay for the M2 pass and the sums are formed; without
    // them a value is dead once it is stored (`has statistics` hoisted like `has addend`: the 64 kept values are what the
    // row-set forms at 128 registers have no room for next to the addend in flight)
    auto walk = [&](auto add_tag, auto keep_tag) {
      constexpr bool ADD = decltype(add_tag)::value;
      constexpr bool KEEP = decltype(keep_tag)::value;
      float ad[2][ADD ? TN : 1][4];    // [parity of the group]
      auto fetch = [&](int gi) {       // single output plane: N == Nc, the addend's offsets are the store's
        unsigned ro[4];                // (read again when the group is stored: eight registers less across the walk)
        row_offsets(gi, ro);
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const unsigned lo = ro[e] != NOROW ? ro[e] : 0u;
#pragma unroll
          for (int j = 0; j < TN; j++)
            ad[gi & 1][j][e] = *reinterpret_cast<const float*>(Ab + (lo + (cok[j] ? c4[j] : 0u)));
        }
      };
      if constexpr (ADD) fetch(0);
      // the per-column constants have arrived before the first store is issued (one counted wait, here)
#pragma unroll
      for (int j = 0; j < TN; j++) asm volatile("" : "+v"(bias_v[j]), "+v"(sc_v[j]), "+v"(sh_v[j]));
#pragma unroll
      for (int gi = 0; gi < NG; gi++) {
        const int i = gi >> 2, r0 = (gi & 3) * 4;
        const int ml0 = mlw + i * 32 + (gi & 3) * 8;
        if constexpr (ADD) {
          if (gi + 1 < NG) fetch(gi + 1);
        }
        // the next group's requests stand before this group's stores; (round 6) and the row addresses of four accumulator
        // registers at a time: left alone, the scheduler forms all 64 store addresses first - 150-170 registers for a kernel
        // whose k loop needs 112, i.e. one block per CU instead of two
        __builtin_amdgcn_sched_barrier(0);
        unsigned ro[4];
        row_offsets(gi, ro);
        float vg[TN][4];               // the group's values
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int r = r0 + e;
          const bool rok = ro[e] != NOROW;
#pragma unroll
          for (int j = 0; j < TN; j++) {
            float v = __builtin_ldexpf(val[i][j][r], descale) + bias_v[j];     // descale: exact (two-fp16-slice mode), else 0
            if (g.act_scale != nullptr) v = fmaf(v, sc_v[j], sh_v[j]);
            if (g.act_relu) v = fmaxf(v, 0.f);
            if constexpr (ADD) v += ad[gi & 1][j][e];    // (what a row or column that does not exist gets is dropped below)
            // the value is formed (and kept) for every lane - what a row that does not exist keeps is never used: the sums,
            // the pair sums and the M2 pass all ask for the row - and only the store stands under the lane's condition:
            // sunk into that branch, what is kept is a copy of its whole tile on either side of it
            asm volatile("" : "+v"(v));
            vg[j][e] = v;
            if constexpr (KEEP) val[i][j][r] = v;
            if (!pair && rok && cok[j]) {
#ifdef P2M_PL_ABL_NOSTORE
              if (v == 12345.678f)
#endif
              *reinterpret_cast<float*>(Cb[j] + (ro[e] + c4[j])) = v;
            }
          }
        }
        if (pair) {   // rows (r, r+1), r even: the two children of one coarse vertex
#pragma unroll
          for (int e = 0; e < 4; e += 2) {
            if (m0 + ml0 + e < g.M) {
#pragma unroll
              for (int j = 0; j < TN; j++)
                if (cok[j]) {
                  const float pv = vg[j][e] + (m0 + ml0 + e + 1 < g.M ? vg[j][e + 1] : 0.f);
                  *reinterpret_cast<float*>(Cb[j] + ((unsigned)((ml0 + e) >> 1) * pitch + c4[j])) = pv;
                  vmax = fmaxf(vmax, amax_abs(pv));
                }
            }
          }
        } else {
          // sums and maximum of the group, from the values just kept (an element that does not exist adds + 0 and max(., 0):
          // csum and vmax are never -0, they stay as they were); the weights are read when the addend's registers are free
          f32x4 w4 = {0.f, 0.f, 0.f, 0.f};
          if (KEEP && wst) w4 = *reinterpret_cast<const f32x4*>(wtab + ml0);
#pragma unroll
          for (int e = 0; e < 4; e++)
#pragma unroll
            for (int j = 0; j < TN; j++) {
              const float v = vg[j][e];
              const bool ok = ro[e] != NOROW && cok[j];
              if constexpr (KEEP) {
                const float term = wst ? w4[e] * v : v;
                csum[j] += ok ? term : 0.f;
              }
              vmax = fmaxf(vmax, ok ? amax_abs(v) : 0.f);
            }
        }
        // formed HERE: left to the compiler the sums and the maximum sink behind the whole walk, with every weight and lane
        // condition of the 64 elements kept until then (254 registers)
#pragma unroll
        for (int j = 0; j < TN; j++) asm volatile("" : "+v"(csum[j]));
        asm volatile("" : "+v"(vmax));
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    // The staged copy-out (round 9, CO).  The value chain per element is the walk's; a wave writes the values of a row group -
    // 8 consecutive tile rows x its WTN columns - into a strip of its own (ds_write_b32), reads the strip back as 16-byte row
    // segments and stores those: lane -> (strip row lane >> 3, column quad lane & 7 of the 32-column tile j), so a store
    // instruction covers eight rows of 128 contiguous bytes, and the output plane of a store is uniform as in the walk.  Two
    // strips per wave: the reads of group gi are in flight while the values of group gi + 1 are staged; the wave's own LDS
    // wait stands between its writes and its reads, no block barrier.
    // Banks.  ds_write_b32 (two 32-lane halves, bank = dword % 32): a half writes the 32 consecutive dwords of one strip row
    // and one tile j - every bank once, whatever the row stride.  ds_read_b128 (four 16-lane groups, e.g. lanes {0-3, 12-15,
    // 20-27}, bank = dword % 64): a group reads quads 0-3 of strip row 0, quads 4-7 of rows 1 and 2, quads 0-3 of row 3 (the
    // other groups likewise).  WTN = 32: the row stride of 32 dwords puts these at dwords 0-15, 48-63, 80-95 = 16-31, 96-111 =
    // 32-47 mod 64: every bank once.  WTN = 64: the stride is 0 mod 64 and rows 1 and 2 would meet, so tile j of strip row s
    // lies in the half j ^ (s & 1) of its row: dwords 0-15, 64 + 32 + 16.. = 48-63, 128 + 16.. = 16-31, 192 + 32.. = 32-47.
    // The addend (never together with statistics here) is loaded in the copy-out layout one group ahead of the stores, before
    // the stores of the group in front of it, and added at copy-out: v + addend is the same sum whichever lane forms it.  The
    // maximum is formed at copy-out over the values stored; the sums keep their lanes and their order (KEEP, as in the walk).
    auto walk_co = [&](auto add_tag, auto keep_tag) {
      constexpr bool ADD = decltype(add_tag)::value;
      constexpr bool KEEP = decltype(keep_tag)::value;
      static_assert(!(ADD && KEEP), "statistics with an addend keep the 4-byte walk");
      constexpr int SB = EPI_STRIP_ROWS * WTN;                               // words of one strip
      float* const strip = smem + EPI_RED_WORDS(BN) + (wm * 2 + wnu) * 2 * SB;
      // (opaque: what the copy-out derives from the lane is formed here, not in front of the k loop and carried through it)
      int lane = lhi * 32 + l31;
      asm volatile("" : "+v"(lane));
      const int srow = lane >> 3;
      const unsigned col16 = (unsigned)(lane & 7) * 16u;
      float* const wr = strip + (lane >> 5) * 4 * WTN + (lane & 31);
      const int rd0 = srow * WTN + (TN == 2 ? (srow & 1) * 32 : 0) + (lane & 7) * 4;
      const float* rd[TN];
      char* Cc[TN];                      // uniform: Cb + the first column of tile j inside its plane
      const char* Ac[TN];
      bool ju[TN];                       // uniform: tile j lies inside N (N % 32 == 0: all of its columns or none)
#pragma unroll
      for (int j = 0; j < TN; j++) {
        const int nu = n0 + wnu * WTN + j * 32;
        const int q = (nu >= g.Nc ? 1 : 0) + (nu >= 2 * g.Nc ? 1 : 0);
        ju[j] = nu < g.N;
        Cc[j] = Cb[j] + (unsigned)(nu - q * g.Nc) * 4u;
        Ac[j] = Ab + (ADD && ju[j] ? (unsigned)nu * 4u : 0u);
        rd[j] = strip + (rd0 ^ (j * 32));
      }
      // byte offset of the lane's 16 bytes in the row it copies out of group gi, from the block's first row, or NOROW
      auto co_row = [&](int gi) {
        const int tr = wm * 64 + (gi >> 2) * 32 + (gi & 3) * 8 + srow;
        unsigned ro;
        if (ROWS) {
          const int rl = rowtab[tr];
          ro = rl >= 0 ? (unsigned)(rl - rowbase32) * pitch + col16 : NOROW;
        } else {
          ro = m0 + tr < g.M ? (unsigned)tr * pitch + col16 : NOROW;
        }
        asm volatile("" : "+v"(ro));     // (opaque, as in the walk)
        return ro;
      };
      f32x4 cp[TN];
      f32x4 ad[2][ADD ? TN : 1];
      unsigned ro_cur = NOROW, ro_nxt = co_row(0);
#pragma unroll
      for (int j = 0; j < TN; j++) asm volatile("" : "+v"(bias_v[j]), "+v"(sc_v[j]), "+v"(sh_v[j]));
      // values of group gi -> strip gi & 1 (and, KEEP, the sums); the addend of the group is requested first
      auto stage = [&](int gi) {
        if constexpr (ADD) {             // (a row or a tile that does not exist reads the block's first row / column)
          const unsigned lo = ro_nxt != NOROW ? ro_nxt : col16;
#pragma unroll
          for (int j = 0; j < TN; j++) ad[gi & 1][j] = *reinterpret_cast<const f32x4*>(Ac[j] + lo);
        }
        __builtin_amdgcn_sched_barrier(0);
        const int i = gi >> 2, r0 = (gi & 3) * 4;
        unsigned ro4[4] = {0u, 0u, 0u, 0u};
        f32x4 w4 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (KEEP) {
          row_offsets(gi, ro4);
          if (wst) w4 = *reinterpret_cast<const f32x4*>(wtab + mlw + i * 32 + (gi & 3) * 8);
        }
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
          for (int j = 0; j < TN; j++) {
            const int r = r0 + e;
            float v = __builtin_ldexpf(val[i][j][r], descale) + bias_v[j];     // descale: exact (two-fp16-slice mode), else 0
            if (g.act_scale != nullptr) v = fmaf(v, sc_v[j], sh_v[j]);
            if (g.act_relu) v = fmaxf(v, 0.f);
            asm volatile("" : "+v"(v));
            if constexpr (KEEP) {
              val[i][j][r] = v;
              const float term = wst ? w4[e] * v : v;
              csum[j] += (ro4[e] != NOROW && cok[j]) ? term : 0.f;
            }
            wr[(gi & 1) * SB + e * WTN + (TN == 2 ? (j ^ (e & 1)) * 32 : 0)] = v;
          }
        if constexpr (KEEP) {
#pragma unroll
          for (int j = 0; j < TN; j++) asm volatile("" : "+v"(csum[j]));
        }
      };
      // strip gi & 1 -> registers, in the copy-out layout, with the row of the lane; the row of the next group is asked for
      // in front of the strip (LDS returns in order: the next group's addend request waits for the row only)
      auto fetch = [&](int gi) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the wave's own strip writes, before it reads them
        ro_cur = ro_nxt;
        if (gi + 1 < NG) ro_nxt = co_row(gi + 1);
#pragma unroll
        for (int j = 0; j < TN; j++) cp[j] = *reinterpret_cast<const f32x4*>(rd[j] + (gi & 1) * SB);
      };
      auto copy_out = [&](int gi) {
#pragma unroll
        for (int j = 0; j < TN; j++) {
          f32x4 v = cp[j];
          if constexpr (ADD) v += ad[gi & 1][j];
          const bool ok = ro_cur != NOROW && ju[j];
          if (ok) *reinterpret_cast<f32x4*>(Cc[j] + ro_cur) = v;
          const float m4 = fmaxf(fmaxf(amax_abs(v[0]), amax_abs(v[1])), fmaxf(amax_abs(v[2]), amax_abs(v[3])));
          vmax = fmaxf(vmax, ok ? m4 : 0.f);
        }
        asm volatile("" : "+v"(vmax));
      };
      // without statistics the copy-out of a group runs one group behind its staging (its strip reads are in flight meanwhile);
      // with them (the 64 values stay in registers for the M2 pass) a group is staged, read back and stored in turn: eight
      // registers less across the walk
      constexpr bool PIPE = !KEEP;
#pragma unroll
      for (int gi = 0; gi <= NG; gi++) {
        if (gi < NG) stage(gi);
        if constexpr (PIPE) {
          if (gi >= 1) copy_out(gi - 1);
          if (gi < NG) fetch(gi);
        } else if (gi < NG) {
          fetch(gi);
          copy_out(gi);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    const bool add = EXTRA && g.addend != nullptr;
    if constexpr (CO) {
      // the staged forms (never launched for pair sums); statistics together with an addend (no launch of the train step) keep
      // the 4-byte walk
      if (has_stats) {
        if (add) walk(std::true_type{}, std::true_type{});
        else walk_co(std::false_type{}, std::true_type{});
      } else {
        if (add) walk_co(std::true_type{}, std::false_type{});
        else walk_co(std::false_type{}, std::false_type{});
      }
    } else if (has_stats) {
      if (add) walk(std::true_type{}, std::true_type{});
      else walk(std::false_type{}, std::true_type{});
    } else {
      if (add) walk(std::true_type{}, std::false_type{});
      else walk(std::false_type{}, std::false_type{});
    }
  }

  if (has_stats) {
    // column sums over the 128-row tile: lane^32 holds the same column, the other wm wave the other 64 rows
    float* red = smem;             // [2 (wm)][BN] sums      (safe: all waves passed the last __syncthreads of the k loop)
    float* red2 = smem + 2 * BN;   // [2 (wm)][BN] M2
    long rows_valid = ROWS ? (long)(g.nset - rs_i0) : g.M - m0;
    if (rows_valid > BM) rows_valid = BM;
    if (live) {
#pragma unroll
      for (int j = 0; j < TN; j++) {
        csum[j] += __shfl_xor(csum[j], 32);
        if (lhi == 0) red[wm * BN + wn * WTN + j * 32 + l31] = csum[j];
      }
    }
    __syncthreads();
    if (live) {
      float mean[TN], m2[TN];
#pragma unroll
      for (int j = 0; j < TN; j++) {
        const int cl = wn * WTN + j * 32 + l31;
        const float tot = red[cl] + red[BN + cl];
        mean[j] = tot / (wst ? wtab[BM] + wtab[BM + 1] : (float)rows_valid);
        m2[j] = 0.f;
        csum[j] = tot;
      }
#pragma unroll
      for (int gi = 0; gi < NG; gi++) {
        const int i = gi >> 2, r0 = (gi & 3) * 4;
        const int ml0 = mlw + i * 32 + (gi & 3) * 8;
        int rl[4];
        epi_group_rows<ROWS>(rowtab, m0, g.M, ml0, rl);
        f32x4 w4 = {0.f, 0.f, 0.f, 0.f};
        if (wst) w4 = *reinterpret_cast<const f32x4*>(wtab + ml0);
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
          for (int j = 0; j < TN; j++) {
            // (w d) d + m2 with the last product fused, as this sum has always been compiled; written out so that it stays so
            const float d = val[i][j][r0 + e] - mean[j];
            const float wd = wst ? w4[e] * d : d;
            m2[j] = rl[e] >= 0 ? fmaf(wd, d, m2[j]) : m2[j];
          }
      }
#pragma unroll
      for (int j = 0; j < TN; j++) {
        m2[j] += __shfl_xor(m2[j], 32);
        if (lhi == 0) red2[wm * BN + wn * WTN + j * 32 + l31] = m2[j];
      }
    }
    __syncthreads();
    if (live && wm == 0 && lhi == 0) {
#pragma unroll
      for (int j = 0; j < TN; j++) {
        const int cl = wn * WTN + j * 32 + l31;
        const int n = n0 + cl;
        if (n < g.N) {
          float* st = g.stats + (long)mt * 2 * g.N;
          st[n] = csum[j];
          st[g.N + n] = red2[cl] + red2[BN + cl];
        }
      }
    }
  }
  if (g.amax_out != nullptr) amax_commit(g.amax_out, vmax);
}

// KB = K chunk staged per barrier (16: 34 KB LDS -> 3 blocks/CU; 32: 67 KB -> 2 blocks/CU);
// EXTRA compiles in the addend / pair-sum epilogue (kept out of the plain variant: it costs registers -> occupancy)
template <int BN, int KB, bool EXTRA, bool ROWS = false>
__global__ __launch_bounds__(256, 2) void k_gemm_planes(GemmArgs g) {
  constexpr int WTN = BN / 2;    // wave tile N
  constexpr int TN = WTN / 32;   // MFMA tiles along N per wave
  constexpr int TM = 2;          // wave tile M = 64
  constexpr int LDA = KB + 1;    // [m][k] row stride: bank = (m + k) % 32 -> conflict-free fragment reads
  constexpr int APASS = BM * KB / 4 / 256;        // float4 A loads per thread per chunk
  constexpr int AROWS = 256 / (KB / 4);           // rows of A covered per pass
  constexpr int BPASS = KB * BN / 4 / 256;        // float4 B loads per thread per chunk
  constexpr int BROWS = 256 / (BN / 4);           // rows of B covered per pass
  __shared__ __attribute__((aligned(16))) float smem[2 * BM * LDA + 2 * KB * BN + (ROWS ? ROWTAB_WORDS : 0)];   // (16: the epilogue reads the row table four rows at a time)
  float* As = smem;
  float* Bs = smem + 2 * BM * LDA;
  int* rowtab = reinterpret_cast<int*>(smem + 2 * BM * LDA + 2 * KB * BN);   // ROWS: actual row of each tile row, -1 = none

  int mt, nt;
  if (!tile_of_block(blockIdx.x, g.ntm, g.ntn, mt, nt)) return;
  const long m0 = (long)mt * BM;      // flat mode: first row of the tile; ROWS mode: unused for addressing
  const int n0 = nt * BN;
  const int t = threadIdx.x;
  // ROWS mode: tile -> (sample, tile within the sample's row set)
  const int rs_b = ROWS ? mt / g.tps : 0;
  const int rs_i0 = ROWS ? (mt - rs_b * g.tps) * BM : 0;
  if (ROWS && t < BM) {
    const int i = rs_i0 + t;
    rowtab[t] = (i < g.nset) ? rs_b * g.V + g.ids[i] : -1;
    if (g.row_w != nullptr) rows_weights_fill(g, rowtab, i, t);
  }
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

  const int cpp = g.Ka / KB;              // chunks per plane
  const int nchunks = g.nplanesA * cpp;

  // staging registers
  float4 ra[APASS];
  float4 rb[BPASS];
  const int a_row = t / (KB / 4), a_k4 = (t % (KB / 4)) * 4;
  const int b_row = t / (BN / 4), b_c4 = (t % (BN / 4)) * 4;
  // ROWS mode: per-thread source rows of its APASS tile rows (plane 0: full layout, planes 1,2: compact)
  long rs_full[ROWS ? APASS : 1], rs_comp[ROWS ? APASS : 1];
  if (ROWS) {
#pragma unroll
    for (int ps = 0; ps < APASS; ps++) {
      const int i = rs_i0 + ps * AROWS + a_row;
      if (i < g.nset) {
        rs_full[ps] = (long)rs_b * g.V + g.ids[i];
        rs_comp[ps] = (long)rs_b * g.nset + i;
      } else {
        rs_full[ps] = -1;
        rs_comp[ps] = -1;
      }
    }
  }

  auto load_chunk = [&](int kc) {
    const int p = kc / cpp;
    const int k0 = (kc - p * cpp) * KB;
    const float* Ap = g.A[p];
    const int sh = (p == 0) ? g.a0_shift : 0;
#pragma unroll
    for (int ps = 0; ps < APASS; ps++) {
      if (ROWS) {
        const long r = (p == 0 || !g.compact) ? rs_full[ps] : rs_comp[ps];
        if (r >= 0)
          ra[ps] = *reinterpret_cast<const float4*>(Ap + (r >> sh) * g.Ka + k0 + a_k4);
        else
          ra[ps] = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        long r = m0 + ps * AROWS + a_row;
        if (r < g.M)
          ra[ps] = *reinterpret_cast<const float4*>(Ap + (r >> sh) * g.Ka + k0 + a_k4);
        else
          ra[ps] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    const float* Bp = g.Bm + (long)(p * g.Ka + k0) * g.N;
#pragma unroll
    for (int ps = 0; ps < BPASS; ps++) {
      int kr = ps * BROWS + b_row;
      int n = n0 + b_c4;
      if (n < g.N)
        rb[ps] = *reinterpret_cast<const float4*>(Bp + (long)kr * g.N + n);
      else
        rb[ps] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store_chunk = [&](int buf) {
    float* as = As + buf * BM * LDA;
#pragma unroll
    for (int ps = 0; ps < APASS; ps++) {
      float* d = as + (ps * AROWS + a_row) * LDA + a_k4;
      d[0] = ra[ps].x; d[1] = ra[ps].y; d[2] = ra[ps].z; d[3] = ra[ps].w;
    }
    float* bs = Bs + buf * KB * BN;
#pragma unroll
    for (int ps = 0; ps < BPASS; ps++)
      *reinterpret_cast<float4*>(bs + (ps * BROWS + b_row) * BN + b_c4) = rb[ps];
  };

  load_chunk(0);
  store_chunk(0);
  __syncthreads();

  for (int kc = 0; kc < nchunks; kc++) {
    const int cur = kc & 1;
    if (kc + 1 < nchunks) load_chunk(kc + 1);
    const float* as = As + cur * BM * LDA + (wm * 64 + l31) * LDA + lhi;
    const float* bs = Bs + cur * KB * BN + lhi * BN + wn * WTN + l31;
#pragma unroll
    for (int ks = 0; ks < KB / 2; ks++) {
      float a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; i++) a[i] = as[i * 32 * LDA + 2 * ks];
#pragma unroll
      for (int j = 0; j < TN; j++) b[j] = bs[2 * ks * BN + j * 32];
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (kc + 1 < nchunks) store_chunk(cur ^ 1);
    __syncthreads();
  }

  gemm_epilogue<BN, EXTRA, ROWS>(g, acc, smem, rowtab, mt, m0, n0, rs_i0, wm, wn, l31, lhi);
}

// ---------------------------------------------------------------------------------------------
// fp32 contraction on the BF16 matrix pipe (16x the rate of the f32 MFMA on gfx950).
//
// Every fp32 operand is cut into three bf16 slices by TRUNCATION: x = h + m + l exactly (8 + 8 + 8 significand bits;
// each remainder x - h, x - h - m is exact in fp32).  The product keeps the six slice pairs of weight >= 2^-16,
//     x*y ~= h h' + (h m' + m h') + (h l' + l h' + m m'),
// each pair exact inside v_mfma_f32_32x32x16_bf16 (8b x 8b significands) and accumulated in fp32; the dropped pairs
// (m l', l m', l l') are <= 2^-23 |x y| together - one fp32 rounding.  tests/test_gpu_ops.py checks the result against
// float64 with the same bound as the native f32 MFMA kernel.  Six bf16 MFMAs cost 6/16 of one f32 MFMA per flop.
//
// Same block/wave tiling, row addressing and epilogue as k_gemm_planes.  A is split while it is staged (fp32 global ->
// 3 bf16 planes in LDS, split3_pack4 in p2m_split.h); the weights arrive pre-split and k-contiguous (p2m_weight_split),
// so their staging is a straight 16-byte copy.  LDS rows hold 16 bf16 + 8 pad: the 48-byte row stride makes the 16-lane
// groups of ds_read_b128 hit all 64 banks once.
// ---------------------------------------------------------------------------------------------
// Wave-specialised: 512 threads = 4 consumer waves (fragment reads + MFMAs, the 2 x 2 wave tiling of k_gemm_planes) +
// 4 producer waves (global loads, slice arithmetic, LDS stores).  The hardware places waves i and i+4 of a block on the
// same SIMD, so each SIMD runs one MFMA stream and one VALU/memory stream side by side instead of one wave doing both
// in turn (a 4-wave form of the same kernel spent 24 % of a wave's phase in MFMAs).
//   * producers: two register stages of lead (they hold no accumulators), loads unconditional in the steady state,
//     LDS ring of two 16-wide chunks; during iteration kc they store chunk kc+1 and refill that stage with chunk kc+3;
//   * one LDS-only block barrier per chunk.  2 blocks (16 waves) per CU, 74 KB of LDS each (where the registers allow:
//     see the launch bound below).
// (Measured and removed in round 3: the 4-wave form, a 3-chunk ring with double-buffered fragments at 1 block per CU
//  (-1.4 % on the step), the BatchNorm-backward reduction in this kernel's epilogue (its 4-byte strided reads of the
//  layer's raw input cost the contraction +4.5 ms, the pass they replace 3.3 ms).)
// ---------------------------------------------------------------------------------------------
template <int BN, bool EXTRA, bool ROWS, int NS, bool CO>
// Round 6: the ROW-SET instantiations are held to 128 registers (launch bound 4 waves per SIMD = TWO blocks per CU, as this
// header always assumed): hipcc gave the 128-wide ones 152-174 - one block per CU, one MFMA wave per SIMD and nothing to
// cover its fragment reads and barriers.  At 128 the epilogue spills 28-46 dwords per lane (none in the k loop) and
// k_gemm_planes_ws<128, true, true, 3> (the paired backward) runs 360 instead of 513 us, <128, false, true, 3> 94 instead of
// 103 us; the plain-row ones measured 4 % slower that way and keep their bound (same-box rocprofv3 --stats, 9 steps).
__global__ __launch_bounds__(512, (BN == 128 && ROWS) ? 4 : 2) void k_gemm_planes_ws(GemmArgs g) {
  constexpr int KB = 16;
  // the staged row-set forms at 128 registers are not launched with statistics (launch_gemm_planes): next to the 64 values kept
  // for the M2 pass the staged walk spills more than the 4-byte one (192 against 148-152 bytes per lane), and without any
  // statistics code these forms need no scratch at all
  constexpr bool CO_STATS = CO && !(BN == 128 && ROWS);
  typedef typename SliceFrag<NS>::type frag_t;
  constexpr int NBUF = 2, NST = 2;    // LDS ring of two chunks, two register stages of lead (three: no change, round 6)
  constexpr int AHEAD = NBUF - 1;     // the producers store chunk kc + AHEAD during iteration kc
  constexpr int WTN = BN / 2;
  constexpr int TN = WTN / 32;
  constexpr int TM = 2;
  constexpr int LDX = KB + 8;
  constexpr int APASS = BM * KB / 4 / 256;
  constexpr int AROWS = 256 / (KB / 4);
  constexpr int A_BUF = NS * BM * LDX;
  constexpr int B_BUF = NS * BN * LDX;
  constexpr int SM_WORDS = NBUF * (A_BUF + B_BUF) / 2 + (ROWS ? ROWTAB_WORDS : 0);
  static_assert(EPI_LDS_WORDS(BN, CO) <= NBUF * (A_BUF + B_BUF) / 2,
                "the epilogue's reduction buffers and copy-out strips live in the ring, in front of the row table");
  __shared__ __attribute__((aligned(16))) float smem[SM_WORDS];
  __shared__ __attribute__((aligned(16))) float actco[2 * 256];        // activation on load: scale | shift of plane 0's columns
  unsigned short* As = reinterpret_cast<unsigned short*>(smem);
  unsigned short* Bs = As + NBUF * A_BUF;
  int* rowtab = reinterpret_cast<int*>(smem + NBUF * (A_BUF + B_BUF) / 2);

  int mt, nt;
  if (!tile_of_block(blockIdx.x, g.ntm, g.ntn, mt, nt)) return;
  const bool in_act = g.in_scale != nullptr;                             // block-uniform
  if (in_act) {
    if (threadIdx.x < g.Ka) {
      actco[threadIdx.x] = g.in_scale[threadIdx.x];
      actco[256 + threadIdx.x] = g.in_shift[threadIdx.x];
    }
    __syncthreads();            // (LDS, not a second global load per chunk: the staging waves' vmcnt bookkeeping stays as it is)
  }
  const long m0 = (long)mt * BM;
  const int n0 = nt * BN;
  const int t = threadIdx.x;
  const bool producer = t >= 256;          // wave-uniform
  const int pt = t & 255;
  const int rs_b = ROWS ? mt / g.tps : 0;
  const int rs_i0 = ROWS ? (mt - rs_b * g.tps) * BM : 0;
  if (ROWS && t < BM) {
    const int i = rs_i0 + t;
    rowtab[t] = (i < g.nset) ? rs_b * g.V + g.ids[i] : -1;
    if (g.row_w != nullptr) rows_weights_fill(g, rowtab, i, t);
  }
  const int lane = t & 63, wave = (t >> 6) & 3;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int cpp = g.Ka / KB;
  const int n = g.nplanesA * cpp;           // chunks
  auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  // two-fp16-slice mode: the A planes are staged times 2^sa, the weight arrives times 2^sb (p2m_weight_split)
  float a_sc = 1.f;
  int descale = 0;
  if (NS == 2) {
    const int sa = slice_scale_exp(*g.a_amax, g.a_bits);
    a_sc = exp2_int(sa);
    descale = -(sa + slice_scale_exp(*g.b_amax, 0));
  }

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

  if (producer) {
    // LDS stores without bank conflicts.  A row of a slice image is LDX = 24 bf16 = 12 dwords; a ds_write_b64 is serviced
    // in groups of 16 consecutive lanes (4 rows x 4 k-quads, an 8-dword window per row) over 32 banks, and rows r, r+3
    // overlap (12 * 3 = 36 = 4 mod 32): 2-way conflicts on every store, 33 % of all LDS cycles of the round-2 kernel
    // (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE).  Rows {0,2,4,6} (and {1,3,5,7}) of an 8-row group start at dwords
    // 0,24,16,8 (12,4,28,20) mod 32 and tile the 32 banks exactly, so each 16-lane group takes the even or the odd rows of
    // its 8-row group.  The global loads only permute rows inside a wave's 16 rows: same 64-byte segments, same coalescing.
    const int a_rl = (pt >> 2) & 7;
    const int a_row = ((pt >> 5) << 3) | ((a_rl & 3) << 1) | (a_rl >> 2), a_k4 = (pt % (KB / 4)) * 4;
    static_assert(KB == 16, "the conflict-free row permutation assumes 4 k-quads per row");
    // Addresses = wave-uniform 64-bit base (plane + first row of this block's sample / tile, + k0 per chunk: SALU) +
    // per-thread 32-BIT byte offset inside that sample / tile (fixed for the whole kernel): the loads take the
    // `global_load v, v_off, s[base]` form and the chunk loop carries no 64-bit vector address arithmetic - the
    // contraction is issue-bound, every VALU instruction of a staging wave delays an MFMA of the wave it shares a SIMD with
    unsigned voff0[APASS], voff12[APASS];
    long sbase0, sbase12;              // element offsets of the block's first row in plane 0 / planes 1,2
    if (ROWS) {
      sbase0 = (((long)rs_b * g.V) >> g.a0_shift) * g.Ka;        // V is even whenever a0_shift = 1
      sbase12 = (g.compact ? (long)rs_b * g.nset : (long)rs_b * g.V) * g.Ka;
    } else {
      sbase0 = (m0 >> g.a0_shift) * g.Ka;                         // m0 is a multiple of 128
      sbase12 = m0 * g.Ka;
    }
#pragma unroll
    for (int ps = 0; ps < APASS; ps++) {
      int lf, lc;                        // row relative to the block's base row, in plane 0 / planes 1,2
      if (ROWS) {
        int i = rs_i0 + ps * AROWS + a_row;
        if (i >= g.nset) i = g.nset - 1;
        lf = g.ids[i];
        lc = g.compact ? i : lf;
      } else {
        long rf = m0 + ps * AROWS + a_row;
        if (rf >= g.M) rf = g.M - 1;
        lf = (int)(rf - m0);
        lc = lf;
      }
      voff0[ps] = (unsigned)(((lf >> g.a0_shift) * g.Ka + a_k4) * 4);
      voff12[ps] = (unsigned)((lc * g.Ka + a_k4) * 4);
    }
    // same for the B image: a ds_write_b128 is serviced in groups of 8 consecutive lanes (4 columns x 2 halves)
    const int b_nl = (pt >> 1) & 7;
    const int b_n = ((((pt % (BN * 2)) >> 1) >> 3) << 3) | ((b_nl & 3) << 1) | (b_nl >> 2), b_half = (pt & 1) * 8;
    const unsigned bx_voff = (unsigned)((((n0 + b_n) * 16) + b_half) * 2);       // bytes inside one slice of one chunk
    const long bx_slice = (long)g.Npad * 16;

    f32x4 ra[NST][APASS];
    u32x4 rb[NST][NS];
    auto load_chunk = [&](int kc, f32x4 (&a)[APASS], u32x4 (&b)[NS]) {
      const int p = kc / cpp;
      const int k0 = (kc - p * cpp) * KB;
      const char* Ab = reinterpret_cast<const char*>(g.A[p] + (p == 0 ? sbase0 : sbase12) + k0);     // uniform
#pragma unroll
      for (int ps = 0; ps < APASS; ps++)
#ifdef P2M_PL_ABL_NOLOAD
        a[ps] = f32x4{__uint_as_float(voff0[ps]), 1.f, 2.f, (float)(long)Ab};
#else
        a[ps] = *reinterpret_cast<const f32x4*>(Ab + (p == 0 ? voff0[ps] : voff12[ps]));
#endif
      const char* src0 = reinterpret_cast<const char*>(g.Bx + (long)((p * g.Ka + k0) >> 4) * (NS * bx_slice));   // uniform
#pragma unroll
      for (int sl = 0; sl < NS; sl++) b[sl] = *reinterpret_cast<const u32x4*>(src0 + sl * 2 * bx_slice + bx_voff);
    };
    auto store_chunk = [&](int kc, f32x4 (&a)[APASS], const u32x4 (&b)[NS]) {
      const int buf = kc % NBUF;
      unsigned short* as = As + buf * A_BUF;
#pragma unroll
      for (int ps = 0; ps < APASS; ps++) asm volatile("" : "+v"(a[ps]));
      if (in_act && kc < cpp) {                  // plane 0 (chunks 0 .. cpp - 1): BatchNorm + ReLU of the previous conv on load
        const f32x4 sc = *reinterpret_cast<const f32x4*>(&actco[kc * KB + a_k4]);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(&actco[256 + kc * KB + a_k4]);
#pragma unroll
        for (int ps = 0; ps < APASS; ps++)
#pragma unroll
          for (int e = 0; e < 4; e++) a[ps][e] = fmaxf(fmaf(a[ps][e], sc[e], sh[e]), 0.f);
      }
#pragma unroll
      for (int ps = 0; ps < APASS; ps++) {
        u32x2 sl[NS];
#ifdef P2M_PL_ABL_NOSLICE
        for (int q = 0; q < NS; q++) sl[q] = u32x2{__float_as_uint(a[ps][q & 1]), __float_as_uint(a[ps][2 + (q & 1)])};
#else
        split_pack4<NS>(a[ps][0], a[ps][1], a[ps][2], a[ps][3], a_sc, sl);
#endif
        unsigned short* d = as + (ps * AROWS + a_row) * LDX + a_k4;
#pragma unroll
        for (int q = 0; q < NS; q++) *reinterpret_cast<u32x2*>(d + q * BM * LDX) = sl[q];
      }
      unsigned short* d = Bs + buf * B_BUF + b_n * LDX + b_half;
#pragma unroll
      for (int q = 0; q < NS; q++) *reinterpret_cast<u32x4*>(d + q * BN * LDX) = b[q];
    };
    const int last = n - 1;
    // chunk c lives in register stage c % NST and LDS buffer c % NBUF.  Prologue: chunks 0..AHEAD-1 stored, the next NST
    // chunks in flight.
#pragma unroll
    for (int i = 0; i < NST; i++) load_chunk(i < last ? i : last, ra[i], rb[i]);
#pragma unroll
    for (int i = 0; i < AHEAD; i++) {
      if (i < n) store_chunk(i, ra[i], rb[i]);
      load_chunk(NST + i < last ? NST + i : last, ra[i], rb[i]);
    }
    lds_barrier();
    // iteration kc (consumers: MFMAs of chunk kc): store chunk kc+AHEAD, refill its stage with chunk kc+AHEAD+NST
    int kc = 0;
    for (; kc + (NST - 1) + AHEAD + NST < n; kc += NST) {     // steady state: every load below is in range
#pragma unroll
      for (int i = 0; i < NST; i++) {
        store_chunk(kc + i + AHEAD, ra[(i + AHEAD) % NST], rb[(i + AHEAD) % NST]);
        load_chunk(kc + i + AHEAD + NST, ra[(i + AHEAD) % NST], rb[(i + AHEAD) % NST]);
        lds_barrier();
      }
    }
    for (; kc < n; kc += NST) {                                // tail: same rotation, range-checked
#pragma unroll
      for (int i = 0; i < NST; i++) {
        if (kc + i < n) {
          if (kc + i + AHEAD < n) store_chunk(kc + i + AHEAD, ra[(i + AHEAD) % NST], rb[(i + AHEAD) % NST]);
          if (kc + i + AHEAD + NST < n) load_chunk(kc + i + AHEAD + NST, ra[(i + AHEAD) % NST], rb[(i + AHEAD) % NST]);
          lds_barrier();
        }
      }
    }
  } else {
    frag_t fa[NBUF - 1][NS][TM], fb[NBUF - 1][NS][TN];       // [register set][slice, high first][tile]
    auto read_frags = [&](int kc, frag_t (&a)[NS][TM], frag_t (&b)[NS][TN]) {
      const int buf = kc % NBUF;
      const unsigned short* as = As + buf * A_BUF + (wm * 64 + l31) * LDX + lhi * 8;
      const unsigned short* bs = Bs + buf * B_BUF + (wn * WTN + l31) * LDX + lhi * 8;
#pragma unroll
      for (int sl = 0; sl < NS; sl++) {
#pragma unroll
        for (int i = 0; i < TM; i++)
          a[sl][i] = __builtin_bit_cast(frag_t, *reinterpret_cast<const u32x4*>(as + (sl * BM + i * 32) * LDX));
#pragma unroll
        for (int j = 0; j < TN; j++)
          b[sl][j] = __builtin_bit_cast(frag_t, *reinterpret_cast<const u32x4*>(bs + (sl * BN + j * 32) * LDX));
      }
    };
    auto mfmas = [&](const frag_t (&a)[NS][TM], const frag_t (&b)[NS][TN]) {
#define P2M_PAIR(SA, SB)                                                                       \
  _Pragma("unroll") for (int i = 0; i < TM; i++) _Pragma("unroll") for (int j = 0; j < TN; j++) \
      acc[i][j] = slice_mfma<NS>(a[SA][i], b[SB][j], acc[i][j]);
#ifdef P2M_PL_ABL_NOMFMA
      if constexpr (NS == 3) {
        P2M_PAIR(0, 0)
        for (int sl = 1; sl < NS; sl++)
          for (int i = 0; i < TM; i++) for (int j = 0; j < TN; j++) { asm volatile("" :: "v"(a[sl][i])); asm volatile("" :: "v"(b[sl][j])); }
      } else
#endif
      if constexpr (NS == 3) {          // smallest products first
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
    };
    lds_barrier();                              // the first AHEAD chunks are in LDS
    for (int kc = 0; kc < n; kc++) {
      read_frags(kc, fa[0], fb[0]);
      mfmas(fa[0], fb[0]);
      lds_barrier();
    }
  }
  __syncthreads();   // staging buffers are free: the epilogue reuses them
  if (!producer) {
    gemm_epilogue<BN, EXTRA, ROWS, CO, CO_STATS>(g, acc, smem, rowtab, mt, m0, n0, rs_i0, wm, wn, l31, lhi, descale);
  } else {
    if ((!CO || CO_STATS) && g.stats != nullptr) {        // the block barriers of the statistics reduction
#pragma unroll
      for (int b = 0; b < EPI_BARRIERS; b++) __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_gemm_rows_k1: the row-set contraction with ONE A plane and Ka <= 256 in the slice arithmetics (the class-representative
// convs of the split levels, forward and dX, and the two projections of the final conv).  k_gemm_planes_ws was shaped for
// K = 3 Ka = 384 .. 768: at 2 .. 16 chunks its ring is prologue and drain, with at most 16 KB of A in flight per block.  Here:
//   * 4 waves, every one loads, splits AND multiplies; no chunk ring.  K is walked in passes of KP = 64 (32 when Ka is no
//     multiple of 64) columns; the loads of two passes - the whole K up to Ka = 128 - are requested before anything waits,
//     32 .. 64 KB in flight per block, and pass p + 2 is requested as soon as pass p sits in LDS;
//   * LDS holds one slice image of the A tile (activation on load and the split applied on the way in), NS x 128 x (KP + 8)
//     (row stride 36 / 20 dwords: conflict-free ds_read_b128 fragments and, KP = 32 with its row permutation, ds_write_b64);
//   * B fragments come from the pre-split image (p2m_weight_split layout) straight into registers, one k step ahead: the
//     weight is <= 256 x 256 and L2-resident, and the fragment a lane needs is 16 contiguous bytes of it;
//   * one LDS barrier between "image stored" and "MFMAs", one before the image is overwritten;
//   * a wave whose columns all lie beyond N (the 64-wide tile of N = 32) skips its B loads and MFMAs: nothing of them is stored.
// 256 threads and launch bound 2 = two blocks per CU at up to 256 registers: no spill, the epilogue included.
// Results are BITWISE those of k_gemm_planes_ws: k ascending in steps of 16, the same product order per accumulator, the same
// accumulator -> (row, column) mapping, the same tile -> rows mapping, and gemm_epilogue itself.
// ---------------------------------------------------------------------------------------------
#ifdef P2M_K1_TRACE
// probe build (tools/k1_trace.sh, tools/probes/rows_k1_probe.py): s_memtime stamps of thread 0 of the first 4096 blocks -
// 0 start, 1 first image stored (row table, first loads, split), 2 k loop done, 3 epilogue done
__device__ unsigned long long g_k1_tr[4096][4];
#define P2M_K1T(ev)                                                                      \
  do {                                                                                   \
    if (threadIdx.x == 0 && blockIdx.x < 4096) g_k1_tr[blockIdx.x][ev] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define P2M_K1T(ev) do { } while (0)
#endif

template <int BN, bool EXTRA, int NS, int KP, bool CO>
__global__ __launch_bounds__(256, 2) void k_gemm_rows_k1(GemmArgs g) {
  typedef typename SliceFrag<NS>::type frag_t;
  constexpr bool ROWS = true;
  constexpr int WTN = BN / 2;
  constexpr int TN = WTN / 32;
  constexpr int TM = 2;
  constexpr int LDX = KP + 8;
  constexpr int TPR = KP / 4;             // threads per row (one float4 each)
  constexpr int RPS = 256 / TPR;          // rows per sweep of the block
  constexpr int NSW = BM / RPS;           // sweeps = float4 loads per thread and pass
  constexpr int KSTEPS = KP / 16;         // MFMA k steps per pass (2 or 4: the B double buffer's parity is static)
  constexpr int A_IMG = NS * BM * LDX;    // bf16 / fp16 elements
  static_assert(KP == 64 || KP == 32, "pass width");
  static_assert(A_IMG / 2 >= EPI_LDS_WORDS(BN, CO),
                "the epilogue's two reduction buffers and its copy-out strips live in the image, in front of the row table");
  __shared__ __attribute__((aligned(16))) float smem[A_IMG / 2 + ROWTAB_WORDS];
  __shared__ __attribute__((aligned(16))) float actco[2 * 256];
  unsigned short* As = reinterpret_cast<unsigned short*>(smem);
  int* rowtab = reinterpret_cast<int*>(smem + A_IMG / 2);

  int mt, nt;
  if (!tile_of_block(blockIdx.x, g.ntm, g.ntn, mt, nt)) return;
  P2M_K1T(0);
  const int t = threadIdx.x;
  const long m0 = (long)mt * BM;
  const int n0 = nt * BN;
  const int rs_b = mt / g.tps;
  const int rs_i0 = (mt - rs_b * g.tps) * BM;
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int npass = g.Ka / KP;
  const bool in_act = g.in_scale != nullptr;                             // block-uniform
  const bool live = n0 + wn * WTN < g.N;                                  // wave-uniform
  float a_sc = 1.f;
  int descale = 0;
  if (NS == 2) {
    const int sa = slice_scale_exp(*g.a_amax, g.a_bits);
    a_sc = exp2_int(sa);
    descale = -(sa + slice_scale_exp(*g.b_amax, 0));
  }

  // the small tables first (their loads are older than the A loads: filling LDS from them waits for nothing else)
  int rt_row = -1;
  float rt_w = 0.f, co_sc = 0.f, co_sh = 0.f;
  if (t < BM) {
    const int i = rs_i0 + t;
    if (i < g.nset) {
      rt_row = rs_b * g.V + g.ids[i];
      if (g.row_w != nullptr) rt_w = g.row_w[i];
    }
  }
  if (in_act && t < g.Ka) {
    co_sc = g.in_scale[t];
    co_sh = g.in_shift[t];
  }

  // A addresses: wave-uniform 64-bit base + a 32-bit byte offset per thread and sweep, fixed for the kernel; rows past the
  // set re-read its last row (their accumulators are dropped by the epilogue)
  const int a_g = t / TPR;                                               // row group of the thread inside a sweep
  const int a_row = KP == 64 ? a_g : (((a_g & 1) << 2) | ((a_g >> 1) & 3) | ((a_g >> 3) << 3));
  const int a_k4 = (t % TPR) * 4;
  const long sbase0 = (((long)rs_b * g.V) >> g.a0_shift) * g.Ka;         // V is even whenever a0_shift = 1
  unsigned voff[NSW];
#pragma unroll
  for (int ps = 0; ps < NSW; ps++) {
    int i = rs_i0 + ps * RPS + a_row;
    if (i >= g.nset) i = g.nset - 1;
    voff[ps] = (unsigned)((((g.ids[i] >> g.a0_shift) * g.Ka) + a_k4) * 4);
  }
  f32x4 ra[2][NSW];
  auto load_pass = [&](int p, f32x4 (&a)[NSW]) {
    const char* Ab = reinterpret_cast<const char*>(g.A[0] + sbase0 + p * KP);                        // uniform
#pragma unroll
    for (int ps = 0; ps < NSW; ps++) a[ps] = *reinterpret_cast<const f32x4*>(Ab + voff[ps]);
  };
  auto store_pass = [&](int p, f32x4 (&a)[NSW]) {
    if (in_act) {                          // BatchNorm + ReLU of the previous conv on load
      const f32x4 sc = *reinterpret_cast<const f32x4*>(&actco[p * KP + a_k4]);
      const f32x4 sh = *reinterpret_cast<const f32x4*>(&actco[256 + p * KP + a_k4]);
#pragma unroll
      for (int ps = 0; ps < NSW; ps++)
#pragma unroll
        for (int e = 0; e < 4; e++) a[ps][e] = fmaxf(fmaf(a[ps][e], sc[e], sh[e]), 0.f);
    }
#pragma unroll
    for (int ps = 0; ps < NSW; ps++) {
      u32x2 sl[NS];
      split_pack4<NS>(a[ps][0], a[ps][1], a[ps][2], a[ps][3], a_sc, sl);
      unsigned short* d = As + (ps * RPS + a_row) * LDX + a_k4;
#pragma unroll
      for (int q = 0; q < NS; q++) *reinterpret_cast<u32x2*>(d + q * BM * LDX) = sl[q];
    }
  };

  load_pass(0, ra[0]);
  if (npass > 1) load_pass(1, ra[1]);                                  // block-uniform

  // B fragments of k step kc (16 rows of the weight): Bx[kc][slice][n][16], 16 bytes per lane
  const long bx_slice = (long)g.Npad * 16;
  const int nsteps = g.Ka / 16;
  unsigned bx_voff[TN];
#pragma unroll
  for (int j = 0; j < TN; j++) bx_voff[j] = (unsigned)((((n0 + wn * WTN + j * 32 + l31) * 16) + lhi * 8) * 2);
  frag_t fb[2][NS][TN];
  auto load_b = [&](int kc, frag_t (&b)[NS][TN]) {
    const char* src0 = reinterpret_cast<const char*>(g.Bx + (long)kc * (NS * bx_slice));              // uniform
#pragma unroll
    for (int sl = 0; sl < NS; sl++)
#pragma unroll
      for (int j = 0; j < TN; j++)
        b[sl][j] = __builtin_bit_cast(frag_t, *reinterpret_cast<const u32x4*>(src0 + sl * 2 * bx_slice + bx_voff[j]));
  };
  if (live) load_b(0, fb[0]);

  if (t < BM) {
    rowtab[t] = rt_row;
    if (g.row_w != nullptr) {              // rows_weights_fill, from the value already loaded
      float* wtab = reinterpret_cast<float*>(rowtab + BM);
      wtab[t] = rt_w;
      float s = rt_w;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if ((t & 63) == 0) wtab[BM + (t >> 6)] = s;
    }
  }
  if (in_act) {
    if (t < g.Ka) {
      actco[t] = co_sc;
      actco[256 + t] = co_sh;
    }
    lds_block_barrier();
  }

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

  auto mfma_pass = [&](int p) {
    const unsigned short* as = As + (wm * 64 + l31) * LDX + lhi * 8;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ks++) {
      const int kc = p * KSTEPS + ks;
      frag_t fa[NS][TM];
#pragma unroll
      for (int sl = 0; sl < NS; sl++)
#pragma unroll
        for (int i = 0; i < TM; i++)
          fa[sl][i] = __builtin_bit_cast(frag_t, *reinterpret_cast<const u32x4*>(as + (sl * BM + i * 32) * LDX + ks * 16));
      frag_t (&b)[NS][TN] = fb[ks & 1];
      load_b(kc + 1 < nsteps ? kc + 1 : kc, fb[(ks + 1) & 1]);            // one step ahead (the last one re-reads itself)
#define P2M_PAIR(SA, SB)                                                                       \
  _Pragma("unroll") for (int i = 0; i < TM; i++) _Pragma("unroll") for (int j = 0; j < TN; j++) \
      acc[i][j] = slice_mfma<NS>(fa[SA][i], b[SB][j], acc[i][j]);
      if constexpr (NS == 3) {          // smallest products first
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
    }
  };

  for (int p = 0; p < npass; p += 2) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int pp = p + h;
      if (pp < npass) {                                                   // block-uniform
        if (pp > 0) lds_block_barrier();                                  // every wave is done with the previous image
        store_pass(pp, ra[h]);
        if (pp + 2 < npass) load_pass(pp + 2, ra[h]);
        lds_block_barrier();
        if (pp == 0) P2M_K1T(1);
        if (live) mfma_pass(pp);
      }
    }
  }
  P2M_K1T(2);
  __syncthreads();   // the image is free: the epilogue's reduction reuses it
  gemm_epilogue<BN, EXTRA, ROWS, CO>(g, acc, smem, rowtab, mt, m0, n0, rs_i0, wm, wn, l31, lhi, descale);
  P2M_K1T(3);
}

// scalar fall-back (first conv Fin=5 -> K=15; last conv Fout=3): one thread per (row, n)
__global__ void k_naive_gemm_planes(GemmArgs g) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= g.M * g.N) return;
  long r = idx / g.N;
  int n = (int)(idx - r * g.N);
  float acc = 0.f;
  for (int p = 0; p < g.nplanesA; p++) {
    const float* a = g.A[p] + (r >> (p == 0 ? g.a0_shift : 0)) * g.Ka;
    const float* b = g.Bm + (long)p * g.Ka * g.N + n;
    for (int k = 0; k < g.Ka; k++) acc = fmaf(a[k], b[(long)k * g.N], acc);
  }
  if (g.bias) acc += g.bias[n];
  if (g.act_scale) acc = fmaf(acc, g.act_scale[n], g.act_shift[n]);
  if (g.act_relu) acc = fmaxf(acc, 0.f);
  if (g.addend) acc += g.addend[r * g.N + n];
  int q = n / g.Nc;
  g.C[q][r * g.Nc + (n - q * g.Nc)] = acc;
}

// per-128-row-tile statistics for the naive path (same partial format as the MFMA epilogue)
__global__ void k_naive_tile_stats(const float* __restrict__ Y, float* __restrict__ stats, long M, int N) {
  int tile = blockIdx.x;
  long r0 = (long)tile * BM;
  long r1 = r0 + BM < M ? r0 + BM : M;
  for (int n = threadIdx.x; n < N; n += blockDim.x) {
    float s = 0.f;
    for (long r = r0; r < r1; r++) s += Y[r * N + n];
    float mean = s / (float)(r1 - r0);
    float m2 = 0.f;
    for (long r = r0; r < r1; r++) {
      float d = Y[r * N + n] - mean;
      m2 += d * d;
    }
    stats[(long)tile * 2 * N + n] = s;
    stats[(long)tile * 2 * N + N + n] = m2;
  }
}

}  // namespace p2m

using namespace p2m;

extern "C" int32_t p2m_stats_tile_rows(void) { return BM; }

// P2M_ROWS_K1 (read once per process): 1 (default) = row-set launches with one A plane and Ka <= 256
// in the slice arithmetics (both) take k_gemm_rows_k1; 0 = k_gemm_planes_ws as before - the A/B switch, bitwise the same results.
static bool rows_k1() {
  static const bool v = [] { const char* e = getenv("P2M_ROWS_K1"); return e ? atoi(e) != 0 : true; }();
  return v;
}
// P2M_EPI_COPYOUT (read once per process): 1 = the slice-arithmetic contractions copy their output
// tile out through wave-private LDS strips with 16-byte stores (gemm_epilogue<.., CO = true>); 0 = the 4-byte walk.  Bitwise the
// same results.  The staged forms need every output plane, and the addend, 16-byte aligned (rows then are: Nc % 32 == 0); a
// launch that is not takes the walk, as do the pair-sum launches.
static bool epi_copyout() {
  static const bool v = [] { const char* e = getenv("P2M_EPI_COPYOUT"); return e ? atoi(e) != 0 : P2M_EPI_COPYOUT_DEFAULT; }();
  return v;
}

// picks the instantiation: tile width from N, EXTRA epilogue, native f32 MFMA or slices (g.Bx != nullptr; two fp16
// slices when g.a_amax is set)
template <bool ROWS>
static void launch_gemm_planes(GemmArgs& g, bool extra, hipStream_t s) {
  const bool wide = (g.N % 128 == 0);
  g.ntn = wide ? g.N / 128 : cdiv(g.N, 64);
  const dim3 grid(cdiv(g.ntm, 8) * 8 * g.ntn);
  const bool co = epi_copyout() && !g.pair_out && aligned16(g.C[0]) && aligned16(g.C[1]) && aligned16(g.C[2]) &&
                  aligned16(g.addend);              // (planes that are not there are NULL)
  const bool f16 = g.a_amax != nullptr;
  if constexpr (ROWS) {
    if (g.nplanesA == 1 && g.Ka <= 256 && g.Bx != nullptr && rows_k1()) {
      with_bools([&](auto wide_t, auto extra_t, auto f16_t, auto kp64_t, auto co_t) {
        constexpr int BN = decltype(wide_t)::value ? 128 : 64, NS = decltype(f16_t)::value ? 2 : 3;
        constexpr int KP = decltype(kp64_t)::value ? 64 : 32;
        constexpr bool EX = decltype(extra_t)::value, CO = decltype(co_t)::value;
        hipLaunchKernelGGL((k_gemm_rows_k1<BN, EX, NS, KP, CO>), grid, dim3(256), 0, s, g);
      }, wide, extra, f16, g.Ka % 64 == 0, co);
      return;
    }
  }
  if (g.Bx != nullptr) {
    // (the 128-wide row-set forms have no staged walk with statistics: k_gemm_planes_ws)
    const bool co_ws = co && !(ROWS && wide && g.stats != nullptr);
    with_bools([&](auto wide_t, auto extra_t, auto f16_t, auto co_t) {
      constexpr int BN = decltype(wide_t)::value ? 128 : 64, NS = decltype(f16_t)::value ? 2 : 3;
      constexpr bool EX = decltype(extra_t)::value, CO = decltype(co_t)::value;
      hipLaunchKernelGGL((k_gemm_planes_ws<BN, EX, ROWS, NS, CO>), grid, dim3(512), 0, s, g);
    }, wide, extra, f16, co_ws);
  } else {
    with_bools([&](auto wide_t, auto extra_t) {
      constexpr int BN = decltype(wide_t)::value ? 128 : 64;
      constexpr bool EX = decltype(extra_t)::value;
      hipLaunchKernelGGL((k_gemm_planes<BN, 32, EX, ROWS>), grid, dim3(256), 0, s, g);
    }, wide, extra);
  }
}

extern "C" int p2m_gemm_planes(const float* A0, const float* A1, const float* A2, int32_t nplanesA, int32_t Ka,
                               int32_t a0_shift, const float* Bm, const void* Bsplit, int32_t arith,
                               const void* a_amax, int32_t a_bits, const float* bias,
                               const float* addend, float* C0, float* C1, float* C2, int32_t nplanesC, int32_t Nc,
                               int32_t pair_out, int64_t M, float* stats, const float* act_scale,
                               const float* act_shift, int32_t act_relu, void* amax_out, void* stream) {
  P2M_CHECK_ARG(nplanesA >= 1 && nplanesA <= 3 && nplanesC >= 1 && nplanesC <= 3, "plane count must be 1..3");
  P2M_CHECK_ARG(arith == P2M_ARITH_F32 || arith == P2M_ARITH_BF16X3 || arith == P2M_ARITH_F16X2, "unknown arithmetic");
  P2M_CHECK_ARG((act_scale == nullptr) == (act_shift == nullptr), "act_scale / act_shift must both be given or both NULL");
  P2M_CHECK_ARG(!((act_scale || act_relu) && (stats || pair_out)), "fused activation excludes stats and pair_out");
  P2M_CHECK_ARG(A0 && Bm && C0 && Ka > 0 && Nc > 0, "null pointer or empty shape");
  P2M_CHECK_ARG(a0_shift == 0 || a0_shift == 1, "a0_shift must be 0 or 1");
  if (M <= 0) return P2M_OK;
  GemmArgs g;
  g.A[0] = A0; g.A[1] = A1; g.A[2] = A2;
  g.C[0] = C0; g.C[1] = C1; g.C[2] = C2;
  for (int p = 0; p < nplanesA; p++) P2M_CHECK_ARG(g.A[p] != nullptr, "missing A plane");
  for (int p = 0; p < nplanesC; p++) P2M_CHECK_ARG(g.C[p] != nullptr, "missing C plane");
  P2M_CHECK_ARG((addend == nullptr && !pair_out) || nplanesC == 1, "addend / pair_out need a single output plane");
  P2M_CHECK_ARG(!(pair_out && stats), "pair_out and stats are mutually exclusive");
  g.Bm = Bm; g.bias = bias; g.addend = addend; g.pair_out = pair_out; g.stats = stats; g.M = M;
  g.act_scale = act_scale; g.act_shift = act_shift; g.act_relu = act_relu;
  g.nplanesA = nplanesA; g.Ka = Ka; g.a0_shift = a0_shift;
  g.N = nplanesC * Nc; g.Nc = Nc;
  g.amax_out = static_cast<unsigned*>(amax_out);
  hipStream_t s = (hipStream_t)stream;
  const bool mfma_ok = (Ka % BK == 0) && (g.N % 32 == 0) && (Nc % 32 == 0);
  if (!mfma_ok) {
    P2M_CHECK_ARG(!pair_out, "pair_out needs the MFMA path (Ka % 32 == 0, N % 32 == 0)");
    P2M_CHECK_ARG(!amax_out, "amax_out needs the MFMA path (Ka % 32 == 0, N % 32 == 0)");
    long tot = M * g.N;
    hipLaunchKernelGGL(k_naive_gemm_planes, dim3(cdiv(tot, 256)), dim3(256), 0, s, g);
    if (stats) {
      P2M_CHECK_ARG(nplanesC == 1, "stats need a single output plane");
      hipLaunchKernelGGL(k_naive_tile_stats, dim3(cdiv(M, BM)), dim3(64), 0, s, C0, stats, (long)M, g.N);
    }
    return check_launch("gemm_planes(naive)");
  }
  if (arith != P2M_ARITH_F32) {
    P2M_CHECK_ARG(Bsplit != nullptr, "the slice arithmetics need the pre-split weight (p2m_weight_split)");
    P2M_CHECK_ARG(arith != P2M_ARITH_F16X2 || a_amax != nullptr, "P2M_ARITH_F16X2 needs the amax word of the A planes");
    g.Bx = static_cast<const unsigned short*>(Bsplit);
    g.Npad = cdiv(g.N, 128) * 128;
    g.Ktot = nplanesA * Ka;
    if (arith == P2M_ARITH_F16X2) {
      g.a_amax = static_cast<const unsigned*>(a_amax);
      g.a_bits = a_bits;
      g.b_amax = weight_amax_word(Bsplit, arith, g.Npad, g.Ktot);
    }
  }
  g.ntm = cdiv(M, BM);
  launch_gemm_planes<false>(g, addend != nullptr || pair_out, s);
  return check_launch("gemm_planes");
}

extern "C" int p2m_gemm_planes_rows(p2m_graph_t gh, int32_t row_set, int32_t B, const float* A0, const float* A1,
                                    const float* A2, int32_t nplanesA, int32_t Ka, int32_t a0_shift,
                                    int32_t planes_compact, const float* Bm, const void* Bsplit, int32_t arith,
                                    const void* a_amax, int32_t a_bits, const float* bias,
                                    const float* addend, float* C, int32_t N, float* stats, const float* act_scale,
                                    const float* act_shift, int32_t act_relu, void* amax_out, const float* in_scale,
                                    const float* in_shift, void* stream) {
  P2M_CHECK_ARG(gh && A0 && Bm && C, "null pointer");
  P2M_CHECK_ARG((in_scale == nullptr) == (in_shift == nullptr), "in_scale / in_shift must both be given or both NULL");
  P2M_CHECK_ARG(in_scale == nullptr || (arith != P2M_ARITH_F32 && Ka <= 256),
                "activation on load exists in the slice arithmetics only, for Ka <= 256");
  P2M_CHECK_ARG(arith == P2M_ARITH_F32 || arith == P2M_ARITH_BF16X3 || arith == P2M_ARITH_F16X2, "unknown arithmetic");
  P2M_CHECK_ARG(arith == P2M_ARITH_F32 || Bsplit != nullptr, "the slice arithmetics need the pre-split weight (p2m_weight_split)");
  P2M_CHECK_ARG(arith != P2M_ARITH_F16X2 || a_amax != nullptr, "P2M_ARITH_F16X2 needs the amax word of the A planes");
  P2M_CHECK_ARG((act_scale == nullptr) == (act_shift == nullptr), "act_scale / act_shift must both be given or both NULL");
  P2M_CHECK_ARG(!((act_scale || act_relu) && stats), "fused activation excludes stats");
  P2M_CHECK_ARG(row_set_valid(row_set), "row_set must be 1 (real), 2 (fake), 3 (paired real) or 4 (paired fake)");
  P2M_CHECK_ARG(nplanesA >= 1 && nplanesA <= 3, "plane count must be 1..3");
  P2M_CHECK_ARG(Ka > 0 && Ka % BK == 0 && N > 0 && N % 32 == 0, "Ka and N must be positive multiples of 32");
  P2M_CHECK_ARG(a0_shift == 0 || a0_shift == 1, "a0_shift must be 0 or 1");
  const Graph& gr = *reinterpret_cast<const Graph*>(gh);
  const RowSet rs = row_set_of(gr, row_set);
  if (B <= 0 || rs.n == 0) return P2M_OK;
  // the epilogue addresses C and the addend as sample base + a 32-bit byte offset (as the k loop does A)
  P2M_CHECK_ARG((long)rs.V * N < (1l << 30), "one sample of C must stay below 4 GiB (V * N < 2^30)");
  GemmArgs g;
  g.A[0] = A0; g.A[1] = A1; g.A[2] = A2;
  for (int p = 0; p < nplanesA; p++) P2M_CHECK_ARG(g.A[p] != nullptr, "missing A plane");
  g.C[0] = C;
  g.Bm = Bm; g.bias = bias; g.addend = addend; g.stats = stats;
  g.act_scale = act_scale; g.act_shift = act_shift; g.act_relu = act_relu;
  g.nplanesA = nplanesA; g.Ka = Ka; g.a0_shift = a0_shift; g.N = N; g.Nc = N;
  g.ids = rs.ids; g.nset = rs.n; g.V = rs.V; g.tps = cdiv(rs.n, BM); g.compact = planes_compact;
  g.row_w = (stats != nullptr && row_set == 2) ? gr.fake_wts : nullptr;   // representatives count once per class member
  g.Bx = arith == P2M_ARITH_F32 ? nullptr : static_cast<const unsigned short*>(Bsplit);
  g.Npad = cdiv(N, 128) * 128;
  g.Ktot = nplanesA * Ka;
  if (arith == P2M_ARITH_F16X2) {
    g.a_amax = static_cast<const unsigned*>(a_amax);
    g.a_bits = a_bits;
    g.b_amax = weight_amax_word(Bsplit, arith, g.Npad, g.Ktot);
  }
  g.amax_out = static_cast<unsigned*>(amax_out);
  g.in_scale = in_scale; g.in_shift = in_shift;
  g.M = (long)B * g.tps * BM;       // logical (padded) rows; validity comes from the row table
  g.ntm = B * g.tps;
  launch_gemm_planes<true>(g, addend != nullptr, (hipStream_t)stream);
  return check_launch("gemm_planes_rows");
}

// rows per sample tile count of a row set (for the BatchNorm finalize): tiles_per_sample = ceil(n / 128)
extern "C" int32_t p2m_rows_tiles_per_sample(p2m_graph_t gh, int32_t row_set) {
  if (!gh || !row_set_valid(row_set)) return 0;
  const Graph& gr = *reinterpret_cast<const Graph*>(gh);
  return cdiv(row_set_of(gr, row_set).n, BM);
}

#ifdef P2M_K1_TRACE
extern "C" int p2m_k1_trace_dump(unsigned long long* out /* [4096][4] host */) {
  if (hipDeviceSynchronize() != hipSuccess) return P2M_ERR_HIP;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(p2m::g_k1_tr), sizeof(unsigned long long) * 4096 * 4) == hipSuccess ? P2M_OK
                                                                                                                : P2M_ERR_HIP;
}
#endif
