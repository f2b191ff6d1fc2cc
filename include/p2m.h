/*
 * p2m.h -- C ABI of libp2m_hip.so: the MI355X (gfx950) implementation of the Pose2Mesh
 * coarse-to-fine Chebyshev graph-convolution hot path.
 *
 * The reference (hongsukchoi/Pose2Mesh_RELEASE) is pure PyTorch and has no FFI layer; the
 * "kernels" below replace the library ops that the reference dispatches to.  Every entry point
 * cites the reference lines whose arithmetic it replaces (paths relative to the reference root).
 *
 * Conventions
 *  - plain C symbols, device pointers + sizes + hipStream_t (passed as void*); the library never
 *    allocates caller-visible device memory except the immutable per-level graph handle (internally it keeps one small
 *    scratch buffer per (device, stream) for the two-stage BatchNorm finalize, allocated on first use);
 *  - all matrices fp32 row-major; a "row" is one (sample, vertex) pair, r = b*V + v;
 *  - return 0 on success, negative p2m_status on error; p2m_last_error_string() has the detail;
 *    nothing throws across the boundary;
 *  - thread-safe: no mutable global state besides the thread-local error string; the one kernel-variant knob of the
 *    library (P2M_BASIS_TILED) is read once from the environment and never changes;
 *  - `shift` arguments implement the reference's nearest x2 vertex un-pooling
 *    (lib/models/meshnet.py:71-78) *virtually*: a tensor stored at V/2 vertices is read as if it
 *    had V vertices through row index r>>1 (valid because V is even and r = b*V+v).
 */
#ifndef P2M_H_
#define P2M_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  P2M_OK = 0,
  P2M_ERR_INVALID = -1,   /* bad argument / unsupported shape */
  P2M_ERR_HIP = -2,       /* HIP runtime error (launch, alloc, copy) */
  P2M_ERR_NOMEM = -3
} p2m_status;

/* Arithmetic of the dense contractions.  All compute the SAME fp32 contraction with fp32 accumulation:
 * F32     native f32 MFMA (v_mfma_f32_32x32x2_f32), bitwise an fmaf chain;
 * BF16X3  every fp32 operand cut EXACTLY into three bf16 slices (8+8+8 significand bits), the six slice products of
 *         weight >= 2^-16 on v_mfma_f32_32x32x16_bf16; dropped terms <= 2^-23 |a b| (one fp32 rounding);
 * F16X2   every operand TENSOR multiplied by a power of two 2^s that brings an upper bound U of its magnitudes into
 *         [2^14, 2^15), then cut into two fp16 slices (11+11 significand bits, round to nearest); three slice products
 *         on v_mfma_f32_32x32x16_f16, the accumulator rescaled exactly (v_ldexp) in the epilogue.  An operand carries
 *         x (1 + d), |d| <= 2^-22, for |x| >= 2^-18 U and an absolute error <= 2^-40 U below; a product additionally
 *         drops <= 2^-22 |a b|.  Half the matrix-core work of BF16X3.  U comes from an AMAX WORD: a uint32 in device
 *         memory holding the bits of a non-negative float >= max |x| over the tensor, produced on the device by
 *         whoever wrote the tensor (the amax_out arguments, p2m_amax, p2m_amax_rows; NaN and infinity are left out,
 *         so a non-finite element poisons its own rows of a contraction, as in fp32, not the scale) - it only has to BOUND the
 *         magnitudes; `bits` arguments add binades of headroom for operands derived from the bounded tensor inside
 *         the same call (Chebyshev planes: p2m_graph_plane_bits).                                                  */
enum { P2M_ARITH_F32 = 0, P2M_ARITH_BF16X3 = 1, P2M_ARITH_F16X2 = 2 };

typedef struct p2m_graph* p2m_graph_t;

/* Thread-local description of the last error returned on this thread. */
const char* p2m_last_error_string(void);
/* Library version / build info (e.g. "p2m-hip 0.3 (gfx950; ...)"). */
const char* p2m_version(void);
/* Identity of the stream capture `stream` is recording into: *id_out = the runtime's capture id (hipStreamGetCaptureInfo),
 * 0 when the stream is not capturing.  Host-side only (no launch): the amax-word pool of the Python layer keys its chunks
 * on it, so that two captures taken back to back never share graph-private memory.  No reference counterpart (the
 * reference has no stream captures). */
int p2m_stream_capture_id(void* stream, unsigned long long* id_out);

/* ---- graph handle: one per coarsening level ------------------------------------------------
 * Replaces sparse_python_to_torch (lib/graph_utils.py:98-109) and the per-forward
 * `self.graph_L[i].cuda()` upload (lib/models/meshnet.py:81).  Input: host CSR of the rescaled
 * Laplacian L (fp32, V x V, symmetric).  The handle bakes, on the current device, the merged
 * CSR of L and L2 = 2*L*L - I (double accumulation on the host, rounded once to fp32) so the
 * K=3 Chebyshev recurrence T1 = L x, T2 = 2 L T1 - x (lib/models/backbones/cheby_graph_conv.py:25,28)
 * becomes ONE gather pass  T1 = L x, T2 = L2 x.  It also bakes the lists of real / isolated (padding) vertices
 * and, for levels that have both, the tile plans of the LDS-staged basis kernel (consecutive real rows grouped
 * by the union of their neighbourhoods: one plan per un-pool shift, one for the paired operator S L | S L2).
 * The handle is immutable afterwards, with one exception: p2m_graph_set_classes, to be called (once) before the
 * handle is used.                                                                                          */
int p2m_graph_create(const int32_t* row_ptr, const int32_t* col, const float* val,
                     int32_t V, int32_t nnz, p2m_graph_t* out);
int p2m_graph_destroy(p2m_graph_t g);
/* info[0]=V, info[1]=nnz(L), info[2]=nnz(merged L|L2), info[3]=max merged row length */
int p2m_graph_info(p2m_graph_t g, int32_t info[4]);

/* ---- Chebyshev basis (sparse stage, HBM-bound) ----------------------------------------------
 * cheby_graph_conv.py:16-34 without the permute/cat/permute shuffles.
 * X: (B, V>>in_shift, F)   T1, T2: (B, V, F).   T0 = X is never rewritten.
 * Algorithmic HBM bytes per call: 4*B*V*F*(1/(1<<in_shift) + 2).                               */
int p2m_cheb_basis_fwd(p2m_graph_t g, const float* X, float* T1, float* T2,
                       int32_t B, int32_t F, int32_t in_shift, void* stream);

/* Backward of the basis stage (autograd of cheby_graph_conv.py:25-28; L symmetric,
 * asserted at lib/coarsening.py:23):  dX = d0 + L d1 + L2 d2  (+ resid, same shape as d0).
 * d0,d1,d2,resid: (B, V, F).  dX: (B, V>>out_shift, F); with out_shift=1 the two children of a
 * coarse vertex are summed (backward of nn.Upsample nearest, meshnet.py:74).                  */
int p2m_cheb_basis_bwd(p2m_graph_t g, const float* d0, const float* d1, const float* d2,
                       const float* resid, float* dX,
                       int32_t B, int32_t F, int32_t out_shift, void* stream);

/* Narrow-output convolution by linearity (the final 64 -> 3 layer, cheby_graph_conv.py:25-37 re-associated):
 *   y = [x|Lx|L2x] W == P0 + L P1 + L2 P2 with P = x [W0|W1|W2] computed first by p2m_gemm_planes.
 * combine: Y[r, c] = bias[c] + P[r, c] + sum_j a_j P[col_j, nc+c] + b_j P[col_j, 2nc+c],  c < nc <= 4;
 *          P rows are ldp floats wide (ldp >= 3 nc), Y is [B*V, nc].
 * expand (its backward): E[r] = [ G[r] | (L G)[r] | (L2 G)[r] | 0.. ], G: [B*V, nc], E rows lde floats wide. */
int p2m_cheb_combine_small(p2m_graph_t g, const float* P, int32_t ldp, int32_t nc, const float* bias,
                           float* Y, int32_t B, void* stream);
int p2m_cheb_expand_small(p2m_graph_t g, const float* G, int32_t nc, float* E, int32_t lde, int32_t B,
                          void* stream);
/* Inference form of the combine: only the REAL vertices of the level are computed (padding vertices never reach a
 * caller: lib/core/base.py:201, demo/run.py:170 gather graph_perm_reverse[:nv]); P needs valid rows at real vertices
 * only.  out_index == NULL: Y is [B*V, nc], rows of padding vertices are left untouched.  out_index != NULL
 * ([V] int32, -1 = drop): vertex v goes to row out_index[v] of Y = [B, out_rows, nc], multiplied by scale -- the
 * perm-reverse gather (and the Tester's x1000) folded into the last conv's store.                                  */
int p2m_cheb_combine_small_real(p2m_graph_t g, const float* P, int32_t ldp, int32_t nc, const float* bias, float* Y,
                                int32_t B, const int32_t* out_index, int32_t out_rows, float scale, void* stream);

/* ---- weights ------------------------------------------------------------------------------
 * nn.Linear(Fin*K, Fout).weight is [Fout][fin*K + k] (cheby_graph_conv.py:32-37).  Packs it into
 *   Wt [k*Fin + fin][Fout]   (B operand of the forward contraction, K-major)
 *   W2 [Fout][k*Fin + fin]   (B operand of dZ = g W; may be NULL)
 *   W3 [k*Fout + fout][fin]  (B operand of the fused backward dX = [g|Lg|L2g] W3; may be NULL)
 * K=1 gives a plain transpose (used for fc, meshnet.py:36-37).                                */
int p2m_weight_pack(const float* W, float* Wt, float* W2, float* W3, int32_t Fout, int32_t Fin, int32_t K,
                    void* stream);
/* Sums `nchunks` partial gradients P[chunk][k*Fin+fin][Fout], Pdb[chunk][Fout] produced by
 * p2m_gemm_tn and writes dW in nn.Linear layout [Fout][fin*K+k] and db[Fout].
 * accumulate!=0 adds into dW/db instead of overwriting.  layout 1: P[chunk][fin][k*Fout+fout] (the
 * gradient taken as X^T [g|Lg|L2g]); layout 2 (K = 1): P[chunk][fout][fin] - a plain Linear's gradient taken as G^T X (the
 * operands of p2m_gemm_tn swapped), already in nn.Linear layout: coalesced on both sides (Pdb is then the wrong column sum:
 * pass NULL and reduce the bias gradient separately).  pdb_stride = row stride of Pdb (the N of the p2m_gemm_tn call); the
 * first Fout floats of a row count.  db and Pdb may each be NULL: db is then neither written nor read.               */
int p2m_weight_grad_unpack(const float* P, const float* Pdb, int32_t nchunks, float* dW, float* db,
                           int32_t Fout, int32_t Fin, int32_t K, int32_t accumulate, int32_t layout,
                           int32_t pdb_stride, void* stream);

/* ---- dense contraction (fp32; on the BF16 or the f32 MFMA pipe, see P2M_ARITH_*) -------------
 * C[r, n] = sum_p sum_k A_p[r (>> a0_shift if p==0), k] * Bm[p*Ka + k, n]  + bias[n]
 * A_p: nplanesA row-major [M, Ka] matrices (the Chebyshev basis planes X|T1|T2, or one plane);
 * Bm: [nplanesA*Ka, N] row-major; C is split in nplanesC column planes of width Nc (N = nplanesC*Nc),
 * C_q: [M, Nc].  Replaces `cl(x)` (cheby_graph_conv.py:37), `self.fc` (meshnet.py:105) and the
 * autograd dZ = g W.  If stats != NULL it receives per-row-tile BatchNorm partials
 * stats[tile][0][n] = sum_r y, stats[tile][1][n] = sum_r (y - tile_mean)^2, tile = 128 rows
 * (cheby_graph_conv.py:39 batch statistics; fake vertices included).
 * Shapes with Ka%32!=0 or N%32!=0 take a scalar (VALU) path.
 * addend (optional, single output plane): [M, N] added to the result (the block residual's gradient);
 * pair_out (single output plane): C is [M/2, N] and receives the sum of the two children rows of every
 * coarse vertex -- backward of nn.Upsample (meshnet.py:74) in the epilogue.  The backward uses this entry
 * point in "forward form": dX = [g | L g | L2 g] W3 with the planes from p2m_cheb_basis_fwd(g).
 *
 * Arithmetic (P2M_ARITH_* above).  arith = P2M_ARITH_F32: native f32 MFMA (bitwise an fmaf chain), Bsplit ignored.
 * The slice arithmetics run the same fp32 contraction on the 16-bit matrix pipe and need Bsplit, made from the same Bm
 * by p2m_weight_split with the SAME arith; P2M_ARITH_F16X2 also needs a_amax (amax word bounding ALL the A planes after
 * a_bits binades of headroom).  amax_out (optional, MFMA path): atomic max of |value stored| into a zeroed amax word -
 * the bound for whoever consumes C next.
 *
 * Fused activation (optional; inference): act_scale/act_shift != NULL applies v = fmaf(acc + bias, act_scale[n],
 * act_shift[n]) and act_relu != 0 then v = max(v, 0) before the store -- eval-mode BatchNorm (p2m_bn_eval_coeffs) and
 * F.relu (cheby_graph_conv.py:39, meshnet.py:100) folded into the contraction with the SAME two roundings as the
 * separate p2m_bn_act_fwd pass (bitwise the unfused result).  Excludes stats and pair_out.                          */
int p2m_gemm_planes(const float* A0, const float* A1, const float* A2, int32_t nplanesA, int32_t Ka,
                    int32_t a0_shift, const float* Bm, const void* Bsplit, int32_t arith, const void* a_amax,
                    int32_t a_bits, const float* bias, const float* addend,
                    float* C0, float* C1, float* C2, int32_t nplanesC, int32_t Nc, int32_t pair_out,
                    int64_t M, float* stats, const float* act_scale, const float* act_shift, int32_t act_relu,
                    void* amax_out, void* stream);
/* Bx[k / 16][s][n][k % 16] (uint16 bit patterns; n < ceil(N/128)*128, zero padded; K % 16 == 0):
 *   P2M_ARITH_BF16X3  s < 3 bf16 slices of Bm[k][n], Bm = slice 0 + slice 1 + slice 2 exactly;
 *   P2M_ARITH_F16X2   s < 2 fp16 slices of Bm[k][n] 2^sb, followed by the amax word the scale came from, from which
 *                     every consumer re-derives sb.  amax_in = NULL: max |Bm|, computed here (one extra small launch);
 *                     else the word of a tensor that bounds Bm after amax_bits binades - e.g. the parameter Bm is a
 *                     permutation of (0 bits), or W0 + a W1 + b W2 (p2m_weight_eff: ceil(log2(1 + |a| + |b|)) bits) -
 *                     so that one amax pass per parameter serves all of its derived operands.
 * p2m_weight_split_elems = number of uint16 elements of Bx (0: unsupported shape / arith).                          */
int64_t p2m_weight_split_elems(int32_t K, int32_t N, int32_t arith);
int p2m_weight_split(const float* Bm, int32_t K, int32_t N, int32_t arith, const void* amax_in, int32_t amax_bits,
                     void* Bx, void* stream);
/* Every slice image of a network's conv weights in two launches (instead of p2m_weight_pack + p2m_weight_eff x 2 +
 * p2m_weight_split x 4 + p2m_amax per layer and optimizer step).  dev_desc: DEVICE array of n descriptors, one per conv
 * layer with weight W[Fout][Fin * 3 + k] (nn.Linear layout, cheby_graph_conv.py:37): the images (each sized by
 * p2m_weight_split_elems for its [K, N]; NULL = not wanted)
 *   Bx_f   [3 Fin, Fout]   forward, real rows            Bx_ef  [Fin, Fout]   forward, padding rows: W0 + a W1 + b W2
 *   Bx_b   [3 Fout, Fin]   backward dX, real rows        Bx_eb  [Fout, Fin]   backward dX, padding rows
 * and, for P2M_ARITH_F16X2, the parameter's amax word (written here; eff_bits = ceil(log2(1 + |a| + |b|)) is the headroom
 * of the two effective forms).  The buffers and the descriptor array can be allocated once and reused every step.      */
typedef struct p2m_conv_weights {
  const float* W;
  int32_t Fout, Fin;
  float fake_a, fake_b;
  int32_t eff_bits, reserved;
  void *Bx_f, *Bx_ef, *Bx_b, *Bx_eb;
  void* amax;
} p2m_conv_weights;
int p2m_conv_weights_prepare(const p2m_conv_weights* dev_desc, int32_t n, int32_t arith, void* stream);
/* amax words: atomic max of |x| into *word (uint32, device; the caller zeroes it before the first contribution).
 * p2m_amax: n contiguous floats.  p2m_amax_rows: rows of a [B, V, F] tensor of a level -
 * row_set 0 = every row that holds data (all rows; the live rows once classes are declared), 1..4 = that row set.   */
int p2m_amax(const float* x, int64_t n, void* word, void* stream);
int p2m_amax_rows(p2m_graph_t g, int32_t row_set, const float* x, int32_t B, int32_t F, void* word, void* stream);
/* rows per BatchNorm partial tile and the number of tiles for M rows */
int32_t p2m_stats_tile_rows(void);

/* Weight-gradient contraction (G = [G0|G1|G2], nplanesG column planes of width Gc, N = nplanesG*Gc):
 *   P[chunk][p*Ka + k][n] = sum_{r in chunk} A_p[r][k] * G[r][n],
 * Pdb[chunk][n] = sum_{r in chunk} G[r][n];  chunk c covers rows [c*chunk_rows, (c+1)*chunk_rows).
 * (autograd of cheby_graph_conv.py:37 / meshnet.py:105.)                                       */
int p2m_gemm_tn(const float* A0, const float* A1, const float* A2, int32_t nplanesA, int32_t Ka,
                int32_t a0_shift, const float* G0, const float* G1, const float* G2, int32_t nplanesG,
                int32_t Gc, int64_t M, int64_t chunk_rows, float* P, float* Pdb, int32_t arith,
                const void* a_amax, int32_t a_bits, const void* g_amax, int32_t g_bits, void* stream);

/* ---- BatchNorm1d over B*V rows + ReLU + residual (cheby_graph_conv.py:39, meshnet.py:100,108-115)
 * finalize: reduces the GEMM's partials to batch mean / biased var, writes
 *   mean[N], invstd[N], scale = gamma*invstd, shift = beta - mean*scale and updates
 *   running_mean/var (momentum, unbiased var) exactly like nn.BatchNorm1d in train().         */
int p2m_bn_finalize(const float* stats, int32_t ntiles, int64_t M, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps,
                    float* mean, float* invstd, float* scale, float* shift, int32_t N, int32_t tile_rows,
                    void* stream);
/* eval(): scale/shift/invstd from the running statistics. */
int p2m_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* mean, float* invstd, float* scale,
                       float* shift, int32_t N, void* stream);
/* x[r,f] = act(y[r,f]*scale[f] + shift[f]) + lerp_F(resid[r>>res_shift, 0..Fres))[f]
 * act = ReLU if relu!=0; scale/shift may be NULL (identity); resid may be NULL.
 * lerp_F is F.interpolate(mode='linear', align_corners=False) along the FEATURE axis
 * (meshnet.py:109,114).  Rows: all M; with `classes` (a level's handle) the live rows of a level with declared
 * classes (holes are skipped); with real_rows_only != 0 only the handle's real vertices (inference on the real rows:
 * the other rows of y hold no data and x's stay untouched).  amax_out (optional, F % 4 == 0): atomic max of |x stored|
 * into a zeroed amax word (P2M_ARITH_F16X2 above) - the bound for the contraction that consumes x.                  */
int p2m_bn_act_fwd(const float* y, const float* scale, const float* shift, int32_t relu,
                   const float* resid, int32_t Fres, int32_t res_shift,
                   float* x, int64_t M, int32_t F, p2m_graph_t classes /* or NULL */, int32_t real_rows_only,
                   void* amax_out, void* stream);
/* backward through ReLU + BatchNorm (train: batch statistics; eval: running statistics).
 *   go = gx * (y*scale+shift > 0 or !relu)
 *   reduce:   part[blk][0][f] = sum go, part[blk][1][f] = sum go * yhat       (nblk = p2m_bn_bwd_blocks(M,F))
 *   finalize: dgamma, dbeta (accumulate!=0 adds), coef[0][f]=dbeta/M, coef[1][f]=dgamma/M
 *   apply:    gy = gamma*invstd*(go - coef0 - yhat*coef1)   (training)   |   gamma*invstd*go (eval, coef NULL) */
int32_t p2m_bn_bwd_blocks(int64_t M, int32_t F);
int32_t p2m_bn_bwd_blocks_classes(p2m_graph_t classes, int64_t M, int32_t F);   /* blocks when `classes` is passed */
/* classes (optional graph handle with p2m_graph_set_classes; NULL = every row counts): the passes walk the live rows
 * of the level only (holes are neither read nor written; part then has p2m_bn_bwd_blocks_classes blocks), and the apply
 * pass adds the constant term of a representative once per class member.                                           */
int p2m_bn_bwd_reduce(const float* gx, const float* y, const float* scale, const float* shift,
                      const float* mean, const float* invstd, int32_t relu, float* part,
                      int64_t M, int32_t F, p2m_graph_t classes, void* stream);
int p2m_bn_bwd_finalize(const float* part, int32_t nblk, int64_t M, float* dgamma, float* dbeta,
                        float* coef, int32_t accumulate, int32_t F, void* stream);
/* The reduce pass over the FAKE-vertex rows of a level only (b * V + fake id; with classes: the representatives, which
 * carry their class's summed gradient) - the complement of a reduction whose real-vertex rows were summed by the kernel
 * that produced gx (p2m_cheb_tile_gemm, bnr_*).  part: [p2m_bn_bwd_blocks_fake(g, B, F)][2][F]; F in {32, 64, 128, 256}.  */
int32_t p2m_bn_bwd_blocks_fake(p2m_graph_t g, int32_t B, int32_t F);
int p2m_bn_bwd_reduce_fake(p2m_graph_t g, const float* gx, const float* y, const float* scale, const float* shift,
                           const float* mean, const float* invstd, int32_t relu, float* part, int32_t B, int32_t F,
                           void* stream);
/* pair_gx / pair_gy (optional, [M/2, F]; M even, F in {32,64,128,256}): by-products pair_gx[q] = gx[2q] + gx[2q+1] and
 * pair_gy[q] = gy[2q] + gy[2q+1] -- the pair-sums the backward of an un-pooled conv needs (residual gradient for the
 * coarser level; plane S g of the paired operator), produced while the rows are in registers anyway.
 * amax_out (optional): atomic max of |gy stored| into a zeroed amax word (the pair sums are bounded by twice it).
 * zero_holes (with classes): the pass walks EVERY row and stores zeros at the holes (and at pair sums of two holes) instead
 * of leaving them untouched - for levels whose other kernels read all rows; no memset of the outputs is needed.        */
int p2m_bn_bwd_apply(const float* gx, const float* y, const float* scale, const float* shift,
                     const float* mean, const float* invstd, const float* gamma, const float* coef,
                     int32_t relu, float* gy, float* pair_gx, float* pair_gy, int64_t M, int32_t F,
                     p2m_graph_t classes, int32_t zero_holes, void* amax_out, void* stream);

/* out[p, f] = in[2p, f] + in[2p+1, f]   (backward of the x2 nearest un-pool, meshnet.py:74) */
int p2m_pair_sum(const float* in, float* out, int64_t Mout, int32_t F, p2m_graph_t classes /* of `in`'s level, or NULL */,
                 void* stream);
/* dst[r, i] += sum_j w(j,i) g[r, j]: transpose of the feature-axis resize (meshnet.py:109,114);
 * g: [M, F], dst: [M, Fres].                                                                   */
int p2m_lerp_bwd_add(const float* g, float* dst, int64_t M, int32_t F, int32_t Fres, void* stream);

/* ---- fake-vertex split (row-set launches) ----------------------------------------------------------------
 * Padding ("fake") vertices of the coarsening tree are isolated (lib/coarsening.py:236-245): their merged
 * CSR row is the diagonal alone and identical for the whole level, so T1 = a x, T2 = b x and the contraction of
 * cheby_graph_conv.py:37 needs only K = Fin with W_eff = W0 + a W1 + b W2 -- 2/3 of the MFMA work on 30-40 % of the
 * rows disappears, and the basis planes are only formed (compactly, [B*n_real, F]) for real vertices.
 * Rows are selected by row_set: 1 = real vertices, 2 = fake vertices (sorted id lists baked in the handle; 3 / 4: the
 * paired sets below, over V/2 rows); tensors
 * keep their (B, V, F) layout, only the launches iterate over the subset.  BatchNorm statistics still cover ALL
 * rows (the reference includes fake vertices, cheby_graph_conv.py:39): p2m_bn_finalize_rows merges both launches. */
int p2m_graph_split_info(p2m_graph_t g, int32_t counts[2] /* n_real, n_fake */, float coef[2] /* a, b */);
/* in_shift 1 needs an even V, as in p2m_cheb_basis_fwd (refused otherwise) */
int p2m_cheb_basis_fwd_real(p2m_graph_t g, const float* X, float* T1c, float* T2c, int32_t B, int32_t F,
                            int32_t in_shift, const float* act_scale /* or NULL */, const float* act_shift, void* stream);
/* ---- paired operator: the backward of an un-pooled conv at the COARSE resolution ------------------------------
 * A conv whose input was un-pooled x2 (meshnet.py:71-78,111) sees X_fine[r] = X_coarse[r >> 1], so with S = the
 * pair-sum (the un-pool's transpose) and L symmetric:
 *     dX_coarse = S ([g | L g | L2 g] W3) = [S g | S L g | S L2 g] W3,     dW = X_coarse^T [S g | S L g | S L2 g]
 * -- both contractions run over V/2 rows.  The handle of the FINE level bakes S L and S L2 as one more tile plan
 * (row c = merged row 2c + merged row 2c+1) and two more row sets over the coarse index space: row_set 3 = coarse
 * vertices with at least one real child (compact plane order), row_set 4 = both children fake (S L g = a S g,
 * S L2 g = b S g: effective weight, as for row_set 2).  counts = {0, 0}: no paired operator on this level.
 * p2m_cheb_basis_pair: P1c = S L g, P2c = S L2 g over row_set 3, compact [B*counts[0], F]; g: [B*V, F];
 * F = 32, 64 or a multiple of 128.  (S g itself is p2m_pair_sum.)                                                   */
int p2m_graph_pair_info(p2m_graph_t g, int32_t counts[2] /* n_pair_real, n_pair_fake */);
/* tiles of the LDS-staged basis kernel's plans: [in_shift 0, in_shift 1, paired]; 0 = no plan, the row kernel runs */
int p2m_graph_plan_info(p2m_graph_t g, int32_t ntiles[3]);
int p2m_cheb_basis_pair(p2m_graph_t g, const float* G, float* P1c, float* P2c, int32_t B, int32_t F, void* stream);
/* C[b*V + ids[i], :] = [A0[..] | A1 | A2] Bm + bias (+ addend): A0 is read at the actual row (>> a0_shift), A1/A2 at
 * the compact row b*n + i when planes_compact.  stats: [B * ceil(n/128)][2][N] per-sample tiles; for row_set 2 of a handle
 * with classes (p2m_graph_set_classes) every representative counts once per class member, as p2m_stats_rows_w would
 * count it (the tile weights for p2m_bn_finalize_split are the handle's).  in_scale / in_shift [Ka]
 * (optional; slice arithmetics, Ka <= 256): activation on load of PLANE 0, as in p2m_cheb_tile_gemm - A0 holds the raw
 * output y of the previous conv and the operand is max(fma(y, in_scale[k], in_shift[k]), 0) (A1 / A2 are then the planes
 * p2m_cheb_basis_fwd_real formed with the same act_scale / act_shift); a_amax must bound the activated operand.      */
int p2m_gemm_planes_rows(p2m_graph_t g, int32_t row_set, int32_t B, const float* A0, const float* A1,
                         const float* A2, int32_t nplanesA, int32_t Ka, int32_t a0_shift, int32_t planes_compact,
                         const float* Bm, const void* Bsplit, int32_t arith, const void* a_amax, int32_t a_bits,
                         const float* bias, const float* addend, float* C,
                         int32_t N, float* stats, const float* act_scale, const float* act_shift, int32_t act_relu,
                         void* amax_out, const float* in_scale /* or NULL */, const float* in_shift, void* stream);
int32_t p2m_rows_tiles_per_sample(p2m_graph_t g, int32_t row_set);
/* P[b*splits + s][k][n] = sum over the s-th slice of the row set of sample b of A[row][k] * G[row][n]
 * (G0 at the actual row, G1/G2 compact when planes_compact); Pdb likewise.  a_scale / a_shift [Ka] (optional, slice
 * arithmetics only): activation on load of A, as in p2m_cheb_tile_gemm - A holds the raw conv output y and the operand is
 * max(fma(y, a_scale[k], a_shift[k]), 0); a_amax then bounds that (p2m_act_bound).
 * splits <= -2 (round 6; slice arithmetics only): a chunk is -splits consecutive WHOLE samples instead of a slice of one -
 * P[c] (c < ceil(B / -splits)) sums the row sets of samples c * -splits ... : fewer partials where a sample has few rows.  */
int p2m_gemm_tn_rows(p2m_graph_t g, int32_t row_set, int32_t B, const float* A, int32_t Ka, int32_t a0_shift,
                     const float* G0, const float* G1, const float* G2, int32_t nplanesG, int32_t Gc,
                     int32_t planes_compact, int32_t splits, float* P, float* Pdb, int32_t arith,
                     const void* a_amax, const void* g_amax, int32_t g_bits, const float* a_scale,
                     const float* a_shift, void* stream);
/* We[k][n] = Wt[k][n] + a Wt[Ka+k][n] + b Wt[2Ka+k][n]  (Wt = [3Ka, N]) */
int p2m_weight_eff(const float* Wt, float* We, int32_t Ka, int32_t N, float a, float b, void* stream);
/* dW (nn.Linear layout) from the real-vertex partials P[c][fin][k*Fout+fo] plus the fake-vertex partials
 * P2[c][fin][fo] entering plane k with factor (1, s1, s2)[k]; db from both.  accumulate != 0 adds into dW/db (the
 * caller's gradient buffer, e.g. a slice of optim.FlatAdam.flat_grad) instead of overwriting.  K must be 3.  Pdb rows are
 * 3 Fout floats wide (the first Fout count), Pdb2 rows Fout.  db, Pdb and Pdb2 may each be NULL: db is written only when db
 * and Pdb are both given (Pdb2 alone does not reach it); with Pdb2 NULL db is the sum of Pdb alone.                  */
int p2m_weight_grad_unpack2(const float* P, const float* Pdb, int32_t nchunks, const float* P2, const float* Pdb2,
                            int32_t nchunks2, float s1, float s2, float* dW, float* db, int32_t Fout, int32_t Fin,
                            int32_t K, int32_t accumulate, void* stream);
int p2m_bn_finalize_rows(const float* stats_a, int32_t tps_a, int32_t rows_a, const float* stats_b, int32_t tps_b,
                         int32_t rows_b, int32_t B, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float momentum, float eps, float* mean, float* invstd, float* scale,
                         float* shift, int32_t N, void* stream);

/* Same, for the two launches of one split conv, with the sizes (and, with classes, the weights) taken from the handle. */
int p2m_bn_finalize_split(p2m_graph_t g, const float* stats_real, const float* stats_fake, int32_t B,
                          const float* gamma, const float* beta, float* running_mean, float* running_var,
                          float momentum, float eps, float* mean, float* invstd, float* scale, float* shift,
                          int32_t N, void* stream);

/* ---- Chebyshev basis inside the contraction (default on levels with a tile plan) ---------------------------------
 * The real rows of one graph convolution (lib/models/backbones/cheby_graph_conv.py:16-37) in ONE kernel - the planes
 * T1 = L X, T2 = (2 L L - I) X are formed per tile in LDS, cut into bf16 slices and contracted without touching HBM:
 *     C[b, v, :] = [ A0[b, v >> a0_shift] | (L X)[b, v] | (L2 X)[b, v] ] W (+ bias) (+ addend[b, v, :])
 * over the rows of the level's tile plan `plan` (p2m_graph_plan_info):
 *     0  real vertices v of the level;        X [B, V, Ka],   A0 [B, V, Ka]   (usually A0 = X),   C [B, V, N]
 *     1  the same with an un-pooled input:     X [B, V/2, Ka], A0 [B, V/2, Ka] read at v >> 1,     C [B, V, N]
 *     2  the paired operator (row set 3):      X [B, V, Ka],   A0 [B, V/2, Ka] = S X (pair-sums),  C [B, V/2, N],
 *        planes S L X, S L2 X - the backward of an un-pooled conv at the coarse resolution
 * Bx = p2m_weight_split of the [3 Ka, N] operand (rows k * Ka + fin).  N in {64, 128, 256}, Ka % 32 == 0
 * (p2m_cheb_tile_gemm_supported).  Rows of C outside the row set are not touched (fake vertices: p2m_gemm_planes_rows,
 * row set 2 / 4, with p2m_weight_eff).  Optional: stats[B * ntiles(plan)][2][N] BatchNorm partials per (sample, tile)
 * for p2m_bn_finalize_tiles; E1 / E2 [B * nset, Ka]: the two gathered planes, compact, for the weight gradient
 * p2m_gemm_tn_rows - bitwise those of p2m_cheb_basis_fwd_real / p2m_cheb_basis_pair where the kernel gathers with the
 * same fmaf chain (P2M_ARITH_BF16X3; N = 256), equal to fp32 round-off where the gather itself runs on the matrix cores
 * (P2M_ARITH_F16X2 with N <= 128: the tile's operator as a dense fp16-sliced block, baked with the plan); act_*: fused eval-mode
 * BatchNorm + ReLU as in p2m_gemm_planes (excludes stats).  arith: P2M_ARITH_BF16X3 or P2M_ARITH_F16X2 (Bx split with
 * the same arith; x_amax = amax word bounding X and A0, the kernel adds the level's p2m_graph_plane_bits for the planes
 * it forms).  amax_out as in p2m_gemm_planes.
 * in_scale / in_shift [Ka] (optional; both slice arithmetics and both gather forms since round 5; no planes out): ACTIVATION ON LOAD - X and A0 hold the
 * raw output y of the previous conv and the operand is x = max(fma(y, in_scale[f], in_shift[f]), 0), its BatchNorm + ReLU
 * (lib/models/backbones/cheby_graph_conv.py:39, lib/models/meshnet.py:100) with the two roundings of p2m_bn_act_fwd, applied in
 * the producer waves between the global load and the LDS image: the activated tensor never exists in HBM.  With
 * P2M_ARITH_F16X2 x_amax must then bound x (p2m_act_bound); P2M_ARITH_BF16X3 needs no bound.
 * bnr_y / bnr_co / bnr_part (optional, all or none; round 6): the BatchNorm-backward REDUCTION of the layer in front, fused
 * into the store of C.  In the backward pass C is g = dL/dx with x = relu(batch_norm(y)) the input of this conv
 * (lib/models/backbones/cheby_graph_conv.py:39, lib/models/meshnet.py:100), and the next step is p2m_bn_bwd_reduce over g
 * and y.  With bnr_y = y [B, c_rows, N] and bnr_co = [4][N] (mean, invstd, scale, shift of that BatchNorm) every block sums
 * g m and g m yhat (m = [y scale + shift > 0], yhat = (y - mean) invstd - the arithmetic of p2m_bn_bwd_reduce) over the
 * rows it stores and writes bnr_part[slot][2][N], slot < p2m_cheb_tile_gemm_bnr_slots (0: this arithmetic / width has no
 * fused reduction).  The fake-vertex rows of C come from another launch: p2m_bn_bwd_reduce_fake sums those, and
 * p2m_bn_bwd_finalize takes both partial sets as one array.  Saves the stand-alone pass over g and y for the real rows.  */
int32_t p2m_cheb_tile_gemm_supported(p2m_graph_t g, int32_t plan, int32_t Ka, int32_t N);
int32_t p2m_cheb_tile_gemm_bnr_slots(p2m_graph_t g, int32_t plan, int32_t arith, int32_t N, int32_t B);
/* 1 when a p2m_cheb_tile_gemm launch of this arithmetic and output width forms the planes with the gather ON THE MATRIX
 * CORES (the tile's operator as a dense pre-sliced block, TilePlan::ltx / ltx3): P2M_ARITH_F16X2 (two scaled fp16 slices,
 * 4 samples per unit) and - round 5 - P2M_ARITH_BF16X3 (three exact bf16 slices of operator and operand, 2 samples per
 * unit; OPT-IN, environment P2M_MG_EXACT=1 read once per process: it measured equal to the VALU gather), N <= 128.  The
 * optional planes E1 / E2 then agree with p2m_cheb_basis_fwd_real to fp32 round-off instead of bitwise.              */
int32_t p2m_cheb_tile_gemm_mg(int32_t arith, int32_t N);
int p2m_cheb_tile_gemm(p2m_graph_t g, int32_t plan, const float* X, const float* A0, int32_t Ka, const void* Bx,
                       int32_t arith, const void* x_amax, const float* bias, const float* addend, float* C, int32_t N,
                       float* stats, float* E1, float* E2, const float* act_scale, const float* act_shift,
                       int32_t act_relu, void* amax_out, const float* in_scale, const float* in_shift,
                       const float* bnr_y, const float* bnr_co, float* bnr_part, int32_t B, void* stream);
/* Bound of x = max(fma(y, scale[f], shift[f]), 0) over a tensor y whose amax word is y_amax:
 *     atomic max of max_f fma(amax(y), |scale[f]|, max(shift[f], 0)) into the amax word `word`
 * (a true bound in fp32: fma and max are monotone) - the x_amax / a_amax of a consumer that applies the activation on
 * load.  N <= 4096.                                                                                                        */
int p2m_act_bound(const float* scale, const float* shift, int32_t N, const void* y_amax, void* word, void* stream);
/* Binades of headroom that cover the Chebyshev planes of a level: ceil(log2(max(1, max_v sum_u |L_vu|, max_v sum_u
 * |L2_vu|))) for plan 0 / 1 (|L x|, |L2 x| <= 2^bits max |x|), one more for plan 2 (the pair sums).                */
int32_t p2m_graph_plane_bits(p2m_graph_t g, int32_t plan);
int p2m_bn_finalize_tiles(p2m_graph_t g, int32_t plan, const float* stats_real, const float* stats_fake, int32_t B,
                          const float* gamma, const float* beta, float* running_mean, float* running_var,
                          float momentum, float eps, float* mean, float* invstd, float* scale, float* shift,
                          int32_t N, void* stream);

/* ---- classes of identical fake rows ------------------------------------------------------------------------
 * Inside the coarse-to-fine stack every descendant of a fake vertex is fake, isolated and produced by the same per-row
 * arithmetic from the same un-pooled value (meshnet.py:71-78: both children copy the parent): in the tree order the
 * descendants of one fake vertex at a finer level are an aligned run of 2^j bitwise IDENTICAL rows.  The caller, who
 * knows how many un-pool steps lie above a level, declares these runs with rep_of[V] (host array: the first row of the
 * run for its members, v itself for everything else).  Afterwards the handle's fake row sets (2 and 4) list only the
 * representatives, the other members ("holes") are never written nor read:
 *   forward   BatchNorm statistics count a representative once per member (the `stats` of p2m_gemm_planes_rows, or
 *             p2m_stats_rows_w over a finished tensor; then p2m_bn_finalize_split);
 *             p2m_cheb_combine_small (the final conv) fills the holes of its OUTPUT with the representative's value;
 *   backward  a representative carries the SUM of its class's gradients -- everything downstream (BatchNorm backward,
 *             contractions, pair-sums, the weight gradient) is linear in it; p2m_class_reduce forms that sum from the
 *             incoming gradient, the BatchNorm-backward passes take the handle (`classes`) to skip holes and to add
 *             the constant term once per member.
 * Results are those of the full computation (fp32 round-off class: the statistics' summation order changes).       */
int p2m_graph_fake_ids(p2m_graph_t g, int32_t* out /* host, n_fake entries */);
/* The REAL (non-padding) vertices of the level in COMPACT ROW ORDER: row i of every compact plane ([B * n_real, F]:
 * p2m_cheb_basis_fwd_real, the planes out of p2m_cheb_tile_gemm, planes_compact of p2m_gemm_planes_rows / p2m_gemm_tn_rows)
 * belongs to vertex out[i].  A permutation of the real vertex ids - since round 5 a LOCALITY order (greedy patches over the
 * level's graph, so that the 32-row tiles of the tile plans have small neighbourhood unions), not the ascending one;
 * P2M_TILE_ORDER=tree (environment, read once) keeps the ascending coarsening-tree order.  out: [n_real] int32, host.  */
int p2m_graph_real_ids(p2m_graph_t g, int32_t* out);
int p2m_graph_set_classes(p2m_graph_t g, const int32_t* rep_of /* host, V entries */);
int p2m_graph_class_info(p2m_graph_t g, int32_t counts[3] /* has classes, representatives, all fake vertices */);
/* weighted BatchNorm partials of the representatives of y [B*V, N]: stats [B * ceil(n_rep/128)][2][N] */
int p2m_stats_rows_w(p2m_graph_t g, const float* y, int32_t B, int32_t N, float* stats, void* stream);
/* out[r] = sum of in over the class of r (representatives), in[r] (real vertices), 0 (holes); in, out: [B*V, F] */
int p2m_class_reduce(p2m_graph_t g, const float* in, float* out, int32_t B, int32_t F, void* stream);

/* ---- composite: one Chebyshev graph convolution (cheby_graph_conv.py:5-40, K=3) ------------
 * Y = [X|L X|L2 X] Wt + bias, BatchNorm partials in `stats` (may be NULL).  T1/T2 are caller
 * workspaces of B*V*Fin floats each and hold the basis planes afterwards (saved for backward).
 * Convenience entry: native f32 MFMA arithmetic, unsplit rows; the network path composes the pieces itself
 * (p2m_cheb_basis_fwd_real + p2m_weight_split + p2m_gemm_planes_rows).                                  */
int p2m_chebconv_fwd(p2m_graph_t g, const float* X, const float* Wt, const float* bias,
                     float* T1, float* T2, float* Y, float* stats,
                     int32_t B, int32_t Fin, int32_t Fout, int32_t in_shift, void* stream);

/* ---- mesh losses of the train step, value AND gradient (lib/core/base.py:130-143, lib/core/loss.py) --------
 * losses[0..3] = L1(pred_mesh, gt_mesh)*w_vertex, normal-vector loss*w_normal, edge-length loss*w_edge,
 * L1(J_regressor @ (pred_mesh*1000), gt_pose)*w_joint, where pred_mesh[b, v] = cam_mesh[b, perm[v]] (the
 * perm-reverse gather of base.py:130).  grad_cam (optional) receives d(sum of the four)/d cam_mesh, [B, V0, 3],
 * zero on fake vertices.  faces: [F,3] int32; vf_ptr/vf_idx: CSR vertex -> (face*3 + corner).  The joint regressor
 * (dense [J, nv] in the reference, 107 non-zeros of 117 130 for h36m) is passed sparse, by joint (jr_*: CSR, used for
 * the regression) and by vertex (vj_*: CSC, used for the gradient).  valid_mesh: [B, nv] or NULL, valid_pose: [B, J]
 * or NULL (the reference's masks are [B, nv, 1] / [B, J, 1], data/Human36M/dataset.py:392-394).  A weight of 0
 * switches the term AND its gradient off (the reference does not evaluate the edge loss before
 * cfg.TRAIN.edge_loss_start, base.py:141-143).  workspace: p2m_mesh_loss_workspace(...) floats.                */
int64_t p2m_mesh_loss_workspace(int32_t B, int32_t nv, int32_t F, int32_t J);
int p2m_mesh_loss(const float* cam_mesh, int32_t V0, const int32_t* perm, int32_t nv, const float* gt_mesh,
                  const float* valid_mesh, const int32_t* faces, int32_t F, const int32_t* vf_ptr,
                  const int32_t* vf_idx, const int32_t* jr_ptr, const int32_t* jr_idx, const float* jr_val,
                  const int32_t* vj_ptr, const int32_t* vj_idx, const float* vj_val, int32_t J,
                  const float* gt_pose, const float* valid_pose, float w_vertex, float w_normal, float w_edge,
                  float w_joint, float* workspace, float* losses, float* grad_cam, int32_t B, void* stream);

/* CoordLoss of a small tensor (lib/core/loss.py:10-23; the lifted-pose term of lib/core/base.py:128,139), value and gradient
 * in one launch:  loss[0] = w * mean |pred * valid - target * valid|,  grad[i] = w * sign(..) * valid / n   (grad optional).
 * valid (optional): one mask value per `per_mask` consecutive elements (per_mask = 3: the reference's [B, J, 1] masks).   */
int p2m_coord_loss(const float* pred, const float* target, const float* valid, int32_t per_mask, int64_t n, float w,
                   float* loss, float* grad, void* stream);

/* ---- test-step / demo epilogue (lib/core/base.py:200-204, demo/run.py:169-171) -------------------------------
 * mesh[b, i] = scale * cam_mesh[b, perm[i]], i < nv  (tree order incl. fake vertices -> mesh-model vertex order;
 * scale = 1000 in the Tester, 1 in the demo);  joints[b, j] = sum_k jr_val[k] * mesh[b, jr_idx[k]] over CSR row j.
 * mesh: [B, nv, 3] or NULL; joints: [B, J, 3] or NULL.                                                          */
int p2m_mesh_epilogue(const float* cam_mesh, int32_t V0, const int32_t* perm, int32_t nv, float scale,
                      const int32_t* jr_ptr, const int32_t* jr_idx, const float* jr_val, int32_t J,
                      float* mesh, float* joints, int32_t B, void* stream);

/* ---- evaluation (lib/coord_utils.py:127-149, data/PW3D/dataset.py:273-286,322-375, data/Human36M/dataset.py:514-572) ----
 * Batched similarity (Procrustes) alignment, rigid_transform_3D / rigid_align (coord_utils.py:127-149): for each of nb
 * pairs of point sets A, B [N, 3] (N >= 1): cA, cB centroids, H = (A - cA)^T (B - cB) / N, R the proper rotation
 * maximising tr(R H) (the reference's SVD with its det < 0 fix), c = (s1 + s2 +- s3) / varP (varP: population variance of
 * A summed over the axes), t = cB - c R cA, and optionally A2 = c R A + t.  Out: c [nb], R [nb, 3, 3] (row-major,
 * A2 = c R a + t), t [nb, 3], A2 [nb, N, 3] or NULL.  Centroids, H and varP are accumulated in fp64 and the 3x3 solve
 * runs in fp64.  varP == 0 (all points of a set coincide): that set's c, t and A2 are non-finite, as in the reference.
 * One wave per set for N <= 256, one block per set above.                                                            */
int p2m_rigid_align(const float* A, const float* B, int32_t nb, int32_t N, float* c, float* R, float* t, float* A2,
                    void* stream);
/* The Tester's / dataset.evaluate()'s per-sample metrics of a batch, one block per sample, one launch:
 *   stage A  JA = RA @ pred (CSR ra_*, JA <= 64 joints) or pred_joints_A [B, JA, 3]; the ground truth's joints are
 *            gt_joints_A [B, JA, 3] or RA @ gt (given joints are used as given: compute_both_err's pred_joint and
 *            reg_pose3d; ra_* may be NULL when both are given).  Both meshes and both joint sets are centred on their own joint
 *            root_A.  mpjpe_A [B, nsub_A] = per-joint L2 over the subset sub_A (NULL: all JA joints, nsub_A ignored),
 *            mpvpe [B] = mean per-vertex L2                              (dataset.py:273-286; PW3D 339-352, H36M 535-545)
 *   stage E  (JE > 0) JE = RE @ (A-centred mesh); the ground truth is gt_joints_E [B, JE, 3] (the annotation's joint_cam,
 *            used as given) or RE @ (A-centred gt), both re-centred on root_E and cut to sub_E.  mpjpe_E, pa_mpjpe_E
 *            [B, nsub_E]: per-joint L2 before / after p2m_rigid_align's alignment of prediction onto ground truth
 *                                                                        (PW3D 363-372, H36M 558-567)
 *   pa_mesh  the A-centred prediction mesh aligned onto the A-centred ground truth mesh: pa_mpvpe [B] = mean per-vertex L2
 *            (FreiHAND's PA-MPVPE; PW3D 360-361, commented out there)
 * pred_mesh, gt_mesh [B, nv, 3] in mesh-model order; gt_mesh is read as gt_mesh * gt_mesh_scale (the Tester's x 1000,
 * base.py:201).  Rows b >= B_real are padding: never read, their outputs written as 0.  Accumulation in fp64, fixed
 * reduction orders, no atomics: bitwise reproducible; no allocation or synchronisation (capturable).
 * sample_means [B, 5] (fp64, optional): the per-sample means of mpjpe_E, pa_mpjpe_E, mpjpe_A, mpvpe, pa_mpvpe.
 * totals (fp64, optional; needs sample_means): [n_groups + 1][6] running sums, ADDED to by a one-block launch behind the
 * evaluation in sample order: row 0 all samples, row 1 + g the samples with group[b] == g (group: [B] int32 or NULL;
 * ids outside [0, n_groups) count in row 0 only); column 0 the sample count, 1..5 the sums of the five means.           */
int p2m_mesh_eval(const float* pred_mesh, const float* gt_mesh, int32_t B, int32_t B_real, int32_t nv, float gt_mesh_scale,
                  const int32_t* ra_ptr, const int32_t* ra_idx, const float* ra_val, int32_t JA, int32_t root_A,
                  const int32_t* sub_A, int32_t nsub_A, const float* pred_joints_A, const float* gt_joints_A,
                  const int32_t* re_ptr, const int32_t* re_idx, const float* re_val, int32_t JE, int32_t root_E, const int32_t* sub_E,
                  int32_t nsub_E, const float* gt_joints_E, int32_t pa_mesh, float* mpjpe_A, float* mpvpe, float* mpjpe_E,
                  float* pa_mpjpe_E, float* pa_mpvpe, double* sample_means, const int32_t* group, int32_t n_groups,
                  double* totals, void* stream);

/* ---- F-scores: batched nearest-vertex distances (csrc/fscore.hip) ------------------------------------------------------
 * FreiHAND's F@th.  The reference ships no F-score code (its numbers come from the challenge server), so this comment is
 * the definition and tests/fscore_ref.py its float64 restatement.  Per sample, with P the prediction and G the ground
 * truth (G read as gt_mesh * gt_mesh_scale), both [nv, 3] after the variant's transform:
 *   d_pred[i] = min_j |P_i - G_j|,  d_gt[j] = min_i |G_j - P_i|      (Euclidean; the index correspondence is not used)
 *   near_pred = #{i: d_pred[i] < th} / nv,  near_gt = #{j: d_gt[j] < th} / nv                      (strict comparison)
 *   F = 2 near_pred near_gt / (near_pred + near_gt), 0 when the sum is 0
 * Variants (variants: bit 0 centred, bit 1 aligned; at least one):
 *   centred  each mesh minus its own centre point: row `root` of the CSR regressor r_* (J rows) applied to that mesh (fp64),
 *            or pred_centre / gt_centre [B, 3] (used as given; both or neither), or nothing (all NULL)
 *   aligned  the centred prediction similarity-aligned onto the centred ground truth over all vertices: exactly
 *            p2m_mesh_eval's pa_mesh transform (fp64), the published FreiHAND numbers
 * A prepare launch writes the sets fp32 and coordinate-major into the workspace, about one per-sample origin (the centred
 * ground truth's centroid) subtracted in fp64 before the rounding; the search takes min (px-qx)^2 + (py-qy)^2 + (pz-qz)^2
 * in fp32 over LDS tiles of targets and sqrtf at the end: with M the largest |coordinate| of a sample's staged sets and
 * u = 2^-24, a distance is within (2 sqrt(3) M + 6 d) u of the exact one.  A third launch adds the per-block integer
 * counts in a fixed order and computes near_* and F in fp64.  No float atomics, no allocation, no synchronisation
 * (capturable); bitwise reproducible, and a sample's results do not depend on the batch around it.
 *   thresholds   HOST array of 1..4 positive finite values (read before the launch, passed by value)
 *   workspace    p2m_nn_workspace(B, nv, nv) bytes of device memory, 16-byte aligned
 *   d_pred, d_gt, pa_d_pred, pa_d_gt   [B, nv] or NULL (a variant that is off is never written)
 *   counts       [B][nvar][2][n_thresholds] int32 or NULL: direction 0 counts d_pred, 1 counts d_gt; nvar = variants
 *                present, centred first
 *   scores       [B][nvar][3][n_thresholds] fp64 or NULL: near_pred, near_gt, F
 *   totals       (optional; needs scores) [n_groups + 1][1 + nvar * 3 * n_thresholds] fp64 running sums, ADDED to in sample
 *                order: row 0 all samples, row 1 + g the samples with group[b] == g (ids outside [0, n_groups) count in row 0
 *                only); column 0 the sample count, then the sums of the scores in their layout
 * Rows b >= B_real are padding: never read, every output of theirs written as 0, not counted.
 * p2m_point_nn: the bare two-way search between nb pairs of point sets A [nb, nA, 3], B [nb, nB, 3] (nA != nB allowed): dAB
 * [nb, nA] = distance of each point of A to the nearest of B, dBA [nb, nB] the other way (one of them may be NULL).  No
 * transform; the sets are still staged about a per-pair origin (the centroid of B).  Workspace: p2m_nn_workspace(nb, nA, nB).
 * p2m_nn_target_tile: targets per LDS tile; p2m_nn_query_tile(n): queries per block for sets of at most n points (the
 * search picks the queries per lane by the larger set of the call); tests walk the edges of both.
 * Errors (P2M_ERR_INVALID, nothing launched): NULL required pointers, nv < 1, n_thresholds outside 1..4, a non-positive or
 * non-finite threshold, B * nv * 3 >= 2^31, a workspace that is too small or misaligned.                                 */
int32_t p2m_nn_target_tile(void);
int32_t p2m_nn_query_tile(int32_t n);
int64_t p2m_nn_workspace(int32_t B, int32_t nA, int32_t nB);
int p2m_mesh_fscore(const float* pred_mesh, const float* gt_mesh, int32_t B, int32_t B_real, int32_t nv, float gt_mesh_scale,
                    const int32_t* r_ptr, const int32_t* r_idx, const float* r_val, int32_t J, int32_t root,
                    const float* pred_centre, const float* gt_centre, int32_t variants, const float* thresholds,
                    int32_t n_thresholds, void* workspace, int64_t workspace_bytes, float* d_pred, float* d_gt,
                    float* pa_d_pred, float* pa_d_gt, int32_t* counts, double* scores, const int32_t* group, int32_t n_groups,
                    double* totals, void* stream);
int p2m_point_nn(const float* A, const float* B, int32_t nb, int32_t nA, int32_t nB, float* dAB, float* dBA, void* workspace,
                 int64_t workspace_bytes, void* stream);

/* ---- error profiles: per-point errors, PCK histograms, running per-group and per-point totals (csrc/profile.hip) ---------
 * What PCK curves, their AUC (FreiHAND's other two columns), PCK at a cut-off (MPI-INF-3DHP's PCK@150 mm), per-joint error
 * tables and a dataset-mean per-vertex error map are derived from.  Neither the reference nor the FreiHAND server code is
 * in this tree: this comment is the definition and tests/profile_ref.py its float64 restatement.
 * pred, gt [B, N, 3] fp32, corresponding points; gt is read as gt * gt_scale (the product of two fp32 values, exact in
 * fp64).  valid [B, N] uint8 or NULL: a point with valid == 0 is not counted (its error is written as 0, its coordinates
 * are never read).  thresholds: DEVICE array t[0 .. K-1] of fp64, finite and ascending, 2 <= K <= 256; the caller uploads it
 * from the host, so a table such as linspace(lo, hi, steps) arrives bit for bit (the order is the caller's contract: it is
 * not checked on the device, and whatever the table holds every bin stays inside [0, K]).
 * Per sample b < B_real, all in fp64:
 *   1. root >= 0: both sets minus their own point `root` (root == -1: as they are)
 *   2. align != 0: the prediction is similarity-aligned onto the ground truth over the counted points: centroids cP, cG,
 *      H = sum (p - cP)(g - cG)^T / n, varP = sum |p - cP|^2 / n, the solve of p2m_rigid_align / p2m_mesh_eval's pa_mesh;
 *      p <- c R p + t.  All counted points of the prediction coincide: c is non-finite and so is every error of the sample
 *   3. e_i = sqrt(dx dx + dy dy + dz dz), d = p_i - g_i: three products and two sums, left to right, no fma contraction
 *   4. bin_i = the number of thresholds < e_i, i.e. the first k with e_i <= t[k], and K if there is none (non-strict, unlike
 *      the F-score's comparison).  A non-finite e_i goes to bin K
 *   error [B, N] = e (0 where not counted), sample_pck [B, K + 1] int32 = the points of the sample per bin,
 *   sample_mean [B] = the sum of e over the counted points / their number (NaN when there is none), the sum taken in a fixed
 *   order: lane l of 256 adds its points l, l + 256, ... in ascending order (a point that is not counted adds 0), the 64 lanes
 *   of a wave are added by the xor butterfly 32, 16, 8, 4, 2, 1, then the four wave totals in wave order.
 * Running totals, ADDED to by launches behind the per-sample one, in sample order, starting from the value found there (so two
 * calls over 4 and 5 samples leave bitwise the state of one call over the 9):
 *   group_sum [n_groups + 1] fp64, group_count [n_groups + 1] int64, group_hist [n_groups + 1][K + 1] int64 (all three or
 *     none): row 0 all samples, row 1 + g the samples with group[b] == g (group: [B] int32 or NULL; ids outside [0, n_groups)
 *     count in row 0 only): the per-sample sums, the points counted, the bins
 *   point_sum [N] fp64, point_count [N] int64, point_hist [N][K + 1] int64 (all three or none): over all samples, per point:
 *     its errors, the samples that count it, its bins
 * Integer sums only in the histograms (LDS integer atomics per sample); no float atomics, no allocation, no synchronisation
 * (capturable); bitwise reproducible.  Rows b >= B_real are padding: never read, their outputs written as 0, not counted.
 * workspace: p2m_error_profile_workspace(B, N) bytes of device memory, 16-byte aligned (-1 for B < 0 or N < 1).
 * Errors (P2M_ERR_INVALID, nothing launched): NULL required pointers, N < 1, B_real outside [0, B], K outside 2..256, root
 * outside [-1, N), B * N * 3 >= 2^31, incomplete totals, n_groups outside 0..65535, a workspace too small or misaligned.    */
int64_t p2m_error_profile_workspace(int32_t B, int32_t N);
int p2m_error_profile(const float* pred, const float* gt, const uint8_t* valid, int32_t B, int32_t B_real, int32_t N,
                      float gt_scale, int32_t root, int32_t align, const double* thresholds, int32_t K, void* workspace,
                      int64_t workspace_bytes, double* error, double* sample_mean, int32_t* sample_pck, const int32_t* group,
                      int32_t n_groups, double* group_sum, int64_t* group_count, int64_t* group_hist, double* point_sum,
                      int64_t* point_count, int64_t* point_hist, void* stream);

/* ---- PoseNet, the 2D -> 3D lifter in front of MeshNet (lib/models/posenet.py:11-92) ---------------------------------
 * A 4096-wide residual MLP over B rows.  Every Linear (posenet.py:19,22,59,68: F.linear and its autograd) is a
 * weight-streaming contraction at these batch sizes and runs on p2m_gemm_tn, the reduction-split contraction with both
 * operands row-major over the reduction index:
 *   forward  z = a W^T + b      P[ch][m][n] = sum_{k in ch} a^T[k][m] * W^T[k][n]      (A = a^T, G = p2m_weight_pack(W, K = 1))
 *   dX       g_a = g_z W        P[ch][m][k] = sum_{n in ch} g_z^T[n][m] * W[n][k]      (A = g_z^T, G = W as nn.Linear stores it)
 *   dW       W.grad += g_z^T a  p2m_gemm_tn_acc: the whole reduction (the B rows) in one chunk, added straight into .grad
 * p2m_gemm_tn_acc: P[k][n] += sum_{r < M} A[r][k] * G[r][n]   (A: [M, Ka], G: [M, N], P: [Ka, N]; same arithmetics).  */
int p2m_gemm_tn_acc(const float* A, int32_t Ka, const float* G, int32_t N, int64_t M, float* P, int32_t arith,
                    const void* a_amax, const void* g_amax, void* stream);
/* The elementwise stage between two contractions, forward (posenet.py:28-38,79-87).  A block owns 32 columns and ALL B
 * rows of them, so BatchNorm1d's batch statistics are block-local and the whole stage is one launch:
 *   z = sum_{ch < nch} P[ch] + bias (+ resid)                       written to z (z == NULL: P is the tensor itself)
 *   has_bn: a = dropout(relu(batch_norm(z)));  else a = z           written row-major to a and / or TRANSPOSED to aT [F, B]
 * batch_norm: training != 0 -> batch mean / biased variance over the B rows, running statistics updated with `momentum`
 * and the unbiased variance (nn.BatchNorm1d); else the running statistics.  mean / invstd receive the statistics used
 * (saved for the backward).  dropout: rnd = uniform [0, 1) numbers drawn by the caller, keep where rnd >= p_drop, scale
 * 1 / (1 - p_drop) (nn.Dropout); rnd == NULL or p_drop == 0: identity.  amax_out: atomic max of |a| (P2M_ARITH_F16X2).
 * B_real (round 6; 0 = B): the first B_real of the B rows hold samples, the rest are PADDING - the contractions want
 * B >= 32 and B % 4 == 0, so the caller zero-pads any other batch (B = 1 of demo/run.py:160 included).  Padding rows are
 * left out of the batch statistics (mean, variance and the unbiased-variance factor use B_real) and their a / aT values
 * are stored as 0, so they stay exactly zero through every Linear; in the backward their gradient is 0 in and 0 out. */
int p2m_pn_stage_fwd(const float* P, int32_t nch, const float* bias, const float* resid, float* z, int32_t has_bn,
                     int32_t training, const float* gamma, const float* beta, float* running_mean, float* running_var,
                     float momentum, float eps, const float* rnd, float p_drop, float* a, float* aT, float* mean,
                     float* invstd, void* amax_out, int32_t B, int32_t F, int32_t B_real, void* stream);
/* ... and backward (autograd of the same lines): g_a = sum_{ch < nch} P[ch] is the gradient w.r.t. the stage's output a;
 *   has_bn: g_u = g_a * dropout mask * [batch_norm(z) > 0];  dbeta = sum_r g_u;  dgamma = sum_r g_u xhat;
 *           g_z = gamma invstd (g_u - dbeta / B - xhat dgamma / B)  (training)   /   gamma invstd g_u  (running statistics)
 *   else    g_z = g_a;
 *   g_z += addend (the residual branch's gradient, posenet.py:38);  stored row-major (gz) and transposed (gzT, [F, B]);
 *   dbias = sum_r g_z: the bias gradient of the Linear that produced z.  accumulate != 0: dgamma / dbeta / dbias are
 *   added into (the parameters' .grad), else overwritten.  z, mean, invstd: what the forward saved.                  */
int p2m_pn_stage_bwd(const float* P, int32_t nch, const float* addend, int32_t has_bn, int32_t training, const float* z,
                     const float* mean, const float* invstd, const float* gamma, const float* beta, const float* rnd,
                     float p_drop, float* gz, float* gzT, float* dgamma, float* dbeta, float* dbias, int32_t accumulate,
                     void* amax_out, int32_t B, int32_t F, int32_t B_real, void* stream);

/* ---- optimizer step over a flat fp32 buffer ------------------------------------------------
 * torch.optim.Adam semantics (lib/funcs_utils.py:92-96, stepped at lib/core/base.py:148): one fused
 * launch for the whole model.  grad is multiplied by grad_scale first (1/world_size after a
 * sum all-reduce).  step counts from 1.                                                         */
int p2m_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  int64_t step, float lr, float beta1, float beta2, float eps, float grad_scale,
                  void* stream);

/* torch.optim.RMSprop semantics with the defaults the reference's yaml recipes use (lib/funcs_utils.py:87-91,
 * the asset/yaml recipes, `optimizer: 'rmsprop'`: alpha 0.99, eps 1e-8, no momentum, not centered):
 *   v = alpha v + (1-alpha) g^2;  p -= lr g / (sqrt(v) + eps),  g = grad * grad_scale.                              */
int p2m_rmsprop_step(float* param, const float* grad, float* square_avg, int64_t n, float lr, float alpha,
                     float eps, float grad_scale, void* stream);
/* The same two steps with the step-dependent scalars in DEVICE memory, hp = {lr, 1 - beta1^t, sqrt(1 - beta2^t),
 * grad_scale} (RMSprop reads hp[0] and hp[3]): the launches are then identical from step to step and can be part of a
 * captured hipGraph (train.GraphedTrainStep); the host refreshes hp before each replay.                            */
int p2m_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* hp,
                      float beta1, float beta2, float eps, void* stream);
int p2m_rmsprop_step_dev(float* param, const float* grad, float* square_avg, int64_t n, const float* hp, float alpha,
                         float eps, void* stream);

/* ---- body-model layer: batched SMPL / MANO forward (csrc/body.hip) ----------------------------------------------------
 * The forward of smplpytorch's SMPL_Layer (smpl_layer.py:65-158) and manopth's ManoLayer (manolayer.py:109-273, use_pca =
 * False, axis-angle root) for a batch, all in device memory: batch_rodrigues through the quaternion (with its + 1e-8),
 * v_posed = template + shapedirs beta + posedirs (R_j - I)_{j >= 1}, rest joints, the kinematic chain over `parents`, dense
 * linear blend skinning, then + trans or - centre joint, times scale.  fp32 FMA in fixed orders, no atomics: a sample's
 * result does not depend on the batch it is in.  Three launches on `stream`; nothing allocates or synchronises.
 *   pose [B, 3 J] axis-angle; pose_mean [3 J] added to every row (MANO: zeros for the root, then hands_mean) or NULL;
 *   betas [B, nb] (betas_per_sample != 0) or one [nb] row for all samples; trans [B, 3], or NULL: then chain joint
 *   center_joint (>= 0) is subtracted from vertices and joints.
 *   v_template [3 V]; dirs [nb + 9 (J - 1)][3 V]: shapedirs then posedirs, coefficient-major; weights_t [J][V];
 *   joint_template [J, 3] = J_regressor . template and joint_shapedirs [J, 3, nb] = J_regressor . shapedirs (folded on the
 *   host); parents [J] with parents[j] < j for j >= 1 (the CALLER validates: the table is device memory).
 *   joints [B, n_joints_out, 3]: chain joint j goes to slot joint_slot[j] (-1: dropped), vertex tip_vert[t] of the result
 *   to slot tip_slot[t] (ManoLayer's finger tips; the caller validates the indices).
 *   extra [B, n_extra, 3] = regressor @ verts for a CSR regressor (xr_ptr / xr_idx / xr_val, fp64 accumulation), n_extra = 0: none.
 *   workspace: p2m_body_workspace(B, J, nb) bytes, 16-byte aligned.
 * Limits: 1 <= J <= 64, nb + 9 (J - 1) <= 640, n_tips, n_extra <= 64, every buffer 4-byte aligned.
 * p2m_body_sample_tile / p2m_body_vertex_tile: samples / vertices per block of the skinning kernel (tests walk their edges). */
int32_t p2m_body_sample_tile(void);
int32_t p2m_body_vertex_tile(void);
int64_t p2m_body_workspace(int32_t B, int32_t J, int32_t nb);
int p2m_body_forward(const float* pose, const float* pose_mean, const float* betas, int32_t betas_per_sample,
                     const float* trans, int32_t center_joint, float scale, int32_t B, int32_t V, int32_t J, int32_t nb,
                     const float* v_template, const float* dirs, const float* weights_t, const float* joint_template,
                     const float* joint_shapedirs, const int32_t* parents, const int32_t* joint_slot, int32_t n_joints_out,
                     const int32_t* tip_vert, const int32_t* tip_slot, int32_t n_tips, const int32_t* xr_ptr,
                     const int32_t* xr_idx, const float* xr_val, int32_t n_extra, void* workspace, int64_t workspace_bytes,
                     float* verts, float* joints, float* extra, void* stream);

/* ---- body-model layer: backward (csrc/body_bwd.hip) --------------------------------------------------------------------------
 * Gradients of a scalar loss with respect to pose, betas and trans of ONE p2m_body_forward call, from its gradients with
 * respect to verts, joints and extra.  The caller passes the inputs and tables of that call again and the forward workspace
 * as that call left it (fwd_workspace: coefficient rows, skinning matrices, offsets; read only) - nothing else is kept
 * between the two.  has_trans != 0: the forward was given trans (then center_joint is ignored, as there).
 *   g_verts [B, V, 3], g_joints [B, n_joints_out, 3], g_extra [B, n_extra, 3]: contiguous, each may be NULL (no gradient
 *   arrives through that output; no zeros are read), at least one is not.
 *   g_pose [B, 3 J], g_betas [B, nb], g_trans [B, 3]: written (not accumulated); each may be NULL (not wanted, its work is
 *   skipped), at least one is not.  g_betas needs betas_per_sample != 0, g_trans needs has_trans != 0.
 *   dirs_t [3 V][Kp], Kp = nb + 9 (J - 1) rounded up to a multiple of 4: the direction table vertex-major (row g = entry g
 *   of every coefficient, zero padded); needed for g_pose / g_betas, else it may be NULL.
 *   xc_ptr [V + 1] / xc_idx / xc_val: the extra regressor by COLUMN (CSC: the entries of vertex v, joints ascending);
 *   needed when g_extra is given.
 *   workspace: p2m_body_backward_workspace(B, V, J, nb) bytes, 16-byte aligned: per-block partial sums
 *   [ceil(V / 64)][B] x (12 (J + 1) doubles + Kp floats), written and read once.
 * Two launches on `stream`; nothing allocates or synchronises.  No atomics: the vertex stage reduces each 64-vertex tile in a
 * fixed order (float64 inside the tile for the skinning-matrix and offset sums), the pose stage folds the tiles in tile order
 * and runs the chain and batch_rodrigues' derivative (its + 1e-8 included, no special case at a zero rotation) in float64.
 * A sample's gradient is bitwise the same in any batch.  Limits and alignment as p2m_body_forward. */
int64_t p2m_body_backward_workspace(int32_t B, int32_t V, int32_t J, int32_t nb);
int p2m_body_backward(const float* pose, const float* pose_mean, const float* betas, int32_t betas_per_sample,
                      int32_t has_trans, int32_t center_joint, float scale, int32_t B, int32_t V, int32_t J, int32_t nb,
                      const float* v_template, const float* dirs, const float* dirs_t, const float* weights_t,
                      const float* joint_template, const float* joint_shapedirs, const int32_t* parents,
                      const int32_t* joint_slot, int32_t n_joints_out, const int32_t* tip_vert, const int32_t* tip_slot,
                      int32_t n_tips, const int32_t* xc_ptr, const int32_t* xc_idx, const float* xc_val, int32_t n_extra,
                      const void* fwd_workspace, int64_t fwd_workspace_bytes, const float* g_verts, const float* g_joints,
                      const float* g_extra, void* workspace, int64_t workspace_bytes, float* g_pose, float* g_betas,
                      float* g_trans, void* stream);

/* ---- training-sample noise: synthetic 2D detector errors (csrc/sample.hip, csrc/p2m_philox.h) ---------------------------
 * Every released recipe of the reference trains on noisy 2D input (use_gt_input: False): the dataset replaces the clean
 * projected joints by synthetic detector errors on a dataloader worker (data/AMASS/dataset.py:311-330 and its siblings).
 * These two entry points draw that noise on the device.  No allocation, no host synchronisation (capturable).
 *
 * Random numbers: ONE counter-based stream, Philox4x32-10 (multipliers D2511F53 / CD9E8D57, Weyl constants 9E3779B9 /
 * BB67AE85).  key = the 64-bit seed; counter words 0, 1 = the 64-bit GLOBAL sample index first_index + b, word 2 =
 * joint | stage << 8, word 3 = the draw-block index.  So a sample's result depends on (seed, its global index) alone, never
 * on the batch it sits in.  state: two uint64 words in DEVICE memory {seed, first_index} - a captured graph replays with
 * fresh numbers once the caller has advanced state[1] by B with an ordinary (captured) tensor add.
 * A uniform is (word >> 8) * 2^-24: exact in fp32 and fp64.  A candidate point is (angle, radius) = two uniforms; one draw
 * block holds two candidates: candidate c of a stage is block c >> 1, words 0, 1 (angle, radius) for even c, words 2, 3 for
 * odd c.  Normals are Box-Muller on (1 - u0, u1): sqrt(-2 ln(1 - u0)) (cos, sin)(2 pi u1).  Stages:
 *   0 jitter      500 candidates, radius in [ks_85, ks_50] around the joint itself
 *   1 miss count, source 0 (the joint itself)   2000 candidates, radius in [ks_50, ks_10]
 *   2 miss count, source 1 (the partner)        2000 candidates, likewise
 *   3 miss point, source 0     4 miss point, source 1    up to 2000 candidates each, likewise
 *   5 inversion   500 candidates, radius in [0, ks_50] around the partner
 *   6 good        125 candidates, radius in [0, ks_85] around the joint itself
 *   7 select      block 0: word 0 the miss-source uniform, word 1 the category uniform
 *   8 table       block 0: word 0 the Bernoulli uniform, words 1, 2 the Box-Muller pair (u0, u1)
 *   9 augment     joint 0, block 0: word 0 flip, words 1, 2 the rotation's Box-Muller pair, word 3 rot = 0 (p2m_train_sample)
 *  10 camera start   joint 0, block 0: words 0, 1, 2 the start (s, tx, ty) of the camera fit (p2m_camera_fit)
 *  11 person colour  joint 0, block 0: word 0 the hue of a person's colour (p2m_person_colours)
 * with ks_q = sqrt(area) 2 sigma_j sqrt(-2 ln q) (get_dist_wrt_ks, lib/noise_utils.py:18-24; a negative or NaN area counts
 * as 0).  tests/sample_ref.py mirrors all of this in numpy, float64.
 *
 * p2m_pose_noise_coco: the distribution of synthesize_pose(joints, area, num_overlap = 0) (lib/noise_utils.py:17-285).
 *   joints [B, 17, 3] (x, y, valid), area [B], sigmas [17] (the COCO OKS sigmas / 10), out [B, 17, 3] (x, y, 1 - or all 0 when
 *   no error type was available), kind [B, 17] int8 or NULL: 0 jitter, 1 miss, 2 inversion, 4 good, -1 joint zeroed.
 *   EVERY joint is synthesised, valid or not (the reference loops over all 17); validity enters through num_valid_joint
 *   (the probability tables :70-83, :105-125, :161-166) and through the partner.  Facts of the reference that are kept:
 *   near_joints has no valid entry and swap_exist is False (:14, :189, :231), so a joint's candidate sources are its own
 *   position and, when its left / right partner's ORIGINAL validity is > 0, the partner's CURRENT coordinates: the loop
 *   updates synth_joints in place, so the higher joint of a pair (2, 4, .., 16) sees the already synthesised lower one, (0, 0)
 *   if that was zeroed.  Nine independent units per sample - the nose and eight pairs of two sequential steps -, one wave each.
 *   Sampling scheme - EQUAL IN DISTRIBUTION to the reference, but restated, and defined here:
 *     jitter / inversion / good   the reference draws N iid candidates and picks uniformly among those passing the distance
 *                  mask (distance to the other source > r).  That has the distribution of the FIRST passing candidate of
 *                  the sequence, and the type is unavailable if none of the N passes.  64 lanes evaluate 128 candidates a
 *                  step and the first ballot hit ends the stage.  Without a second source candidate 0 is taken.
 *     miss         n_s = passing candidates among 2000 of source s (mask: distance to the OTHER source > ks_50).  The pool
 *                  of :143-151 is n_0 points of source 0 plus n_1 / 4 (integer) of source 1: the source is chosen by
 *                  (word >> 8) (n_0 + n_1 / 4) < n_0 2^24 (exact integers), the point is the first passing candidate of
 *                  that source's SEPARATE point stage, so it does not depend on the counts; unavailable when the pool is
 *                  empty (or when none of the point stage's 2000 candidates passes).  Sources further apart than
 *                  (ks_10 + ks_50) (1 + 2^-10) cannot fail each other's mask: then n_0 = n_1 = 2000 without counting.
 *     category     availability zeroing and renormalisation of :256-276, then the category uniform times the sum of the
 *                  available weights against their running sums in the order [jitter, miss, inversion, good] (swap = 0).
 *   fp32; angles through sincospif(2 u) (accurate, not the fast intrinsics: the robustness band of tests/sample_ref.py is
 *   derived from this operation sequence).  out must not overlap joints.
 *
 * p2m_pose_noise_table: generate_syn_error and its use (data/AMASS/dataset.py:77-89, 327-329) for any joint set:
 *   out[b, j, :] = pose[b, j, :] + [weight_j > u] (mean_j + std_j n) / 256 * (W, H),  n two normals per (sample, joint).
 *   pose, out [B, J, 2] (out may alias pose); mean, std [J, 2]; weight [J]; 1 <= J <= 32.  The reference's own table
 *   (lib/noise_stats.py) is not part of this project: callers load it from their checkout.
 * Errors (P2M_ERR_INVALID, nothing launched): NULL state or another required pointer, B < 1, J outside [1, 32], misaligned
 * buffers (state: 8 bytes), aliasing as above.                                                                            */
int p2m_pose_noise_coco(const float* joints, const float* area, const float* sigmas, const uint64_t* state, float* out,
                        int8_t* kind, int32_t B, void* stream);
int p2m_pose_noise_table(const float* pose, const float* mean, const float* std, const float* weight, int32_t J, float W,
                         float H, const uint64_t* state, float* out, int32_t B, void* stream);

/* ---- training samples: the whole chain mesh + camera -> the tensors of lib/core/base.py:124-126 (csrc/sample.hip) --------
 * What the reference's datasets do per sample in numpy on dataloader workers (data/AMASS/dataset.py:246-330; Human36M,
 * MuCo, COCO and SURREAL differ in where the joints come from), for a batch, in three launches (two without noise) on
 * `stream`; nothing allocates or synchronises.  Steps, per sample b (global index state[1] + b):
 *   joints     mesh_mm = (verts + trans) * mesh_scale in fp32 (trans NULL: 0; AMASS :205-211), joint = regressor row .
 *              mesh_mm with fp64 accumulation, rounded to fp32.  reg set: CSR rr_* [Jr, nv].  input set: CSR ir_* [Ji, nv]
 *              plus n_mid appended midpoints (a + b) / 2 (add_pelvis_and_neck; `midpoints` is a HOST array [n_mid, 2] of
 *              input-row indices), J = Ji + n_mid; ir_ptr NULL: the input set IS the reg set (J = Jr, the human36 input).
 *              The CSR tables are device memory: the CALLER validates 0 <= idx < nv and ptr ascending.
 *   given      given_reg_cam [B, Jr, 3] (mm) replaces the regressed reg joints (Human36M's annotations, data/Human36M/
 *              dataset.py:349); before that fit_err[b] = mean_j |(given_j - mean given) - (regressed_j - mean regressed)|
 *              (get_fitting_error :301-308, for a regressor whose rows sum to 1).  given_reg_img [B, Jr, 2] replaces the
 *              projected 2D joints when the input set is the reg set.  fit_thr > 0 and fit_err > fit_thr: status bit 1,
 *              mesh_valid = 0 and, when the input set is not the reg set, lift_valid = 0 (:396-400).
 *   project    cam2pixel of joint / 1000: x = (X / 1000) / (Z / 1000) * f_x + c_x (focal, princpt [B, 2]).
 *   targets    mesh = (mesh_mm - reg[reg_root]) / 1000 (metres), reg_pose3d = reg - reg[reg_root], lift = input -
 *              input[input_root] (mm) (:263-265).
 *   bbox       get_bbox (tight: min / max of the 2D input joints), process_bbox at aspect W / H (lib/coord_utils.py:21-66).
 *   affine     get_affine_transform(center, scale, rot, (W, H)) is a similarity, used in closed form: with s = W / bbox_w,
 *              (c, sn) = cos / sin of rot degrees, d = p - centre:  x' = s (c d_x + sn d_y) + W / 2,  y' = s (c d_y - sn d_x)
 *              + H / 2.  area = (s tight_w) (s tight_h): the transformed tight box's side lengths (:315-320).
 *   augment    rot [B] (degrees) and flip [B] int32, each given or NULL = drawn (augm_params, lib/aug_utils.py:98-117) from
 *              stage 9, joint 0, block 0: flip = flip_enabled and (uniform(word 0) < 0.5); rot = clip(n rot_factor,
 *              +- 2 rot_factor) with n = sqrt(-2 ln(1 - u(word 1))) cos(2 pi u(word 2)), set to 0 when u(word 3) < 0.5.
 *   noise      noise_mode P2M_SAMPLE_NOISE_COCO: p2m_pose_noise_coco's scheme on the first 17 joints in place, every joint
 *              valid (pelvis and neck keep their clean values; needs J >= 17, sigmas [17]); _TABLE: p2m_pose_noise_table's
 *              on all J joints (tab_mean, tab_std [J, 2], tab_weight [J]); _NONE.  Same stream, same stages as standalone.
 *   flip       2D: x = W - x - 1, then the pair swaps.  3D (j3d_processing, lib/aug_utils.py:67-83), LIFT TARGET ONLY:
 *              rotation by -rot about z, pair swaps, x = -x.  The mesh and the reg joints are neither rotated nor flipped:
 *              that is how the reference trains (data/AMASS/dataset.py:282-284, 301), and it is kept.
 *              flip_pairs: HOST array [n_pairs, 2], n_pairs <= 16, disjoint.
 *   normalise  pose2d / (W, H), then per sample and axis (x - mean) / std with the population std (:286-292).
 * Outputs: pose2d [B, J, 2], mesh [B, nv, 3], lift_pose3d [B, J, 3], reg_pose3d [B, Jr, 3], mesh_valid [B, nv], lift_valid
 * [B, J], reg_valid [B, Jr] (1 / 0), status [B] int32; optional (NULL: skipped) fit_err [B], kind [B, 17] int8 (coco noise;
 * not written for a sample with status bit 0), rot_flip [B, 2] (the rot and flip used).
 *   status bit 0: degenerate bbox (process_bbox would return None), non-finite 2D joints, or a zero std - the sample's
 *                 outputs are all zero and its masks 0;   bit 1: fit error over the threshold.
 * workspace: p2m_train_sample_workspace(B) bytes of device memory, 4-byte aligned.
 * Errors (P2M_ERR_INVALID, nothing launched): NULL state or required pointer, Jr or J = Ji + n_mid outside [1, 32], n_mid
 * > 4, roots / midpoints / pairs out of range, unknown noise_mode, coco noise with J < 17, W or H <= 0, small workspace. */
enum { P2M_SAMPLE_NOISE_NONE = 0, P2M_SAMPLE_NOISE_COCO = 1, P2M_SAMPLE_NOISE_TABLE = 2 };
int64_t p2m_train_sample_workspace(int32_t B);
int p2m_train_sample(const float* verts, const float* trans, float mesh_scale, const float* focal, const float* princpt,
                     int32_t B, int32_t nv, const int32_t* rr_ptr, const int32_t* rr_idx, const float* rr_val, int32_t Jr,
                     int32_t reg_root, const int32_t* ir_ptr, const int32_t* ir_idx, const float* ir_val, int32_t Ji,
                     const int32_t* midpoints, int32_t n_mid, int32_t input_root, const float* given_reg_cam,
                     const float* given_reg_img, float fit_thr, const float* rot, const int32_t* flip, float rot_factor,
                     int32_t flip_enabled, int32_t noise_mode, const float* sigmas, const float* tab_mean,
                     const float* tab_std, const float* tab_weight, const int32_t* flip_pairs, int32_t n_pairs, float W,
                     float H, const uint64_t* state, void* workspace, int64_t workspace_bytes, float* pose2d, float* mesh,
                     float* lift_pose3d, float* reg_pose3d, float* mesh_valid, float* lift_valid, float* reg_valid,
                     int32_t* status, float* fit_err, int8_t* kind, float* rot_flip, void* stream);

/* ---- dataset annotations -> camera-frame body parameters, and the gender bank's choice (csrc/annot.hip) -------------------
 * What get_smpl_coord / get_mano_coord of the reference's datasets do per sample on the PARAMETERS, in numpy and
 * transforms3d on a dataloader worker (data/Human36M/dataset.py:253-299, data/AMASS/dataset.py:182-213, data/FreiHAND/
 * dataset.py:110-134; PW3D, SURREAL, MuCo and COCO are subsets), for a batch of row indices into annotation tables that
 * live in device memory: one launch on `stream`; nothing allocates or synchronises.
 * Tables, N rows each, fp32 unless noted: pose [N, 3 J], betas [N, nb] (NULL with nb = 0), trans [N, 3] (NULL: zeros), cam_R
 * [N, 9] row-major (NULL: identity), cam_t [N, 3] (NULL: zeros), focal, princpt [N, 2], gender [N] uint8 (NULL: all 0),
 * given_cam [N, Jr, 3] and given_img [N, Jr, 2] (NULL, or Jr = 0: skipped).  idx [B]: int32, or int64 with idx_is_int64, device
 * memory.  root_template [G, 3] and root_shapedirs [G, 3, nb]: the rest position and the shape directions of chain joint 0
 * (the root) of each of the G models, i.e. row 0 of the regressor folded into the template and the shape directions.
 * Per sample b with row r = idx[b]; ALL arithmetic in float64, each output rounded to fp32 once:
 *   betas_out   the row; with beta_reset all zeros when any |beta_k| > beta_limit (Human36M :264, which resets a shape with an
 *               entry beyond 3 to the mean shape).  A NaN compares false and is kept, as there.
 *   pose_out    the row; with rotate_root its first three values become the PRINCIPAL LOGARITHM of R . exp(root) (:267-273).
 *               exp is the exact Rodrigues formula of axangle2mat(root / |root|, |root|): with (x, y, z) the unit axis, c, s
 *               the cosine and sine, C = 1 - c: [[x x C + c, x y C - z s, z x C + y s], [x y C + z s, y y C + c, y z C - x s],
 *               [z x C - y s, y z C + x s, z z C + c]].  log goes through the quaternion of the product M: of tr M, M00, M11,
 *               M22 the largest picks Shepperd's branch (ties: in that order), e.g. s = 2 sqrt(1 + tr), w = s / 4, (x, y, z)
 *               = (M21 - M12, M02 - M20, M10 - M01) / s; the sign is flipped to w >= 0; rotvec = 2 atan2(|v|, w) v / |v|, and
 *               zero when |v| = 0.  The quaternion is not normalised: atan2 does not need it, so an R that is a rotation only
 *               to fp32 rounding is taken as it is.  mat2axangle returns the same vector for every angle below pi; at
 *               exactly pi the sign of the axis is undefined in both.
 *               DELIBERATE DIFFERENCE: a zero root pose is the identity rotation here (pose_out = log R).  The reference
 *               divides 0 / 0 (root_pose / angle) and hands NaNs to the body model.
 *   trans_out   R trans + t_scale cam_t, and with compensate_root + R J0 - J0, where J0 = root_template[g] + root_shapedirs[g]
 *               . betas_out (the betas AFTER the reset) and g the sample's gender: Human36M :286-291 with t_scale = 1 / 1000;
 *               AMASS / FreiHAND: trans NULL, t_scale = 1, no compensation.  DELIBERATE DIFFERENCE: the reference subtracts
 *               the root joint its layer returned in fp32; J0 is the rest root from tables folded in float64 and stored in
 *               fp32 - the two differ by fp32 rounding of a metre-sized value.
 *   focal_out, princpt_out, given_cam_out, given_img_out: the rows, bit for bit.  gender_out [B] int32: the row's gender.
 *   status [B] int32   bit 0: idx outside [0, N) - every output of the sample is zero, gender_out 0, and NO table is read at
 *               that index;  bit 1: gender >= G - model 0's root is used and gender_out = 0;  bit 2: the beta reset fired;
 *               bit 3: a non-finite value among the three root values or (cam_R given) R - with rotate_root the root is
 *               then copied through unchanged; trans_out is what the arithmetic gives.
 * Errors (P2M_ERR_INVALID, nothing launched): NULL pose, focal, princpt, idx, betas with nb > 0, or a required output
 * (given_*_out where given_* is read); B < 1 or N < 1; J outside [1, 64], nb outside [0, 64], G outside [1, 4], Jr outside [0,
 * 32]; compensate_root without the root tables; a NaN scalar; misaligned buffers (4 bytes; an int64 idx: 8).
 *
 * p2m_body_select: out[b] = src[gender[b]][b] for verts [B, V, 3], joints [B, NJ, 3] and (JX > 0) extra [B, JX, 3] in one
 * launch - the choice between the results of G forwards of p2m_body_forward over the same batch.  verts_src, joints_src and
 * extra_src are HOST arrays of G device pointers.  A gender outside [0, G) counts as 0.  The result is bit for bit the chosen
 * source.  A streaming copy: 16-byte stores wherever the output's base allows (any 4-byte-aligned base is accepted), 16-byte
 * loads where the four elements come from one sample's source at an aligned address, else the source is chosen per element.
 * Errors (P2M_ERR_INVALID, nothing launched): NULL required pointers, G outside [1, 4], B, V or NJ < 1, an output of 2^31
 * floats or more, misaligned buffers, an output that overlaps a source. */
int p2m_annot_gather(const float* pose, const float* betas, const float* trans, const float* cam_R, const float* cam_t,
                     const float* focal, const float* princpt, const uint8_t* gender, const float* given_cam,
                     const float* given_img, int64_t N, int32_t J, int32_t nb, int32_t Jr, const void* idx,
                     int32_t idx_is_int64, int32_t B, const float* root_template, const float* root_shapedirs, int32_t G,
                     int32_t rotate_root, int32_t beta_reset, int32_t compensate_root, double beta_limit, double t_scale,
                     float* pose_out, float* betas_out, float* trans_out, float* focal_out, float* princpt_out,
                     int32_t* gender_out, float* given_cam_out, float* given_img_out, int32_t* status, void* stream);
int p2m_body_select(const float* const* verts_src, const float* const* joints_src, const float* const* extra_src, int32_t G,
                    const int32_t* gender, int32_t B, int32_t V, int32_t NJ, int32_t JX, float* verts, float* joints,
                    float* extra, void* stream);

/* ---- Rendering: batched z-buffer rasteriser and image overlay (csrc/render.hip) ------------------------------------------
 * The device counterpart of demo/renderer.py + demo/run.py:46-67 (trimesh, pyrender, OpenGL / EGL, host compositing).  That
 * code needs an OpenGL context and cannot run where this library is built and tested, so this comment is the contract and
 * tests/render_ref.py its float64 / exact-integer restatement.  GEOMETRY follows the reference (renderer.py:28-35 the weak-
 * perspective projection matrix, :68-71 the 180 degree turn about x, :85-91,103-104 the identity camera pose, GL's viewport
 * and depth test, the top-down read-back): a vertex (x, y, z) of mesh b with cam[b] = (sx, sy, tx, ty) and an H x W image
 * lands at
 *   px = W/2 (1 + sx (x + tx)),  py = H/2 (1 + sy (y + ty)),  depth = z   (smaller is nearer; kept for zmin <= depth <= zmax,
 *                                                                          the reference's clip volume is [-1, 1])
 * with the centre of pixel (row i, column j) at (j + 0.5, i + 0.5).  A face is front-facing when its normal (v1 - v0) x
 * (v2 - v0) points to -z in these mesh coordinates; back faces are culled with flag bit 0 (pyrender's default).  SHADING is
 * this project's, not pyrender's metallic-roughness model: faces are flat-shaded (the reference's smooth=False),
 *   I = ambient + sum_l k_l max(0, n . l_l),   rgb_c = floor(255 min(1, colour_c I) + 0.5)
 * with n the unit face normal turned towards the viewer (n_z <= 0), l_l the unit vector towards light l (lights: HOST array
 * [nl][4] = direction x, y, z and k_l, nl <= 4, normalised in fp64 before the launch), everything in fp64 per face.
 * Compositing is renderer.py:112-113: a covered pixel shows its face's rgb, every other pixel the background (NULL: zeros).
 * COVERAGE IS EXACT.  Per mesh, in fp64 on the device, each operation rounded once:
 *   ax = (W/2) sx,  bx = (W/2) (1 + sx tx),  ay = (H/2) sy,  by = (H/2) (1 + sy ty)
 *   X = rint(256 fma(ax, x, bx)),  Y = rint(256 fma(ay, y, by))      (ties to even; int32; clamped to +-2^23, status bit 0;
 *                                                                     a NaN counts as +2^23)
 * Everything after is integer.  With area2 = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0): a face with area2 = 0 covers nothing;
 * it is front-facing iff area2 sgn(ax ay) < 0; s = sgn(area2).  For the edges k = 0: v0 -> v1, 1: v1 -> v2, 2: v2 -> v0
 * (a -> b) and a pixel centre P = (256 j + 128, 256 i + 128), in int64,
 *   E_k(P) = A_k (Px - Xa) + B_k (Py - Ya),   A_k = -s (Yb - Ya),   B_k = s (Xb - Xa)        (interior: E_k > 0)
 * and the pixel is covered iff, for every k, E_k > 0, or E_k = 0 on a left edge (A_k > 0) or a top edge (A_k = 0 and
 * B_k > 0): the D3D top-left rule, so a mesh is watertight - a centre on a shared edge belongs to exactly one face.
 * DEPTH at a covered pixel, all in fp32 (conversions and divisions correctly rounded):
 *   l1 = (float)E_2 / (float)|area2|,  l2 = (float)E_0 / (float)|area2|,  depth = fmaf(l2, z2 - z0, fmaf(l1, z1 - z0, z0))
 * within 12 x 2^-24 max|z| of the exact plane value (derivation in tests/render_ref.py).  A fragment is kept when
 * zmin <= depth <= zmax.  The VISIBLE fragment of a pixel is the minimum of a 64-bit key over its fragments,
 *   batch mode, scene mode with flag bit 1 (depth order):  [order-preserving bits of depth : 32][mesh rank : 8][face id : 24]
 *   scene mode without it (list order, run.py:311-315):    [255 - mesh rank : 8][the same depth bits : 32][face id : 24]
 * (rank = the mesh's index in scene mode, 0 in batch mode): nearest first and an exact depth tie to the lower rank, then the
 * lower face id; in list order a later mesh paints over an earlier one.  The minimum is taken with integer atomics in LDS,
 * per 64 x 64-pixel tile: no float atomics, bitwise reproducible, a mesh's pixels do not depend on the batch around it.
 *   verts [B, nv, 3] fp32, faces [nf, 3] int32 (shared by the meshes), cam [B, 4] fp32, colours [B, 3] fp32: device memory
 *   flags        bit 0 cull back faces, bit 1 depth order (scene mode)
 *   mode         0 batch: mesh b is rendered into image b (B images);  1 scene: all meshes into one image
 *   background   uint8 [H, W, 3] (bg_per_mesh = 0) or [B, H, W, 3] (bg_per_mesh = 1, batch mode only) or NULL
 *   image uint8 [n, H, W, 3], face_id int32 [n, H, W] (-1: background), mesh_id int32 [n, H, W] (the mesh's index b, -1:
 *   background), depth fp32 [n, H, W] (+inf: background), n = B or 1; each may be NULL
 *   status       int32 [B] or NULL: bit 0 a snapped coordinate of a referenced vertex was clamped, bit 1 a face index outside
 *                [0, nv) (that face covers nothing and its vertices are never read)
 *   workspace    p2m_mesh_render_workspace bytes of device memory, 16-byte aligned
 * One memset node and two kernels on `stream`: no allocation, no synchronisation, no data-dependent grid (capturable).
 * p2m_mesh_project: xy_fix [B, nv, 2] = (X, Y) of every vertex, by the same code; status bit 0 as above, over all vertices.
 * Errors (P2M_ERR_INVALID, nothing launched): NULL required pointers, nf < 1 or nf >= 2^24, more than 255 meshes in scene
 * mode (65535 in batch mode), H or W outside [1, 8192], nl outside [0, 4], a zero or non-finite light direction, B nf >= 2^31,
 * unknown mode or flag bits, a per-mesh background in scene mode, a misaligned workspace.                                 */
enum { P2M_RENDER_BATCH = 0, P2M_RENDER_SCENE = 1 };
enum { P2M_RENDER_CULL = 1, P2M_RENDER_DEPTH_ORDER = 2 };
int p2m_mesh_project(const float* verts, const float* cam, int32_t B, int32_t nv, int32_t H, int32_t W, int32_t* xy_fix,
                     int32_t* status, void* stream);
int p2m_mesh_render_workspace(int32_t B, int32_t nf, int32_t H, int32_t W, int32_t mode, int64_t* bytes_out);
int p2m_mesh_render(const float* verts, const int32_t* faces, int32_t nf, const float* cam, const float* colours,
                    const float* lights, int32_t nl, float ambient, float zmin, float zmax, int32_t flags,
                    const uint8_t* background, int32_t bg_per_mesh, int32_t B, int32_t nv, int32_t H, int32_t W, int32_t mode,
                    uint8_t* image, int32_t* face_id, int32_t* mesh_id, float* depth, int32_t* status, void* workspace,
                    void* stream);

/* ---- Shading a visibility buffer: vertex normals, smooth shading, vertex colours, attributes, wireframe (csrc/shade.hip) ---
 * A second, deferred pass over what p2m_mesh_render wrote (face_id, mesh_id): the reference's smooth-shaded result figures
 * (asset/quality_result.png), the `wireframe` switch of demo/renderer.py (RenderFlags.ALL_WIREFRAME) and any per-vertex
 * quantity carried to the pixels (an error as colour, part labels, skinning weights, normal maps, correspondences).  As above,
 * the reference's own renderer cannot run here: this comment is the contract and tests/shade_ref.py its numpy restatement.
 * Both calls: one memset node and one kernel on `stream`, no allocation, no synchronisation, grids from shapes only (capturable);
 * no float atomics and no LDS atomics, so a result is reproducible bit for bit and a mesh's values do not depend on the batch
 * around it.
 *
 * p2m_vertex_normals: area-weighted unit vertex normals of B meshes that share one face list.
 *   verts [B, nv, 3] fp32, faces [nf, 3] int32; vf_ptr int32 [nv + 1], vf_idx int32 [n_idx]: the vertex-to-face table - vertex v
 *   lists the ids of its incident faces, ascending, in vf_idx[vf_ptr[v] .. vf_ptr[v + 1]) (a CSR; render.vertex_face_table builds
 *   it); normals [B, nv, 3] fp32; status int32 [B] or NULL.  All device memory.  In fp64, every operation rounded once (nothing
 *   fused), for vertex v of mesh b: for each listed face f = (i0, i1, i2) in table order, with p_k the fp32 vertices widened,
 *     a = p1 - p0,  b = p2 - p0,  c = (ay bz - az by,  az bx - ax bz,  ax by - ay bx)    (two products and one difference each)
 *     n += c                                                                           (component-wise, from n = 0)
 *   then q = (nx nx + ny ny) + nz nz and normal = (float)(n / sqrt(q)), the division and the square root correctly rounded.
 *   If q is 0 or not finite (an isolated vertex, cancelling faces, a NaN or overflowing input) the normal is (0, 0, 0) and status
 *   bit 0 of the mesh is set.  A table entry outside [0, nf), a face with an index outside [0, nv), or a vertex whose table range
 *   is not inside [0, n_idx] contributes nothing, is never used as an index, and sets status bit 1 of the mesh.  The normals are
 *   the mesh's own: they are not turned towards a viewer.  A gather (one thread per vertex): no float atomics.
 *   Errors (P2M_ERR_INVALID, nothing launched): NULL pointers (status may be NULL; vf_idx when n_idx = 0), B < 0, more than 65535
 *   meshes, nv < 1, nf < 1, n_idx < 0, B nv 3 >= 2^31, a buffer not 4-byte aligned, an output that overlaps an input or the other
 *   output.
 *
 * p2m_mesh_shade: one pass over the pixels of a visibility buffer.
 *   face_id, mesh_id int32 [n, H, W] as p2m_mesh_render writes them (n = B, or 1 in scene mode); verts, faces, nf, cam, B, nv, H,
 *   W, mode, lights (HOST array), nl, ambient, background, bg_per_mesh exactly as that call took them.  Each of the following may
 *   be NULL / 0 when unused:
 *     colours [B, 3] fp32 or vertex_colours fp32 [B, nv, 3] (vertex_colours_shared = 0) / [nv, 3] for all meshes (= 1): an image
 *                     takes exactly one of the two
 *     normals [B, nv, 3] fp32 (p2m_vertex_normals' output, or any other): NULL means flat shading
 *     attrs   [B, nv, C] fp32, 1 <= C <= 16
 *     wire_T  int32 in [0, 2^16]: the line's half width in 1/256 pixel, 0: no wire;  wire_rgb: HOST uint8[3];  wire_only: a flag
 *     attr_fill: what attr_out shows off the mesh
 *   Outputs, each may be NULL: image uint8 [n, H, W, 3], bary fp32 [n, H, W, 3], attr_out fp32 [n, H, W, C], status int32 [B].
 *   OFF THE MESH.  A pixel with face_id < 0 shows the background (NULL: zeros), bary = 0 and attr_out = attr_fill.  A pixel with
 *   face_id >= nf, with mesh_id outside [0, B), whose face has an index outside [0, nv) or area2 = 0 (none of which the rasteriser
 *   writes) is treated the same way and sets status bit 1 of mesh 0; such a value is never used as an index.  The mesh of a
 *   covered pixel is mesh_id's value in both modes (in batch mode p2m_mesh_render wrote the image's own index there).
 *   BARYCENTRICS.  For a covered pixel of mesh b and face f: X, Y of the three vertices by the projection and snap above (the same
 *   code), area2, s and E_0, E_1, E_2 at the pixel centre exactly as defined above (integers), then in fp32, conversions and
 *   divisions correctly rounded,
 *     l0 = (float)E_1 / (float)|area2|,  l1 = (float)E_2 / (float)|area2|,  l2 = (float)E_0 / (float)|area2|     bary = (l0, l1, l2)
 *   the weights of v0, v1, v2; l1 and l2 are the ones of the depth formula.
 *   ATTRIBUTES.  attr_out[c] = fmaf(l2, a2[c], fmaf(l1, a1[c], l0 * a0[c])) in fp32, a_k the attribute rows of the face's vertices.
 *   WIRE (wire_T = T > 0).  The pixel is on the wire iff E_k^2 <= T^2 (A_k^2 + B_k^2) for some edge k of its own visible face,
 *   decided exactly in 128-bit integers (equality is on the wire): the centre lies within T / 256 pixel of the edge's line.  Only
 *   the visible face's edges are tested: hidden lines are removed, an interior edge is 2 T wide (T from each neighbour), a
 *   silhouette edge T.  A wire pixel shows wire_rgb, unshaded; with wire_only a covered pixel off the wire shows the background.
 *   SHADING of the other covered pixels, in fp64, each operation rounded once, with dk = (double)lk:
 *     colour  c = colours[b], or per channel c = (d0 c0 + d1 c1) + d2 c2 of the vertices' colours
 *     normal  without normals: the unit face normal turned towards the viewer, and I, exactly as p2m_mesh_render computes them;
 *             with normals:  m = (d0 n0 + d1 n1) + d2 n2 per component,  q = (mx mx + my my) + mz mz;  q zero or not finite: the
 *             face normal as above;  otherwise u = m / sqrt(q), negated when the face is back-facing (area2 sgn(ax ay) > 0:
 *             visible only where the rasteriser did not cull), and
 *             I = ambient + sum_l k_l max(0, (ux lx + uy ly) + uz lz)   accumulated in the lights' order
 *     rgb_c = floor(255 min(1, c_c I) + 0.5)                             (the rasteriser's rounding: negative and NaN give 0)
 *   With no normals, no vertex_colours and no wire, image is bit for bit the image p2m_mesh_render wrote.
 *   ALIASING.  image may be the very buffer the rasteriser wrote (the pass never reads it).  No output may overlap an input or
 *   another output.
 *   Errors (P2M_ERR_INVALID, nothing launched): as for p2m_mesh_render (NULL face_id, mesh_id, verts, faces or cam, the shape
 *   limits, nl, a zero or non-finite light direction, a per-mesh background in scene mode), and: C outside [1, 16] with attrs,
 *   attr_out without attrs, wire_T outside [0, 2^16] or wire_T > 0 without wire_rgb, both or neither of colours / vertex_colours
 *   with an image, a buffer not 4-byte aligned (image and background: 1 byte), an output that overlaps an input or an output.  */
enum { P2M_SHADE_DEGENERATE = 1, P2M_SHADE_BAD_INDEX = 2 };
int p2m_vertex_normals(const float* verts, const int32_t* faces, const int32_t* vf_ptr, const int32_t* vf_idx, int32_t n_idx,
                       int32_t B, int32_t nv, int32_t nf, float* normals, int32_t* status, void* stream);
int p2m_mesh_shade(const int32_t* face_id, const int32_t* mesh_id, const float* verts, const int32_t* faces, int32_t nf,
                   const float* cam, const float* colours, const float* vertex_colours, int32_t vertex_colours_shared,
                   const float* normals, const float* lights, int32_t nl, float ambient, const float* attrs, int32_t C,
                   int32_t wire_T, const uint8_t* wire_rgb, int32_t wire_only, const uint8_t* background, int32_t bg_per_mesh,
                   float attr_fill, int32_t B, int32_t nv, int32_t H, int32_t W, int32_t mode, uint8_t* image, float* bary,
                   float* attr_out, int32_t* status, void* stream);

/* ---- The demo's camera: batched 2D-pose preparation and the L1 Adam fit (csrc/camfit.hip) ---------------------------------
 * The piece of demo/run.py between its two device halves (optimize_cam_param, :149-197): pixels of 2D joints -> the network's
 * input and the fit's target (p2m_pose_prepare); 3D joints + target -> the weak-perspective camera of the crop
 * (p2m_camera_fit).  One launch each on `stream`, no allocation, no synchronisation (capturable).  tests/camfit_ref.py restates
 * both in numpy, float64.
 *
 * p2m_pose_prepare: run.py:150-159 for a batch.  joints [B, J, 2] fp32, pixels of the original image; in_W, in_H the network's
 *   input shape (288 x 384 for the bodies); crop the side of the virtual crop (500 in the demo).  One wave per sample, lane j =
 *   joint j, fp32, each operation rounded once and none fused:
 *     tight    (x0, y0, tw, th) = (min x, min y, max x - min x, max y - min y)                 (get_bbox, coord_utils.py:21-39)
 *     box(aspect, scale)  w = tw - 1, h = th - 1;  cx = x0 + w / 2, cy = y0 + h / 2;  w > aspect h: h = w / aspect;
 *              w < aspect h: w = h aspect;  w = w scale, h = h scale                           (process_bbox, :42-66)
 *     bbox2 = box(in_W / in_H, 1.0),  bbox1 = box(1, 1.25); both share the centre (cx, cy)
 *     affine   the rot = 0 similarity of get_affine_transform in closed form, as in p2m_train_sample: with s = res_w / bbox_w,
 *              x' = s (x - cx) + res_w / 2,  y' = s (y - cy) + res_h / 2
 *     target   = affine of (crop, crop) with bbox1;   p = affine of (in_W, in_H) with bbox2, then p / (in_W, in_H)
 *     pose2d   = (p - mean) / std per sample and axis, the population std; sums over the lanes in the butterfly order below
 *     bbox     = (cx - w1 / 2, cy - h1 / 2, w1, h1): the reference's bbox1, what crop_cam_to_image takes
 *   status [B] int32, bit 0 as p2m_train_sample's: a degenerate box (tw th <= 0, tw < 1 or th < 1: process_bbox would return
 *   None), a non-finite joint, a zero or non-finite std.  That sample's pose2d, target and bbox are then all zero.
 *   Inputs are float.  The reference's demo file is int64, and aug_utils.py:59 writes the transformed points back into that
 *   integer array, truncating them: a property of that fixture (kept in oracle/demo_oracle.py), not of this entry point.
 *   Errors (P2M_ERR_INVALID, nothing launched): NULL pointers, B < 1, J outside [1, 64], in_W, in_H or crop not in (0, 1e6).
 *
 * p2m_camera_fit: OptimzeCamLayer (lib/models/project_net.py:7-17) + nn.L1Loss + torch.optim.Adam + the rate steps of
 *   run.py:176-189, for B independent samples.  One wave per sample, lane j holds joint j for the whole fit.
 *     joints3d [B, J, 3] fp32 (only x, y are read), target [B, J, 2], weight [B, J] or NULL (w_j = 1), cam0 [B, 3] or NULL,
 *     state: the two device words {seed, first_index} of the noise stream (may be NULL when cam0 is given), sched: at most 8
 *     (first_step, lr) pairs by value, first_step[0] = 0 and strictly ascending: step i (zero-based) runs at the lr of the last
 *     entry with first_step <= i.  The reference lowers the rate AFTER the steps with j == 500 and j == 1000, so its schedule
 *     is ((0, 0.1), (501, 0.05), (1001, 0.001)) with steps = 1500.  img_res = crop / 2.
 *   All arithmetic is fp32, each operation rounded once and none fused (no fma), except where fp64 is named.
 *   SUMS over the joints are taken over the wave's 64 lanes (lanes >= J hold +0) in ONE fixed butterfly order:
 *     v1[l] = v[l] + v[l ^ 1],  v2[l] = v1[l] + v1[l ^ 2],  v4[l] = v2[l] + v2[l ^ 4],  ..,  v32[l] = v16[l] + v16[l ^ 32]
 *   fp32 addition commutes, so every lane ends with the same bits, and a sample's result depends on the sample alone.
 *   Setup:   W = sum_j w_j,  c_j = (w_j / (2 W)) r   (r = img_res);  cam = cam0[b], or drawn (below)
 *   Step t = 1 .. steps, with (s, tx, ty) = cam:
 *     q_j = (x_j + tx, y_j + ty),  pred_j = (q_j s) r + r        (the module's order),   e_j = pred_j - t_j
 *     g_j = sign(e_j) c_j per axis, sign(0) = 0 (torch's)
 *     grad = (sum_j (g_jx q_jx + g_jy q_jy),  sum_j g_jx s,  sum_j g_jy s)                    three butterfly sums
 *     m = m + (grad - m) (float)(1 - beta1)                                                   (lerp_)
 *     v = v (float)beta2 + ((float)(1 - beta2) grad) grad                                     (mul_, addcmul_)
 *     cam = cam - (step_size_t m) / (sqrt(v) / c2_t + (float)eps)                             (addcdiv_)
 *     step_size_t = (float)(lr_t / (1 - beta1^t)),  c2_t = (float)sqrt(1 - beta2^t): torch computes the two corrections in
 *     float64 on the host with pow(); HERE beta1^t and beta2^t are running fp64 products on the device (one multiply per
 *     step), the division and square root are fp64, and each is rounded to fp32 once per step.
 *   Outputs: cam [B, 3] after the last step; loss [B] = (sum_j w_j (|e_jx| + |e_jy|)) / (2 W), evaluated once more at exactly
 *   those parameters (one butterfly sum of the lane terms w_j (|e_jx| + |e_jy|)); steps = 0 returns the start bitwise.
 *   Start: with cam0 NULL the reference's torch.rand((1, 3)) is drawn from the project's one Philox stream as
 *     stage 10 "camera start", joint 0, block 0: (s, tx, ty) = words 0, 1, 2 as (word >> 8) 2^-24, counter = the global sample
 *     index state[1] + b  (stages 0-9: "training-sample noise" above).  The caller advances state[1] by B with a tensor add.
 *   status [B] int32: bit 0 a non-finite value among the sample's x, y, target, weights or start, or W <= 0: cam = 0, loss = 0,
 *   the other samples are untouched;  bit 1: s <= 0 at the end (the mirrored solution; reported, not altered).
 *   Errors (P2M_ERR_INVALID, nothing launched): NULL required pointers, both cam0 and state NULL, misaligned state, B < 1, J
 *   outside [1, 64], steps outside [0, 65535], sched.n outside [1, 8], first_step[0] != 0 or not strictly ascending, an lr
 *   that is not finite, img_res <= 0 or not finite, betas outside [0, 1), eps < 0.                                         */
typedef struct p2m_fit_schedule {
  int32_t n;
  int32_t first_step[8];
  double lr[8];
} p2m_fit_schedule;
int p2m_pose_prepare(const float* joints, int32_t B, int32_t J, float in_W, float in_H, float crop, float* pose2d, float* target,
                     float* bbox, int32_t* status, void* stream);
int p2m_camera_fit(const float* joints3d, const float* target, const float* weight, const float* cam0, const uint64_t* state,
                   int32_t B, int32_t J, p2m_fit_schedule sched, int32_t steps, float img_res, double beta1, double beta2,
                   double eps, float* cam, float* loss, int32_t* status, void* stream);

/* ---- Video evaluation: One-Euro smoothing and the per-video metrics (csrc/video.hip) ---------------------------------------
 * The second half of the reference's 3DPW protocol (data/PW3D/dataset.py:383-417): smooth_pose (lib/smooth_utils.py), then
 * compute_error_accel (lib/coord_utils.py:194-222), MPJPE and PA-MPJPE per video.  Launches on `stream` only, no allocation,
 * no synchronisation (capturable).  tests/video_ref.py restates both entries in numpy.
 *
 * Sequences: seq_ptr [S + 1] int32 on the device, ascending from 0 to N; sequence s owns rows seq_ptr[s] .. seq_ptr[s + 1] - 1
 * and may be empty.  The kernels clamp what they read from seq_ptr to [0, N].
 *
 * p2m_one_euro: the filter over a ragged batch.  x [N, C] fp32, a row is one frame of C scalars; rows [N] int32 or NULL: the
 *   input row of frame i is x[rows[i]] (every entry must name a row of x), or x[i]; y [N, C] is written in sequence order and
 *   may be x itself only when rows is NULL.  With f() = round to fp32, the parameters enter as
 *     mc = f(min_cutoff), b = f(beta), te = f(dt), k2 = f(2 pi), kd = f(2 pi d_cutoff)   (that product taken in double)
 *   and every operation below is one fp32 operation, rounded once and never fused; divisions are correctly rounded:
 *     first frame of a sequence:  y = x,  xp = x,  dxp = 0
 *     after that:  rd = kd te              ad = rd / (rd + 1)
 *                  dx = (x - xp) / te      dxh = ad dx + (1 - ad) dxp
 *                  cut = mc + b |dxh|      r = (k2 cut) te          a = r / (r + 1)
 *                  y = a x + (1 - a) xp    xp = y,  dxp = dxh
 *   This is OneEuroFilter.__call__ on float32 arrays as smooth_pose drives it (t_e = 1 there), bit for bit.  A NaN or an
 *   infinity in one coordinate stays in that coordinate of that sequence.
 *   Carried state (all three or none): state_x, state_dx [S, C] fp32 and started [S] int32.  started[s] == 0: the first frame
 *   of sequence s in this call initialises the filter; otherwise (xp, dxp) continue from the state.  After the call the state
 *   holds the last xp and dxp of every non-empty sequence and their started is 1; empty sequences keep theirs.  The flags are
 *   written by a second launch on the stream, after the filter has read them.  Without state every sequence starts fresh.
 *   One lane per (sequence, coordinate) with 4-byte accesses; 8- and 16-byte lane accesses where C and the alignment of x, y
 *   and the state allow it AND the batch is large enough to fill the device at that width (csrc/video.hip);  loads run
 *   p2m_one_euro_lookahead() frames ahead of the recurrence.
 *   Errors (P2M_ERR_INVALID, nothing launched): NULL x, seq_ptr or y; N < 0, S < 1, C < 1; N C or S C >= 2^31; the state given
 *   in part; rows together with y == x; a parameter that is not finite, dt <= 0, a cutoff < 0, or a parameter whose fp32
 *   rounding is infinite (or 0, for dt).
 *
 * p2m_video_eval: the metrics of every video in one call.  pred, gt [N, J, 3] fp32 in sequence order, 1 <= J <= 64; vis [N]
 *   uint8 or NULL (all visible).  Everything is accumulated in fp64 from the fp32 inputs and rounded once where stored as fp32.
 *     accel [N], accel_valid [N] uint8: for frame i with i + 2 inside its sequence and vis[i], vis[i + 1], vis[i + 2] all
 *       non-zero, mean_j |(p_i - 2 p_i+1 + p_i+2) - (g_i - 2 g_i+1 + g_i+2)|  (compute_error_accel; its np.roll wrap-around
 *       never survives the [:-2]); elsewhere 0 and accel_valid = 0
 *     mpjpe [N, J]: |p - g| per joint;   pa_mpjpe [N, J] (want_pa): the same after the similarity alignment of the frame's
 *       prediction onto its ground truth, the solve of p2m_rigid_align (this unit is built without fma contraction, so the two
 *       agree to the last bits of the fp64 solve, not bitwise)
 *     frame_sums [N, 4] fp64, workspace and output: accel, accel_valid, sum_j mpjpe, sum_j pa_mpjpe per frame
 *     seq_stats [S, 8] fp64: frames, valid accelerations, mean accel (NaN without one), mean of mpjpe over frames x joints (NaN
 *       when empty), sum of pa_mpjpe, count of pa_mpjpe values (0 without want_pa), 0, 0
 *     totals [8] fp64, the reference's aggregation: [0] accel error = unweighted mean over videos of the per-video means,
 *       [1] MPJPE = unweighted mean over videos of the per-video means, [2] PA-MPJPE = mean pooled over all frames and joints,
 *       [3] videos in [0], [4] videos left out of [0], [5] videos in [1], [6] empty videos, [7] frames
 *   DIFFERENT from the reference on purpose: a video without a valid acceleration frame (fewer than 3 frames, or no visible
 *   triple) has a NaN per-video value, and np.mean would make the reference's total NaN; here it is left out of totals[0] and
 *   counted in totals[4].  Empty videos are left out of totals[1] in the same way and counted in totals[6].  A total over no
 *   video is NaN.
 *   Fixed reduction orders, no atomics: bitwise reproducible, and a sequence's results do not depend on the other sequences.
 *   Errors (P2M_ERR_INVALID, nothing launched): NULL required pointers (pa_mpjpe is required with want_pa), N < 0, S < 1, J
 *   outside [1, 64], N J 3 >= 2^31.                                                                                       */
int32_t p2m_one_euro_lookahead(void);
int p2m_one_euro(const float* x, const int32_t* seq_ptr, const int32_t* rows, int32_t N, int32_t S, int32_t C,
                 double min_cutoff, double beta, double d_cutoff, double dt, float* state_x, float* state_dx, int32_t* started,
                 float* y, void* stream);
int p2m_video_eval(const float* pred, const float* gt, const int32_t* seq_ptr, const uint8_t* vis, int32_t N, int32_t S,
                   int32_t J, int32_t want_pa, float* accel, uint8_t* accel_valid, float* mpjpe, float* pa_mpjpe,
                   double* frame_sums, double* seq_stats, double* totals, void* stream);

/* ---- 2D pose overlay: batched anti-aliased lines, discs and rings on uint8 images (csrc/overlay.hip) -------------------------
 * The device counterpart of lib/vis.py's vis_2d_keypoints (:77-113; vis_2d_pose is the same on an image) and
 * vis_coco_skeleton (:10-74).  GEOMETRY AND SEMANTICS follow the reference: which primitives are drawn, where, in which order,
 * with which thickness, on a copy that is then blended with the image.  THE PIXEL ARITHMETIC is this project's: the reference
 * draws with OpenCV's LINE_AA tables, and OpenCV is not a dependency here, so this comment is the contract and
 * tests/overlay_ref.py its exact-integer restatement.  It is held bit for bit; parity with OpenCV's pixels is not claimed.
 * INPUTS, device memory unless stated:
 *   poses    fp32 [B, P, J, C], C = 2 or 3: x, y in pixels of image b, then an optional confidence.  Image b receives its P
 *            people in index order (the demo's crowd loop is B = 1, a batch of crops P = 1)
 *   bones    int32 [L, 2] joint indices (NULL allowed when L = 0)
 *   colours  uint8, in the image's own channel order (the kernels never swap channels); colour_mode 0: [L, 3], one per bone
 *            (vis_2d_keypoints);  1: [B, P, 3], one per person (vis_coco_skeleton's given_color).  NULL allowed when L = 0
 *   boxes    fp32 [B, P, 4, 2] or NULL: the four corners of vis_2d_keypoints' bbox;  box_rgb: HOST value, channel 0 in bits
 *            0-7, channel 1 in bits 8-15, channel 2 in bits 16-23
 *   src, dst uint8 [B, H, W, 3].  src == dst is allowed and is the normal use; when they differ every pixel of dst is written
 *            (they must then not overlap).  Rows are 3 W bytes at any byte offset: 4-byte accesses are used for a lane's 12
 *            bytes where they are 4-byte aligned, single bytes elsewhere
 *   thr      host float;  line_h2, mark_h2, box_h2: host, thickness in HALF pixels, in [0, 64] (h2 = 2 is OpenCV's thickness 2,
 *            a filled radius-3 disc is h2 = 6);  mark_r16: host, -1 a disc, >= 0 a ring of radius r16 / 16 pixels, at most
 *            1024;  alpha256: host, in [0, 256]
 *   status   int32 [B, P] or NULL, written (not accumulated) by every call
 * SNAPPING.  A coordinate v becomes the integer (int)v, truncated towards zero (vis.py's astype(np.int32)).  A joint is
 * UNUSABLE when a coordinate is not finite or |v| >= 16384: status bit 0 of its person is set (for any of the person's J
 * joints, used by a bone or not) and the joint is invisible.  A joint is VISIBLE iff it is usable and, with C = 3, conf > thr
 * (strict; a NaN confidence is invisible).  Pixel (row i, column j) is the point (j, i), as in OpenCV.  A box with an unusable
 * corner is skipped as a whole and status bit 1 is set.
 * PRIMITIVES AND PAINT ORDER within an image: persons p = 0 .. P - 1; for each, with boxes, the four box edges corner k ->
 * corner (k + 1) mod 4 (thickness box_h2, colour box_rgb); then for each bone l = 0 .. L - 1 (i1, i2) three primitives:
 * the line i1 - i2 (line_h2) iff both joints are visible, the mark at i1 iff i1 is visible, the mark at i2 iff i2 is visible
 * (mark_h2, mark_r16).  That is the order of vis.py's loops; a later primitive paints over an earlier one.  A bone index
 * outside [0, J) is an error of the caller: this entry cannot see device memory, so the check belongs to the owner of the
 * host copy (overlay.PoseOverlay refuses at construction); the kernels never follow such an index, the bone draws nothing.
 * COVERAGE, exact.  Pixel q, segment a - b (a mark: a = b), all integers: d = b - a, w = q - a, L2 = d.d, t = w.d.
 *   L2 = 0 or t <= 0:  (num, den) = (w.w, 1);    t >= L2:  (num, den) = (|q - b|^2, 1);
 *   otherwise, with c = w.x d.y - w.y d.x:       (num, den) = (c^2, L2)
 *   D = floor(16 sqrt(num / den)) = the unique integer with D^2 den <= 256 num < (D + 1)^2 den;   a ring: D <- |D - r16|
 *   cov = clamp(8 h2 + 8 - D, 0, 16) sixteenths: clamp(h + 1/2 - dist, 0, 1) on a 1/16 grid, within 1/16 of the analytic value
 * D only matters below 8 h2 + 8 + r16 <= 1544, so the kernel estimates it in fp32 and settles it with the two exact 64-bit
 * comparisons; |c| >= 2^26 is more than 1400 pixels from the line (cov = 0), and below that 256 c^2 fits 64 bits.  No square
 * root and no division is named, so nothing rests on how either is rounded.
 * BLENDING, exact integers per channel: m = src; for each primitive in paint order with cov > 0:
 *   m <- m + (((colour - m) cov + 8) >> 4)      (arithmetic shift: a floor)
 * and at the end dst = (src (256 - alpha256) + m alpha256 + 128) >> 8, cv2.addWeighted(img, 1 - alpha, kp_mask, alpha):
 * alpha256 = 256 gives m, 0 gives src.
 * Two kernels on `stream`, always the same two: no allocation, no memset, no synchronisation, no data-dependent grid, no
 * float atomics and no atomics in global memory - capturable, reproducible bit for bit, and an image's pixels do not depend on
 * the batch around it.  A 32 x 32-pixel tile that no primitive's inflated bbox meets is not touched when src == dst.
 *   workspace  p2m_pose_overlay_workspace(B, P, L, with_boxes) bytes of device memory, 16-byte aligned: 24 bytes per slot
 * Errors (P2M_ERR_INVALID, nothing launched): a NULL required pointer (poses, src, dst, workspace; bones and colours when
 * L > 0), B < 0, H or W outside [1, 8192], J or P outside [1, 64], L outside [0, 64], L = 0 without boxes, C not 2 or 3, an
 * h2 outside [0, 64], mark_r16 outside [-1, 1024], alpha256 outside [0, 256], an unknown colour_mode, B P (3 L + 4) >= 2^31,
 * 2^31 tiles or more, a small or misaligned workspace.  B = 0 is a no-op.                                                   */
enum { P2M_OVERLAY_COLOUR_PER_BONE = 0, P2M_OVERLAY_COLOUR_PER_PERSON = 1 };
int p2m_pose_overlay_workspace(int32_t B, int32_t P, int32_t L, int32_t with_boxes, int64_t* bytes_out);
int p2m_pose_overlay(const float* poses, int32_t B, int32_t P, int32_t J, int32_t C, const int32_t* bones, int32_t L,
                     const uint8_t* colours, int32_t colour_mode, const float* boxes, uint32_t box_rgb, const uint8_t* src,
                     uint8_t* dst, int32_t H, int32_t W, float thr, int32_t line_h2, int32_t mark_h2, int32_t mark_r16,
                     int32_t box_h2, int32_t alpha256, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The crowd demo's front end: who is in the picture, and their colours (csrc/crowd.hip) -----------------------------------
 * The head of the crowd branch of demo/run.py: add_pelvis / add_neck (:127-146), the score filter and the greedy suppression
 * of duplicate detections (:276-306), and one random colour per accepted person (:314).  One launch each on `stream`, no
 * allocation, no synchronisation (capturable).  tests/crowd_ref.py restates both in numpy, float64.
 *
 * p2m_crowd_select: dets fp32 [B, P, J, 3] = (x, y, confidence) of up to P detections per image in the detector's list order;
 *   num int32 [B] on the device or NULL: how many of the P slots of image b are filled (clamped to [0, P]; NULL: all P).  A slot
 *   at or beyond num[b] is never read.  midpoints: HOST array [n_mid, 2] of input-joint indices in [0, J), n_mid in [0, 8],
 *   Jo = J + n_mid <= 64, P in [1, 64].  pose_thr, score_thr, min_diff: the reference's 0.1, 1.5, 20.
 *   One block per image.  ALL DECISION ARITHMETIC IS FLOAT64 on the fp32 inputs widened exactly, every operation rounded once
 *   and none fused (this unit is built with -ffp-contract=off).  Per image, with i, d slots and j < Jo joints:
 *     midpoints  joint J + m = midpoint m of (a, b):  xy = (xy_a + xy_b) * 0.5,  conf = conf_a * conf_b  (the product)
 *     valid      valid_ij = conf_ij > pose_thr  (strict; over all Jo joints)
 *     score      score_i = ((conf_i0 + conf_i1) + conf_i2) + .. + conf_i,Jo-1: sequential, in index order (Python's sum)
 *     non-finite a slot with a NaN or an infinity among the x, y, confidence of its J INPUT joints: reason 3.  This rule is this
 *                project's: in the reference such a detection poisons the mean of every later comparison.  Here it is dropped,
 *                never enters the accepted list and so suppresses nobody.
 *     low score  score_i < score_thr (strict): reason 1; never enters the accepted list.
 *     duplicate(i, d), d an ACCEPTED slot before i:  the terms t = |v_i - v_d| for v = x_j, y_j of every joint j with valid_ij
 *                and valid_dj, walked JOINT-MAJOR, x BEFORE y (j = 0: x, y; j = 1: x, y; ..); a term equal to 0 is left out (two
 *                coinciding coordinates do not count, as a masked joint does not: the reference's diff[diff != 0]);
 *                S = sum of the kept terms, added sequentially in that order, n = their number;
 *                n == 0: a duplicate;  otherwise mean = S / n (one correctly rounded division) and a duplicate iff
 *                mean < min_diff (strict).
 *     greedy     slots are visited in list order; slot i with reason 0 so far is compared with every slot accepted before it
 *                and ONLY those: a duplicate of any of them gets reason 2 and dup_of = the lowest such slot; otherwise it is
 *                accepted (reason 0).  A slot suppressed by an accepted one suppresses nobody itself.
 *   The pair tests are independent and spread over the block's waves (a 64-bit mask of matching earlier slots per slot, built
 *   by ballots: no atomics), the greedy scan over the masks is serial on one wave, the compaction a popcount of the accepted
 *   mask below each bit.  An image's outputs depend on that image alone and are reproducible bit for bit.
 *   Outputs:  joints fp32 [B, P, Jo, 3]: the accepted slots of each image compacted to the front in list order, (x, y, conf)
 *             with the midpoints rounded ONCE from float64 to fp32; every remaining slot is filled with quiet NaNs (7FC00000):
 *             p2m_pose_prepare zeroes such a sample (status bit 0), p2m_camera_fit returns cam = 0 for it, the rasteriser
 *             skips its faces, p2m_pose_overlay draws nothing of it - an absent person needs no host round trip
 *             count int32 [B];  index int32 [B, P]: the input slot of compacted person k, -1 for k >= count
 *             per INPUT slot: reason int8 [B, P] (0 accepted, 1 low score, 2 duplicate, 3 non-finite, -1 at or beyond num),
 *             dup_of int32 [B, P] (-1 unless reason 2), score fp64 [B, P] (the quiet NaN 7FF8000000000000 for reasons 3 and
 *             -1), keep uint8 [B, P] = (reason == 0)
 *   Errors (P2M_ERR_INVALID, nothing launched): a NULL required pointer (everything but num; midpoints when n_mid > 0), B
 *   outside [1, 2^24], P outside [1, 64], J < 1, n_mid outside [0, 8], Jo > 64, a midpoint index outside [0, J), a threshold
 *   that is not finite, score not 8-byte aligned.
 *
 * p2m_person_colours: n colours, colorsys.hsv_to_rgb(h_k, s, v) with the hue drawn from the project's one Philox stream
 *   ("training-sample noise" above) as
 *     stage 11 "person colour", joint 0, block 0: h = (word 0 >> 8) 2^-24, counter = the global index state[1] + k
 *   (stages 0-10 are untouched; the caller advances state[1] by n with a tensor add, as for p2m_camera_fit).  Float64, every
 *   operation rounded once:  s == 0: (v, v, v);  otherwise i = (int)(6 h), f = 6 h - i, p = v (1 - s), q = v (1 - s f),
 *   t = v (1 - s (1 - f)), and by i mod 6:  0 (v, t, p)  1 (q, v, p)  2 (p, v, t)  3 (p, q, v)  4 (t, p, v)  5 (v, p, q).
 *   rgb fp32 [n, 3]: each channel rounded once to fp32 (what p2m_mesh_render's colours take);  u8 uint8 [n, 3]: 255 times the
 *   FLOAT64 channel, rounded half to even (what p2m_pose_overlay's per-person colours take; the same channel order - nothing
 *   here swaps channels).  Either output may be NULL, not both.
 *   Errors (P2M_ERR_INVALID, nothing launched): NULL or misaligned (8 bytes) state, both outputs NULL, n outside [1, 2^24], s or
 *   v outside [0, 1] or not finite.                                                                                          */
int p2m_crowd_select(const float* dets, const int32_t* num, int32_t B, int32_t P, int32_t J, const int32_t* midpoints,
                     int32_t n_mid, double pose_thr, double score_thr, double min_diff, float* joints, int32_t* count,
                     int32_t* index, int8_t* reason, int32_t* dup_of, double* score, uint8_t* keep, void* stream);
int p2m_person_colours(const uint64_t* state, int32_t n, double s, double v, float* rgb, uint8_t* u8, void* stream);

/* ---- Tracking people across frames: stable slots and ids (csrc/track.hip) ------------------------------------------------------
 * p2m_crowd_select hands out the people of a frame in the detector's list order, which changes from frame to frame; the
 * streaming filter p2m_one_euro needs row b to be the same person in every call.  p2m_pose_track joins them: a state machine
 * per video stream that gives every person a track SLOT that stays theirs and a unique id.  The reference has no tracker (its
 * 3DPW data carries person ids): the contract below is this project's, tests/track_ref.py restates it in numpy, float64.  One
 * block per stream, one launch per call on `stream`, no allocation, no synchronisation, the grid from the shapes alone
 * (capturable).  The first call on a device opts the kernel in to its largest LDS size (no stream operation).
 *
 *   people fp32 [F, S, P, Jo, 3] = (x, y, confidence): F >= 1 frames of each of S streams, up to P <= 64 people per frame,
 *   Jo <= 64 joints - p2m_crowd_select's joints: [1, B, ..] for one frame of B streams, [B, 1, ..] for B frames of one video.
 *   A person slot is PRESENT iff all its 3 Jo values are finite; absent slots may sit anywhere in the list.
 *   State, device memory of the caller's, persistent across calls, updated in place:  pose fp32 [S, T, Jo, 3];  uid int32
 *   [S, T], -1 = a free slot;  missed int32 [S, T];  next_uid int32 [S];  T <= 64 track slots per stream.  A fresh state is
 *   uid = -1, missed = 0, next_uid = 0 (pose is never read of a free slot).
 *   pose_thr, gate, min_common, max_missed: 0.1, 0.3, 3, 10 are this project's defaults - a choice, not measured optima.
 *
 *   Per stream, the frames of a call in order.  ALL DECISION ARITHMETIC IS FLOAT64 on the fp32 values widened exactly, every
 *   operation rounded once and none fused (this unit is built with -ffp-contract=off):
 *     valid      a joint of a person, or of a stored track pose, is valid iff conf > pose_thr (strict)
 *     cost(p, t) of a present person p and an alive track t (uid >= 0 AT THE START of the frame): the terms |v_p - v_t| for
 *                v = x_j, y_j of every joint j valid in both, walked JOINT-MAJOR, x BEFORE y.  Every term counts, a zero too
 *                (unlike p2m_crowd_select's duplicate test).  S = the terms added sequentially in that order, n = their number
 *                (twice the common joints).  n < 2 min_common: no candidate.  size_t = max(max x - min x, max y - min y) over
 *                the track's valid joints; if size_t >= 1 is false, size_t = 1.  cost = (S / n) / size_t, two correctly rounded
 *                divisions.  The pair is a candidate iff cost < gate (strict).
 *     greedy     globally ascending: repeatedly the candidate pair of least cost among the persons and tracks not yet taken;
 *                ties go to the lower track slot, then to the lower person index; until no candidate is left.
 *     births     the present persons left unmatched, in person order, each take the lowest slot that was free AT THE START of
 *                the frame; a born slot gets uid = next_uid[s]++.  With no such slot left the person is dropped (slot_of = -2,
 *                counted in dropped).
 *     update     a slot with a person takes that person's Jo x 3 values bit for bit (low-confidence joints too), missed = 0.
 *                An alive slot without one: missed += 1, and it is retired (uid = -1; missed keeps its value) when
 *                missed > max_missed.  A slot retired in a frame is free from the NEXT frame on, never within it.
 *   Outputs per frame, each may be NULL:
 *     joints fp32 [F, S, T, Jo, 3]  the slot's person this frame; quiet NaNs (7FC00000) otherwise, which the modules behind
 *                                   read as "nobody" (see p2m_crowd_select)
 *     slot_of int32 [F, S, P]       the person's slot; -1 absent, -2 dropped
 *     person_of int32 [F, S, T]     the slot's person, -1 none
 *     uid int32 [F, S, T]           after the frame
 *     flags uint8 [F, S, T]         bit 0 alive after the frame, bit 1 has a person this frame, bit 2 born, bit 3 FRESH = has a
 *                                   person and (born or missed > 0 before the frame), bit 4 retired this frame
 *     cost fp64 [F, S, T]           the matched pair's cost; the quiet NaN 7FF8000000000000 for a born or empty slot
 *     dropped int32 [F, S]
 *   A stream's results depend on that stream alone; F frames in one call equal F calls of one frame bit for bit, state
 *   included; everything is reproducible bit for bit (no atomics; the greedy arg-min is an exact comparison of (cost, t, p)).
 *   Errors (P2M_ERR_INVALID, nothing launched): NULL people or a NULL state pointer, F or S outside [1, 2^24], P, T or Jo
 *   outside [1, 64], min_common outside [1, Jo], max_missed < 0, pose_thr or gate not finite, cost not 8-byte aligned.       */
int p2m_pose_track(const float* people, int32_t F, int32_t S, int32_t P, int32_t T, int32_t Jo, double pose_thr, double gate,
                   int32_t min_common, int32_t max_missed, float* st_pose, int32_t* st_uid, int32_t* st_missed,
                   int32_t* st_next_uid, float* joints, int32_t* slot_of, int32_t* person_of, int32_t* uid, uint8_t* flags,
                   double* cost, int32_t* dropped, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* P2M_H_ */
