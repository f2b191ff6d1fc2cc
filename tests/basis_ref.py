"""Float64 restatements of the sparse stage of csrc/basis.hip (p2m_cheb_basis_fwd / _fwd_real / _bwd / _pair, p2m_cheb_combine_small /
_small_real, p2m_cheb_expand_small), the error bound the suite holds them to, a graph family whose merged rows have every length
the unrolled gathers can meet, and the tables of cases that tests/test_gpu_basis_edges.py runs.  No GPU and no library:
tests/test_basis_ref_cpu.py audits the tables, checks the restated coefficients against dense float64 algebra, shows that a
sequential float32 evaluation stays inside the bound and that planted faults do not.

Coefficients.  merged(L) repeats the bake of p2m_graph_create (csrc/capi.hip): per row the sorted union of the patterns of L, of
L L and the diagonal, a = fp32(sum L_ij), b = fp32(sum_k 2 L_ik L_kj - delta_ij), accumulated in double from the fp32 values that
ops.DeviceGraph uploads, in the library's loop order.  The references below use THESE coefficients (as float64 arrays that hold
fp32 values) and fp32 inputs widened to float64, so that a kernel differs from its reference only by the rounding of its
accumulation chain.

The bound.  An output element that a kernel accumulates from n terms t_1 .. t_n may differ from the float64 reference by at most
    2 (n + 2) 2^-24 sum |t_i|.
This is the forward-error bound of a recursive sum of n products in fp32 (unit round-off 2^-24; n u instead of gamma_n, which the
factor 2 also pays for), doubled for a multiply-add that is not fused; the + 2 covers a coefficient restated one ulp off and the
rounding of the result.  n: the merged row length for the forward planes (entries, not distinct source rows); over the children of
an output row, twice the row length plus d0 and resid, for the backward; twice the row length plus P0 and the bias for the combine
(one more for the multiplication by `scale`).  The bound is derived, not measured, and every reference returns it per element.

Layouts.  Activations are [B, rows, F] arrays; shift 1 reads a coarse input of V / 2 rows per sample (vertex v reads row v >> 1)
or, backward, sums the two children 2p, 2p + 1 of coarse row p."""
import numpy as np
import scipy.sparse as sp

import tile_plan_ref as tp

U = 2.0 ** -24                 # unit round-off of fp32
ROWS_PER_BLOCK = 4             # basis.hip: rows per block of k_basis_fwd / k_basis_bwd, one per wave
SMALL_SPB = 8                  # samples per block of k_combine_small_tile / k_expand_small_tile
BASIS_SPB = 8                  # basis_spb(): samples per block of k_basis_tile
ROW_WIDTHS = (32, 64, 128, 256)            # widths of the vector row kernels (LPR = F / 4 lanes per sample)
TILE_WIDTHS = (32, 64, 256, 384)           # widths run through k_basis_tile (384: three 128-feature slices)
GENERIC_WIDTHS = (3, 5, 96)


def f32(x):
    """Round to fp32, keep as float64."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---- the merged operator --------------------------------------------------------------------------------------------------------

class Merged:
    """CSR rows (rp, col, a, b) over `ncols` source rows; a, b are float64 arrays of fp32 values."""

    def __init__(self, rp, col, a, b, ncols):
        self.rp, self.col = np.asarray(rp, dtype=np.int64), np.asarray(col, dtype=np.int64)
        self.a, self.b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        self.nrows, self.ncols = len(self.rp) - 1, int(ncols)
        self.lens = np.diff(self.rp)

    def csr(self, which, shift=0, absolute=False):
        """Sparse matrix of the a or b coefficients; shift 1: column c reads source row c >> 1 (equal columns add up)."""
        v = self.a if which == "a" else self.b
        return sp.csr_matrix((np.abs(v) if absolute else v, self.col >> shift, self.rp), shape=(self.nrows, self.ncols >> shift))

    def row(self, r):
        s, e = self.rp[r], self.rp[r + 1]
        return self.col[s:e], self.a[s:e], self.b[s:e]

    def edited(self, r, keep=None, swap=False):
        """A copy with row r cut to the entries keep (positions in the row) and / or with its a and b swapped (planted faults)."""
        s, e = int(self.rp[r]), int(self.rp[r + 1])
        pos = np.arange(e - s) if keep is None else np.asarray(keep)
        col, a, b = self.col[s:e][pos], self.a[s:e][pos], self.b[s:e][pos]
        if swap:
            a, b = b, a
        rp = self.rp.copy()
        rp[r + 1:] += len(pos) - (e - s)
        return Merged(rp, np.concatenate([self.col[:s], col, self.col[e:]]), np.concatenate([self.a[:s], a, self.a[e:]]),
                      np.concatenate([self.b[:s], b, self.b[e:]]), self.ncols)


def merged(L):
    """p2m_graph_create's bake of L (any scipy sparse matrix), entry for entry and in its order of accumulation."""
    L = tp._csr(L)
    V = L.shape[0]
    rp_l, col_l = L.indptr.tolist(), L.indices.tolist()
    val = L.data.astype(np.float32).astype(np.float64).tolist()
    rp, mc, ma, mb = [0], [], [], []
    for i in range(V):
        acc_a, acc_b = {}, {}
        for j in range(rp_l[i], rp_l[i + 1]):
            k, lik = col_l[j], val[j]
            if k not in acc_a:
                acc_a[k], acc_b[k] = 0.0, 0.0
            acc_a[k] += lik
            for q in range(rp_l[k], rp_l[k + 1]):
                c = col_l[q]
                if c not in acc_a:
                    acc_a[c], acc_b[c] = 0.0, 0.0
                acc_b[c] += 2.0 * lik * val[q]
        if i not in acc_a:
            acc_a[i], acc_b[i] = 0.0, 0.0
        acc_b[i] -= 1.0
        for c in sorted(acc_a):
            mc.append(c)
            ma.append(acc_a[c])
            mb.append(acc_b[c])
        rp.append(len(mc))
    return Merged(rp, mc, f32(ma), f32(mb), V)


def paired(m):
    """Rows of the paired operator (capi.hip, plan 2) for EVERY coarse vertex c: merged row 2c + merged row 2c + 1, equal columns
    summed in double and rounded to fp32.  The library keeps the rows of tile_plan_ref.Plans.pair_order."""
    assert m.nrows % 2 == 0
    rp, col, a, b = [0], [], [], []
    for c in range(m.nrows // 2):
        cu, au, bu = m.row(2 * c)
        cw, aw, bw = m.row(2 * c + 1)
        cols = np.union1d(cu, cw)
        sa, sb = np.zeros(len(cols)), np.zeros(len(cols))
        iu, iw = np.searchsorted(cols, cu), np.searchsorted(cols, cw)
        sa[iu] += au
        sb[iu] += bu
        sa[iw] += aw
        sb[iw] += bw
        col.append(cols)
        a.append(f32(sa))
        b.append(f32(sb))
        rp.append(rp[-1] + len(cols))
    return Merged(rp, np.concatenate(col), np.concatenate(a), np.concatenate(b), m.ncols)


# ---- float64 references, each with its per-element bound --------------------------------------------------------------------

def _apply(M, X):
    """M [R, C] (sparse) on X [B, C, F] -> [B, R, F]."""
    B, C, F = X.shape
    Y = M @ np.ascontiguousarray(X.transpose(1, 0, 2)).reshape(C, B * F)
    return np.ascontiguousarray(np.asarray(Y).reshape(M.shape[0], B, F).transpose(1, 0, 2))


def _bound(n, S):
    return 2.0 * (n + 2.0) * U * S


def planes(m, X, shift):
    """T1 = L x, T2 = L2 x of X [B, ncols >> shift, F] -> (T1, T2, bound1, bound2), each [B, nrows, F]."""
    X = np.asarray(X, dtype=np.float64)
    assert X.shape[1] == m.ncols >> shift
    n = m.lens[None, :, None].astype(np.float64)
    T1, T2 = _apply(m.csr("a", shift), X), _apply(m.csr("b", shift), X)
    Xa = np.abs(X)
    return T1, T2, _bound(n, _apply(m.csr("a", shift, True), Xa)), _bound(n, _apply(m.csr("b", shift, True), Xa))


def bwd(m, d0, d1, d2, resid, shift):
    """dX[p] = sum over the children r of p of d0[r] + resid[r] + sum_j a_j d1[col_j] + b_j d2[col_j] -> (dX, bound),
    [B, V >> shift, F]."""
    d0, d1, d2 = (np.asarray(t, dtype=np.float64) for t in (d0, d1, d2))
    full = d0 + _apply(m.csr("a"), d1) + _apply(m.csr("b"), d2)
    S = np.abs(d0) + _apply(m.csr("a", 0, True), np.abs(d1)) + _apply(m.csr("b", 0, True), np.abs(d2))
    n = (2.0 * m.lens + 1.0)[None, :, None] * np.ones_like(full)
    if resid is not None:
        resid = np.asarray(resid, dtype=np.float64)
        full, S, n = full + resid, S + np.abs(resid), n + 1.0
    if shift:
        B, V, F = full.shape
        full, S, n = (t.reshape(B, V // 2, 2, F).sum(2) for t in (full, S, n))
    return full, _bound(n, S)


def combine(m, P, nc, ldp, bias, scale=None):
    """Y = P0 + L P1 + L2 P2 (+ bias) (* scale) from P [B, V, ldp], columns [0, nc) = P0, [nc, 2 nc) = P1, [2 nc, 3 nc) = P2
    -> (Y, bound), [B, V, nc]."""
    P = np.asarray(P, dtype=np.float64)
    assert P.shape[2] == ldp >= 3 * nc
    P0, P1, P2 = P[..., :nc], P[..., nc:2 * nc], P[..., 2 * nc:3 * nc]
    Y = P0 + _apply(m.csr("a"), P1) + _apply(m.csr("b"), P2)
    S = np.abs(P0) + _apply(m.csr("a", 0, True), np.abs(P1)) + _apply(m.csr("b", 0, True), np.abs(P2))
    n = (2.0 * m.lens + 1.0)[None, :, None]
    if bias is not None:
        bias = np.asarray(bias, dtype=np.float64)
        Y, S, n = Y + bias, S + np.abs(bias), n + 1.0
    if scale is not None:
        Y, S, n = Y * scale, S * abs(scale), n + 1.0
    return Y, _bound(n, S)


def expand(m, G, nc, lde):
    """E = [G | L G | L2 G | 0 ...] with rows lde wide from G [B, V, nc] -> (E, bound); G and the zeros are exact."""
    G = np.asarray(G, dtype=np.float64)
    assert G.shape[2] == nc and lde >= 3 * nc
    T1, T2, e1, e2 = planes(m, G, 0)
    E = np.zeros(G.shape[:2] + (lde,))
    bound = np.zeros_like(E)
    E[..., :nc], E[..., nc:2 * nc], E[..., 2 * nc:3 * nc] = G, T1, T2
    bound[..., nc:2 * nc], bound[..., 2 * nc:3 * nc] = e1, e2
    return E, bound


def pair_planes(m, G):
    """S L g and S L2 g (S = the pair-sum) of G [B, V, F] for every coarse row -> (P1, P2, bound1, bound2), [B, V / 2, F]."""
    if not hasattr(m, "_paired"):
        m._paired = paired(m)
    return planes(m._paired, G, 0)


# ---- graphs ---------------------------------------------------------------------------------------------------------------------

STAR_SIZES = {
    "starsA": tuple(range(2, 18)) + (24, 33, 64, 203),                      # 476 real vertices: 119 blocks of 4 rows
    "starsB": tuple(range(2, 17)) + (24, 33, 64, 203),                      # without the 17-star: 459, an odd count
    "starsC": (2,) + tuple(range(2, 18)) + (24, 33, 64, 203),               # one more 2-star: 478 -> 120 blocks, a multiple of 8
}


def stars(sizes, V, seed):
    """Disjoint stars on the first sum(sizes) vertices, the rest isolated, all vertices renumbered at random.  Every merged row of
    a star of s vertices has exactly s entries (a leaf reaches the other leaves through the centre)."""
    assert sum(sizes) <= V
    rows, cols, at = [], [], 0
    for s in sizes:
        rows.append(np.full(s - 1, at))
        cols.append(np.arange(at + 1, at + s))
        at += s
    return tp.permuted(tp.laplacian(tp._sym(np.concatenate(rows), np.concatenate(cols), V), V), seed)


def no_plan_twin(L):
    """L with a star of UCAP + 2 vertices appended as a block of its own: the first V rows keep their merged coefficients, and the
    one row above the union cap leaves the level without a tile plan - the row kernels then run where the tile kernels did."""
    s = tp.UCAP + 2
    star = tp.laplacian(tp._sym(np.zeros(s - 1, dtype=np.int64), np.arange(1, s), s), s)
    return sp.block_diag([tp._csr(L), star]).tocsr()


class GraphCase:
    def __init__(self, name, V, L):
        self.name, self.V, self.L = name, V, L
        self.m = merged(L)
        self.plans = tp.Plans(L)

    @property
    def real_order(self):
        return self.plans.real_order


_graphs = {}


def graph(name, V):
    """The graph `name` on V vertices, with its merged operator and the plans the library should make, once per process."""
    key = (name, V)
    if key not in _graphs:
        if name in STAR_SIZES:
            L = stars(STAR_SIZES[name], V, 11 + V)
        elif name == "band":
            L = tp.band(V, 7 + V)
        else:
            L = tp.family(name)[0]
            assert L.shape[0] == V
        _graphs[key] = GraphCase(name, V, L)
    return _graphs[key]


def inputs(seed, *shapes):
    """Seeded fp32 standard-normal arrays."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(np.float32) for s in shapes]


def out_index(gc, seed, drop=7, spare=5):
    """(out_index [V] int32, out_rows): the real vertices but `drop` of them, scattered over out_rows = kept + spare rows; -1 at the
    dropped and at the padding vertices."""
    rng = np.random.default_rng(seed)
    kept = rng.permutation(np.sort(gc.real_order))[drop:]
    out_rows = len(kept) + spare
    inv = np.full(gc.V, -1, dtype=np.int32)
    inv[kept] = rng.permutation(out_rows)[:len(kept)].astype(np.int32)
    return inv, out_rows


# ---- which kernel a call takes ------------------------------------------------------------------------------------------------

def samples_per_wave(F):
    return 64 // (F // 4)


def row_batches(F):
    """B in {1, S - 1, S, S + 1, 2 S + 1} for the S samples a wave serves."""
    S = samples_per_wave(F)
    return sorted({b for b in (1, S - 1, S, S + 1, 2 * S + 1) if b >= 1})


def row_grid(F, B, nset):
    """Blocks of k_basis_fwd / k_basis_bwd over nset rows: sample groups x blocks of 4 rows."""
    return -(-B // samples_per_wave(F)) * -(-nset // ROWS_PER_BLOCK)


def tile_blocks(ntiles, F, B):
    """Working blocks of k_basis_tile (the grid is this rounded up to a multiple of 8; the rest return at once)."""
    return ntiles * -(-B // BASIS_SPB) * (F // 128 if F >= 128 else 1)


def fwd_real_kernel(gc, F, shift):
    """'tile', 'row' or None (refused): what p2m_cheb_basis_fwd_real launches."""
    if gc.plans.plan[shift] is not None and (F in (32, 64) or F % 128 == 0):
        return "tile"
    return "row" if F in ROW_WIDTHS else None


def narrow_kernels(gc, nc, real_only=False):
    """The launches of the narrow kernels: ('tile', 'row'), ('tile',) or ('row',)."""
    if gc.plans.plan[0] is not None and nc == 3:
        return ("tile",) if real_only else ("tile", "row")
    return ("row",)


# ---- case tables ------------------------------------------------------------------------------------------------------------------
# (V, shift) of the full-size row kernels.  ceil(V / 4) = 136 for V = 541 .. 544 (a multiple of 8: swizzled block ids) and 133 for
# V = 530; shift 1 needs an even V; V % 4 and (V / 2) % 4 take every value.
_ROW_GEO = ((541, 0), (542, 1), (542, 0), (543, 0), (544, 1), (530, 0), (530, 1))


def _row_cases(backward):
    out = []
    for F in ROW_WIDTHS:
        Bs = row_batches(F)
        for i, (V, shift) in enumerate(_ROW_GEO):
            case = ("starsA", V, F, shift, Bs[i % len(Bs)])
            out.append(case + (i % 2 == 0,) if backward else case)
    return out


FWD_CASES = _row_cases(False)              # (graph, V, F, shift, B): p2m_cheb_basis_fwd, k_basis_fwd<F / 4> without ids
BWD_CASES = _row_cases(True)               # (graph, V, F, shift, B, resid): p2m_cheb_basis_bwd, k_basis_bwd<F / 4>

# k_basis_fwd_generic / k_basis_bwd_generic: (graph, V, F, shift, B, resid)
GENERIC_CASES = [(g, V, F, shift, B, resid)
                 for F in GENERIC_WIDTHS
                 for (g, V, shift, B, resid) in (("starsA", 541, 0, 3, True), ("starsA", 542, 1, 2, False),
                                                 ("starsB", 530, 1, 1, True), ("starsA", 543, 0, 2, False))]

# p2m_cheb_basis_fwd_real on levels without a plan, k_basis_fwd<F / 4> with ids: (graph, V, F, shift, B)
_IDS_GEO = (("starsA", 542, 1), ("starsB", 541, 0), ("starsB", 530, 1), ("starsC", 544, 0), ("starsC", 542, 1), ("starsA", 543, 0))
IDS_CASES = [(g, V, F, shift, row_batches(F)[i % len(row_batches(F))])
             for F in ROW_WIDTHS for i, (g, V, shift) in enumerate(_IDS_GEO)]

_PLANNED = (("band", 736), ("hub120", 1472))
_SPB_EDGES = (1, 7, 8, 9, 17)

# p2m_cheb_combine_small ("full") / _small_real without ("real") and with out_index and scale 1000 ("index"):
# (graph, V, nc, ldp, bias, B, mode)
COMBINE_CASES = []
for _nc in (1, 2, 3, 4):
    COMBINE_CASES += [("starsA", 541, _nc, 3 * _nc, True, 3, "full"), ("starsA", 541, _nc, 32, False, 9, "full"),
                      ("starsA", 541, _nc, 3 * _nc, _nc % 2 == 0, 5, "real"), ("starsB", 530, _nc, 32, _nc % 2 == 1, 9, "index")]
for _g, _V in _PLANNED:
    COMBINE_CASES += [(_g, _V, 3, (9, 32)[_i % 2], _i % 3 != 0, _B, "full") for _i, _B in enumerate(_SPB_EDGES)]
    COMBINE_CASES += [(_g, _V, _nc, (3 * _nc, 32)[_nc % 2], _nc != 2, 9, "full") for _nc in (1, 2, 4)]
    COMBINE_CASES += [(_g, _V, 3, 32, True, 8, "index"), (_g, _V, 3, 9, False, 9, "real"), (_g, _V, 3, 9, True, 17, "index"),
                      (_g, _V, 3, 32, True, 16, "real"), (_g, _V, 2, 6, True, 9, "index"), (_g, _V, 4, 32, False, 8, "real")]
COMBINE_CASES += [("mixed", 1472, 3, 32, True, 9, "full"), ("mixed", 1472, 3, 9, True, 9, "index")]

# p2m_cheb_expand_small: (graph, V, nc, lde, B)
EXPAND_CASES = []
for _nc in (1, 2, 3, 4):
    EXPAND_CASES += [("starsA", 541, _nc, 3 * _nc, 1), ("starsA", 541, _nc, 3 * _nc + 1, 9), ("starsB", 530, _nc, 32, 3)]
for _g, _V in _PLANNED:
    EXPAND_CASES += [(_g, _V, 3, (9, 10, 32)[_i % 3], _B) for _i, _B in enumerate(_SPB_EDGES)]
    EXPAND_CASES += [(_g, _V, _nc, (3 * _nc + 1, 32, 3 * _nc)[_nc % 3], 9) for _nc in (1, 2, 4)]
    EXPAND_CASES += [(_g, _V, 3, 32, 16)]
EXPAND_CASES += [("mixed", 1472, 3, 32, 9)]

# nc = 3 on a planned graph against the row kernel alone on no_plan_twin of the same graph, bit for bit: (graph, V, B)
TWIN_CASES = [("band", 736, 9), ("band", 736, 8), ("hub120", 1472, 17)]

# p2m_cheb_basis_fwd_real through k_basis_tile: (graph, V, F, shift, B); every width meets B in {8, 9, 16, 17} and both shifts
TILE_CASES = [("band", 736, 32, 0, 8), ("band", 1472, 32, 1, 9), ("band", 736, 32, 1, 16), ("band", 1472, 32, 0, 17),
              ("band", 1472, 64, 1, 8), ("band", 736, 64, 0, 9), ("band", 1472, 64, 0, 16), ("band", 736, 64, 1, 17),
              ("band", 736, 256, 1, 8), ("band", 736, 256, 0, 9), ("band", 736, 256, 0, 16), ("band", 736, 256, 1, 17),
              ("band", 1472, 256, 1, 9),
              ("band", 736, 384, 0, 8), ("band", 736, 384, 1, 9), ("band", 736, 384, 1, 16), ("band", 736, 384, 0, 17),
              ("band", 1472, 384, 0, 8)]

# p2m_cheb_basis_pair (k_basis_tile over the paired plan): (graph, V, F, B)
PAIR_CASES = [("band", 736, 64, 8), ("band", 1472, 64, 9), ("band", 736, 64, 17), ("band", 736, 384, 8), ("band", 736, 384, 9),
              ("band", 1472, 384, 17)]
