"""Float64 restatements of the dense contractions of include/p2m.h (p2m_gemm_planes, p2m_gemm_planes_rows, p2m_gemm_tn,
p2m_gemm_tn_rows, p2m_gemm_tn_acc) in plain torch, the bounds the suite holds them to, and the table of cases that
tests/test_gpu_gemm_edges.py runs.  No GPU and no library: tests/test_gemm_ref_cpu.py audits the table (which row counts,
stage counts, pipeline depths and tile widths it reaches), checks the restatements against a second formulation and checks that
every case can tell a dropped, doubled or misplaced row from a right answer.

The functions take fp32 torch tensors on any device and return float64 tensors on the same device.

Row sets.  Logical row (b, i), i < n, of a row set with the id list `ids` is the actual row b * V + ids[i]; plane 0 of A is read
at (b * V + ids[i]) >> a0_shift; the planes 1, 2 at the compact row b * n + i when `compact`, else at the actual row.
`weights` ([B * n], default ones) and `rows` ([B * n] actual rows, default from ids) exist for the mutation check only: weight 0
drops a logical row, weight 2 counts it twice, `rows` sends it somewhere else."""
import math

import numpy as np
import torch

import tile_plan_ref as tp

TILE = 128                     # rows per BatchNorm partial tile (p2m_stats_tile_rows)
TN_STAGE_SLICED = 16           # rows per pipeline stage of k_gemm_tn_ws (bf16x3, f16x2)
TN_STAGE_F32 = 32              # ... of the f32 k_gemm_tn
ARITHS = ("f32", "bf16x3", "f16x2")


# ---- bounds (those tests/test_gpu_ops.py holds the same kernels to, on the same input distributions) ------------------------

def tol_fwd(ref):
    return 2e-5 * max(1.0, float(ref.abs().max()) if ref.numel() else 0.0)


def tol_grad(ref, rows):
    return 3e-6 * max(1.0, float(ref.abs().max()) if ref.numel() else 0.0) * math.sqrt(rows)


def tol_pdb(rows):
    return 1e-4 * math.sqrt(rows)


TOL_STAT_SUM, TOL_STAT_M2 = 1e-3, 2e-3


# ---- restatements ------------------------------------------------------------------------------------------------------------

def act_on_load(x, scale, shift):
    """max(fma(x, scale[k], shift[k]), 0) in fp32, the operand an activation on load forms."""
    return torch.clamp_min(torch.addcmul(shift.float(), x.float(), scale.float()), 0.0)


def logical_rows(ids, V, B, device="cpu"):
    """Actual row b * V + ids[i] of every logical row, [B * n]."""
    ids = torch.as_tensor(np.asarray(ids, dtype=np.int64), device=device)
    return (torch.arange(B, device=device)[:, None] * V + ids[None, :]).reshape(-1)


def tile_stats(Y, B, n, weights=None):
    """[B * ceil(n / TILE)][2][N]: weighted sum and centred M2 of every (sample, tile) of Y [B * n, N]."""
    N = Y.shape[1]
    tps = -(-n // TILE)
    w = torch.ones(B * n, dtype=torch.float64, device=Y.device) if weights is None else weights.double()
    st = torch.zeros(B * tps, 2, N, dtype=torch.float64, device=Y.device)
    for b in range(B):
        for t in range(tps):
            lo, hi = b * n + t * TILE, b * n + min((t + 1) * TILE, n)
            y, wt = Y[lo:hi], w[lo:hi, None]
            st[b * tps + t, 0] = (wt * y).sum(0)
            mean = st[b * tps + t, 0] / wt.sum().clamp_min(1e-300)
            st[b * tps + t, 1] = (wt * (y - mean) ** 2).sum(0)
    return st


def _epilogue(Y, bias, act):
    if bias is not None:
        Y = Y + bias.double()
    if act is not None:
        scale, shift, relu = act
        Y = Y * scale.double() + shift.double()
        if relu:
            Y = Y.clamp_min(0.0)
    return Y


def planes_rows_ref(ids, V, B, A, a0_shift, compact, Bm, bias=None, addend=None, in_act=None, act=None, weights=None,
                    rows=None):
    """p2m_gemm_planes_rows.  A: 1 .. 3 planes ([B * V >> a0_shift, Ka]; [B * n, Ka] compact or [B * V, Ka]); Bm [planes * Ka, N];
    addend [B * V, N]; in_act = (scale[Ka], shift[Ka]) on plane 0; act = (scale[N], shift[N], relu) on acc + bias.
    Returns (rows [B * n], Y [B * n, N] - what row rows[j] of C receives -, stats of the per-sample tiles)."""
    n = len(ids)
    dev = A[0].device
    if rows is None:
        rows = logical_rows(ids, V, B, dev)
    comp = torch.arange(B * n, device=dev)
    a0 = A[0][rows >> a0_shift]
    if in_act is not None:
        a0 = act_on_load(a0, *in_act)
    Z = torch.cat([a0.double()] + [(p[comp] if compact else p[rows]).double() for p in A[1:]], 1)
    Y = _epilogue(Z @ Bm.double(), bias, act)
    if addend is not None:
        Y = Y + addend[rows].double()
    return rows, Y, tile_stats(Y, B, n, weights)


def tn_chunk_rows(n, splits, sliced):
    """Rows of one slice of a sample's row set for splits >= 1: ceil(n / splits), in the slice arithmetics rounded up to a
    multiple of 16 (trailing slices may then be empty)."""
    cr = -(-n // splits)
    return -(-cr // 16) * 16 if sliced else cr


def tn_chunks(n, B, splits, sliced):
    """The chunks of p2m_gemm_tn_rows as lists of (sample, first logical row, end): splits >= 1 - chunk b * splits + s is
    slice s of sample b; splits = -S - chunk c holds the whole row sets of the samples c * S ... (the last chunk: what is left)."""
    if splits >= 1:
        cr = tn_chunk_rows(n, splits, sliced)
        return [[(b, min(s * cr, n), min((s + 1) * cr, n))] for b in range(B) for s in range(splits)]
    S = -splits
    return [[(b, 0, n) for b in range(c * S, min((c + 1) * S, B))] for c in range(-(-B // S))]


def tn_rows_ref(ids, V, B, A, a0_shift, G, compact, a_act=None, splits=1, sliced=True, weights=None, rows=None):
    """p2m_gemm_tn_rows.  A [B * V >> a0_shift, Ka]; G: 1 .. 3 column planes (plane 0 [B * V, Gc]; the others [B * n, Gc]
    compact or [B * V, Gc]).  Returns (P [Ka, N] and Pdb [N] summed over the chunks, P and Pdb per chunk, rows reduced per
    chunk)."""
    n = len(ids)
    dev = A.device
    if rows is None:
        rows = logical_rows(ids, V, B, dev)
    comp = torch.arange(B * n, device=dev)
    a = A[rows >> a0_shift]
    if a_act is not None:
        a = act_on_load(a, *a_act)
    a = a.double()
    g = torch.cat([G[0][rows].double()] + [(p[comp] if compact else p[rows]).double() for p in G[1:]], 1)
    if weights is not None:
        g = g * weights.double()[:, None]
    Pc, Pdbc, nrows = [], [], []
    for chunk in tn_chunks(n, B, splits, sliced):
        P = torch.zeros(a.shape[1], g.shape[1], dtype=torch.float64, device=dev)
        Pdb = torch.zeros(g.shape[1], dtype=torch.float64, device=dev)
        cnt = 0
        for b, lo, hi in chunk:
            P += a[b * n + lo:b * n + hi].t() @ g[b * n + lo:b * n + hi]
            Pdb += g[b * n + lo:b * n + hi].sum(0)
            cnt += hi - lo
        Pc.append(P)
        Pdbc.append(Pdb)
        nrows.append(cnt)
    Pc, Pdbc = torch.stack(Pc), torch.stack(Pdbc)
    return Pc.sum(0), Pdbc.sum(0), Pc, Pdbc, nrows


def _unpool(a, shift, M):
    return a.repeat_interleave(2, 0)[:M] if shift else a[:M]


def gemm_planes_ref(A, a0_shift, Bm, M, bias=None, addend=None, act=None):
    """p2m_gemm_planes, one output plane: (Y [M, N], stats [ceil(M / TILE), 2, N])."""
    Z = torch.cat([_unpool(p, a0_shift if q == 0 else 0, M).double() for q, p in enumerate(A)], 1)
    Y = _epilogue(Z @ Bm.double(), bias, act)
    if addend is not None:
        Y = Y + addend.double()
    nt = -(-M // TILE)
    st = torch.zeros(nt, 2, Y.shape[1], dtype=torch.float64, device=Y.device)
    for t in range(nt):
        y = Y[t * TILE:(t + 1) * TILE]
        st[t, 0] = y.sum(0)
        st[t, 1] = ((y - y.mean(0)) ** 2).sum(0)
    return Y, st


def gemm_tn_ref(A, a0_shift, G, M, chunk_rows):
    """p2m_gemm_tn: (P [nchunks, planes * Ka, N], Pdb [nchunks, N], rows per chunk); chunk c = rows [c, c + 1) * chunk_rows."""
    Z = torch.cat([_unpool(p, a0_shift if q == 0 else 0, M).double() for q, p in enumerate(A)], 1)
    g = torch.cat([p[:M].double() for p in G], 1)
    nch = -(-M // chunk_rows)
    P = torch.stack([Z[c * chunk_rows:(c + 1) * chunk_rows].t() @ g[c * chunk_rows:(c + 1) * chunk_rows] for c in range(nch)])
    Pdb = torch.stack([g[c * chunk_rows:(c + 1) * chunk_rows].sum(0) for c in range(nch)])
    return P, Pdb, [min((c + 1) * chunk_rows, M) - c * chunk_rows for c in range(nch)]


def gemm_tn_acc_ref(A, G, P0):
    """p2m_gemm_tn_acc: P0 + A^T G."""
    return P0.double() + A.double().t() @ G.double()


# ---- graphs ------------------------------------------------------------------------------------------------------------------
# name -> (V, real vertices, seed of the renumbering): tp.band(V, seed, nreal=...).  Every graph gives two row counts, n_real
# (row set 1) and V - n_real (row set 2); the small counts are the fake sets.  V even (a0_shift = 1), V <= 320, n_real >= 40.
GRAPHS = {
    "r41f1": (42, 41, 1), "r49f15": (64, 49, 2), "r48f16": (64, 48, 3), "r47f17": (64, 47, 4), "r63f33": (96, 63, 5),
    "r127f81": (208, 127, 6), "r129f31": (160, 129, 7), "r128f32": (160, 128, 8), "r200f54": (254, 200, 9),
    "r217f103": (320, 217, 10), "r73f97": (170, 73, 11), "r255f65": (320, 255, 12),
}
# Row sets 3 / 4 (the paired sets over V / 2 coarse rows) exist only on a level with a paired tile plan: at least 256 real
# vertices, some fake ones and 128 coarse vertices with a real child (csrc/capi.hip).  With tp.band's default 40 % of fake
# vertices, 428 is the smallest even V whose int(0.6 V) reaches 256 (tests/test_gemm_ref_cpu.py checks both sides).
PAIR_GRAPH, PAIR_V, PAIR_SEED = "pair428", 428, 5

_graphs = {}


def graph_ids(name):
    """(L, V, {row set: ids}) of a graph of the table, from the restated planner, once per process (row sets 3 / 4: coarse
    vertex ids, over V / 2 rows)."""
    if name not in _graphs:
        if name == PAIR_GRAPH:
            L = tp.band(PAIR_V, PAIR_SEED)
            p = tp.Plans(L)
            both = p.fake[0::2] & p.fake[1::2]
            ids = {1: p.real_order, 2: np.where(p.fake)[0], 3: p.pair_order, 4: np.where(both)[0]}
            assert p.n_pair_real > 0
        else:
            V, nreal, seed = GRAPHS[name]
            L = tp.band(V, seed, nreal=nreal)
            p = tp.Plans(L)
            assert (p.n_real, p.n_fake) == (nreal, V - nreal) and p.plan_tiles == (0, 0, 0)
            ids = {1: p.real_order, 2: np.where(p.fake)[0]}
        _graphs[name] = (L, p.V, {k: np.asarray(v, dtype=np.int64) for k, v in ids.items()})
    return _graphs[name]


def set_rows(name, row_set):
    """(ids, V of the row space) of a row set of a graph of the table."""
    _, V, ids = graph_ids(name)
    return ids[row_set], (V // 2 if row_set >= 3 else V)


# ---- the case table ----------------------------------------------------------------------------------------------------------
K_PIPE = [(32, 1), (64, 1), (32, 3), (128, 1), (64, 3)]      # (Ka, planes): 2, 4, 6, 8, 12 chunks of 16 (1, 2, 3, 4, 6 of 32)
FWD_N = [32, 96, 128]                                         # a 64-wide tile half empty, two 64-wide tiles, one 128-wide tile
GRAD_N = [(1, 32), (1, 64), (1, 128), (3, 64)]                # (planes of G, Gc)
GRAD_K = [32, 96, 192]


def _planes_rows_cases():
    cases, i = [], 0
    for name in GRAPHS:
        for rs in (1, 2):
            Ka, planes = K_PIPE[i % 5]
            cases.append(dict(graph=name, row_set=rs, B=2 + (i // 2) % 2, Ka=Ka, planes=planes, N=FWD_N[i % 3], a0_shift=i % 2,
                              compact=(i // 2) % 2, addend=bool((i // 3) % 2), stats=True, in_act=False, act=None,
                              sliced_only=False))
            i += 1
    base = dict(B=2, a0_shift=0, compact=1, addend=False, stats=True, in_act=False, act=None, sliced_only=False)
    # activation on load of plane 0 (slice arithmetics), the last tile / the only tile partial
    cases.append(dict(base, graph="r129f31", row_set=1, Ka=64, planes=3, N=128, in_act=True, sliced_only=True))
    cases.append(dict(base, graph="r49f15", row_set=2, Ka=32, planes=1, N=32, in_act=True, sliced_only=True, a0_shift=1))
    # activation in the epilogue (excludes the statistics), with and without the ReLU
    cases.append(dict(base, graph="r129f31", row_set=1, Ka=32, planes=3, N=96, stats=False, act="relu"))
    cases.append(dict(base, graph="r47f17", row_set=2, Ka=64, planes=1, N=128, stats=False, act="affine"))
    # the paired sets
    cases.append(dict(base, graph=PAIR_GRAPH, row_set=3, Ka=64, planes=3, N=128, addend=True))
    cases.append(dict(base, graph=PAIR_GRAPH, row_set=3, Ka=32, planes=3, N=96, compact=0, B=3))
    cases.append(dict(base, graph=PAIR_GRAPH, row_set=4, Ka=64, planes=1, N=128, addend=True))
    cases.append(dict(base, graph=PAIR_GRAPH, row_set=4, Ka=128, planes=1, N=32, B=3))
    return cases


def _tn_rows_cases():
    cases, i = [], 0
    for name in GRAPHS:
        for rs in (1, 2):
            gp, Gc = GRAD_N[i % 4]
            cases.append(dict(graph=name, row_set=rs, B=2 + (i // 3) % 2, Ka=GRAD_K[i % 3], gplanes=gp, Gc=Gc, a0_shift=i % 2,
                              compact=(i // 4) % 2, splits=1, a_act=False, sliced_only=False))
            i += 1
    base = dict(B=2, Ka=32, gplanes=1, Gc=64, a0_shift=0, compact=1, splits=1, a_act=False, sliced_only=False)
    # slices of a sample's rows; in the slice arithmetics 17 rows / 4, 129 rows / 4 and 1 row / 2 leave trailing slices empty
    cases.append(dict(base, graph="r47f17", row_set=2, splits=4, Ka=96, gplanes=3))                 # 8 chunks
    cases.append(dict(base, graph="r41f1", row_set=2, splits=2, B=3, Gc=32))
    cases.append(dict(base, graph="r63f33", row_set=2, splits=2, Gc=128, a0_shift=1))
    cases.append(dict(base, graph="r129f31", row_set=1, splits=4, B=3, Ka=192, gplanes=3, compact=0))    # 12 chunks
    cases.append(dict(base, graph="r127f81", row_set=2, splits=2, Ka=96, Gc=128))
    cases.append(dict(base, graph="r255f65", row_set=1, splits=4, Gc=32, a0_shift=1))
    cases.append(dict(base, graph="r128f32", row_set=1, splits=2, Ka=192))
    cases.append(dict(base, graph="r73f97", row_set=2, splits=4, Ka=96, gplanes=3))
    # whole samples per chunk (slice arithmetics), B = 5: the last chunk is short; 1, 2, 3, 6 and 7 stages per sample
    neg = dict(base, B=5, sliced_only=True)
    cases.append(dict(neg, graph="r41f1", row_set=2, splits=-2))
    cases.append(dict(neg, graph="r47f17", row_set=2, splits=-2, Ka=96, Gc=128))
    cases.append(dict(neg, graph="r47f17", row_set=2, splits=-3, gplanes=3, a0_shift=1))
    cases.append(dict(neg, graph="r63f33", row_set=2, splits=-2, Ka=192, gplanes=3, compact=0))
    cases.append(dict(neg, graph="r63f33", row_set=2, splits=-3, Gc=32))
    cases.append(dict(neg, graph="r127f81", row_set=2, splits=-3, Ka=96))
    cases.append(dict(neg, graph="r217f103", row_set=2, splits=-2, Gc=128))
    # activation on load of A (slice arithmetics), the last stage partial
    cases.append(dict(base, graph="r49f15", row_set=2, Ka=96, a_act=True, sliced_only=True))
    cases.append(dict(base, graph="r129f31", row_set=1, Gc=128, a_act=True, sliced_only=True, splits=2))
    # the paired sets
    cases.append(dict(base, graph=PAIR_GRAPH, row_set=3, Ka=96, gplanes=3))
    cases.append(dict(base, graph=PAIR_GRAPH, row_set=3, Ka=32, gplanes=3, compact=0, splits=2))
    cases.append(dict(base, graph=PAIR_GRAPH, row_set=4, Gc=128))
    cases.append(dict(neg, graph=PAIR_GRAPH, row_set=4, splits=-3, Ka=192))
    return cases


PLANES_ROWS_CASES = _planes_rows_cases()
TN_ROWS_CASES = _tn_rows_cases()

# rows of a chunk of k_gemm_tn_ws: every stage count 1 .. 9, the remainders 0, 1, 15 and one each of 4 q + 1, 4 q + 2, 4 q + 3
TN_ROW_COUNTS = [1, 15, 16, 17, 33, 54, 73, 81, 103, 128, 129]

# flat p2m_gemm_planes: (M, Ka, planes, N, a0_shift, addend, act) - every pipeline depth at every width; M % 128 in {1, 127, 0, 44}
FLAT_PLANES_CASES = [((129, 255, 256, 300)[i % 4], Ka, pl, N, i % 2, bool((i // 2) % 2), None)
                     for i, (Ka, pl, N) in enumerate((Ka, pl, N) for Ka, pl in K_PIPE for N in FWD_N)] + \
                    [(129, 32, 1, 96, 0, False, "relu"), (300, 64, 3, 128, 0, False, "affine")]
# flat p2m_gemm_tn: (M, chunk_rows, Ka, planes, gplanes, Gc, a0_shift) - one chunk of r rows, then full chunks + a short one
FLAT_TN_CASES = [(r, -(-r // 32) * 32, (32, 32, 64)[i % 3], (1, 3, 3)[i % 3], GRAD_N[i % 4][0], GRAD_N[i % 4][1], i % 2)
                 for i, r in enumerate(TN_ROW_COUNTS)] + \
                [(3 * 64 + 17, 64, 32, 3, 1, 128, 0), (8 * 32 + 5, 32, 64, 1, 3, 64, 1), (2 * 96 + 33, 96, 64, 3, 1, 64, 0)]
# p2m_gemm_tn_acc: (M, Ka, N) - both tile widths
TN_ACC_CASES = [(M, Ka, N) for M in (32, 36, 100) for Ka, N in ((32, 64), (96, 128), (192, 32))]

# The contractions in PoseNet's role (pose2mesh_release_amd/posenet.py), where the BATCH is a tile dimension; the batches are
# those of tests/posenet_ref.py's stage cases.  Tables of their own: the ones above are read by the CPU mutation check.
# dW: p2m_gemm_tn_acc reduces the whole batch in one chunk: (M, Ka, N) - M = 128 .. 516 rows: 8 .. 33 stages of 16, 4 .. 17 of 32
PN_TN_ACC_CASES = [(M, Ka, N) for M in (128, 132, 260, 516) for Ka, N in ((32, 64), (96, 128))]
# forward and dX: p2m_gemm_tn with the batch as Ka, the rows of P - no multiple of 32, below, just past one and just past two
# K tiles of TILE rows: (M, chunk_rows, Ka, planes, gplanes, Gc, a0_shift), M = 256 reduced in 4 chunks of 64
PN_TN_CASES = [(256, 64, Ka, 1, 1, Gc, 0) for Ka in (36, 132, 260) for Gc in (64, 128)]


# ---- inputs (seeded, on the CPU: the GPU test and the mutation check use the same tensors) ------------------------------------

def planes_rows_inputs(case, index):
    """A planes, Bm, bias, addend, in_act, act of a case of PLANES_ROWS_CASES (randn; Bm randn / sqrt(Ktot))."""
    ids, V = set_rows(case["graph"], case["row_set"])
    n, B, Ka, N, pl = len(ids), case["B"], case["Ka"], case["N"], case["planes"]
    gen = torch.Generator().manual_seed(1000 + index)
    A = [torch.randn((B * V) >> case["a0_shift"], Ka, generator=gen)]
    A += [torch.randn(B * n if case["compact"] else B * V, Ka, generator=gen) for _ in range(pl - 1)]
    Bm = torch.randn(pl * Ka, N, generator=gen) / math.sqrt(pl * Ka)
    bias = torch.randn(N, generator=gen)
    addend = torch.randn(B * V, N, generator=gen) if case["addend"] else None
    in_act = act = None
    if case["in_act"]:           # shift > 0: act(0) != 0, a row that should be zero shows
        in_act = (torch.rand(Ka, generator=gen) + 0.5, 0.3 + 0.3 * torch.rand(Ka, generator=gen))
    if case["act"]:
        act = (torch.rand(N, generator=gen) + 0.5, 0.3 * torch.randn(N, generator=gen), case["act"] == "relu")
    return dict(A=A, Bm=Bm, bias=bias, addend=addend, in_act=in_act, act=act)


def tn_rows_inputs(case, index):
    """A, G planes, a_act of a case of TN_ROWS_CASES (randn)."""
    ids, V = set_rows(case["graph"], case["row_set"])
    n, B, Ka, Gc = len(ids), case["B"], case["Ka"], case["Gc"]
    gen = torch.Generator().manual_seed(2000 + index)
    A = torch.randn((B * V) >> case["a0_shift"], Ka, generator=gen)
    G = [torch.randn(B * V, Gc, generator=gen)]
    G += [torch.randn(B * n if case["compact"] else B * V, Gc, generator=gen) for _ in range(case["gplanes"] - 1)]
    a_act = None
    if case["a_act"]:
        a_act = (torch.rand(Ka, generator=gen) + 0.5, 0.3 + 0.3 * torch.rand(Ka, generator=gen))
    return dict(A=A, G=G, a_act=a_act)


def planes_rows_case_ref(case, inp, ids, V, **kw):
    return planes_rows_ref(ids, V, case["B"], inp["A"], case["a0_shift"], case["compact"], inp["Bm"], inp["bias"],
                           inp["addend"], inp["in_act"], inp["act"], **kw)


def tn_rows_case_ref(case, inp, ids, V, sliced, **kw):
    return tn_rows_ref(ids, V, case["B"], inp["A"], case["a0_shift"], inp["G"], case["compact"], inp["a_act"],
                       case["splits"], sliced, **kw)


def tn_rows_chunk_rows(case, sliced):
    """Rows reduced by every chunk of a case of TN_ROWS_CASES in the sliced (16-row stages) or the f32 (32-row stages) kernel;
    for chunks of whole samples: the rows per sample (each sample runs the pipeline once)."""
    n = len(set_rows(case["graph"], case["row_set"])[0])
    if case["splits"] < 0:
        return [n]
    return sorted({hi - lo for ch in tn_chunks(n, 1, case["splits"], sliced) for _, lo, hi in ch})
