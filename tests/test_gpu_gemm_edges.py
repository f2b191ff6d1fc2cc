"""-m gpu: the dense contractions of csrc/gemm_planes.hip (k_gemm_planes, k_gemm_planes_ws) and csrc/gemm_tn.hip (k_gemm_tn,
k_gemm_tn_ws), flat and row-set forms, in f32, bf16x3 and f16x2, at their row-count and pipeline edges, against the float64
restatements of tests/gemm_ref.py.

The cases are the tables of tests/gemm_ref.py (tests/test_gemm_ref_cpu.py audits what they reach: 1 .. 9 stages of 16 rows and
every tail of k_gemm_tn_ws, 1 .. 4 stages of 32 rows of k_gemm_tn, 2 .. 12 K chunks of the plane contractions, every tile width,
slices of a sample's rows with empty trailing slices, chunks of whole samples with a short last chunk, row sets 1 .. 4).  The
kernels are called through the C ABI, so chunk_rows and splits are the test's choice.  Per case:
  values      against float64 with the bounds tests/test_gpu_ops.py uses for these input distributions (gemm_ref.tol_*), per
              chunk for the gradients; an empty chunk must be exactly zero;
  poison      every row of A, G and the addend that the row set does not name holds 1e30 / inf / NaN: the results are finite and
              bitwise those of the clean run (f16x2: the amax words are taken from compact copies of the set's rows and passed in);
  sentinel    C, P and Pdb are prefilled with a NaN bit pattern: rows of C outside the set keep it, everything else is written.
Every achieved figure is printed before it is asserted (pytest -rP), the worst per test last."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as gr

pytestmark = pytest.mark.gpu

CODE = {"f32": 0, "bf16x3": 1, "f16x2": 2}
SENTINEL = 0x7FC0BEEF              # a quiet NaN with a payload: untouched memory is recognised bit for bit


@pytest.fixture(scope="module")
def ops(hip_libs):
    from pose2mesh_release_amd import ops as o
    return o


@pytest.fixture(params=list(CODE))
def arith(request):
    return request.param


# ---- plumbing ------------------------------------------------------------------------------------------------------------------

def _hip():
    from pose2mesh_release_amd import _lib
    return _lib.hip()


def _ck(rc, what):
    from pose2mesh_release_amd._lib import check
    check(rc, what)


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cu(t):
    return None if t is None else t.cuda().contiguous()


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


_PAT = None


def _poison(t2d, rows):
    """Fill the rows `rows` of the 2-D tensor with a mix of 1e30, inf and NaN of both signs (tests/test_gpu_amax.py)."""
    global _PAT
    if _PAT is None:
        _PAT = torch.tensor([1e30, float("inf"), float("nan"), -1e30, -float("inf")], device="cuda")
    n, F = rows.numel(), t2d.shape[1]
    if n:
        t2d[rows] = _PAT[torch.arange(n * F, device="cuda") % 5].view(n, F)
    return t2d


def _complement(rows, total):
    keep = torch.ones(total, dtype=torch.bool, device="cuda")
    keep[rows] = False
    return torch.nonzero(keep).reshape(-1)


def _split(Bm, arith):
    """p2m_weight_split image of Bm for the slice arithmetics (its own maximum as the f16x2 bound)."""
    if arith == "f32":
        return None
    K, N = Bm.shape
    Bx = torch.empty(int(_hip().p2m_weight_split_elems(K, N, CODE[arith])), dtype=torch.int16, device="cuda")
    _ck(_hip().p2m_weight_split(_vp(Bm), K, N, CODE[arith], None, 0, _vp(Bx), _st()), "p2m_weight_split")
    return Bx


def _word(arith, *tensors, act=None):
    """f16x2: one amax word over compact copies (p2m_amax of each); act = (scale, shift): the first tensor is a raw operand that
    is activated on load - its bound comes from p2m_act_bound, as in the network."""
    if arith != "f16x2":
        return None
    w = torch.zeros(1, dtype=torch.int32, device="cuda")
    for i, t in enumerate(tensors):
        t = t.contiguous()
        if i == 0 and act is not None:
            wy = torch.zeros(1, dtype=torch.int32, device="cuda")
            _ck(_hip().p2m_amax(_vp(t), t.numel(), _vp(wy), _st()), "p2m_amax")
            _ck(_hip().p2m_act_bound(_vp(act[0]), _vp(act[1]), act[0].numel(), _vp(wy), _vp(w), _st()), "p2m_act_bound")
        else:
            _ck(_hip().p2m_amax(_vp(t), t.numel(), _vp(w), _st()), "p2m_amax")
    return w


class _Worst:
    """Prints every figure with its bound, keeps the worst ratio per kind, asserts at the end of a case (all figures of a
    failing case are printed first)."""

    def __init__(self, title):
        self.title, self.worst, self.failed = title, {}, []

    def chk(self, kind, what, err, tol):
        err, tol = float(err), float(tol)
        print(f"    {what}: {kind} err {err:.3e}  bound {tol:.3e}")
        ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
        if kind not in self.worst or ratio > self.worst[kind][0]:
            self.worst[kind] = (ratio, err, tol, what)
        if not err <= tol:
            self.failed.append((kind, what, err, tol))

    def done(self):
        for kind, (ratio, err, tol, what) in self.worst.items():
            print(f"  WORST {self.title} {kind}: err {err:.3e} = {ratio:.3f} of its bound {tol:.3e} ({what})")
        assert not self.failed, self.failed


_graphs = {}


def _dev_graph(ops, name):
    """(device graph, {row set: ids}) of a graph of the table, once per process; the library's id lists are the restated ones."""
    if name not in _graphs:
        L, V, ids = gr.graph_ids(name)
        g = ops.DeviceGraph(L, "cuda:0")
        assert g.V == V and np.array_equal(g.real_ids_host(), ids[1]) and np.array_equal(g.fake_ids_host(), ids[2])
        if 3 in ids:
            assert (g.n_pair_real, g.n_pair_fake) == (len(ids[3]), len(ids[4]))
        _graphs[name] = (g, ids)
    return _graphs[name]


# ---- the row-set forms ------------------------------------------------------------------------------------------------------------

def _run_planes_rows(g, case, arith, A, Bm, Bx, word, bias, addend, in_act, act):
    B, N, n = case["B"], case["N"], g.set_size(case["row_set"])
    V = g.V // 2 if case["row_set"] >= 3 else g.V
    C = _sentinel(B * V, N)
    tps = int(_hip().p2m_rows_tiles_per_sample(g.handle, case["row_set"]))
    assert tps == -(-n // gr.TILE)
    st = _sentinel(B * tps, 2, N) if case["stats"] else None
    a = [_vp(t) for t in A] + [None] * (3 - len(A))
    _ck(_hip().p2m_gemm_planes_rows(g.handle, case["row_set"], B, a[0], a[1], a[2], len(A), case["Ka"], case["a0_shift"],
                                    case["compact"], _vp(Bm), _vp(Bx), CODE[arith], _vp(word), 0, _vp(bias), _vp(addend),
                                    _vp(C), N, _vp(st), _vp(act[0]) if act else None, _vp(act[1]) if act else None,
                                    int(bool(act and act[2])), None, _vp(in_act[0]) if in_act else None,
                                    _vp(in_act[1]) if in_act else None, _st()), "p2m_gemm_planes_rows")
    torch.cuda.synchronize()
    return C, st


def test_planes_rows_edges(ops, arith):
    """p2m_gemm_planes_rows (k_gemm_planes<., 32, ., true> / k_gemm_planes_ws<., ., true, 3 | 2>) over PLANES_ROWS_CASES."""
    worst = _Worst(f"gemm_planes_rows {arith}")
    ran = []
    for index, case in enumerate(gr.PLANES_ROWS_CASES):
        if case["sliced_only"] and arith == "f32":
            continue
        g, idsets = _dev_graph(ops, case["graph"])
        ids, V = gr.set_rows(case["graph"], case["row_set"])
        assert np.array_equal(ids, idsets[case["row_set"]]) and g.set_size(case["row_set"]) == len(ids)
        n, B, sh = len(ids), case["B"], case["a0_shift"]
        what = (f"case {index} {case['graph']} set {case['row_set']}: {n} rows x B {B}, Ka {case['Ka']} x {case['planes']}, "
                f"N {case['N']}, shift {sh}, compact {case['compact']}")
        print("  " + what)
        ran.append(n)
        inp = gr.planes_rows_inputs(case, index)
        A = [_cu(t) for t in inp["A"]]
        Bm, bias, addend = _cu(inp["Bm"]), _cu(inp["bias"]), _cu(inp["addend"])
        in_act = tuple(_cu(t) for t in inp["in_act"]) if inp["in_act"] else None
        act = (_cu(inp["act"][0]), _cu(inp["act"][1]), inp["act"][2]) if inp["act"] else None
        rows, Yref, stref = gr.planes_rows_ref(ids, V, B, A, sh, case["compact"], Bm, bias, addend, in_act, act)
        comp_rows = [A[0][rows >> sh]] + [p if case["compact"] else p[rows] for p in A[1:]]
        word = _word(arith, *comp_rows, act=in_act)
        Bx = _split(Bm, arith)
        C, st = _run_planes_rows(g, case, arith, A, Bm, Bx, word, bias, addend, in_act, act)
        worst.chk("value", what, (C[rows].double() - Yref).abs().max(), gr.tol_fwd(Yref))
        outside = _complement(rows, B * V)
        assert bool((_bits(C[outside]) == SENTINEL).all()), ("a row outside the row set was written", what)
        if st is not None:
            worst.chk("stat sum", what, (st[:, 0].double() - stref[:, 0]).abs().max(), gr.TOL_STAT_SUM)
            worst.chk("stat M2", what, (st[:, 1].double() - stref[:, 1]).abs().max(), gr.TOL_STAT_M2)
        # poison: plane 0 at the coarse rows none of whose children is in the set, the other planes / the addend outside the set
        Ap = [t.clone() for t in A]
        _poison(Ap[0], _complement(rows >> sh, Ap[0].shape[0]))
        if not case["compact"]:
            for p in Ap[1:]:
                _poison(p, outside)
        addp = None if addend is None else _poison(addend.clone(), outside)
        Cp, stp = _run_planes_rows(g, case, arith, Ap, Bm, Bx, word, bias, addp, in_act, act)
        assert bool(torch.isfinite(Cp[rows]).all()), ("poison reached C", what)
        assert torch.equal(_bits(Cp), _bits(C)), ("C differs with the other rows poisoned", what)
        if st is not None:
            assert bool(torch.isfinite(stp).all()) and torch.equal(_bits(stp), _bits(st)), ("statistics and poison", what)
        if worst.failed:
            worst.done()
    print(f"  rows per sample run: {sorted(set(ran))}; tiles per sample {sorted({-(-r // 128) for r in ran})}")
    worst.done()


def _run_tn_rows(g, case, arith, A, G, wa, wg, a_act, nch):
    Ka, N = case["Ka"], case["gplanes"] * case["Gc"]
    P, Pdb = _sentinel(nch, Ka, N), _sentinel(nch, N)
    gp = [_vp(t) for t in G] + [None] * (3 - len(G))
    _ck(_hip().p2m_gemm_tn_rows(g.handle, case["row_set"], case["B"], _vp(A), Ka, case["a0_shift"], gp[0], gp[1], gp[2], len(G),
                                case["Gc"], case["compact"], case["splits"], _vp(P), _vp(Pdb), CODE[arith], _vp(wa), _vp(wg), 0,
                                _vp(a_act[0]) if a_act else None, _vp(a_act[1]) if a_act else None, _st()), "p2m_gemm_tn_rows")
    torch.cuda.synchronize()
    return P, Pdb


def test_tn_rows_edges(ops, arith):
    """p2m_gemm_tn_rows (k_gemm_tn<., true> / k_gemm_tn_ws<., true, 3 | 2>) over TN_ROWS_CASES: every chunk against float64."""
    worst = _Worst(f"gemm_tn_rows {arith}")
    sliced = arith != "f32"
    stage = gr.TN_STAGE_SLICED if sliced else gr.TN_STAGE_F32
    ran, empties = set(), 0
    for index, case in enumerate(gr.TN_ROWS_CASES):
        if case["sliced_only"] and not sliced:
            continue
        g, idsets = _dev_graph(ops, case["graph"])
        ids, V = gr.set_rows(case["graph"], case["row_set"])
        assert np.array_equal(ids, idsets[case["row_set"]]) and g.set_size(case["row_set"]) == len(ids)
        n, B, sh, S = len(ids), case["B"], case["a0_shift"], case["splits"]
        what = (f"case {index} {case['graph']} set {case['row_set']}: {n} rows x B {B}, Ka {case['Ka']}, G {case['gplanes']} x "
                f"{case['Gc']}, shift {sh}, compact {case['compact']}, splits {S}")
        print("  " + what)
        inp = gr.tn_rows_inputs(case, index)
        A, G = _cu(inp["A"]), [_cu(t) for t in inp["G"]]
        a_act = tuple(_cu(t) for t in inp["a_act"]) if inp["a_act"] else None
        Pt, Pdbt, Pref, Pdbref, nrows = gr.tn_rows_ref(ids, V, B, A, sh, G, case["compact"], a_act, S, sliced)
        nch = len(nrows)
        assert nch == (B * S if S >= 1 else -(-B // -S))
        ran |= set(gr.tn_rows_chunk_rows(case, sliced))
        rows = gr.logical_rows(ids, V, B, "cuda")
        wa = _word(arith, A[rows >> sh], act=a_act)
        wg = _word(arith, G[0][rows], *[p if case["compact"] else p[rows] for p in G[1:]])
        P, Pdb = _run_tn_rows(g, case, arith, A, G, wa, wg, a_act, nch)
        for c in range(nch):
            tag = f"{what}, chunk {c} ({nrows[c]} rows)"
            if nrows[c] == 0:
                empties += 1
                assert bool((P[c] == 0).all()) and bool((Pdb[c] == 0).all()), ("an empty chunk is not zero", tag)
            worst.chk("P", tag, (P[c].double() - Pref[c]).abs().max(), gr.tol_grad(Pref[c], nrows[c]))
            worst.chk("Pdb", tag, (Pdb[c].double() - Pdbref[c]).abs().max(), gr.tol_pdb(nrows[c]))
        worst.chk("P", what + ", all chunks", (P.double().sum(0) - Pt).abs().max(), gr.tol_grad(Pt, B * n))
        worst.chk("Pdb", what + ", all chunks", (Pdb.double().sum(0) - Pdbt).abs().max(), gr.tol_pdb(B * n))
        outside = _complement(rows, B * V)
        Ap = _poison(A.clone(), _complement(rows >> sh, A.shape[0]))
        Gp = [_poison(G[0].clone(), outside)] + [p if case["compact"] else _poison(p.clone(), outside) for p in G[1:]]
        Pp, Pdbp = _run_tn_rows(g, case, arith, Ap, Gp, wa, wg, a_act, nch)
        assert bool(torch.isfinite(Pp).all()) and bool(torch.isfinite(Pdbp).all()), ("poison reached P", what)
        assert torch.equal(_bits(Pp), _bits(P)) and torch.equal(_bits(Pdbp), _bits(Pdb)), ("P differs with poison", what)
        if worst.failed:
            worst.done()
    ran.discard(0)
    print(f"  rows per chunk run: {sorted(ran)}; stages of {stage} rows: {sorted({-(-r // stage) for r in ran})}; "
          f"{empties} empty chunks")
    assert empties > 0
    worst.done()


# ---- the flat forms ---------------------------------------------------------------------------------------------------------------

def test_gemm_planes_flat(arith, hip_libs):
    """p2m_gemm_planes (k_gemm_planes<., 32, ., false> / k_gemm_planes_ws<., ., false, .>): 2 .. 12 K chunks at every tile width,
    M % 128 in {0, 1, 127, 44}, with the statistics; two cases with the activation in the epilogue."""
    worst = _Worst(f"gemm_planes {arith}")
    for index, (M, Ka, pl, N, sh, with_add, act_kind) in enumerate(gr.FLAT_PLANES_CASES):
        what = f"case {index}: M {M}, Ka {Ka} x {pl}, N {N}, shift {sh}, addend {with_add}, act {act_kind}"
        print("  " + what)
        gen = torch.Generator().manual_seed(3000 + index)
        A = [torch.randn((M + 1) >> sh if q == 0 else M, Ka, generator=gen).cuda() for q in range(pl)]
        Bm = (torch.randn(pl * Ka, N, generator=gen) / (pl * Ka) ** 0.5).cuda()
        bias = torch.randn(N, generator=gen).cuda()
        addend = torch.randn(M, N, generator=gen).cuda() if with_add else None
        act = None
        if act_kind:
            act = ((torch.rand(N, generator=gen) + 0.5).cuda(), (0.3 * torch.randn(N, generator=gen)).cuda(), act_kind == "relu")
        Yref, stref = gr.gemm_planes_ref(A, sh, Bm, M, bias, addend, act)
        C = _sentinel(M, N)
        st = None if act else _sentinel(-(-M // gr.TILE), 2, N)
        a = [_vp(t) for t in A] + [None] * (3 - pl)
        _ck(_hip().p2m_gemm_planes(a[0], a[1], a[2], pl, Ka, sh, _vp(Bm), _vp(_split(Bm, arith)), CODE[arith],
                                   _vp(_word(arith, *A)), 0, _vp(bias), _vp(addend), _vp(C), None, None, 1, N, 0, M, _vp(st),
                                   _vp(act[0]) if act else None, _vp(act[1]) if act else None, int(bool(act and act[2])), None,
                                   _st()), "p2m_gemm_planes")
        torch.cuda.synchronize()
        worst.chk("value", what, (C.double() - Yref).abs().max(), gr.tol_fwd(Yref))
        if st is not None:
            worst.chk("stat sum", what, (st[:, 0].double() - stref[:, 0]).abs().max(), gr.TOL_STAT_SUM)
            worst.chk("stat M2", what, (st[:, 1].double() - stref[:, 1]).abs().max(), gr.TOL_STAT_M2)
    worst.done()


def _tn_flat(arith, A, Ka, sh, G, Gc, M, chunk_rows, nch):
    Ktot, N = len(A) * Ka, len(G) * Gc
    P, Pdb = _sentinel(nch, Ktot, N), _sentinel(nch, N)
    a = [_vp(t) for t in A] + [None] * (3 - len(A))
    gp = [_vp(t) for t in G] + [None] * (3 - len(G))
    _ck(_hip().p2m_gemm_tn(a[0], a[1], a[2], len(A), Ka, sh, gp[0], gp[1], gp[2], len(G), Gc, M, chunk_rows, _vp(P), _vp(Pdb),
                           CODE[arith], _vp(_word(arith, *A)), 0, _vp(_word(arith, *G)), 0, _st()), "p2m_gemm_tn")
    torch.cuda.synchronize()
    return P, Pdb


def test_gemm_tn_flat(arith, hip_libs):
    """p2m_gemm_tn with an explicit chunk_rows: one chunk of r rows (chunk_rows = r rounded up to 32) for r over TN_ROW_COUNTS,
    then full chunks and a short last one (9 chunks: the XCD-aware block mapping of k_gemm_tn_ws)."""
    worst = _Worst(f"gemm_tn {arith}")
    for index, (M, cr, Ka, pl, gpl, Gc, sh) in enumerate(gr.FLAT_TN_CASES):
        what = f"case {index}: M {M}, chunk_rows {cr}, Ka {Ka} x {pl}, G {gpl} x {Gc}, shift {sh}"
        print("  " + what)
        gen = torch.Generator().manual_seed(4000 + index)
        A = [torch.randn((M + 1) >> sh if q == 0 else M, Ka, generator=gen).cuda() for q in range(pl)]
        G = [torch.randn(M, Gc, generator=gen).cuda() for _ in range(gpl)]
        Pref, Pdbref, nrows = gr.gemm_tn_ref(A, sh, G, M, cr)
        P, Pdb = _tn_flat(arith, A, Ka, sh, G, Gc, M, cr, len(nrows))
        for c, r in enumerate(nrows):
            worst.chk("P", f"{what}, chunk {c} ({r} rows)", (P[c].double() - Pref[c]).abs().max(), gr.tol_grad(Pref[c], r))
            worst.chk("Pdb", f"{what}, chunk {c} ({r} rows)", (Pdb[c].double() - Pdbref[c]).abs().max(), gr.tol_pdb(r))
    worst.done()


def test_gemm_tn_acc(arith, hip_libs):
    """p2m_gemm_tn_acc, P += A^T G over M in {32, 36, 100} rows in one chunk, both tile widths: P prefilled with 0.25."""
    worst = _Worst(f"gemm_tn_acc {arith}")
    for index, (M, Ka, N) in enumerate(gr.TN_ACC_CASES):
        what = f"case {index}: M {M}, Ka {Ka}, N {N}"
        gen = torch.Generator().manual_seed(5000 + index)
        A, G = torch.randn(M, Ka, generator=gen).cuda(), torch.randn(M, N, generator=gen).cuda()
        P = torch.full((Ka, N), 0.25, device="cuda")
        ref = gr.gemm_tn_acc_ref(A, G, P) - 0.25
        _ck(_hip().p2m_gemm_tn_acc(_vp(A), Ka, _vp(G), N, M, _vp(P), CODE[arith], _vp(_word(arith, A)), _vp(_word(arith, G)),
                                   _st()), "p2m_gemm_tn_acc")
        torch.cuda.synchronize()
        worst.chk("P", what, ((P.double() - 0.25) - ref).abs().max(), gr.tol_grad(ref, M))
    worst.done()


# ---- the contractions in PoseNet's role: the batch as a tile dimension ---------------------------------------------------------

def test_gemm_tn_acc_posenet_batches(arith, hip_libs):
    """p2m_gemm_tn_acc as PoseNet's dW (pose2mesh_release_amd/posenet.py: dW += g_z^T a): the WHOLE batch reduced in one chunk,
    M in {128, 132, 260, 516} rows - 8 .. 33 stages of 16 rows (4 .. 17 of 32 in f32), with a 4-row tail at 132, 260 and 516 -
    at both tile widths; P prefilled with 0.25."""
    worst = _Worst(f"gemm_tn_acc (PoseNet batches) {arith}")
    for index, (M, Ka, N) in enumerate(gr.PN_TN_ACC_CASES):
        what = f"case {index}: M {M}, Ka {Ka}, N {N}"
        gen = torch.Generator().manual_seed(6000 + index)
        A, G = torch.randn(M, Ka, generator=gen).cuda(), torch.randn(M, N, generator=gen).cuda()
        P = torch.full((Ka, N), 0.25, device="cuda")
        ref = gr.gemm_tn_acc_ref(A, G, P) - 0.25
        _ck(_hip().p2m_gemm_tn_acc(_vp(A), Ka, _vp(G), N, M, _vp(P), CODE[arith], _vp(_word(arith, A)), _vp(_word(arith, G)),
                                   _st()), "p2m_gemm_tn_acc")
        torch.cuda.synchronize()
        worst.chk("P", what, ((P.double() - 0.25) - ref).abs().max(), gr.tol_grad(ref, M))
    worst.done()


def test_gemm_tn_posenet_batches(arith, hip_libs):
    """p2m_gemm_tn as PoseNet's forward and dX, where the batch is Ka - the ROWS of P: Ka in {36, 132, 260}, no multiple of 32,
    below, 4 rows past one and 4 rows past two K tiles of p2m_stats_tile_rows() rows; one A plane, one G plane of 64 or 128
    columns, M = 256 reduced in 4 chunks of 64.  P and Pdb lie in sentinel-filled buffers and are wholly written; per chunk and
    summed over the chunks (what the stage kernels then add up) against float64."""
    assert int(_hip().p2m_stats_tile_rows()) == gr.TILE
    assert [(Ka % 32 != 0, -(-Ka // gr.TILE), Ka % gr.TILE) for Ka in sorted({c[2] for c in gr.PN_TN_CASES})] == \
        [(True, 1, 36), (True, 2, 4), (True, 3, 4)]
    worst = _Worst(f"gemm_tn (PoseNet batches) {arith}")
    for index, (M, cr, Ka, pl, gpl, Gc, sh) in enumerate(gr.PN_TN_CASES):
        what = f"case {index}: M {M}, chunk_rows {cr}, Ka {Ka} x {pl}, G {gpl} x {Gc}, shift {sh}"
        print("  " + what)
        gen = torch.Generator().manual_seed(7000 + index)
        A = [torch.randn((M + 1) >> sh if q == 0 else M, Ka, generator=gen).cuda() for q in range(pl)]
        G = [torch.randn(M, Gc, generator=gen).cuda() for _ in range(gpl)]
        Pref, Pdbref, nrows = gr.gemm_tn_ref(A, sh, G, M, cr)
        assert nrows == [64] * 4
        P, Pdb = _tn_flat(arith, A, Ka, sh, G, Gc, M, cr, len(nrows))
        assert not (_bits(P) == SENTINEL).any() and not (_bits(Pdb) == SENTINEL).any(), what
        for c, r in enumerate(nrows):
            worst.chk("P", f"{what}, chunk {c} ({r} rows)", (P[c].double() - Pref[c]).abs().max(), gr.tol_grad(Pref[c], r))
            worst.chk("Pdb", f"{what}, chunk {c} ({r} rows)", (Pdb[c].double() - Pdbref[c]).abs().max(), gr.tol_pdb(r))
        worst.chk("P", f"{what}, summed", (P.double().sum(0) - Pref.sum(0)).abs().max(), gr.tol_grad(Pref.sum(0), M))
        worst.chk("Pdb", f"{what}, summed", (Pdb.double().sum(0) - Pdbref.sum(0)).abs().max(), gr.tol_pdb(M))
    worst.done()
