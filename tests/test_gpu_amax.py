"""-m gpu: the arithmetic contract of the default mode (P2M_ARITH_F16X2, include/p2m.h): every operand tensor is scaled by a
power of two taken from an AMAX WORD that must bound max |x| over the rows its consumer reads, with about one binade of margin.
A word that is a little too small is silent on Gaussian data, so every producer of a word is pinned here on data whose maximum
is PLANTED where a kernel most easily misses it (tail rows, the last partial tile, the last sample of a sample group, a
representative, a lane past the end), and on tensors whose no-data rows are POISONED (1e30, inf, NaN).

  1. test_word_*       every producer: word == max |finite value stored| over the rows the contract names, bit for bit
  2. test_headroom_*   p2m_graph_plane_bits, eff_bits, and operands that reach their bound (no overflow of the fp16 slices)
  3. test_conv_weights_prepare_*   the four slice images of p2m_conv_weights_prepare == weight_pack -> (weight_eff) -> weight_split
  4. test_tag_*        the tag plumbing of ops.py (stale tags, views, row sets)
  5. test_graph_conv_cheby_outliers   one conv, forward + backward, with one element 256 times too large, against float64
  6. test_pn_stage_*   the PoseNet stages on small shapes against a float64 restatement, padding rows poisoned

The exact maximum is computed with torch in float32 from the tensor the kernel itself stored (self-consistency: the values are
checked against float64 in the other test files and in 5. and 6.).  Every figure is printed before it is asserted
(pytest -s / -rP)."""
import ctypes

import numpy as np
import pytest
import torch

import posenet_ref as pnr
import tile_plan_ref as tp

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
CODE = {"bf16x3": 1, "f16x2": 2}


@pytest.fixture(scope="module")
def ops(hip_libs):
    from pose2mesh_release_amd import ops as o
    return o


# ---- plumbing ----------------------------------------------------------------------------------------------------------------

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


def _zero_word():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _word(w):
    """Reading a word: synchronise, then the float whose bits it holds."""
    torch.cuda.synchronize()
    return float(w.view(torch.float32))


def _exact(t):
    """max |finite entries| of t, in float32 (0 for none)."""
    a = t.detach().float().abs().reshape(-1)
    a = a[torch.isfinite(a)]
    return float(a.max()) if a.numel() else 0.0


def _chk(what, err, tol):
    err, tol = float(err), float(tol)
    print(f"    {what}: err {err:.3e}  bound {tol:.3e}")
    assert err <= tol, (what, err, tol)


def _same(what, word, exact):
    print(f"    {what}: word {word!r}  stored max {exact!r}")
    assert word == exact, (what, word, exact)


def _unchanged(what, word, clean):
    print(f"    {what}: word {word!r}  without the poison {clean!r}")
    assert word == clean, (what, word, clean)


def _finite_abs(t):
    return torch.nan_to_num(t.detach().float().abs(), nan=0.0, posinf=0.0, neginf=0.0)


def _argmax(t2d):
    """(row, column) of the largest finite magnitude of a 2-D tensor."""
    return divmod(int(_finite_abs(t2d).argmax()), t2d.shape[-1])


_PAT = None


def _poison(t2d, rows):
    """Fill the rows `rows` (index tensor / array) of the 2-D tensor with a mix of 1e30, inf and NaN of both signs."""
    global _PAT
    if _PAT is None:
        _PAT = torch.tensor([1e30, INF, NAN, -1e30, -INF], device="cuda")
    rows = torch.as_tensor(rows if torch.is_tensor(rows) else np.asarray(rows), device="cuda", dtype=torch.long)
    n, F = rows.numel(), t2d.shape[1]
    if n:
        t2d[rows] = _PAT[torch.arange(n * F, device="cuda") % 5].view(n, F)
    return t2d


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _all_rows(B, V, ids):
    """b * V + ids over all samples, as a device index tensor."""
    ids = torch.as_tensor(np.asarray(ids, dtype=np.int64), device="cuda")
    return (torch.arange(B, device="cuda")[:, None] * V + ids[None, :]).reshape(-1)


_graphs = {}


def _fam(ops, name):
    """(L, restated plans, device graph, dense float64 L on the device) of a tile_plan_ref family, once per process."""
    if name not in _graphs:
        L, p = tp.family(name)
        _graphs[name] = (L, p, ops.DeviceGraph(L, "cuda:0"), torch.from_numpy(tp.dense(L)).cuda())
    return _graphs[name]


class _Band:
    """tp.band(V, seed) on the device, optionally with the classes of depth 1 declared: real / fake / live / hole vertex lists."""

    def __init__(self, ops, V, seed, classes):
        self.L = tp.band(V, seed)
        g = self.g = ops.DeviceGraph(self.L, "cuda:0")
        self.V = g.V
        self.real = g.real_ids_host().astype(np.int64)
        self.fake_all = np.sort(g.fake_ids_host().astype(np.int64))
        self.fake_mask = np.zeros(g.V, dtype=bool)
        self.fake_mask[self.fake_all] = True
        if classes:
            rep, _ = ops.class_representatives(g.V, self.fake_all, 1)
            g.set_classes(rep)
            assert g.classes
        self.fake = g.fake_ids_host().astype(np.int64)               # the representatives once classes are declared
        self.live = np.sort(np.concatenate((self.real, self.fake)))
        self.holes = np.setdiff1d(np.arange(g.V), self.live)
        assert (self.holes.size > 0) == bool(classes)


def _band(ops, V, seed, classes):
    key = ("band", V, seed, classes)
    if key not in _graphs:
        _graphs[key] = _Band(ops, V, seed, classes)
    return _graphs[key]


# ---- 1. every producer's word ----------------------------------------------------------------------------------------------------

def _amax(x, n, w):
    _ck(_hip().p2m_amax(_vp(x), int(n), _vp(w), _st()), "p2m_amax")
    return w


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4 * 1024 * 3 + 7, 4 * 2 ** 20 + 5])
def test_word_amax(hip_libs, n):
    """p2m_amax (k_amax: scalar head up to the 16-byte boundary, float4 body - the last size reaches the 1024-block
    grid-stride loop with its 4-way unroll -, scalar tail), through views 0 .. 3 floats off a 16-byte boundary; +-50 planted
    at index 0, the last head element, the first aligned element, either side of the tail's start and the last element."""
    base = torch.randn(n + 8, generator=torch.Generator().manual_seed(n)).cuda()
    assert base.data_ptr() % 16 == 0
    for off in range(4):
        x = base[off:off + n]
        head = min((4 - off) % 4, n)
        tail = (n - head) % 4
        print(f"  n {n} offset {off}: head {head} tail {tail}")
        _same("as drawn", _word(_amax(x, n, _zero_word())), _exact(x))
        for p in sorted({q for q in (0, head - 1, head, n - tail - 1, n - tail, n - 1) if 0 <= q < n}):
            old = x[p].clone()
            x[p] = -50.0 if p % 2 else 50.0
            assert int(x.abs().argmax()) == p
            _same(f"planted at {p}", _word(_amax(x, n, _zero_word())), 50.0)
            x[p] = old


def test_word_amax_accumulates_and_skips(hip_libs):
    """Two calls into one word keep the larger value, n = 0 leaves the word alone, an all-zero tensor leaves it 0, NaN and
    infinity do not enter."""
    gen = torch.Generator().manual_seed(1)
    a, b = torch.randn(1001, generator=gen).cuda(), (3 * torch.randn(777, generator=gen)).cuda()
    for first, second in ((a, b), (b, a)):
        w = _zero_word()
        _amax(first, first.numel(), w)
        _amax(second, second.numel(), w)
        _same("two calls", _word(w), max(_exact(a), _exact(b)))
    w = torch.tensor([3.0]).view(torch.int32).cuda()
    _amax(a, 0, w)
    _same("n = 0", _word(w), 3.0)
    w = _zero_word()
    _amax(torch.zeros(4099, device="cuda"), 4099, w)
    torch.cuda.synchronize()
    assert int(w) == 0
    c = a.clone()
    c[0], c[5], c[1000] = NAN, INF, -INF
    _same("NaN / inf left out", _word(_amax(c, c.numel(), _zero_word())), _exact(c))
    assert _exact(c) < 10.0


def _amax_rows(g, row_set, x, B, F):
    w = _zero_word()
    _ck(_hip().p2m_amax_rows(g.handle, row_set, _vp(x), B, F, _vp(w), _st()), "p2m_amax_rows")
    return w


def _rows_word_case(what, g, row_set, B, R, F, ids, seed):
    """x [B, R, F]: the word over the rows `ids` of every sample - with the complement poisoned - equals the exact maximum,
    bitwise what it is without the poison; +-50 planted at the last entry of the last sample and the first of sample 0."""
    ids = np.asarray(ids, dtype=np.int64)
    comp = np.setdiff1d(np.arange(R), ids)
    x = torch.randn(B, R, F, generator=torch.Generator().manual_seed(seed)).cuda()
    print(f"  {what}: row set {row_set}, {ids.size} of {R} rows, B {B} F {F}")
    clean = _word(_amax_rows(g, row_set, x, B, F))
    xp = x.clone()
    _poison(xp.view(B * R, F), _all_rows(B, R, comp))
    idx = torch.as_tensor(ids, device="cuda")
    got = _word(_amax_rows(g, row_set, xp, B, F))
    _same("complement poisoned", got, _exact(xp[:, idx]))
    _unchanged("complement poisoned", got, clean)
    for b, i, c, val in ((B - 1, ids.size - 1, F - 1, -50.0), (0, 0, 0, 50.0)):
        xq = xp.clone()
        xq[b, ids[i], c] = val
        sel = xq[:, idx].reshape(-1, F)
        assert _argmax(sel) == (b * ids.size + i, c)
        _same(f"planted at sample {b} vertex {ids[i]} column {c}", _word(_amax_rows(g, row_set, xq, B, F)), 50.0)
    xq = xp.clone()
    xq[0, ids[0], 0], xq[B - 1, ids[-1], F - 1] = NAN, INF
    _same("NaN / inf inside the data rows", _word(_amax_rows(g, row_set, xq, B, F)), _exact(xq[:, idx]))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("F", [4, 64])
@pytest.mark.parametrize("classes", [False, True])
def test_word_amax_rows(ops, classes, F, B):
    """p2m_amax_rows, row sets 0 (every row / the live rows under classes), 1 (real) and 2 (fake / the representatives) of
    band(736); without classes also 3 / 4 (a child is real / both children fake) over the V/2 rows of band(1472)."""
    bd = _band(ops, 736, 11, classes)
    for rs, ids in ((0, bd.live), (1, bd.real), (2, bd.fake)):
        _rows_word_case("band(736)" + (" with classes" if classes else ""), bd.g, rs, B, bd.V, F, ids, 100 * rs + F + B)
    if not classes:
        bp = _band(ops, 1472, 5, False)
        assert bp.g.n_pair_real > 0
        both = bp.fake_mask[0::2] & bp.fake_mask[1::2]
        for rs, ids in ((3, np.where(~both)[0]), (4, np.where(both)[0])):
            assert ids.size == bp.g.set_size(rs) and ids.size > 0
            _rows_word_case("band(1472), coarse rows", bp.g, rs, B, bp.V // 2, F, ids, 100 * rs + F + B)


def _gemm_planes(ops, arith, A, Ka, Bm, M, N, bias=None, addend=None, act=None, pair_out=False):
    """p2m_gemm_planes, one output plane, with an amax_out word in either slice arithmetic: (C, word)."""
    Bx = ops.weight_split(Bm)
    a_amax = ops._amax_planes(A) if arith == "f16x2" else None
    C = torch.zeros((M >> 1 if pair_out else M, N), device="cuda")
    w = _zero_word()
    a = [_vp(t) for t in A] + [None] * (3 - len(A))
    _ck(_hip().p2m_gemm_planes(a[0], a[1], a[2], len(A), Ka, 0, _vp(Bm), _vp(Bx), CODE[arith], _vp(a_amax), 0, _vp(bias),
                               _vp(addend), _vp(C), None, None, 1, N, int(pair_out), M, None,
                               _vp(None if act is None else act[0]), _vp(None if act is None else act[1]),
                               int(bool(act and act[2])), _vp(w), _st()), "p2m_gemm_planes")
    return C, w


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("M,Ka,N", [(640, 64, 128), (641, 32, 32), (130, 96, 64), (1, 32, 256)])
def test_word_gemm_planes(ops, monkeypatch, arith, M, Ka, N):
    """amax_out of p2m_gemm_planes (M % 128 in {0, 1, 2}): plain, bias, addend, fused activation with and without ReLU, pair_out
    (the word is the maximum of the pair sums stored); the input row 0, M - 1, 127, 128 scaled by 64 in turn."""
    monkeypatch.setattr(ops, "GEMM_ARITH", arith)
    gen = torch.Generator().manual_seed(M + Ka + N)
    A = torch.randn(M, Ka, generator=gen).cuda()
    Bm = (torch.randn(Ka, N, generator=gen) / Ka ** 0.5).cuda()
    bias, add = torch.randn(N, generator=gen).cuda(), torch.randn(M, N, generator=gen).cuda()
    sc, sh = (torch.rand(N, generator=gen) + 0.5).cuda(), (0.3 * torch.randn(N, generator=gen)).cuda()
    variants = [("plain", {}), ("bias", {"bias": bias}), ("addend", {"bias": bias, "addend": add}),
                ("act, relu", {"bias": bias, "act": (sc, sh, True)}), ("act, no relu", {"act": (sc, sh, False)})]
    if M % 2 == 0:
        variants.append(("pair_out", {"bias": bias, "pair_out": True}))
    print(f"  {arith} M {M} Ka {Ka} N {N}")
    for name, kw in variants:
        C, w = _gemm_planes(ops, arith, [A], Ka, Bm, M, N, **kw)
        _same(name, _word(w), _exact(C))
        for r in sorted({q for q in (0, M - 1, 127, 128) if q < M}):
            Aq = A.clone()
            Aq[r] *= 64.0
            C, w = _gemm_planes(ops, arith, [Aq], Ka, Bm, M, N, **kw)
            got = _word(w)
            assert _argmax(C)[0] == (r >> 1 if kw.get("pair_out") else r), (name, r, _argmax(C))
            _same(f"{name}, row {r} x 64", got, _exact(C))
    if M > 8:
        Aq = A.clone()
        Aq[3, 1], Aq[M - 1, 0] = NAN, INF
        addq = add.clone()
        addq[5, 2] = -INF                   # (a non-finite OPERAND comes out as NaN; an infinity is stored through the addend)
        C, w = _gemm_planes(ops, arith, [Aq], Ka, Bm, M, N, bias=bias, addend=addq)
        assert not torch.isfinite(C[3]).any() and not torch.isfinite(C[M - 1]).any() and C[5, 2] == -INF
        _same("NaN / inf rows left out", _word(w), _exact(C))


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("N", [64, 256])
def test_word_gemm_planes_rows(ops, monkeypatch, arith, N):
    """amax_out of p2m_gemm_planes_rows on hub120, B = 3: row set 1 with compact planes, row set 2 with the effective weight.
    The other set's rows are poisoned in X and in C: the word is bitwise what it is without the poison, those rows of C stay
    bitwise untouched; one word shared by both launches of a conv ends as the maximum over all rows."""
    monkeypatch.setattr(ops, "GEMM_ARITH", arith)
    L, p, g, _ = _fam(ops, "hub120")
    B, Ka, V = 3, 64, g.V
    real, fake = g.real_ids_host().astype(np.int64), g.fake_ids_host().astype(np.int64)
    gen = torch.Generator().manual_seed(N)
    X = torch.randn(B * V, Ka, generator=gen).cuda()
    Wt = (torch.randn(3 * Ka, N, generator=gen) / (3 * Ka) ** 0.5).cuda()
    bias = torch.randn(N, generator=gen).cuda()
    Bx, We, Wex = ops.split_operands(Wt, Ka, N, g.fake_a, g.fake_b)

    def launch(Xc, rs, C, word, poison, addend=None):
        ids, other = (real, fake) if rs == 1 else (fake, real)
        xa = _amax_rows(g, rs, Xc, B, Ka) if arith == "f16x2" else None
        planes = ops.cheb_basis_fwd_real(g, Xc, B, Ka, 0) if rs == 1 else ()
        Xin = Xc.clone()
        if poison:
            _poison(Xin, _all_rows(B, V, other))
            _poison(C, _all_rows(B, V, other))
        before = C.clone()
        if rs == 1:
            ops.gemm_planes_rows(g, 1, B, [Xin, planes[0], planes[1]], Ka, 0, True, Wt, bias, addend, C, N, False, Bx=Bx, amax=xa,
                                 amax_bits=g.plane_bits, amax_out=word)
        else:
            ops.gemm_planes_rows(g, 2, B, [Xin], Ka, 0, False, We, bias, addend, C, N, False, Bx=Wex, amax=xa, amax_out=word)
        torch.cuda.synchronize()
        o = _all_rows(B, V, other)
        assert _bits_equal(C[o], before[o]), "a row outside the row set was written"
        return C[_all_rows(B, V, ids)]

    print(f"  hub120 {arith} N {N}: {real.size} real, {fake.size} fake rows per sample")
    for rs, ids in ((1, real), (2, fake)):
        w0, w1 = _zero_word(), _zero_word()
        launch(X, rs, torch.zeros(B * V, N, device="cuda"), w0, False)
        out = launch(X, rs, torch.zeros(B * V, N, device="cuda"), w1, True)
        _same(f"row set {rs}, other rows poisoned", _word(w1), _exact(out))
        _unchanged(f"row set {rs}", _word(w1), _word(w0))
        for b, i in ((B - 1, ids.size - 1), (0, 0)):
            Xq = X.clone()
            Xq[b * V + ids[i]] *= 64.0
            w = _zero_word()
            out = launch(Xq, rs, torch.zeros(B * V, N, device="cuda"), w, True)
            assert _argmax(out)[0] == b * ids.size + i, (rs, b, i, _argmax(out))
            _same(f"row set {rs}, sample {b} vertex {ids[i]} x 64", _word(w), _exact(out))
        # NaN and inf inside the data rows: their output rows are not finite and stay out of the word (a non-finite OPERAND
        # comes out as NaN; an infinity is stored through the addend)
        Xq = X.clone()
        Xq[ids[1], 1], Xq[(B - 1) * V + ids[-2], 0] = NAN, INF
        addq = torch.zeros(B * V, N, device="cuda")
        out = launch(Xq, rs, torch.zeros(B * V, N, device="cuda"), _zero_word(), True, addq)
        j = int(torch.nonzero(torch.isfinite(out).all(1))[0])            # a row the NaN does not reach through the planes
        addq[_all_rows(B, V, ids)[j], 2] = -INF
        w = _zero_word()
        out = launch(Xq, rs, torch.zeros(B * V, N, device="cuda"), w, True, addq)
        assert out[j, 2] == -INF
        bad = int((~torch.isfinite(out).all(1)).sum())
        print(f"    row set {rs}: {bad} output rows not finite")
        assert not torch.isfinite(out[1]).any() and not torch.isfinite(out[(B - 1) * ids.size + ids.size - 2]).any()
        assert bad < out.shape[0] // 2
        _same(f"row set {rs}, NaN / inf inside the data rows", _word(w), _exact(out))
    w, C = _zero_word(), torch.full((B * V, N), NAN, device="cuda")
    launch(X, 1, C, w, False)
    first = _word(w)
    launch(X, 2, C, w, False)
    assert torch.isfinite(C).all()
    print(f"    after row set 1 alone: word {first!r}")
    _same("one word, both launches", _word(w), _exact(C))
    assert _word(w) >= first


TILE_CASES = [(name, B) for name in ("cliques29", "hub120", "mixed") for B in (1, 3, 5)] + [("cliques56", 3)]


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("name,B", TILE_CASES)
def test_word_cheb_tile_gemm(ops, monkeypatch, name, B, arith):
    """amax_out of p2m_cheb_tile_gemm on partial tiles (cliques29), a one-row tile (hub120) and mixed rows, B never a multiple of
    the sample group, plans 0 and 1 (cliques56: the paired plan 2 only), N = 64 / 128 (matrix-core gather in f16x2) and 256
    (VALU gather), modes plain / stats / addend / act.  The input row behind the last compact row of the last tile in sample
    B - 1, behind the single row of a one-row tile and behind compact row 0 of sample 0 is scaled by 64 in turn (or set to 64 x
    the signs of a weight column where a coupled row would otherwise take the maximum); C is pre-filled with NaN, so the stored
    maximum is that of the plan's rows.  Plan 1: the two children of a coarse vertex read the SAME input row, so the planted
    maximum sits at the row or at its sibling - the assertion is on the pair.  In every mode and width, NaN and inf inside two
    input data rows stay out of the word, and their output rows are not finite (except under the ReLU of `act`)."""
    monkeypatch.setattr(ops, "GEMM_ARITH", arith)
    L, p, g, _ = _fam(ops, name)
    V, Ka = p.V, 64
    for plan in ((2,) if name == "cliques56" else (0, 1)):
        assert p.plan[plan] is not None and g.plan_tiles[plan] == len(p.plan[plan])
        xr = V // 2 if plan == 1 else V
        cr = V // 2 if plan == 2 else V
        rows = np.asarray(p.pair_order if plan == 2 else p.real_order, dtype=np.int64)
        tiles = np.array(p.plan[plan])
        spots = [(B - 1, rows.size - 1), (0, 0)]
        one = np.where(tiles[:, 1] == 1)[0]
        if one.size:
            spots.append((B // 2, int(tiles[one[-1], 0])))
        assert tiles[-1, 0] + tiles[-1, 1] == rows.size
        for N in (64, 128, 256):
            assert _hip().p2m_cheb_tile_gemm_supported(g.handle, plan, Ka, N)
            gen = torch.Generator().manual_seed(7 * plan + N + B)
            X = torch.randn(B * xr, Ka, generator=gen).cuda()
            Wt = (torch.randn(3 * Ka, N, generator=gen) / (3 * Ka) ** 0.5).cuda()
            bias, add = torch.randn(N, generator=gen).cuda(), torch.randn(B * cr, N, generator=gen).cuda()
            sc, sh = (torch.rand(N, generator=gen) + 0.5).cuda(), (0.3 * torch.randn(N, generator=gen)).cuda()
            Bx = ops.weight_split(Wt)
            print(f"  {name} plan {plan} {arith} N {N} B {B}: {len(tiles)} tiles, last tile {tiles[-1, 1]} rows, "
                  f"{one.size} one-row tiles")

            def launch(Xin, mode, addv=None):
                A0 = Xin.view(B, V // 2, 2, Ka).sum(2).reshape(-1, Ka).contiguous() if plan == 2 else Xin
                C, w = torch.full((B * cr, N), NAN, device="cuda"), _zero_word()
                addend = (add if addv is None else addv) if mode == "addend" else None
                ops.cheb_tile_gemm(g, plan, Xin, A0, Ka, Bx, bias, addend, C, N, B,
                                   stats=mode == "stats", act=(sc, sh, True) if mode == "act" else None, amax_out=w)
                return C, _word(w)

            for mode in ("plain", "stats", "addend", "act"):
                C, got = launch(X, mode)
                assert int(torch.isfinite(C).all(1).sum()) == B * rows.size
                _same(mode, got, _exact(C))
                for b, i in spots:
                    v = int(rows[i])
                    want = b * cr + v
                    src = slice(b * V + 2 * v, b * V + 2 * v + 2) if plan == 2 else b * xr + (v >> plan)
                    # the input row x 64; where that leaves the maximum with a neighbour of the vertex (a light row next to
                    # a heavy one in `mixed`, or the ReLU of `act` cutting the row's larger side), 64 x the signs of column 0 of
                    # W0 instead: 64 sum |W0[:, 0]| at (row, column 0), an order of magnitude above any coupled row
                    for recipe in ("x 64", "aligned"):
                        Xq = X.clone()
                        if recipe == "x 64":
                            Xq[src] *= 64.0
                        else:
                            Xq[src] = 64.0 * torch.sign(Wt[:Ka, 0])
                        C, got = launch(Xq, mode)
                        r = _argmax(C)[0]
                        if (r >> 1 == want >> 1) if plan == 1 else (r == want):
                            break
                    assert (r >> 1 == want >> 1) if plan == 1 else (r == want), (mode, b, i, v, r)
                    _same(f"{mode}, sample {b} compact row {i} (vertex {v}) {recipe}", got, _exact(C))
                # NaN and inf inside the data rows
                Xq = X.clone()
                hit = ((0, int(rows[1]), 1, NAN), (B - 1, int(rows[-2]), 0, INF))
                for b, v, c, val in hit:
                    Xq[b * V + 2 * v if plan == 2 else b * xr + (v >> plan), c] = val
                C, got = launch(Xq, mode)
                if mode == "addend":        # a non-finite OPERAND comes out as NaN; an infinity is stored through the addend,
                    j = int(torch.nonzero(torch.isfinite(C).all(1))[0])      # in a row the NaN does not reach
                    addq = add.clone()
                    addq[j, 2] = -INF
                    C, got = launch(Xq, mode, addq)
                    assert C[j, 2] == -INF
                bad = int((~torch.isfinite(C).all(1)).sum()) - (B * cr - B * rows.size)
                print(f"    {mode}: {bad} stored rows not finite")
                for b, v, c, val in hit:                   # (`act`: the ReLU's max turns a NaN into 0, nothing to assert there)
                    assert mode == "act" or not torch.isfinite(C[b * cr + v]).any(), (mode, b, v)
                assert bad < B * rows.size and got > 0.0      # (the 2-ring of a hub is most of a small level: enough rows remain)
                _same(f"{mode}, NaN / inf inside the data rows", got, _exact(C))


def _bn_act(y, sc, sh, relu, resid, Fres, rshift, x, M, F, handle=None, mode=0, word=None):
    _ck(_hip().p2m_bn_act_fwd(_vp(y), _vp(sc), _vp(sh), int(relu), _vp(resid), int(Fres), int(rshift), _vp(x), M, F, handle,
                              mode, _vp(word), _st()), "p2m_bn_act_fwd")


# (scale / shift, ReLU, residual: None / same width / feature-axis lerp, res_shift)
BN_ACT_VARIANTS = [(False, False, None, 0), (True, True, None, 0), (True, False, "same", 0), (True, True, "same", 1),
                   (True, True, "lerp", 0), (False, True, "lerp", 1)]


def _bn_act_inputs(M, F, seed):
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn(M, F, generator=gen).cuda()
    sgn = torch.where(torch.rand(F, generator=gen) < 0.5, -1.0, 1.0)
    sc = ((0.75 + 0.5 * torch.rand(F, generator=gen)) * sgn).cuda()
    sh = (0.3 * torch.randn(F, generator=gen)).cuda()
    Fl = {32: 64, 256: 64, 36: 20}[F]
    res = {None: None, "same": (0.5 * torch.randn(M, F, generator=gen)).cuda(),
           "lerp": (0.5 * torch.randn(M, Fl, generator=gen)).cuda()}
    return y, sc, sh, res


@pytest.mark.parametrize("M,F", [(1, 32), (67, 32), (16 * 32 + 1, 32), (1000, 256), (1, 36), (57, 36), (1000, 36)])
def test_word_bn_act_fwd(hip_libs, M, F):
    """amax_out of p2m_bn_act_fwd: k_bn_act_fwd (F = 32: 32 rows per pass, 16 per thread; F = 256) and k_bn_act_fwd_v4 (F = 36),
    with and without scale / shift, ReLU and a residual of the same width or resized along the feature axis, res_shift 0 / 1;
    +-50 planted in y at row 0, column 0 and in the last row, last column (signed so that the ReLU keeps it)."""
    y, sc, sh, res = _bn_act_inputs(M, F, M + F)
    for affine, relu, kind, rshift in BN_ACT_VARIANTS:
        resid = res[kind]
        Fres = 0 if resid is None else resid.shape[1]
        a = (sc, sh) if affine else (None, None)
        what = f"M {M} F {F} affine {affine} relu {relu} resid {kind} >> {rshift}"

        def launch(yin):
            x, w = torch.zeros(M, F, device="cuda"), _zero_word()
            _bn_act(yin, a[0], a[1], relu, resid, Fres, rshift, x, M, F, word=w)
            return x, _word(w)

        x, got = launch(y)
        _same(what, got, _exact(x))
        for r, c in ((0, 0), (M - 1, F - 1)):
            yq = y.clone()
            yq[r, c] = 50.0 * (float(torch.sign(sc[c])) if affine else 1.0)
            x, got = launch(yq)
            assert _argmax(x) == (r, c), (what, r, c, _argmax(x))
            _same(f"  planted at ({r}, {c})", got, _exact(x))
    yq = y.clone()
    yq[0, 1], yq[M - 1, F - 2] = NAN, INF
    x, w = torch.zeros(M, F, device="cuda"), _zero_word()
    _bn_act(yq, sc, sh, False, None, 0, 0, x, M, F, word=w)
    _same("NaN / inf left out", _word(w), _exact(x))
    assert int((~torch.isfinite(x)).sum()) == 2


@pytest.mark.parametrize("F", [32, 256])
@pytest.mark.parametrize("mode", ["classes", "real_rows_only"])
def test_word_bn_act_fwd_row_maps(ops, F, mode):
    """p2m_bn_act_fwd over the live rows of band(736) with classes (holes poisoned in y, the residual and x) and over the real
    rows only (every other row poisoned): the word is bitwise that of the clean run, the poisoned rows of x stay bitwise
    untouched; planted at the first logical row of sample 0 and the last logical row of sample B - 1."""
    bd = _band(ops, 736, 11, mode == "classes")
    B, V = 3, bd.V
    M = B * V
    ids = bd.live if mode == "classes" else bd.real
    dead = _all_rows(B, V, np.setdiff1d(np.arange(V), ids))
    data = _all_rows(B, V, ids)
    y, sc, sh, res = _bn_act_inputs(M, F, F + len(mode))
    resid = res["same"]
    flag = 0 if mode == "classes" else 1

    def launch(yin, poison):
        yin, rin = yin.clone(), resid.clone()
        x, w = torch.zeros(M, F, device="cuda"), _zero_word()
        if poison:
            for t in (yin, rin, x):
                _poison(t, dead)
        before = x.clone()
        _bn_act(yin, sc, sh, True, rin, F, 0, x, M, F, handle=bd.g.handle, mode=flag, word=w)
        got = _word(w)
        assert _bits_equal(x[dead], before[dead]), "a row that holds no data was written"
        return x[data], got

    print(f"  band(736) {mode} F {F}: {ids.size} of {V} rows per sample")
    _, clean = launch(y, False)
    out, got = launch(y, True)
    _same("no-data rows poisoned", got, _exact(out))
    _unchanged("no-data rows poisoned", got, clean)
    for b, i, c in ((0, 0, 0), (B - 1, ids.size - 1, F - 1)):
        yq = y.clone()
        yq[b * V + ids[i], c] = 50.0 * float(torch.sign(sc[c]))
        out, got = launch(yq, True)
        assert _argmax(out) == (b * ids.size + i, c)
        _same(f"planted at sample {b} vertex {ids[i]} column {c}", got, _exact(out))


def _bn_co(y, gamma, beta, rows=None):
    """[mean, invstd, scale, shift] of a training-mode BatchNorm over (the given rows of) y, fp32."""
    yy = y if rows is None else y[rows]
    mean, var = yy.mean(0), yy.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    return torch.stack([mean, invstd, gamma * invstd, beta - mean * gamma * invstd]).contiguous()


@pytest.mark.parametrize("F", [32, 128, 36])
@pytest.mark.parametrize("M", [2, 258, 1000])
def test_word_bn_bwd_apply(ops, monkeypatch, M, F):
    """The word of gy out of ops.bn_relu_bwd: the templates (F = 32, 128) and the generic kernel (F = 36), training and eval,
    plain and with the pair-sum by-products (max |pair_gy| <= 2 word: the rule consumers rely on); gx[0] and gx[M - 1] scaled by
    64 in turn.  Training mode on the batch statistics, eval mode on running statistics.  (M = 2 in training mode is run as
    drawn only: the two rows of a two-row batch come out as mirror images, so no maximum can be planted in one of them.)
    NaN and inf in gx, at elements the ReLU mask lets through, make gy non-finite there and stay out of the word."""
    monkeypatch.setattr(ops, "GEMM_ARITH", "f16x2")
    gen = torch.Generator().manual_seed(M * F)
    y = (torch.randn(M, F, generator=gen) * 2 + 0.5).cuda()
    gx = torch.randn(M, F, generator=gen).cuda()
    gamma, beta = (torch.rand(F, generator=gen) + 0.5).cuda(), (0.2 * torch.randn(F, generator=gen)).cuda()
    rm, rv = (0.1 * torch.randn(F, generator=gen)).cuda(), (torch.rand(F, generator=gen) + 0.5).cuda()
    for training in (True, False):
        co = _bn_co(y, gamma, beta) if training else ops.bn_eval_coeffs(gamma, beta, rm, rv, 1e-5)
        for pairs in ((False, True) if F in (32, 128) else (False,)):
            open_ = (y * co[2] + co[3]) > 0.1                   # elements the ReLU mask lets through, clear of the kink
            c0, c1 = int(torch.nonzero(open_[0])[0]), int(torch.nonzero(open_[M - 1])[-1])
            for r in (None, "nan") if (M == 2 and training) else (None, 0, M - 1, "nan"):
                g_in = gx.clone()
                if r == "nan":
                    g_in[0, c0], g_in[M - 1, c1] = NAN, INF
                elif r is not None:
                    g_in[r] *= 64.0
                res = ops.bn_relu_bwd(g_in, y, co, gamma, True, training, M, F, pair_in=pairs, pair_out=pairs)
                gy = res[0]
                got = _word(gy._p2m_amax)
                what = f"M {M} F {F} training {training} pairs {pairs}" + \
                    ("" if r is None else ", NaN / inf in gx" if r == "nan" else f", gx[{r}] x 64")
                if r == "nan":
                    assert not torch.isfinite(gy[0, c0]) and not torch.isfinite(gy[M - 1, c1]), what
                elif r is not None:
                    assert _argmax(gy)[0] == r, (what, _argmax(gy))
                _same(what, got, _exact(gy))
                if pairs:
                    pm = _exact(res[4])
                    print(f"      max |pair_gy| {pm!r} <= 2 word")
                    assert pm <= 2.0 * got
                    assert r == "nan" or torch.equal(res[4], gy.view(M // 2, 2, F).sum(1))


@pytest.mark.parametrize("F", [32, 128])
def test_word_bn_bwd_apply_classes(ops, monkeypatch, F):
    """The same on band(736) with classes, holes of gx and y poisoned: skipping the holes and with zero_holes (the holes of gy
    are then exactly 0), plain and with the pair sums - the word is bitwise that of the clean run and the maximum over the live
    rows; without zero_holes a pre-poisoned hole of gy stays bitwise untouched (direct call, eval mode)."""
    monkeypatch.setattr(ops, "GEMM_ARITH", "f16x2")
    bd = _band(ops, 736, 11, True)
    B, V = 2, bd.V
    M = B * V
    live, holes = _all_rows(B, V, bd.live), _all_rows(B, V, bd.holes)
    gen = torch.Generator().manual_seed(F)
    y = (torch.randn(M, F, generator=gen) * 2 + 0.5).cuda()
    gx = torch.randn(M, F, generator=gen).cuda()
    gamma, beta = (torch.rand(F, generator=gen) + 0.5).cuda(), (0.2 * torch.randn(F, generator=gen)).cuda()
    co = _bn_co(y, gamma, beta, live)
    has_live = torch.zeros(M, dtype=torch.bool, device="cuda")
    has_live[live] = True
    has_live = has_live.view(M // 2, 2).any(1)
    print(f"  band(736) with classes: {bd.holes.size} holes, {bd.fake.size} representatives per sample")

    def run(g_in, training, pairs, zero, poison):
        g_in, yin = g_in.clone(), y.clone()
        if poison:
            _poison(g_in, holes)
            _poison(yin, holes)
        res = ops.bn_relu_bwd(g_in, yin, co, gamma, True, training, M, F, pair_in=pairs, pair_out=pairs, classes=bd.g,
                              zero_holes=zero)
        return res, _word(res[0]._p2m_amax)

    for training in (True, False):
        for pairs in (False, True):
            for zero in (False, True):
                what = f"F {F} training {training} pairs {pairs} zero_holes {zero}"
                _, clean = run(gx, training, pairs, zero, False)
                res, got = run(gx, training, pairs, zero, True)
                _same(what + ", holes poisoned", got, _exact(res[0][live]))
                _unchanged(what, got, clean)
                if zero:
                    assert (res[0][holes] == 0).all()
                    _same(what + ", all rows", got, _exact(res[0]))
                if pairs:
                    pg = res[4] if zero else res[4][has_live]
                    print(f"      max |pair_gy| {_exact(pg)!r} <= 2 word")
                    assert torch.isfinite(pg).all() and _exact(pg) <= 2.0 * got
                for b, i in ((B - 1, bd.live.size - 1), (0, 0)):
                    gq = gx.clone()
                    gq[b * V + bd.live[i]] *= 64.0
                    res, got = run(gq, training, pairs, zero, True)
                    out = res[0][live]
                    assert _argmax(out)[0] == b * bd.live.size + i, (what, b, i, _argmax(out))
                    _same(f"{what}, sample {b} vertex {bd.live[i]} x 64", got, _exact(out))
    gp, yp = _poison(gx.clone(), holes), _poison(y.clone(), holes)
    gy = _poison(torch.zeros(M, F, device="cuda"), holes)
    before, w = gy.clone(), _zero_word()
    _ck(_hip().p2m_bn_bwd_apply(_vp(gp), _vp(yp), _vp(co[2]), _vp(co[3]), _vp(co[0]), _vp(co[1]), _vp(gamma), None, 1, _vp(gy),
                                None, None, M, F, bd.g.handle, 0, _vp(w), _st()), "p2m_bn_bwd_apply")
    _same("direct call, holes of gy pre-poisoned", _word(w), _exact(gy[live]))
    assert _bits_equal(gy[holes], before[holes]), "a hole of gy was written"


@pytest.mark.parametrize("N", [1, 64, 257, 4096])
def test_word_act_bound(ops, N):
    """p2m_act_bound: the word is max_f fma(A, |scale_f|, max(shift_f, 0)) in float32 (float64 product and sum, rounded once),
    and it bounds relu(fma(y, scale, shift)) over a tensor with |y| <= A whose extremes +-A sit in every column."""
    gen = torch.Generator().manual_seed(N)
    scale, shift = (torch.randn(N, generator=gen) * 1.5).cuda(), torch.randn(N, generator=gen).cuda()
    y = (torch.rand(37, N, generator=gen) * 2 - 1).cuda() * 2.75
    y[0], y[1] = 2.75, -2.75
    A = _exact(y)
    assert A == 2.75
    yw = _amax(y, y.numel(), _zero_word())
    got = _word(ops.act_bound(scale, shift, yw, _zero_word()))
    want = float((A * scale.double().abs() + shift.double().clamp_min(0)).max().float())
    _same(f"N {N}", got, want)
    x = torch.relu(torch.addcmul(shift.double(), y.double(), scale.double())).float()
    print(f"    max relu(fma(y, scale, shift)) {_exact(x)!r}")
    assert got >= _exact(x)
    w = torch.tensor([1e9]).view(torch.int32).cuda()
    assert _word(ops.act_bound(scale, shift, yw, w)) == float(torch.tensor(1e9))      # an atomic max: a larger word stays


# ---- 2. headroom bits ------------------------------------------------------------------------------------------------------------

def _operators64(Ld):
    """(L, L2) as the handle bakes them, in float64: L rounded to fp32, L2 = 2 L L - I accumulated in double, rounded once."""
    Lf = Ld.float().double()
    L2 = (2 * Lf @ Lf - torch.eye(Lf.shape[0], dtype=torch.float64, device=Lf.device)).float().double()
    return Lf, L2


@pytest.mark.parametrize("name", ["cliques28", "hub120", "mixed", "band1472"])
def test_headroom_plane_bits(ops, name):
    """p2m_graph_plane_bits == ceil(log2(max(1, max row sum of |L|, |L2|))) for plans 0 / 1, one more for plan 2; the float64
    row-sum maxima (1.206, 1.785, 4.590, 1.148 for these four levels) are nowhere near a power of two.  ops.eff_bits covers
    1 + |a| + |b| with the fewest binades."""
    if name == "band1472":
        bd = _band(ops, 1472, 5, False)
        g, Ld = bd.g, torch.from_numpy(tp.dense(bd.L)).cuda()
    else:
        _, _, g, Ld = _fam(ops, name)
    Lf, L2 = _operators64(Ld)
    s = max(float(Lf.abs().sum(1).max()), float(L2.abs().sum(1).max()))
    want = int(np.ceil(np.log2(max(1.0, s))))
    got = [int(_hip().p2m_graph_plane_bits(g.handle, plan)) for plan in range(3)]
    print(f"  {name}: largest row sum {s:.6f} -> {want} bits; library {got}; DeviceGraph.plane_bits {g.plane_bits}")
    assert abs(s - 2.0 ** round(np.log2(s))) > 1e-6
    assert got == [want, want, want + 1] and g.plane_bits == want
    a, b = g.fake_a, g.fake_b
    eb = ops.eff_bits(a, b)
    print(f"    fake rows: a {a!r} b {b!r}, 1 + |a| + |b| = {1 + abs(a) + abs(b):.6f}, eff_bits {eb}")
    assert 2.0 ** eb >= 1 + abs(a) + abs(b) and (eb == 0 or 2.0 ** (eb - 1) < 1 + abs(a) + abs(b))


@pytest.mark.parametrize("name,which", [("hub120", "L2"), ("hub120", "L"), ("mixed", "L2"), ("mixed", "L"), ("cliques56", "L2")])
def test_headroom_saturation(ops, monkeypatch, name, which):
    """Operands AT their bounds: |x| = U everywhere, U = nextafter(2, 0) (all-ones significand: U 2^s sits just under 2^15), one
    feature column carrying the signs of the row of L2 (or L) with the largest absolute row sum, so that plane reaches
    (row sum) U; |W| constant with the signs of (1, a, b), so that W0 + a W1 + b W2 reaches (1 + |a| + |b|) max |W|.  Through
    ops.cheb_tile_gemm (plans 0 and 1; cliques56: the paired plan 2) and ops.gemm_planes_rows (row sets 1 and 2) in f16x2 every
    output is finite and within the bound of test_f16x2_error_is_fp32_class (tests/test_gpu_ops.py) of the float64 dense
    restatement: err / sum |a||b| < 5e-6 and <= 4 x the native f32 contraction's + 2^-20.  `mixed` needs 3 binades: the case that
    overflows the fp16 slices if the headroom is dropped."""
    L, p, g, Ld = _fam(ops, name)
    Lf, L2 = _operators64(Ld)
    Md = L2 if which == "L2" else Lf
    V, B, Ka = p.V, 2, 64
    U = float(np.nextafter(np.float32(2.0), np.float32(0.0)))
    a, b = g.fake_a, g.fake_b
    gen = torch.Generator().manual_seed(len(name))

    def signs(rows, row):
        S = torch.where(torch.rand(B, rows, Ka, generator=gen) < 0.5, -1.0, 1.0).cuda()
        S[:, :, 0] = torch.where(row < 0, -1.0, 1.0).float()
        return (U * S).reshape(B * rows, Ka).contiguous()

    def planes64(Xd):                                        # [B, V, Ka] float64 -> [B, V, 3 Ka]
        return torch.cat((Xd, torch.einsum("uv,bvf->buf", Lf, Xd), torch.einsum("uv,bvf->buf", L2, Xd)), dim=2)

    def err(what, C, rows, Pd, Wd):
        C = C.view(B, -1, C.shape[-1])[:, rows]
        assert torch.isfinite(C).all(), what + ": overflow"
        ref, scale = Pd[:, rows] @ Wd, Pd[:, rows].abs() @ Wd.abs()
        return float(((C.double() - ref).abs() / scale).max())

    figures = {}
    for N in (128, 256):
        c = 0.0625 * U / 2
        s3 = torch.tensor([1.0, 1.0 if a >= 0 else -1.0, 1.0 if b >= 0 else -1.0])
        Wt = (c * s3.repeat_interleave(Ka)[:, None] * torch.ones(3 * Ka, N)).cuda().contiguous()
        Wd = Wt.double()
        if name == "cliques56":
            monkeypatch.setattr(ops, "GEMM_ARITH", "f16x2")
            Mp = Md.view(V // 2, 2, V).sum(1)
            r = int(Mp.abs().sum(1).argmax())
            X = signs(V, Mp[r])
            A0 = X.view(B, V // 2, 2, Ka).sum(2).reshape(-1, Ka).contiguous()
            Pd = planes64(X.double().view(B, V, Ka)).view(B, V // 2, 2, 3 * Ka).sum(2)
            rows = torch.as_tensor(np.asarray(p.pair_order), device="cuda")
            C = torch.full((B * (V // 2), N), NAN, device="cuda")
            ops.cheb_tile_gemm(g, 2, X, A0, Ka, ops.weight_split(Wt), None, None, C, N, B)
            torch.cuda.synchronize()
            T2 = float(Pd[:, r, 2 * Ka].abs().max())
            print(f"  {name} N {N}: paired row {r}, |S L2 x| reaches {T2:.4f} = {T2 / U:.4f} U, headroom "
                  f"{int(_hip().p2m_graph_plane_bits(g.handle, 2))} bits")
            e16 = err("plan 2", C, rows, Pd, Wd)
            # the yardstick: the native f32 contraction on the pair sums of the basis kernel's fp32 planes
            monkeypatch.setattr(ops, "GEMM_ARITH", "f32")
            T1, T2 = ops.cheb_basis_fwd(g, X, B, Ka, 0)
            half = [A0] + [t.view(B * V // 2, 2, Ka).sum(1).contiguous() for t in (T1, T2)]
            (C32,), _ = ops.gemm_planes(half, Ka, 0, Wt, None, B * V // 2, N, 1, False)
            figures[f"plan 2, N {N}"] = (e16, err("f32", C32, rows, Pd, Wd))
            continue
        real = torch.as_tensor(np.asarray(p.real_order), device="cuda")
        fake = torch.as_tensor(np.sort(g.fake_ids_host().astype(np.int64)), device="cuda")
        r = int(Md.abs().sum(1).argmax())
        X = signs(V, Md[r])
        X1 = signs(V // 2, Md[r].view(V // 2, 2).sum(1))
        Pd = planes64(X.double().view(B, V, Ka))
        Pd1 = planes64(X1.double().view(B, V // 2, Ka).repeat_interleave(2, dim=1))
        reach = float(Pd[:, r, (2 if which == "L2" else 1) * Ka].abs().max()) / U
        print(f"  {name} N {N}: row {r} of {which}, the plane reaches {reach:.4f} U with {g.plane_bits} bits of headroom; "
              f"effective weight {float(1 + abs(a) + abs(b)):.4f} max |W| with {ops.eff_bits(a, b)} bits")
        assert which == "L" or reach > 2.0 ** (g.plane_bits - 1)
        # the native f32 contraction on the basis kernel's fp32 planes: the yardstick of the existing bound, like for like -
        # from the same input (own resolution / un-pooled) over the same rows (real / fake) as the figure it is held against
        monkeypatch.setattr(ops, "GEMM_ARITH", "f32")
        T1, T2 = ops.cheb_basis_fwd(g, X, B, Ka, 0)
        (C32,), _ = ops.gemm_planes([X, T1, T2], Ka, 0, Wt, None, B * V, N, 1, False)
        e32 = {0: err("f32", C32, real, Pd, Wd), "fake": err("f32", C32, fake, Pd, Wd)}
        T1, T2 = ops.cheb_basis_fwd(g, X1, B, Ka, 1)
        (C32,), _ = ops.gemm_planes([X1, T1, T2], Ka, 1, Wt, None, B * V, N, 1, False)
        e32[1] = err("f32", C32, real, Pd1, Wd)
        monkeypatch.setattr(ops, "GEMM_ARITH", "f16x2")
        pa = ops.param_amax(Wt)
        Bx, We, Wex = ops.split_operands(Wt, Ka, N, a, b, amax=pa)
        assert float(We.abs().max()) > 2.0 ** (ops.eff_bits(a, b) - 1) * float(Wt.abs().max())
        for plan, Xin, P in ((0, X, Pd), (1, X1, Pd1)):
            C = torch.full((B * V, N), NAN, device="cuda")
            ops.cheb_tile_gemm(g, plan, Xin, Xin, Ka, Bx, None, None, C, N, B)
            figures[f"plan {plan}, N {N}"] = (err(f"plan {plan}", C, real, P, Wd), e32[plan])
        C = torch.full((B * V, N), NAN, device="cuda")
        xa = ops.amax_of(X, g, B)
        T1c, T2c = ops.cheb_basis_fwd_real(g, X, B, Ka, 0)
        ops.gemm_planes_rows(g, 1, B, [X, T1c, T2c], Ka, 0, True, Wt, None, None, C, N, False, Bx=Bx, amax=xa,
                             amax_bits=g.plane_bits)
        ops.gemm_planes_rows(g, 2, B, [X], Ka, 0, False, We, None, None, C, N, False, Bx=Wex, amax=xa)
        figures[f"row set 1, N {N}"] = (err("row set 1", C, real, Pd, Wd), e32[0])
        figures[f"row set 2, N {N}"] = (err("row set 2", C, fake, Pd, Wd), e32["fake"])
    for what, (e, e32) in figures.items():
        print(f"    {what}: max err / sum |a||b| {e:.3e}   (native f32: {e32:.3e})")
    for what, (e, e32) in figures.items():
        assert e32 < 5e-6 and e < 5e-6, (what, e, e32)
        assert e <= 4.0 * e32 + 2.0 ** -20, (what, e, e32)


# ---- 3. weight images ------------------------------------------------------------------------------------------------------------

def _slices(Bx, K, N, arith):
    """(slices [NS, Npad, K] as float64, trailer word or None) of a weight image Bx[k / 16][s][n][k % 16]."""
    NS, Npad = (2, 3)[arith == "bf16x3"], -(-N // 128) * 128
    body = Bx[:NS * Npad * K]
    if arith == "f16x2":
        v = body.view(torch.float16).double()
        trailer = float(Bx[NS * Npad * K:NS * Npad * K + 2].view(torch.float32))
    else:
        v = ((body.to(torch.int32) & 0xFFFF) << 16).view(torch.float32).double()
        trailer = None
    return v.view(K // 16, NS, Npad, 16).permute(1, 2, 0, 3).reshape(NS, Npad, K), trailer


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
def test_conv_weights_prepare_images(ops, monkeypatch, arith):
    """ops.ConvWeightSet.refresh (p2m_conv_weights_prepare: k_conv_weights_amax + k_conv_weights_images) for three layers, one
    weight 4-byte but not 16-byte aligned (the scalar branch of the amax kernel), each with the (a, b) of a real level: the four
    images are BITWISE weight_pack -> (weight_eff) -> weight_split with param_amax and eff_bits (ops.split_operands), trailer word
    included, padding columns zero; words[i] == max |W_i|; the reconstruction bound of test_f16x2_weight_image holds for all four.
    bf16x3: slice 0 + slice 1 + slice 2 is the operand exactly, and the parameter words are left alone (include/p2m.h: the word
    is written for P2M_ARITH_F16X2 only - the exact arithmetic has no scale - so they keep the zeros they were allocated with).
    refresh() rewrites the images after an in-place torch update
    and after bump_weight_epoch(), and is a no-op otherwise."""
    monkeypatch.setattr(ops, "GEMM_ARITH", arith)
    levels = [_fam(ops, "hub120")[2], _fam(ops, "mixed")[2], _band(ops, 736, 11, False).g]
    gen = torch.Generator().manual_seed(3)
    entries = []
    for i, ((Fout, Fin), g) in enumerate(zip(((64, 32), (128, 64), (256, 128)), levels)):
        n = Fout * Fin * 3
        buf = (torch.randn(n + 4, generator=gen) / (3 * Fin) ** 0.5).cuda()
        off = 1 if i == 1 else 0
        W = buf[off:off + n].view(Fout, Fin * 3)
        assert W.is_contiguous() and W.data_ptr() % 16 == 4 * off
        entries.append((i, W, g.fake_a, g.fake_b))
    cws = ops.ConvWeightSet(entries, "cuda:0")

    def check_all():
        torch.cuda.synchronize()
        for i, W, a, b in entries:
            Fout, Fin = W.shape[0], W.shape[1] // 3
            Wt, _, W3 = ops.weight_pack(W, Fin, 3, need_w2=False, need_w3=True)
            pa = ops.param_amax(W)
            want = ops.split_operands(Wt, Fin, Fout, a, b, amax=pa), ops.split_operands(W3, Fout, Fin, a, b, amax=pa)
            got = cws.images[i]
            print(f"  layer {i} ({Fin} -> {Fout}) {arith}: a {a:.4f} b {b:.4f}, eff_bits {ops.eff_bits(a, b)}")
            if arith == "f16x2":
                _same("parameter word", float(cws.words[i:i + 1].view(torch.float32)), _exact(W))
                _same("ops.param_amax", _word(pa), _exact(W))
            else:
                print(f"    parameter word (not written in this arithmetic): {int(cws.words[i])}")
                assert int(cws.words[i]) == 0
            for what, img, ref, Bm, (K, N) in (("forward, real rows", got[0], want[0][0], Wt, (3 * Fin, Fout)),
                                               ("forward, padding rows", got[1], want[0][2], want[0][1], (Fin, Fout)),
                                               ("backward, real rows", got[2], want[1][0], W3, (3 * Fout, Fin)),
                                               ("backward, padding rows", got[3], want[1][2], want[1][1], (Fout, Fin))):
                ncmp = (2 if arith == "f16x2" else 3) * (-(-N // 128) * 128) * K + (2 if arith == "f16x2" else 0)
                diff = int((img[:ncmp] != ref[:ncmp]).sum())          # (slices + trailer word; the last 12 bytes are unused)
                print(f"    {what}: [{K}, {N}] image, {img.numel()} elements, {diff} differ from the composition")
                assert img.shape == ref.shape and diff == 0, (i, what, diff)
                sl, trailer = _slices(img, K, N, arith)
                assert (sl[:, N:, :] == 0).all()
                if arith == "bf16x3":
                    assert torch.equal(sl[:, :N].sum(0).t(), Bm.double())
                else:
                    bits = ops.eff_bits(a, b) if "padding" in what else 0
                    assert trailer == _exact(W) * 2.0 ** bits
                    assert trailer >= _exact(Bm)
                    sb = 14 - int(np.floor(np.log2(trailer)))
                    rec = (sl[0, :N] + sl[1, :N]).t() * 2.0 ** -sb
                    bound = 2.0 ** -22 * Bm.double().abs() + 2.0 ** -40 * trailer
                    _chk("reconstruction / (2^-22 |w| + 2^-40 amax)", ((rec - Bm.double()).abs() / bound).max(), 1.0)

    cws.refresh()
    check_all()
    # no weight moved: a no-op - an image overwritten behind its back stays overwritten, no buffer is replaced
    ptrs = [t.data_ptr() for imgs in cws.images.values() for t in imgs]
    cws.images[0][1].fill_(7)
    cws.refresh()
    torch.cuda.synchronize()
    assert (cws.images[0][1] == 7).all() and ptrs == [t.data_ptr() for imgs in cws.images.values() for t in imgs]
    # an in-place torch update of one weight: everything is rewritten from the current weights
    entries[2][1].mul_(3.0)
    entries[0][1][5, 7] = 9.0
    cws.refresh()
    check_all()
    assert ptrs == [t.data_ptr() for imgs in cws.images.values() for t in imgs]
    # an update behind torch's back (the flat optimizers write through a raw pointer): bump_weight_epoch
    cws.images[1][3].fill_(7)
    cws.refresh()
    torch.cuda.synchronize()
    assert (cws.images[1][3] == 7).all()
    ops.bump_weight_epoch()
    cws.refresh()
    check_all()


# ---- 4. tags ---------------------------------------------------------------------------------------------------------------------

def test_tag_stale_words_are_recomputed(ops, monkeypatch):
    """A tensor tagged by bn_act_fwd and then refilled through torch (mul_, copy_, rebinding .data) gets a fresh, correct word
    from amax_of (the contents grew: the old word would be too small); view_tagged keeps a valid tag and drops a stale one."""
    monkeypatch.setattr(ops, "GEMM_ARITH", "f16x2")
    M, F = 300, 64
    gen = torch.Generator().manual_seed(4)
    y = torch.randn(M, F, generator=gen).cuda()
    big = (5.0 * torch.randn(M, F, generator=gen)).cuda()
    for how in ("mul_", "copy_", ".data"):
        x = ops.bn_act_fwd(y, None, False, None, 0, 0, M, F)
        w0 = x._p2m_amax
        old = _word(w0)
        _same(f"{how}: tagged by bn_act_fwd", old, _exact(x))
        assert ops._tag_valid(x) and ops.amax_of(x) is w0
        v = ops.view_tagged(x, M // 2, 2 * F)
        assert ops._tag_valid(v) and v._p2m_amax is w0 and ops.amax_of(v) is w0
        if how == "mul_":
            x.mul_(3.0)
        elif how == "copy_":
            x.copy_(big)
        else:
            x.data = big.clone()
        assert not ops._tag_valid(x)
        v = ops.view_tagged(x, M // 2, 2 * F)
        assert not ops._tag_valid(v) and getattr(v, "_p2m_amax", None) is None
        w1 = ops.amax_of(x)
        new = _word(w1)
        _same(f"{how}: recomputed", new, _exact(x))
        assert w1 is not w0 and new > old and _word(w0) == old
        assert ops._tag_valid(x) and ops.amax_of(x) is w1


@pytest.mark.parametrize("classes", [False, True])
def test_tag_row_sets(ops, monkeypatch, classes):
    """amax_of(t, g, B, row_set) on an untagged tensor is the row-set maximum (the other rows poisoned); a [B, V/2, F] tensor is
    refused."""
    from pose2mesh_release_amd._lib import P2MError
    monkeypatch.setattr(ops, "GEMM_ARITH", "f16x2")
    bd = _band(ops, 736, 11, classes)
    B, V, F = 3, bd.V, 32
    for rs, ids in ((0, bd.live), (1, bd.real), (2, bd.fake)):
        x = torch.randn(B * V, F, generator=torch.Generator().manual_seed(rs)).cuda()
        _poison(x, _all_rows(B, V, np.setdiff1d(np.arange(V), ids)))
        x[(B - 1) * V + ids[-1], F - 1] = -50.0
        w = ops.amax_of(x, bd.g, B, rs)
        _same(f"classes {classes} row set {rs}", _word(w), 50.0)
        assert _word(w) == _exact(x[_all_rows(B, V, ids)]) and ops.amax_of(x, bd.g, B, rs) is w
    half = torch.randn(B * V // 2, F).cuda()
    with pytest.raises(P2MError):
        ops.amax_of(half, bd.g, B, 0)
    monkeypatch.setattr(ops, "GEMM_ARITH", "bf16x3")
    assert ops.amax_of(torch.randn(8, 32).cuda()) is None


# ---- 5. one conv with outliers, against float64 ------------------------------------------------------------------------------

OUTLIER_SPOTS = ["last_real", "last_fake", "first_real"]


@pytest.mark.parametrize("Fin,Fout", [(64, 128), (64, 256)])
@pytest.mark.parametrize("spot", OUTLIER_SPOTS)
@pytest.mark.parametrize("where", ["x", "w"])
def test_graph_conv_cheby_outliers(ops, monkeypatch, where, spot, Fin, Fout):
    """cheby_graph_conv.graph_conv_cheby on hub120, B = 3, train mode, forward + backward against float64 autograd of the
    reference formula (construction and bounds of test_graph_conv_cheby_with_plans_missing: y within 2e-5 max(1, max |y64|),
    dX, dW, dgamma, dbeta within rel_l2 1e-4), with ONE element of x or of the upstream gradient w multiplied by 256: at the
    last real vertex in compact order of sample B - 1, at the highest fake vertex of sample B - 1, at the first real vertex of
    sample 0.  Both arithmetics run in the same test and both figures are printed.  bf16x3 has no words, so a bound IT missed
    would show the outlier amplifying fp32 round-off through the batch statistics rather than the slices; it misses none
    (measured over the 12 cases: y <= 2.3e-5 in either arithmetic with max |y64| 5.8 ... 73, every gradient <= 3e-7), so both
    arithmetics are held to the project's bounds as they stand."""
    from pose2mesh_release_amd.cheby_graph_conv import graph_conv_cheby
    from helpers import rel_l2
    L, p, g, Ld = _fam(ops, "hub120")
    B, V = 3, p.V
    real, fake = g.real_ids_host(), g.fake_ids_host()
    b, v = {"last_real": (B - 1, int(real[-1])), "last_fake": (B - 1, int(fake.max())), "first_real": (0, int(real[0]))}[spot]
    rng = np.random.default_rng(500 + Fin + Fout)
    x0 = torch.from_numpy(rng.standard_normal((B, V, Fin)).astype(np.float32))
    Wn = rng.uniform(-0.1, 0.1, (Fout, Fin * 3)).astype(np.float32)
    bvec = rng.uniform(-0.1, 0.1, (Fout,)).astype(np.float32)
    gam, bet = rng.uniform(0.5, 1.5, (Fout,)).astype(np.float32), rng.uniform(-0.2, 0.2, (Fout,)).astype(np.float32)
    w0 = torch.from_numpy(rng.standard_normal((B, V, Fout)).astype(np.float32))
    col = 3
    if where == "x":
        x0[b, v, col] *= 256.0
    else:
        w0[b, v, col] *= 256.0
    w = w0.cuda()
    # float64 autograd of the reference formula
    xd = x0.cuda().double().requires_grad_(True)
    Wd, bd = torch.from_numpy(Wn).cuda().double().requires_grad_(True), torch.from_numpy(bvec).cuda().double().requires_grad_(True)
    gd, btd = torch.from_numpy(gam).cuda().double().requires_grad_(True), torch.from_numpy(bet).cuda().double().requires_grad_(True)
    x1 = torch.einsum("uv,bvf->buf", Ld, xd)
    x2 = 2 * torch.einsum("uv,bvf->buf", Ld, x1) - xd
    z = torch.stack((xd, x1, x2), dim=3).reshape(B * V, Fin * 3) @ Wd.t() + bd
    mean, var = z.mean(0), z.var(0, unbiased=False)
    yd = ((z - mean) / torch.sqrt(var + 1e-5) * gd + btd).view(B, V, Fout)
    (yd * w.double()).sum().backward()
    yd = yd.detach()
    print(f"  hub120 {Fin}->{Fout} B {B}: {where}[{b}, {v}, {col}] x 256; max |y64| {float(yd.abs().max()):.3f}")
    errs = {}
    for arith in ("bf16x3", "f16x2"):
        monkeypatch.setattr(ops, "GEMM_ARITH", arith)
        ops.bump_weight_epoch()
        x = x0.cuda().requires_grad_(True)
        cl, bn = torch.nn.Linear(Fin * 3, Fout), torch.nn.BatchNorm1d(Fout)
        with torch.no_grad():
            cl.weight.copy_(torch.from_numpy(Wn))
            cl.bias.copy_(torch.from_numpy(bvec))
            bn.weight.copy_(torch.from_numpy(gam))
            bn.bias.copy_(torch.from_numpy(bet))
        cl, bn = cl.cuda(), bn.cuda().train()
        y = graph_conv_cheby(x, cl, bn, g, Fout, 3)
        (y * w).sum().backward()
        torch.cuda.synchronize()
        assert torch.isfinite(y).all() and torch.isfinite(x.grad).all() and torch.isfinite(cl.weight.grad).all()
        errs[arith] = {"y": float((y.detach().double() - yd).abs().max()), "dX": rel_l2(x.grad, xd.grad),
                       "dW": rel_l2(cl.weight.grad, Wd.grad), "dgamma": rel_l2(bn.weight.grad, gd.grad),
                       "dbeta": rel_l2(bn.bias.grad, btd.grad)}
    tol = {"y": 2e-5 * max(1.0, float(yd.abs().max())), "dX": 1e-4, "dW": 1e-4, "dgamma": 1e-4, "dbeta": 1e-4}
    for k in tol:
        print(f"    {k}: bf16x3 {errs['bf16x3'][k]:.3e}  f16x2 {errs['f16x2'][k]:.3e}  bound {tol[k]:.3e}")
    for k in tol:
        for arith in ("bf16x3", "f16x2"):
            assert errs[arith][k] <= tol[k], (where, spot, Fin, Fout, k, arith, errs[arith][k], tol[k])


# ---- 6. the PoseNet stages directly ------------------------------------------------------------------------------------------

# (bias, residual, BatchNorm: None / "train" / "eval", p_drop); the float64 restatement of a stage is tests/posenet_ref.py
PN_VARIANTS = pnr.PN_VARIANTS
PN_SHAPES = [(32, 0, 32), (36, 33, 68), (64, 64, 4096)]
# input seeds: of the 262 144 elements of the widest case 1 - 2 per BatchNorm variant lie within 1e-5 of the ReLU kink on an
# average draw; with these seeds none does in any variant (counted in float64 on the host)
PN_SEEDS = {(64, 4096, 1): 11, (64, 4096, 3): 169}


def _pn_inputs(B, Br, F, nch, seed):
    d = {k: v.cuda() for k, v in pnr.pn_inputs(B, F, nch, seed).items()}
    pad = torch.arange(Br, B, device="cuda")
    return d, pad


def _pn_fwd(ops, d, B, Br_arg, F, nch, bias, resid, bn, p_drop, poison_rows=None):
    P, R, rnd = d["P"].clone(), d["resid"].clone(), d["rnd"].clone()
    if poison_rows is not None and poison_rows.numel():
        for ch in range(nch):
            _poison(P[ch], poison_rows)
        _poison(R, poison_rows)
        _poison(rnd, poison_rows)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    bnt = None if bn is None else (d["gamma"], d["beta"], rm, rv, 0.1, 1e-5, bn == "train")
    z, a, aT, mean, invstd = ops.pn_stage_fwd(P, nch, B, F, bias=d["bias"] if bias else None, resid=R if resid else None,
                                              bn=bnt, rnd=rnd if (bn and p_drop > 0) else None, p_drop=p_drop, B_real=Br_arg)
    torch.cuda.synchronize()
    return z, a, aT, mean, invstd, rm, rv


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("B,B_real,F", PN_SHAPES)
def test_pn_stage_fwd(ops, monkeypatch, B, B_real, F, nch):
    """ops.pn_stage_fwd against float64 (lib/models/posenet.py:25-38,79-87: sum of partials + bias + residual, BatchNorm1d in
    train / eval mode, ReLU, dropout with the caller's uniform numbers): z, a, mean, invstd and the running statistics (over
    B_real rows) within 1e-5, aT == a.t() bitwise, padding rows of a / aT exactly 0 with P, resid and rnd POISONED there and
    everything bitwise what it is without the poison; the word of a == max |a| over all B rows (NaN and inf left out).
    F = 68 ends in a 4-column block, B = 36 has 3 padding rows."""
    monkeypatch.setattr(ops, "GEMM_ARITH", "f16x2")
    Br = B_real or B
    d, pad = _pn_inputs(B, Br, F, nch, PN_SEEDS.get((B, F, nch), 1))
    for bias, resid, bn, p_drop in PN_VARIANTS:
        what = f"B {B} B_real {B_real} F {F} nch {nch} bias {bias} resid {resid} bn {bn} p_drop {p_drop}"
        print("  " + what)
        z0, a0, aT0, mean0, invstd0, rm0, rv0 = _pn_fwd(ops, d, B, B_real, F, nch, bias, resid, bn, p_drop)
        z, a, aT, mean, invstd, rm, rv = _pn_fwd(ops, d, B, B_real, F, nch, bias, resid, bn, p_drop, pad)
        got = _word(a._p2m_amax)
        assert a._p2m_amax is aT._p2m_amax
        _same("word of a", got, _exact(a))
        _unchanged("word of a", got, _word(a0._p2m_amax))
        assert torch.isfinite(a).all() and torch.equal(aT, a.t()) and torch.equal(a, a0) and torch.equal(aT, aT0)
        assert (a[Br:] == 0).all() and (aT[:, Br:] == 0).all()
        assert torch.equal(z[:Br], z0[:Br])
        # float64
        zd = pnr.z_ref(d["P"], Br, d["bias"] if bias else None, d["resid"] if resid else None)
        _chk("z", (z[:Br].double() - zd).abs().max(), 1e-5)
        ad, _, mu, var, istd = pnr.act_ref(zd, bn, d["gamma"], d["beta"], d["rm"], d["rv"], d["rnd"], p_drop)
        if bn is not None:
            assert torch.equal(mean, mean0) and torch.equal(invstd, invstd0) and torch.equal(rm, rm0) and torch.equal(rv, rv0)
            if bn == "train":
                rmd, rvd = pnr.running_ref(d["rm"], d["rv"], mu, var, Br)
                _chk("running_mean", (rm.double() - rmd).abs().max(), 1e-5)
                _chk("running_var", (rv.double() - rvd).abs().max(), 1e-5)
            else:
                assert torch.equal(rm, d["rm"]) and torch.equal(rv, d["rv"])
            _chk("mean", (mean.double() - mu).abs().max(), 1e-5)
            _chk("invstd", (invstd.double() - istd).abs().max(), 1e-5)
        _chk("a", (a[:Br].double() - ad).abs().max(), 1e-5)
        # the maximum planted at row B_real - 1, last column, and at row 0, column 0 (the column's gamma raised so that the
        # batch normalisation, which caps an outlier at sqrt(B - 1), cannot hide it; its dropout draw set to `keep`)
        for r, c in ((Br - 1, F - 1), (0, 0)):
            dq = {k: v.clone() for k, v in d.items()}
            dq["P"][0, r, c] = 50.0
            dq["gamma"][c] = 8.0
            dq["rnd"][r, c] = 0.9
            _, a, aT, _, _, _, _ = _pn_fwd(ops, dq, B, B_real, F, nch, bias, resid, bn, p_drop, pad)
            assert _argmax(a) == (r, c), (what, r, c, _argmax(a))
            _same(f"planted at ({r}, {c})", _word(a._p2m_amax), _exact(a))
            assert torch.equal(aT, a.t())
        # NaN and inf inside the data rows stay out of the word; where the stage passes them on - no BatchNorm: a = z; eval mode:
        # +inf through a positive gamma and a kept dropout draw (batch statistics of a column that holds one are NaN, which the
        # ReLU's max drops) - a is not finite there
        dq = {k: v.clone() for k, v in d.items()}
        dq["P"][0, 0, 1], dq["P"][0, Br - 1, F - 2] = NAN, INF
        dq["rnd"][Br - 1, F - 2] = 0.9
        _, a, aT, _, _, _, _ = _pn_fwd(ops, dq, B, B_real, F, nch, bias, resid, bn, p_drop, pad)
        print(f"    NaN / inf in P: {int((~torch.isfinite(a)).sum())} elements of a not finite")
        if bn is None:
            assert torch.isnan(a[0, 1]) and torch.isinf(a[Br - 1, F - 2])
        elif bn == "eval":
            assert torch.isinf(a[Br - 1, F - 2])
        _same("NaN / inf inside the data rows", _word(a._p2m_amax), _exact(a))
        assert _bits_equal(aT, a.t()) and (a[Br:] == 0).all()


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("B,B_real,F", PN_SHAPES)
def test_pn_stage_bwd(ops, monkeypatch, B, B_real, F, nch):
    """ops.pn_stage_bwd against float64 autograd of the same lines, on the z / mean / invstd the forward kernel saved: gz within
    2e-5 max(1, max |gz|), dgamma / dbeta / dbias within 1e-5 sqrt(B) max(1, max |.|) in both accumulate modes, gzT == gz.t()
    bitwise, padding rows 0 in and 0 out with P and the addend poisoned there, the word of gz == max |gz| (NaN and inf left out).
    Elements whose float64 pre-activation is within 1e-5 of the ReLU kink are left out of the gz comparison: at most 2 per
    case (PN_SEEDS: the seeds used here give none at all)."""
    monkeypatch.setattr(ops, "GEMM_ARITH", "f16x2")
    Br = B_real or B
    d, pad = _pn_inputs(B, Br, F, nch, PN_SEEDS.get((B, F, nch), 1))
    for bias, resid, bn, p_drop in PN_VARIANTS:
        what = f"B {B} B_real {B_real} F {F} nch {nch} addend {resid} bn {bn} p_drop {p_drop}"
        print("  " + what)
        z, a, aT, mean, invstd, _, _ = _pn_fwd(ops, d, B, B_real, F, nch, bias, resid, bn, p_drop, pad)
        rnd = d["rnd"] if (bn and p_drop > 0) else None

        def bwd(dd, accumulate, poison):
            G, add = dd["G"].clone(), dd["addend"].clone()
            rn = None if rnd is None else dd["rnd"].clone()
            if poison and pad.numel():
                for ch in range(nch):
                    _poison(G[ch], pad)
                _poison(add, pad)
                if rn is not None:
                    _poison(rn, pad)
            init = 1.5 if accumulate else NAN
            dg, db, dbias = (torch.full((F,), init, device="cuda") for _ in range(3))
            bnt = None if bn is None else (dd["z"], mean, invstd, dd["gamma"], dd["beta"], bn == "train")
            gz, gzT = ops.pn_stage_bwd(G, nch, B, F, addend=add if resid else None, bn=bnt, rnd=rn, p_drop=p_drop,
                                       dgamma=dg if bn else None, dbeta=db if bn else None, dbias=dbias, accumulate=accumulate,
                                       B_real=B_real)
            torch.cuda.synchronize()
            return gz, gzT, dg, db, dbias

        d["z"] = z
        # float64 on the saved z: the closed-form backward of tests/posenet_ref.py, which tests/test_posenet_ref_cpu.py holds
        # to torch's float64 autograd of the same lines within 1e-12
        gzd, dgd, dbd, rb, near = pnr.bwd_ref(z[:Br], d["G"].double().sum(0)[:Br], bn, d["gamma"], d["beta"], d["rm"], d["rv"],
                                              d["rnd"], p_drop, d["addend"] if resid else None)
        print(f"    {int(near.sum())} elements within 1e-5 of the ReLU kink")
        assert int(near.sum()) <= 2
        for accumulate in (False, True):
            gz0, gzT0, dg0, db0, dbias0 = bwd(d, accumulate, False)
            gz, gzT, dg, db, dbias = bwd(d, accumulate, True)
            got = _word(gz._p2m_amax)
            _same(f"word of gz (accumulate {accumulate})", got, _exact(gz))
            _unchanged("word of gz", got, _word(gz0._p2m_amax))
            assert gz._p2m_amax is gzT._p2m_amax
            assert torch.isfinite(gz).all() and torch.equal(gzT, gz.t()) and torch.equal(gz, gz0)
            assert (gz[Br:] == 0).all() and (gzT[:, Br:] == 0).all()
            assert torch.equal(dbias, dbias0) and (bn is None or (torch.equal(dg, dg0) and torch.equal(db, db0)))
            base = 1.5 if accumulate else 0.0
            diff = torch.where(near, torch.zeros_like(gzd), gz[:Br].double() - gzd)
            _chk("gz", diff.abs().max(), 2e-5 * max(1.0, float(gzd.abs().max())))
            _chk("dbias", (dbias.double() - base - rb).abs().max(), 1e-5 * np.sqrt(B) * max(1.0, float(rb.abs().max())))
            if bn is not None:
                for nm, gotp, ref in (("dgamma", dg, dgd), ("dbeta", db, dbd)):
                    _chk(nm, (gotp.double() - base - ref).abs().max(), 1e-5 * np.sqrt(B) * max(1.0, float(ref.abs().max())))
        # the maximum of gz planted at row B_real - 1, last column, and at row 0, column 0: the incoming gradient there is 50 and
        # the element is made active (z one standard deviation above the saved mean, gamma 1, beta 0.1, dropout draw `keep`)
        for r, c in ((Br - 1, F - 1), (0, 0)):
            dq = {k: v.clone() for k, v in d.items()}
            dq["G"][0, r, c] = 50.0
            dq["rnd"][r, c] = 0.9
            if bn is not None:
                dq["gamma"][c], dq["beta"][c] = 1.0, 0.1
                dq["z"][r, c] = mean[c] + 1.0 / invstd[c]
            gz, gzT, _, _, _ = bwd(dq, False, True)
            assert _argmax(gz) == (r, c), (what, r, c, _argmax(gz))
            _same(f"planted at ({r}, {c})", _word(gz._p2m_amax), _exact(gz))
            assert torch.equal(gzT, gz.t())
        # NaN and inf in the incoming gradient, at two elements made active in the same way: gz is not finite there (in training
        # mode the whole column) and they stay out of the word
        dq = {k: v.clone() for k, v in d.items()}
        for r, c, val in ((0, 1, NAN), (Br - 1, F - 2, INF)):
            dq["G"][0, r, c] = val
            dq["rnd"][r, c] = 0.9
            if bn is not None:
                dq["gamma"][c], dq["beta"][c] = 1.0, 0.1
                dq["z"][r, c] = mean[c] + 1.0 / invstd[c]
        gz, gzT, _, _, _ = bwd(dq, False, True)
        print(f"    NaN / inf in the incoming gradient: {int((~torch.isfinite(gz)).sum())} elements of gz not finite")
        assert not torch.isfinite(gz[0, 1]) and not torch.isfinite(gz[Br - 1, F - 2])
        _same("NaN / inf inside the data rows", _word(gz._p2m_amax), _exact(gz))
        assert _bits_equal(gzT, gz.t()) and (gz[Br:] == 0).all()
