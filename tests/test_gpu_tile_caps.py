"""-m gpu: the tile kernels (k_basis_tile, k_cheb_tile_gemm, k_cheb_mg_gemm, the per-tile BatchNorm statistics and their
finalize) at the caps of the tile plan (csrc/p2m_common.h: 32 rows, 120 union rows, 896 entries per tile) and on graphs whose
tiles hold rows of very different lengths - tests/tile_plan_ref.py builds the graphs and restates the planner,
tests/test_tile_plan_cpu.py asserts on the CPU that every family reaches what it is meant to reach.

Every check compares a HIP kernel with a float64 dense restatement of the same operation on the device (V <= 2 016), over
every real row of every tile; where an existing test demands bitwise equality with the row kernel, so does this one.  Bounds
are those of the tests these mirror (tests/test_gpu_ops.py: test_cheb_basis_fwd_bwd, test_paired_backward_...,
test_basis_inside_the_contraction_..., test_tile_kernel_sums_...; tests/test_gpu_parity.py:
test_graph_conv_cheby_vs_reference_golden), unchanged.  The order of the file is the order of a careful first run: planner pin,
basis kernel, then the contraction kernels.  Every figure is printed before it is asserted (pytest -s / -rP).

What the library plans for the families (test_planner_pin: equal to the restatement, which supplies the per-tile figures).
Per plan (0 own resolution, 1 un-pooled input, 2 paired operator): tiles / max entries / max padded entries / one-row tiles /
longest row; the caps are 896 entries (992 padded) and 120 union rows = the longest row a plan can hold.

    family          V   real   plan 0                       plan 1                       plan 2
    cliques56      960   560   35 / 896 / 896 / 0 / 56      35 / 896 / 896 / 0 / 56      18 / 896 / 896 / 0 / 56
    cliques56p     960   560   35 / 896 / 896 / 0 / 56      35 / 896 / 896 / 0 / 56      264 / 338 / 344 / 160 / 112
    cliques28      992   588   19 / 896 / 896 / 0 / 28      19 / 896 / 896 / 0 / 28      10 / 896 / 896 / 0 / 28
    cliques29      992   580   20 / 870 / 960 / 0 / 29      20 / 870 / 960 / 0 / 29      10 / 870 / 956 / 0 / 58
    cliques120    2016  1200   180 / 840 / 840 / 10 / 120   172 / 840 / 840 / 0 / 120    90 / 840 / 840 / 0 / 120
    cliques120p   2016  1200   180 / 840 / 840 / 10 / 120   180 / 840 / 840 / 10 / 120   absent
    cliques121    2016  1210   absent                       180 / 847 / 868 / 0 / 121    absent
    hub120        1472   900   31 / 824 / 912 / 1 / 120     30 / 823 / 912 / 0 / 120     absent
    hub120p       1472   900   35 / 838 / 928 / 1 / 120     34 / 838 / 928 / 1 / 120     absent
    hub121        1472   901   absent                       31 / 823 / 912 / 1 / 121     absent
    hub121p       1472   901   absent                       34 / 838 / 928 / 1 / 121     absent
    mixed         1472   648   82 / 873 / 916 / 9 / 120     60 / 873 / 916 / 1 / 120     absent
    mixedp        1472   648   91 / 881 / 924 / 16 / 120    87 / 881 / 924 / 13 / 120    absent
(`p` = all vertices renumbered at random.  cliques(28): tiles of 32 rows and 896 entries at once; mixed: rows of 2 ... 120
entries inside one tile.)"""
import os

import numpy as np
import pytest
import torch

import tile_plan_ref as tp

pytestmark = pytest.mark.gpu

# P2M_TILE_ORDER=tree (read once per process by the library): the compact row order stays the ascending one - the child
# process of test_tree_order_in_a_subprocess runs the planner pin and the basis kernel that way
TREE = os.environ.get("P2M_TILE_ORDER") == "tree"

# (family, batch): B in {1, 3, 5} - never a multiple of the 4 samples a block tile holds; every kernel meets B = 1
CASES = [("cliques56", 3), ("cliques56p", 1), ("cliques28", 5), ("cliques29", 3), ("cliques120", 1), ("cliques120p", 5),
         ("cliques121", 3), ("hub120", 5), ("hub120p", 1), ("hub121", 3), ("hub121p", 5), ("mixed", 1), ("mixedp", 3)]
INDEX = {name: i for i, (name, _) in enumerate(CASES)}


@pytest.fixture(scope="module")
def ops(hip_libs):
    from pose2mesh_release_amd import ops as o
    return o


_ctx = {}


def _case(ops, name):
    """(L, restated plans, device graph, dense float64 L on the device) of a family, once per process."""
    if name not in _ctx:
        L, p = tp.family(name, TREE)
        g = ops.DeviceGraph(L, "cuda:0")
        _ctx[name] = (L, p, g, torch.from_numpy(tp.dense(L)).cuda())
    return _ctx[name]


def _chk(what, err, tol):
    err, tol = float(err), float(tol)
    print(f"    {what}: err {err:.3e}  bound {tol:.3e}")
    assert err <= tol, (what, err, tol)


def _planes64(Ld, Xd):
    """float64 L X and (2 L L - I) X = 2 L (L X) - X  (lib/models/backbones/cheby_graph_conv.py:25,28); Xd: [B, V, F]."""
    T1 = torch.einsum("uv,bvf->buf", Ld, Xd)
    return T1, 2 * torch.einsum("uv,bvf->buf", Ld, T1) - Xd


def _pair(t):
    B, V, F = t.shape
    return t.view(B, V // 2, 2, F).sum(2)


def _existing(p):
    return [k for k in range(3) if p.plan[k] is not None]


# ---- 1. the library's planner against the restatement ----------------------------------------------------------------------

@pytest.mark.parametrize("name,B", CASES)
def test_planner_pin(ops, name, B):
    """p2m_graph_create's fake-vertex rule, locality order and the three greedy tile plans equal the Python restatement:
    counts, tiles per plan (0 = absent) and the compact row order, vertex by vertex."""
    L, p, g, _ = _case(ops, name)
    print(f"  {name}: V {p.V} real {p.n_real} fake {p.n_fake} longest merged row {p.max_row}; library tiles {g.plan_tiles}, "
          f"pair rows {g.n_pair_real}\n    " + p.describe().replace("; ", "\n    "))
    assert (g.V, g.n_real, g.n_fake, g.max_row) == (p.V, p.n_real, p.n_fake, p.max_row)
    assert g.plan_tiles == p.plan_tiles
    assert g.n_pair_real == p.n_pair_real
    assert np.array_equal(g.real_ids_host().astype(np.int64), p.real_order)
    assert np.array_equal(np.sort(g.fake_ids_host().astype(np.int64)), np.where(p.fake)[0])


# ---- 2. k_basis_tile -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B", CASES)
def test_basis_tile_kernel(ops, name, B):
    """ops.cheb_basis_fwd_real (k_basis_tile where the plan exists, the row kernel where it does not), both shifts: bitwise
    the real rows of the row kernel, and within the bounds of test_cheb_basis_fwd_bwd (2e-6 / 4e-6) of float64 dense
    L X, 2 L (L X) - X.  ops.cheb_basis_pair on the paired plan: the pair sums of the float64 planes, bound 1e-5 of
    test_paired_backward_equals_fine_backward_pair_summed; where the paired plan is absent the library refuses."""
    from pose2mesh_release_amd._lib import P2MError
    L, p, g, Ld = _case(ops, name)
    V = p.V
    order = torch.as_tensor(p.real_order, device="cuda")
    for shift in (0, 1):
        F = (32, 64, 128, 256)[(INDEX[name] + shift) % 4]
        gen = torch.Generator().manual_seed(1000 * INDEX[name] + shift)
        X = torch.randn(B * (V >> shift), F, generator=gen).cuda()
        T1, T2 = ops.cheb_basis_fwd(g, X, B, F, shift)
        T1c, T2c = ops.cheb_basis_fwd_real(g, X, B, F, shift)
        torch.cuda.synchronize()
        print(f"  {name} shift {shift} F {F} B {B} tiles {g.plan_tiles[shift]}")
        assert torch.equal(T1c, T1.view(B, V, F)[:, order].reshape(-1, F))
        assert torch.equal(T2c, T2.view(B, V, F)[:, order].reshape(-1, F))
        Xd = X.double().view(B, V >> shift, F)
        if shift:
            Xd = Xd.repeat_interleave(2, dim=1)
        T1d, T2d = _planes64(Ld, Xd)
        _chk("L X vs float64", (T1c.view(B, -1, F).double() - T1d[:, order]).abs().max(), 2e-6 * max(1.0, T1d.abs().max().item()))
        _chk("L2 X vs float64", (T2c.view(B, -1, F).double() - T2d[:, order]).abs().max(), 4e-6 * max(1.0, T2d.abs().max().item()))
    F = (64, 128, 32, 256)[INDEX[name] % 4]
    G = torch.randn(B * V, F, generator=torch.Generator().manual_seed(77 + INDEX[name])).cuda()
    if p.plan[2] is None:
        assert not g.pair and g.n_pair_real == 0
        with pytest.raises(P2MError):
            ops.cheb_basis_pair(g, G, B, F)
        return
    assert g.pair
    P1c, P2c = ops.cheb_basis_pair(g, G, B, F)
    torch.cuda.synchronize()
    T1d, T2d = _planes64(Ld, G.double().view(B, V, F))
    po = torch.as_tensor(p.pair_order, device="cuda")
    print(f"  {name} paired F {F} B {B} tiles {g.plan_tiles[2]}")
    for what, got, ref in (("S L g", P1c, _pair(T1d)[:, po]), ("S L2 g", P2c, _pair(T2d)[:, po])):
        _chk(what + " vs float64", (got.view(B, -1, F).double() - ref).abs().max(), 1e-5 * max(1.0, ref.abs().max().item()))


# ---- 3. + 4. the contraction kernels and their per-tile statistics -----------------------------------------------------------

def _clear_of_the_kink(y, co):
    """Move the few elements of y whose activation mask [y scale + shift > 0] is within round-off of flipping, so that the
    kernel's fp32 fma and the float64 reference agree on every mask bit."""
    for _ in range(4):
        v = y.double() * co[2].double() + co[3].double()
        near = v.abs() < 1e-4
        if not near.any():
            return y
        y = torch.where(near, y + 0.03125, y)
    raise AssertionError("could not move the inputs off the activation kink")


def _tile_gemm_modes(ops, monkeypatch, name, B, plan, arith, Ka, N):
    from pose2mesh_release_amd import _lib
    L, p, g, Ld = _case(ops, name)
    monkeypatch.setattr(ops, "GEMM_ARITH", arith)
    monkeypatch.setattr(ops, "TILE_GEMM", True)
    monkeypatch.setattr(ops, "BN_FUSE", True)
    V = p.V
    xr = V // 2 if plan == 1 else V                      # rows of X per sample
    cr = V // 2 if plan == 2 else V                      # rows of C per sample
    rows_np = p.pair_order if plan == 2 else p.real_order
    rows = torch.as_tensor(rows_np, device="cuda")
    other = torch.ones(cr, dtype=torch.bool, device="cuda")
    other[rows] = False
    n, ntiles = rows.numel(), len(p.plan[plan])
    mg = bool(_lib.hip().p2m_cheb_tile_gemm_mg(ops.arith_code(), N))
    print(f"  {name} plan {plan} {arith} Ka {Ka} N {N} B {B}: {ntiles} tiles, {'matrix-core' if mg else 'VALU'} gather")
    assert g.plan_tiles[plan] == ntiles and ops.tile_gemm_ok(g, plan, Ka, N)
    gen = torch.Generator().manual_seed(31 * INDEX[name] + 7 * plan + Ka + N)
    X = torch.randn(B * xr, Ka, generator=gen).cuda()
    Wt = (torch.randn(3 * Ka, N, generator=gen) / (3 * Ka) ** 0.5).cuda()
    bias = torch.randn(N, generator=gen).cuda()
    add = torch.randn(B * cr, N, generator=gen).cuda()
    Bx = ops.weight_split(Wt)

    def operands(Xin):
        """(A0 as the kernel takes it, float64 [A0 | plane 1 | plane 2] of [B, cr, 3 Ka]) for a gather source Xin."""
        Xd = Xin.double().view(B, xr, Ka)
        if plan == 1:
            Xd = Xd.repeat_interleave(2, dim=1)
        T1d, T2d = _planes64(Ld, Xd)
        if plan == 2:
            A0 = Xin.view(B, V // 2, 2, Ka).sum(2).reshape(-1, Ka).contiguous()     # S X: one fp32 addition, exact in float64
            return A0, torch.cat((A0.double().view(B, cr, Ka), _pair(T1d), _pair(T2d)), dim=2)
        return Xin, torch.cat((Xd, T1d, T2d), dim=2)

    A0, Pd = operands(X)
    yd = Pd @ Wt.double() + bias.double()                # [B, cr, N]

    def check_C(what, y, ref):
        assert torch.isfinite(y).all()
        assert (y.view(B, cr, N)[:, other] == 7.0).all(), what + ": a row outside the plan was written"
        _chk(what, (y.view(B, cr, N)[:, rows].double() - ref[:, rows]).abs().max(), 2e-5 * max(1.0, ref.abs().max().item()))

    def fresh():
        return torch.full((B * cr, N), 7.0, device="cuda")

    # plain
    y = fresh()
    ops.cheb_tile_gemm(g, plan, X, A0, Ka, Bx, bias, None, y, N, B)
    check_C("C", y, yd)
    # statistics + planes out
    y = fresh()
    st, planes = ops.cheb_tile_gemm(g, plan, X, A0, Ka, Bx, bias, None, y, N, B, stats=True, want_planes=True)
    torch.cuda.synchronize()
    check_C("C (stats, planes out)", y, yd)
    T1c, T2c = ops.cheb_basis_pair(g, X, B, Ka) if plan == 2 else ops.cheb_basis_fwd_real(g, X, B, Ka, plan)
    if not mg:                          # VALU gather: the fmaf chain of the basis kernel, bit for bit
        assert torch.equal(planes[0], T1c) and torch.equal(planes[1], T2c)
    else:                               # matrix-core gather: fp32 sums in another order (test_basis_inside_the_contraction_...)
        tol = 2e-6 if arith == "f16x2" else 5e-7
        for got, ref in ((planes[0], T1c), (planes[1], T2c)):
            _chk("plane vs basis kernel", (got - ref).abs().max(), tol * max(1.0, ref.abs().max().item()))
    # per-tile statistics: (sum, M2 about the tile mean) of exactly the rows the restatement puts into each tile.  Bound:
    # every stored value is within e = 2e-5 max(1, |y|max) of float64 (asserted above), so a tile's sum of cnt <= 32 values
    # is within cnt e, plus the fp32 summation's own cnt 2^-24 (cnt |y|max) < cnt e: 2 cnt e.  d M2 / d y = 2 (y - mean),
    # |y - mean| <= 2 |y|max: 4 cnt |y|max e (the summation's round-off is a tenth of that).  A tile of ONE row: M2 = 0.
    tiles = np.array(p.plan[plan])
    cnt = torch.as_tensor(tiles[:, 1], device="cuda").double()
    tile_of = torch.as_tensor(np.repeat(np.arange(ntiles), tiles[:, 1]), device="cuda")
    ydc = yd[:, rows]
    s64 = torch.zeros(B, ntiles, N, dtype=torch.float64, device="cuda").index_add_(1, tile_of, ydc)
    m64 = s64 / cnt[None, :, None]
    q64 = torch.zeros_like(s64).index_add_(1, tile_of, (ydc - m64[:, tile_of]) ** 2)
    stv = st.view(B, ntiles, 2, N).double()
    ymax = max(1.0, yd.abs().max().item())
    e = 2e-5 * ymax
    _chk("tile sums / (2 cnt e)", ((stv[:, :, 0] - s64).abs() / (2 * cnt[None, :, None] * e)).max(), 1.0)
    _chk("tile M2 / (4 cnt |y|max e)", ((stv[:, :, 1] - q64).abs() / (4 * cnt[None, :, None] * ymax * e)).max(), 1.0)
    one = torch.as_tensor(np.where(tiles[:, 1] == 1)[0], device="cuda")
    if one.numel():
        print(f"    {one.numel()} one-row tiles: max |M2| {stv[:, one, 1].abs().max().item():.3e}")
        assert (stv[:, one, 1] == 0).all()
    if plan < 2:
        # ... and the finalize: batch mean / biased variance over all B V rows (fake rows through row set 2, as the network does)
        gamma, beta = (torch.rand(N, generator=gen) + 0.5).cuda(), torch.randn(N, generator=gen).cuda()
        We = ops.weight_eff(Wt, Ka, N, g.fake_a, g.fake_b)
        st2 = ops.gemm_planes_rows(g, 2, B, [X], Ka, plan, False, We, bias, None, y, N, True)
        co = ops.bn_finalize_tiles(g, plan, B, st, st2, gamma, beta, None, None, 0.1, 1e-5)
        torch.cuda.synchronize()
        _chk("fake rows (row set 2)", (y.view(B, cr, N)[:, other].double() - yd[:, other]).abs().max(), 2e-5 * ymax)
        flat = yd.reshape(-1, N)
        mean, var = flat.mean(0), flat.var(0, unbiased=False)
        invstd = 1.0 / torch.sqrt(var + 1e-5)
        co64 = torch.stack((mean, invstd, gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd))
        _chk("bn_finalize_tiles", (co.double() - co64).abs().max(), 2e-5 * max(1.0, co64.abs().max().item()))
    # addend
    y = fresh()
    ops.cheb_tile_gemm(g, plan, X, A0, Ka, Bx, bias, add, y, N, B)
    check_C("C + addend", y, yd + add.double().view(B, cr, N))
    # fused activation
    sc, sh = (torch.rand(N, generator=gen) + 0.5).cuda(), torch.randn(N, generator=gen).cuda()
    y = fresh()
    ops.cheb_tile_gemm(g, plan, X, A0, Ka, Bx, bias, None, y, N, B, act=(sc, sh, True))
    check_C("relu(C scale + shift)", y, (yd * sc.double() + sh.double()).clamp_min(0))
    # activation on load: X (and A0) hold a raw conv output, the operand is relu(raw * scale + shift)
    raw = (torch.randn(B * xr, Ka, generator=gen) * 3.0 + 0.7).cuda()
    isc, ish = (torch.randn(Ka, generator=gen) * 0.8).cuda(), torch.randn(Ka, generator=gen).cuda()
    act64 = (raw.double() * isc.double() + ish.double()).clamp_min(0)
    if plan == 2:
        raw0 = raw.view(B, V // 2, 2, Ka)[:, :, 0].reshape(-1, Ka).contiguous()      # any raw [B, V/2, Ka] tensor will do
        a0_64 = (raw0.double() * isc.double() + ish.double()).clamp_min(0).view(B, cr, Ka)
        T1d, T2d = _planes64(Ld, act64.view(B, V, Ka))
        Pa = torch.cat((a0_64, _pair(T1d), _pair(T2d)), dim=2)
    else:
        raw0 = raw
        xa = act64.view(B, xr, Ka)
        if plan == 1:
            xa = xa.repeat_interleave(2, dim=1)
        Pa = torch.cat((xa,) + _planes64(Ld, xa), dim=2)
    word = ops.act_bound(isc, ish, ops.amax_of(raw), ops.new_amax("cuda:0")) if arith == "f16x2" else None
    y = fresh()
    ops.cheb_tile_gemm(g, plan, raw, raw0, Ka, Bx, bias, None, y, N, B, amax=word, in_act=(isc, ish))
    check_C("C, activation on load", y, Pa @ Wt.double() + bias.double())
    # the BatchNorm-backward reduction of the layer in front, fused into the store of C (three bf16 slices, N <= 128)
    if arith == "bf16x3" and N <= 128:
        got = ops.bnr_parts(g, plan, N, B, X.device)
        assert got is not None
        part, nfake = got
        part.fill_(float("nan"))                          # every slot of the tile kernel's share must be written
        yp = torch.randn(B * cr, N, generator=gen).cuda()                 # raw output of the conv in front
        gm_, bt_ = (torch.rand(N, generator=gen) + 0.5).cuda(), torch.randn(N, generator=gen).cuda()
        mu, var = yp.mean(0), yp.var(0, unbiased=False)
        istd = 1.0 / torch.sqrt(var + 1e-5)
        co = torch.stack([mu, istd, gm_ * istd, bt_ - mu * gm_ * istd]).contiguous()
        yp = _clear_of_the_kink(yp, co).contiguous()
        for addend in (None, add):
            part[nfake:].fill_(float("nan"))
            y = fresh()
            ops.cheb_tile_gemm(g, plan, X, A0, Ka, Bx, None, addend, y, N, B, want_planes=True, bnr=(yp, co, part[nfake:]))
            torch.cuda.synchronize()
            ref = yd - bias.double() + (0 if addend is None else addend.double().view(B, cr, N))
            check_C("C (bnr%s)" % ("" if addend is None else ", addend"), y, ref)
            assert torch.isfinite(part[nfake:]).all()
            m = (yp.double() * co[2].double() + co[3].double()) > 0
            gmask = torch.where(m, y.double(), torch.zeros_like(y, dtype=torch.float64)).view(B, cr, N)[:, rows]
            yhat = ((yp.double() - mu.double()) * istd.double()).view(B, cr, N)[:, rows]
            sums = part[nfake:].double().sum(0)
            for what, gotv, r64 in (("sum g m", sums[0], gmask.sum((0, 1))), ("sum g m yhat", sums[1], (gmask * yhat).sum((0, 1)))):
                _chk(what, (gotv - r64).abs().max(), 2e-5 * r64.abs().max().item())


def _shape(name, plan, k):
    """Ka in {32, 128, 256} and the narrow width in {64, 128}, rotated over families, plans and arithmetics."""
    i = INDEX[name]
    return (32, 128, 256)[(i + plan + k) % 3], (64, 128)[(i + plan) % 2]


@pytest.mark.parametrize("name,B", CASES)
def test_tile_gemm_three_bf16_slices(ops, monkeypatch, name, B):
    """p2m_cheb_tile_gemm, bf16x3, N <= 128 (k_cheb_tile_gemm with the LDS-staged epilogue and the fused BatchNorm-backward
    sums) on every plan the level has: C on the plan's rows against float64 [A0 | L X | L2 X] W + bias, rows outside the plan
    untouched, addend, fused activation, activation on load, planes bitwise the basis kernel's, per-tile statistics and
    their finalize, the bnr partial sums with every slot pre-filled with NaN."""
    p = _case(ops, name)[1]
    for plan in _existing(p):
        Ka, N = _shape(name, plan, 0)
        _tile_gemm_modes(ops, monkeypatch, name, B, plan, "bf16x3", Ka, N)


@pytest.mark.parametrize("name,B", CASES)
def test_tile_gemm_matrix_core_gather(ops, monkeypatch, name, B):
    """The same on k_cheb_mg_gemm (f16x2, N <= 128: the tile's operator as a dense [64][128] fp16 block - with plan 1 the two
    entries of a row that share an un-pooled source fold into one coefficient); planes within 2e-6 of the basis kernel's."""
    p = _case(ops, name)[1]
    for plan in _existing(p):
        Ka, N = _shape(name, plan, 1)
        _tile_gemm_modes(ops, monkeypatch, name, B, plan, "f16x2", Ka, N)


@pytest.mark.parametrize("name,B", CASES)
def test_tile_gemm_wide_output(ops, monkeypatch, name, B):
    """N = 256 (the VALU gather with the register epilogue, 4 producer waves) in both slice arithmetics, alternating."""
    p = _case(ops, name)[1]
    for plan in _existing(p):
        Ka, _ = _shape(name, plan, 2)
        _tile_gemm_modes(ops, monkeypatch, name, B, plan, ("bf16x3", "f16x2")[(INDEX[name] + plan) % 2], Ka, 256)


# ---- 5. dispatch on levels where only some of the three plans exist ----------------------------------------------------------

MISSING = [("cliques121", 3), ("hub121", 3), ("hub121p", 1), ("hub120", 5)]


@pytest.mark.parametrize("name,B", MISSING)
@pytest.mark.parametrize("tile_gemm", ["auto", True])
def test_dispatch_with_plans_missing(ops, monkeypatch, name, B, tile_gemm):
    """tile_gemm_ok says yes exactly for the plans that exist (P2M_TILE_GEMM=1), fold_act_ok never for a conv whose own plan
    is absent; ops.conv_split (the dispatch of the network's split levels) gives the float64 conv on ALL rows for an own
    and an un-pooled input whichever of its two forms it picks - on cliques(121) / hub(121) the own-resolution conv has no
    plan and the un-pooled one has."""
    L, p, g, Ld = _case(ops, name)
    V = p.V
    assert g.split and not g.pair and p.plan[2] is None
    for arith in ("bf16x3", "f16x2"):
        monkeypatch.setattr(ops, "GEMM_ARITH", arith)
        monkeypatch.setattr(ops, "TILE_GEMM", True)
        for plan in range(3):
            for Ka, N in ((128, 128), (64, 128), (256, 256), (32, 64)):
                assert bool(ops.tile_gemm_ok(g, plan, Ka, N)) == (p.plan[plan] is not None), (plan, Ka, N)
        for tg in ("auto", True, "0"):
            monkeypatch.setattr(ops, "TILE_GEMM", tg)
            for Ka, N in ((128, 128), (64, 128), (256, 256), (32, 64)):
                for narrow in (False, True):
                    if ops.fold_act_ok(g, Ka, N, B, narrow=narrow):
                        assert p.plan[0] is not None and not narrow, (tg, Ka, N)
                for plan in range(3):
                    if ops.tile_gemm_ok(g, plan, Ka, N, B=B):
                        assert p.plan[plan] is not None
        monkeypatch.setattr(ops, "TILE_GEMM", tile_gemm)
        for shift, (Ka, N) in ((0, (128, 128)), (1, (64, 128))):
            gen = torch.Generator().manual_seed(5 * INDEX[name] + shift)
            X = torch.randn(B * (V >> shift), Ka, generator=gen).cuda()
            Wt = (torch.randn(3 * Ka, N, generator=gen) / (3 * Ka) ** 0.5).cuda()
            bias = torch.randn(N, generator=gen).cuda()
            C = torch.full((B * V, N), float("nan"), device="cuda")
            T1c, T2c, st1, st2, tiled = ops.conv_split(g, B, X, Ka, shift, Wt, bias, None, C, N, g.fake_a, g.fake_b, stats=True,
                                                       want_planes=True)
            torch.cuda.synchronize()
            print(f"  {name} {arith} TILE_GEMM={tile_gemm} shift {shift}: tile kernel {tiled}")
            assert tiled == bool(ops.tile_gemm_ok(g, shift, Ka, N, True, B=B))
            if tile_gemm is True:
                assert tiled == (p.plan[shift] is not None)
            Xd = X.double().view(B, V >> shift, Ka)
            if shift:
                Xd = Xd.repeat_interleave(2, dim=1)
            T1d, T2d = _planes64(Ld, Xd)
            yd = torch.cat((Xd, T1d, T2d), dim=2) @ Wt.double() + bias.double()
            _chk("conv_split C, all rows", (C.view(B, V, N).double() - yd).abs().max(), 2e-5 * max(1.0, yd.abs().max().item()))
            order = torch.as_tensor(p.real_order, device="cuda")
            tol = (2e-6, 4e-6)
            for k, (got, ref) in enumerate(((T1c, T1d), (T2c, T2d))):
                _chk("plane %d" % (k + 1), (got.view(B, -1, Ka).double() - ref[:, order]).abs().max(),
                     tol[k] * max(1.0, ref.abs().max().item()))
            gamma, beta = (torch.rand(N, generator=gen) + 0.5).cuda(), torch.randn(N, generator=gen).cuda()
            fin = ops.bn_finalize_tiles if tiled else ops.bn_finalize_rows
            co = fin(g, shift, B, st1, st2, gamma, beta, None, None, 0.1, 1e-5) if tiled else \
                fin(g, B, st1, st2, gamma, beta, None, None, 0.1, 1e-5)
            flat = yd.reshape(-1, N)
            mean, var = flat.mean(0), flat.var(0, unbiased=False)
            invstd = 1.0 / torch.sqrt(var + 1e-5)
            co64 = torch.stack((mean, invstd, gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd))
            _chk("statistics finalize", (co.double() - co64).abs().max(), 2e-5 * max(1.0, co64.abs().max().item()))


@pytest.mark.parametrize("name,B", MISSING)
@pytest.mark.parametrize("tile_gemm", ["auto", True])
@pytest.mark.parametrize("Fin,Fout", [(128, 128), (64, 128)])
def test_graph_conv_cheby_with_plans_missing(ops, monkeypatch, name, B, tile_gemm, Fin, Fout):
    """cheby_graph_conv.graph_conv_cheby, train mode, forward + backward on these levels against float64 torch autograd of
    the reference formula (lib/models/backbones/cheby_graph_conv.py:16-39): y, dX, dW, dgamma, dbeta, running statistics -
    inputs and bounds of test_graph_conv_cheby_vs_reference_golden."""
    from pose2mesh_release_amd.cheby_graph_conv import graph_conv_cheby
    from helpers import rel_l2
    L, p, g, Ld = _case(ops, name)
    monkeypatch.setattr(ops, "TILE_GEMM", tile_gemm)
    V = p.V
    rng = np.random.default_rng(300 + INDEX[name] + Fin)
    x = torch.from_numpy(rng.standard_normal((B, V, Fin)).astype(np.float32)).cuda().requires_grad_(True)
    cl = torch.nn.Linear(Fin * 3, Fout)
    bn = torch.nn.BatchNorm1d(Fout)
    with torch.no_grad():
        cl.weight.copy_(torch.from_numpy(rng.uniform(-0.1, 0.1, cl.weight.shape).astype(np.float32)))
        cl.bias.copy_(torch.from_numpy(rng.uniform(-0.1, 0.1, cl.bias.shape).astype(np.float32)))
        bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, (Fout,)).astype(np.float32)))
        bn.bias.copy_(torch.from_numpy(rng.uniform(-0.2, 0.2, (Fout,)).astype(np.float32)))
    cl, bn = cl.cuda(), bn.cuda().train()
    y = graph_conv_cheby(x, cl, bn, g, Fout, 3)
    w = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32)).cuda()
    (y * w).sum().backward()
    torch.cuda.synchronize()
    # float64 autograd of the reference formula
    xd = x.detach().double().requires_grad_(True)
    Wd, bd = cl.weight.detach().double().requires_grad_(True), cl.bias.detach().double().requires_grad_(True)
    gd, btd = bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True)
    x1 = torch.einsum("uv,bvf->buf", Ld, xd)
    x2 = 2 * torch.einsum("uv,bvf->buf", Ld, x1) - xd
    z = torch.stack((xd, x1, x2), dim=3).reshape(B * V, Fin * 3) @ Wd.t() + bd
    mean, var = z.mean(0), z.var(0, unbiased=False)
    yd = ((z - mean) / torch.sqrt(var + bn.eps) * gd + btd).view(B, V, Fout)
    (yd * w.double()).sum().backward()
    print(f"  {name} {Fin}->{Fout} B {B} TILE_GEMM={tile_gemm}")
    _chk("y", (y.detach().double() - yd.detach()).abs().max(), 2e-5)
    _chk("dX", rel_l2(x.grad, xd.grad), 1e-4)
    _chk("dW", rel_l2(cl.weight.grad, Wd.grad), 1e-4)
    _chk("dgamma", rel_l2(bn.weight.grad, gd.grad), 1e-4)
    _chk("dbeta", rel_l2(bn.bias.grad, btd.grad), 1e-4)
    M = B * V
    _chk("running_mean", (bn.running_mean.double() - 0.1 * mean.detach()).abs().max(), 1e-5)
    _chk("running_var", (bn.running_var.double() - (0.9 + 0.1 * var.detach() * M / (M - 1))).abs().max(), 1e-5)


# ---- 6. the coarsening-tree order ---------------------------------------------------------------------------------------

def test_tree_order_in_a_subprocess(hip_libs):
    """P2M_TILE_ORDER=tree is read once per process by the library: the planner pin and the basis kernel on two families
    run in a child process, the restatement skipping its locality order."""
    import subprocess
    import sys
    child_env = dict(os.environ, P2M_TILE_ORDER="tree")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "(planner_pin or basis_tile_kernel) and (hub120p or mixedp)"],
                       env=child_env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "4 passed" in r.stdout
