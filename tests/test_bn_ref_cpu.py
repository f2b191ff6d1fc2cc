"""CPU: pins tests/bn_ref.py (the float64 restatement the GPU tests of csrc/bn.hip compare with) to torch float64 autograd of
F.batch_norm + F.relu + F.interpolate(mode="linear") + repeat_interleave, its "f32" resize weights to fp32 F.interpolate,
and checks the conditions the input generators of tests/test_gpu_bn.py promise (dyadic coefficients and fp32 headroom of
the exact regime, the margin around 0 of the rounding regime and of the chain cases, the shape of the row-map levels)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import bn_ref
import test_gpu_bn as gb

TOL = 1e-12


def _autograd(y, co_src, resid, gx, rshift, training, relu):
    """float64 autograd reference and the coefficient block that belongs to it"""
    gamma, beta, rm, rv = co_src
    ref = gb.chain_reference(y, gamma, beta, rm, rv, resid, gx, rshift, training, relu)
    yd = y.double()
    if training:
        mean, var = yd.mean(0), yd.var(0, unbiased=False)
    else:
        mean, var = rm.double(), rv.double()
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    scale = gamma.double() * invstd
    co = torch.stack([mean, invstd, scale, beta.double() - mean * scale]).numpy()
    return ref, co


@pytest.mark.parametrize("Fres,Fd", gb.RESIZE_PAIRS + ((36, 36), (5, 5)))
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [0, 1])
def test_restatement_against_autograd(Fres, Fd, training, relu):
    for M, rshift in ((40, 0), (41, 1)):                     # odd M with res_shift = 1: the last parent has one child
        y, gamma, beta, rm, rv, resid, gx = gb.chain_inputs(M, Fd, Fres, rshift, 7)
        ref, co = _autograd(y, (gamma, beta, rm, rv), resid, gx, rshift, training, relu)
        x = bn_ref.act_fwd(y, co, relu, resid, Fres, rshift)
        assert np.abs(x - ref["x"].numpy()).max() <= TOL
        db, dg = bn_ref.bwd_sums(gx, y, co, relu)
        assert np.abs(db - ref["dbeta"].numpy()).max() <= TOL and np.abs(dg - ref["dgamma"].numpy()).max() <= TOL
        coef = np.stack([db, dg]) / M if training else None
        gy = bn_ref.bwd_apply(gx, y, co, gamma, coef, relu)
        assert np.abs(gy - ref["gy"].numpy()).max() <= TOL
        # residual gradient: un-pool transpose (pair sums, the odd last row alone), then the resize transpose
        G = bn_ref.f64(gx)
        if rshift:
            Gs = bn_ref.pair_sum(G[:M // 2 * 2])
            if M % 2:
                Gs = np.concatenate([Gs, G[M - 1:]], 0)
        else:
            Gs = G
        dres = Gs if Fres == Fd else bn_ref.lerp_transpose(Gs, Fd, Fres)
        assert np.abs(dres - ref["dres"].numpy()).max() <= TOL
        if not training:
            ec = bn_ref.eval_coeffs(gamma.double(), beta.double(), rm.double(), rv.double(), 1e-5)
            # (eps enters as the fp32 number the C ABI receives: 1e-5 against float32(1e-5), 2.5e-8 relative)
            assert np.abs(ec - co).max() <= 1e-7 and np.array_equal(ec[0], co[0])


@pytest.mark.parametrize("Fres,Fd", gb.RESIZE_PAIRS)
def test_f32_weights_are_atens(Fres, Fd):
    """The "f32" weights are bit for bit what fp32 F.interpolate multiplies with (a one-hot row reads them out), and they
    stay within three roundings of src <= Fres of the float64 weights (the term the GPU bound adds)."""
    i0, i1, w = bn_ref.resize_weights(Fd, Fres, "f32")
    out = Fn.interpolate(torch.eye(Fres).unsqueeze(0), size=Fd, mode="linear").squeeze(0).numpy().T      # [Fd, Fres]
    W32 = np.zeros((Fd, Fres), dtype=np.float32)
    w32 = w.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), w)
    for j in range(Fd):
        W32[j, i0[j]] += np.float32(1) - w32[j]
        W32[j, i1[j]] += w32[j]
    assert np.array_equal(out, W32)
    W64 = bn_ref.resize_matrix(Fd, Fres, "f64")
    assert np.abs(bn_ref.resize_matrix(Fd, Fres, "f32") - W64).max() <= 3 * 2.0 ** -24 * Fres
    if gb.dyadic_ratio(Fres, Fd):
        assert np.array_equal(bn_ref.resize_matrix(Fd, Fres, "f32"), W64)
    # the forward against fp32 F.interpolate on real data: fp32 round-off of two products
    r = torch.randn(5, Fres, generator=torch.Generator().manual_seed(Fres))
    ref = Fn.interpolate(r.unsqueeze(0), size=Fd, mode="linear").squeeze(0).numpy()
    assert np.abs(bn_ref.resize(r, Fd, "f32") - ref).max() <= 3 * 2.0 ** -24 * float(r.abs().max())
    assert np.array_equal(bn_ref.lerp_transpose(np.eye(Fd), Fd, Fres, "f32"), bn_ref.resize_matrix(Fd, Fres, "f32"))


def test_class_forms_against_the_full_computation():
    """A full tensor whose class members are identical, against its holed twin in class-sum form: the class forms give the
    full computation's statistics, class sums of its gy, and pair sums that leave the holes out."""
    rng = np.random.default_rng(3)
    V, B, F = 16, 3, 5
    rep = np.arange(V)
    rep[4:8] = 4
    rep[10:12] = 10
    w = bn_ref.class_weights(rep)
    assert w.tolist() == [1, 1, 1, 1, 4, 0, 0, 0, 1, 1, 2, 0, 1, 1, 1, 1]
    M = B * V
    y = rng.standard_normal((B, V, F))[:, rep].reshape(M, F)
    gx = rng.standard_normal((M, F))
    gamma = rng.standard_normal(F)
    mean, var = y.mean(0), y.var(0)
    invstd = 1 / np.sqrt(var + 1e-5)
    co = np.stack([mean, invstd, gamma * invstd, 0.1 - mean * gamma * invstd])
    live = np.tile(w != 0, B)
    db, dg = bn_ref.bwd_sums(gx, y, co, 1)
    gy = bn_ref.bwd_apply(gx, y, co, gamma, np.stack([db, dg]) / M, 1)
    g_cls = bn_ref.class_reduce(gx, w)
    assert np.array_equal(g_cls[~live], np.zeros_like(g_cls[~live]))
    yh, gh = np.where(live[:, None], y, np.nan), np.where(live[:, None], g_cls, np.nan)
    dbc, dgc = bn_ref.bwd_sums_classes(gh, yh, co, 1, w)
    assert np.abs(dbc - db).max() <= TOL and np.abs(dgc - dg).max() <= TOL
    gyc, lv = bn_ref.bwd_apply_classes(gh, yh, co, gamma, np.stack([db, dg]) / M, 1, w)
    assert np.array_equal(lv, live) and np.isfinite(gyc).all()
    assert np.abs(gyc - bn_ref.class_reduce(gy, w)).max() <= TOL
    x, _ = bn_ref.act_fwd_classes(yh, co, 1, w)
    assert np.array_equal(x[live], bn_ref.act_fwd(y, co, 1)[live])
    ps, lp = bn_ref.pair_sum_classes(np.where(live[:, None], gyc, np.nan), w)
    assert np.abs(ps - bn_ref.pair_sum(gyc)).max() == 0 and lp.tolist() == [True, True, True, False, True, True, True, True] * B
    # weighted statistics of the representatives = the statistics over every member
    ids = np.array([4, 10])
    st = bn_ref.stats_rows_w(yh, ids, w[ids], B, V)
    members = y.reshape(B, V, F)[:, [4, 5, 6, 7, 10, 11]]
    assert np.abs(st[:, 0] - members.sum(1)).max() <= TOL
    assert np.abs(st[:, 1] - ((members - members.mean(1, keepdims=True)) ** 2).sum(1)).max() <= TOL


ALL_F = sorted(set(gb.MAIN_F + gb.V4_F + gb.SCALAR_F + gb.EXTRA_FWD_F + gb.TEMPLATE_F + gb.GENERIC_F))


@pytest.mark.parametrize("F", ALL_F)
def test_exact_generator(F):
    """Dyadic coefficients, small integers, planted pre-activations of exactly 0 that carry gradient, and headroom: every
    term and every partial sum of the exact regime is an fp32 number."""
    M = 1000
    for seed in (11, 21, 51, 61, 71):
        c = gb.exact_case(M, F, seed)
        assert gb.is_dyadic_block(c["co"], c["gamma"], c["beta"])
        if F >= 6:
            assert set(c["gamma"].tolist()) == set(gb.GAMMAS)
        for a in (c["y"], c["gx"]):
            assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 4
        pre = bn_ref.preact(c["y"], c["co"])
        zero = pre == 0
        assert c["planted"].sum() > 0 and zero[c["planted"]].all() and (c["gx"][c["planted"]] != 0).all()
        assert (c["y"] == 0).any() and (c["gx"] == 0).any()
        for relu in (0, 1):
            assert gb.exact_headroom(c["gx"], c["y"], c["co"], relu, 8.0) < 2.0 ** 24
            db, dg = bn_ref.bwd_sums(c["gx"], c["y"], c["co"], relu)
            assert bn_ref.representable_f32(db).all() and bn_ref.representable_f32(dg).all()
        x = bn_ref.act_fwd(c["y"], c["co"], 1, gb.residual_rows("exact", M, 2 * F, 12), 2 * F, 0)
        assert bn_ref.representable_f32(x).all()
        coef = gb._coef_for("exact", F, 52)
        assert np.array_equal(coef * 4, np.round(coef * 4))
        assert bn_ref.representable_f32(bn_ref.bwd_apply(c["gx"], c["y"], c["co"], c["gamma"], coef, 1)).all()
    # the bound on the rows an exact-regime column can take: 4 * 10 per row in units of 1/2
    assert 2 * 4 * 10 * 262145 > 2 ** 24        # (which is why the large cases assert their headroom from the data)


@pytest.mark.parametrize("F", ALL_F)
def test_rounding_generator(F):
    """gamma of both signs with one exact zero whose column sits at exactly 0, planted zeros elsewhere, and NO other
    pre-activation within MARGIN of 0: the float64 reference has no kink a rounding could cross."""
    for seed, M in ((11, 1000), (21, 1000), (51, 257), (71, 1600)):
        c = gb.rounding_case(M, F, seed)
        co = bn_ref.f64(c["co"])
        assert (c["gamma"] == 0).sum() == 1 and (F < 3 or ((c["gamma"] > 0).any() and (c["gamma"] < 0).any()))
        z = int(np.argmax(c["gamma"] == 0))
        assert co[2, z] == 0 and co[3, z] == 0 and c["planted"][:, z].all()
        assert np.array_equal(c["co"][2], (c["gamma"] * c["co"][1]).astype(np.float32))
        pre = bn_ref.preact(c["y"], c["co"])
        assert (pre[c["planted"]] == 0).all()
        assert np.abs(pre[~c["planted"]]).min() >= gb.MARGIN
        assert (c["planted"][:, [f for f in range(F) if f != z]]).sum() > 0
        assert (c["gx"][c["planted"]] != 0).all()
        # self-consistent: shift = beta - mean scale to fp32 round-off
        assert np.abs(co[3] - (bn_ref.f64(c["beta"]) - co[0] * co[2])).max() <= 1e-6


@pytest.mark.parametrize("case", gb.CHAIN_CASES)
def test_chain_cases_have_no_kink_inside_the_margin(case):
    M, Fd, Fres, rshift, training, relu, seed = case
    y, gamma, beta, rm, rv, resid, gx = gb.chain_inputs(M, Fd, Fres, rshift, seed)
    ref = gb.chain_reference(y, gamma, beta, rm, rv, resid, gx, rshift, training, relu)
    assert int((ref["pre"].abs() < gb.CHAIN_MARGIN).sum()) == 0
    assert (gamma > 0).any() and (gamma < 0).any()


def test_chain_cases_cover_what_the_issue_names():
    cs = gb.CHAIN_CASES
    assert any(c[1] == 36 for c in cs) and any(c[1] == 5 for c in cs) and any(not c[5] for c in cs)
    assert any(c[0] % 2 == 1 and c[3] == 1 for c in cs) and any(c[4] for c in cs) and any(not c[4] for c in cs)


def test_row_map_levels():
    """The band level has real classes; the tiny level leaves fewer live rows (pairs) than one pass of any mapped kernel
    covers, so row_adv wraps more than once."""
    _, t = gb.rowmap_level("band736")
    sizes = t["w"]
    assert (sizes > 1).sum() > 10 and sizes.max() >= 4 and (sizes == 0).sum() > 20
    assert np.array_equal(np.sort(np.concatenate([t["real"], t["fake"]])), np.arange(t["V"]))
    _, t = gb.rowmap_level("tiny32")
    assert t["V"] == 32 and t["B"] == 50
    assert 0 < t["live"].size < 32 and 0 < t["live_pairs"].size < 16
    assert (t["w"] == 0).sum() > 0 and t["reps"].size > 0 and t["real"].size >= 8
    assert t["w"].sum() == 32


def test_case_lists():
    assert gb.fwd_rows(32) == [1, 127, 129, 511, 512, 513, 1153] and gb.fwd_rows(1024) == [1, 3, 5, 15, 16, 17, 37]
    assert gb.fwd_rows(36) == [1, 7, 64, 65] and gb.fwd_rows(5) == [1, 86, 1000]
    assert all(gb.main_arm(F) for F in gb.MAIN_F + (64,)) and not any(gb.main_arm(F) for F in gb.V4_F + gb.SCALAR_F + (48,))
    assert gb.apply_rows(32) == [1, 2, 127, 129, 255, 256, 257] and gb.apply_rows(256, True) == [2, 14, 18, 254, 256, 258]
    assert [gb.dyadic_ratio(a, b) for a, b in gb.RESIZE_PAIRS] == [True, True, True, False, False, False, False, False]
