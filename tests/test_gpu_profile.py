"""-m gpu: error profiles on the GPU (p2m_error_profile; evaluate.ErrorProfile) against the float64 restatement of the
definition (tests/profile_ref.py) on the cases of tests/profile_cases.py.  Unaligned, everything is compared for exact
equality: errors, bins (through the per-sample and per-point histograms), counts, sums in the kernel's order, summary().
Aligned, every error within delta = sqrt(3) ALIGN_REL Mc of the restatement's, every cumulative count inside the interval
that delta allows and the AUC between the two bounds.  Then the C ABI with guarded outputs, the refusals and graph capture."""
import ctypes as ct

import numpy as np
import pytest
import torch

import profile_cases as pc
import profile_ref as pr

pytestmark = pytest.mark.gpu


def _cu(x, dtype=torch.float32):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to("cuda", dtype)


def _same(a, b, what=""):
    """Equal bit for bit where finite, NaN where NaN; dicts and arrays alike."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), (what, sorted(a), sorted(b))
        for k in a:
            _same(a[k], b[k], f"{what}.{k}")
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), what


def profile(n, t, **kw):
    from pose2mesh_release_amd import evaluate
    return evaluate.ErrorProfile(n, thresholds=t, **kw)


def call(ep, pred, gt, valid=None, **kw):
    out = ep(_cu(pred), _cu(gt), None if valid is None else _cu(valid, torch.uint8), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_exact(ep, out, ref, state, t, what):
    """One call's outputs and the evaluator's totals and summary against the restatement, bit for bit."""
    _same(out["error"], ref["error"], what + " error")
    _same(out["sample_pck"], ref["sample_pck"], what + " sample_pck")
    _same(out["sample_mean"], ref["sample_mean"], what + " sample_mean")
    _same(ep.totals(), state, what + " totals")
    _same(ep.summary(), pr.summary(state, t), what + " summary")


@pytest.mark.parametrize("B", pc.BS)
@pytest.mark.parametrize("N", pc.NS)
def test_unaligned_is_exact(hip_libs, N, B):
    """N over the block and wave edges, B = 1, 3, 5, each with K = 2, 100, 256 and the non-uniform table.  At B = 1 the
    per-point histogram is the bin of every point."""
    pred, gt = pc.cloud(B, N, seed=100 * N + B)
    for name, t in pc.TABLES.items():
        ep = profile(N, t)
        out = call(ep, pred, gt)
        ref = pr.evaluate(pred, gt, t)
        state = pr.accumulate(pr.new_state(N, len(t)), ref)
        check_exact(ep, out, ref, state, t, f"N={N} B={B} {name}")
        if B == 1:
            hist = ep.totals()["point_hist"]
            assert (hist.sum(1) == 1).all() and np.array_equal(hist.argmax(1), ref["bins"][0])
        assert out["sample_pck"].sum() == B * N


def test_exact_hits(hip_libs):
    """Errors exactly on a threshold: 5.0 in bin 10, 0.0 in bin 0, 10.0 in bin 20 of linspace(0, 50, 101), 100.0 in bin K."""
    pred, gt, want = pc.exact_hits()
    ep = profile(4, (0.0, 50.0, 101))
    assert np.array_equal(ep.thresholds, pc.HIT_TABLE)
    out = call(ep, pred, gt)
    assert out["error"][0].tolist() == [5.0, 0.0, 10.0, 100.0]
    hist = ep.totals()["point_hist"]
    assert hist.argmax(1).tolist() == want.tolist() == [10, 0, 20, 101] and (hist.sum(1) == 1).all()
    ref = pr.evaluate(pred, gt, pc.HIT_TABLE)
    check_exact(ep, out, ref, pr.accumulate(pr.new_state(4, 101), ref), pc.HIT_TABLE, "exact hits")
    s = ep.summary()
    assert s["pck"][0] == 0.25 and s["pck"][10] == 0.5 and s["pck"][20] == 0.75 and s["pck"][100] == 0.75


def test_nan_coordinate(hip_libs):
    """A NaN coordinate: that error is NaN, lands in bin K and makes exactly the sums it enters NaN, as numpy's would."""
    t = pc.TABLES["k100"]
    pred, gt = pc.cloud(3, 65, seed=11)
    pred[1, 5, 2] = np.nan
    ep = profile(65, t)
    out = call(ep, pred, gt)
    ref = pr.evaluate(pred, gt, t)
    check_exact(ep, out, ref, pr.accumulate(pr.new_state(65, 100), ref), t, "nan")
    assert np.isnan(out["error"][1, 5]) and np.isnan(out["sample_mean"][1]) and np.isfinite(out["sample_mean"][[0, 2]]).all()
    tot = ep.totals()
    assert tot["point_hist"][5, 100] == 1 and np.isnan(tot["point_sum"][5]) and np.isfinite(np.delete(tot["point_sum"], 5)).all()


def test_valid_mask_and_a_point_never_valid(hip_libs):
    """valid as uint8, bool and float tensors alike; a point that is never valid: count 0, mean NaN, left out of auc_points.
    The coordinates of points that are not valid are never read (NaN there changes nothing)."""
    t = pc.TABLES["k100"]
    pred, gt = pc.cloud(5, 65, seed=12)
    valid = (np.random.default_rng(13).random((5, 65)) > 0.2).astype(np.uint8)
    valid[:, 7] = 0
    valid[3] = 0                                                # and a sample with nothing to count: its mean is NaN
    pred[valid == 0] = np.nan
    ref = pr.evaluate(pred, gt, t, valid)
    state = pr.accumulate(pr.new_state(65, 100), ref)
    for dtype in (torch.uint8, torch.bool, torch.float32):
        ep = profile(65, t)
        out = ep(_cu(pred), _cu(gt), _cu(valid, dtype))
        check_exact(ep, {k: v.cpu().numpy() for k, v in out.items()}, ref, state, t, f"valid {dtype}")
    s = ep.summary()
    assert s["points"]["count"][7] == 0 and np.isnan(s["points"]["mean"][7]) and np.isfinite(s["auc_points"])
    assert s["auc_points"] == float(np.mean(np.delete(s["points"]["auc"], 7))) and s["count"] == int(valid.sum())
    assert np.isnan(out["sample_mean"][3].item()) and (out["error"][3] == 0).all() and np.isfinite(s["mean"])


def test_padding_rows_groups_root(hip_libs):
    """B_real < B with NaN in the padding rows; group ids inside and outside [0, n_groups), as a host list and as a device
    tensor; root = 0."""
    t = pc.TABLES["steps"]
    pred, gt = pc.cloud(5, 257, seed=14)
    pred[3:], gt[3:] = np.nan, np.nan
    group = [1, 0, 1, 7, -1]
    ep = profile(257, t, root=0, n_groups=4)
    out = call(ep, pred, gt, B_real=3, group=group)
    ref = pr.evaluate(pred, gt, t, root=0, B_real=3)
    state = pr.accumulate(pr.new_state(257, len(t), 4), ref, B_real=3, group=group)
    check_exact(ep, out, ref, state, t, "padding")
    assert (out["error"][3:] == 0).all() and (out["sample_pck"][3:] == 0).all() and (out["sample_mean"][3:] == 0).all()
    assert (out["error"][:3, 0] == 0).all() and sorted(ep.summary()["groups"]) == [0, 1]
    pred, gt = pc.cloud(5, 257, seed=15)
    out = call(ep, pred, gt, group=torch.tensor(group, device="cuda"))
    ref = pr.evaluate(pred, gt, t, root=0)
    pr.accumulate(state, ref, group=group)                      # ids 7 and -1 count in the overall row only
    check_exact(ep, out, ref, state, t, "groups")
    s = ep.summary()
    assert sorted(s["groups"]) == [0, 1] and s["count"] == 8 * 257 and s["groups"][1]["count"] == 4 * 257


def test_mano_fixture_in_metres(hip_libs):
    """gt_scale = 1000 on the reference-made FreiHAND-size fixture (ground truth stored in metres)."""
    pred, gt, gs = pc.mano()
    t = pc.TABLES["k100"]
    ep = profile(778, t, gt_scale=gs)
    out = call(ep, pred, gt)
    ref = pr.evaluate(pred, gt, t, gt_scale=gs)
    check_exact(ep, out, ref, pr.accumulate(pr.new_state(778, 100), ref), t, "mano")
    assert gs == 1000.0 and 20.0 < ep.summary()["mean"] < 200.0


def test_two_calls_equal_one_and_reset(hip_libs):
    """4 + 5 samples leave bitwise the state of one call of 9 (and of the restatement); reset() clears everything."""
    t = pc.TABLES["k100"]
    pred, gt = pc.cloud(9, 257, seed=16)
    group = [1, 0, 1, 7, -1, 3, 3, 0, 2]
    one, two = profile(257, t, n_groups=4), profile(257, t, n_groups=4)
    call(one, pred, gt, group=group)
    call(two, pred[:4], gt[:4], group=group[:4])
    call(two, pred[4:], gt[4:], group=group[4:])
    _same(one.totals(), two.totals(), "4 + 5 vs 9")
    _same(one.totals(), pr.accumulate(pr.new_state(257, 100, 4), pr.evaluate(pred, gt, t), group=group), "9 vs restatement")
    two.reset()
    assert all((v == 0).all() for v in two.totals().values()) and two.summary()["count"] == 0
    call(two, pred, gt, group=group)
    _same(one.summary(), two.summary(), "after reset")
    off = profile(257, t, per_point=False)
    call(off, pred, gt)
    assert "points" not in off.summary() and "point_sum" not in off.totals() and off.summary()["auc"] == one.summary()["auc"]


@pytest.mark.parametrize("name", pc.ALIGNED)
def test_aligned_within_the_alignment_tolerance(hip_libs, name):
    """Every error within delta of the restatement's (numpy's SVD), every cumulative count - per sample and in the totals -
    inside [#(e_ref < t[k] - delta), #(e_ref <= t[k] + delta)], the AUC between the two bounds."""
    pred, gt, gs, t = pc.aligned_case(name)
    B, N = pred.shape[:2]
    ep = profile(N, t, align=True, gt_scale=gs)
    out = call(ep, pred, gt)
    ref = pr.evaluate(pred, gt, t, gt_scale=gs, align=True)
    delta = pr.align_delta(pred, gt, gt_scale=gs)
    ratio = np.abs(out["error"] - ref["error"]).max(1) / delta
    print(f"{name}: delta {delta.max():.3e}, worst |e - e_ref| / delta {ratio.max():.3e}")
    assert (ratio <= 1.0).all(), ratio
    on = np.ones((B, N), bool)
    lo, hi = np.zeros(len(t), np.int64), np.zeros(len(t), np.int64)
    for b in range(B):
        lb, hb = pr.count_bounds(ref["error"][b], on[b], t, delta[b])
        cum = np.cumsum(out["sample_pck"][b])
        assert cum[-1] == N and (lb <= cum[:-1]).all() and (cum[:-1] <= hb).all(), (name, b)
        lo, hi = lo + lb, hi + hb
    if name == "mano778":
        assert np.array_equal(lo, hi)                           # (audited on the CPU: tests/test_profile_cpu.py)
    tot, s = ep.totals(), ep.summary()
    cum = np.cumsum(tot["group_hist"][0])
    assert tot["group_count"][0] == B * N and (lo <= cum[:-1]).all() and (cum[:-1] <= hi).all()
    assert np.array_equal(tot["point_hist"].sum(0), tot["group_hist"][0]) and (tot["point_count"] == B).all()

    def auc_of(cum):                                            # the AUC of a curve given by its cumulative counts
        hist = np.append(np.diff(np.append(0, cum)), B * N - cum[-1])
        return pr.curves(np.zeros(1), np.array([B * N]), hist[None], t)[2][0]
    auc_lo, auc_hi = auc_of(lo), auc_of(hi)
    print(f"{name}: auc {s['auc']:.6f} in [{auc_lo:.6f}, {auc_hi:.6f}]")
    assert auc_lo <= s["auc"] <= auc_hi
    assert abs(s["mean"] - ref["error"].mean()) <= delta.max() and abs(s["auc_points"] - s["auc"]) <= 1e-12
    if name == "mano778":
        assert 0.50 <= s["auc"] <= 0.54


def test_aligned_degenerate_sample(hip_libs):
    """All predicted points of one sample coincide (varP = 0): its errors are non-finite and land in bin K; the other samples
    are bitwise what they are without it."""
    t = pc.TABLES["k100"]
    pred, gt = pc.cloud(3, 65, seed=17)
    clean = call(profile(65, t, align=True), pred, gt)
    pred[1] = pred[1, 0]
    ep = profile(65, t, align=True)
    out = call(ep, pred, gt)
    assert not np.isfinite(out["error"][1]).any() and out["sample_pck"][1].tolist() == [0] * 100 + [65]
    assert not np.isfinite(out["sample_mean"][1])
    for k in out:
        assert np.array_equal(out[k][[0, 2]], clean[k][[0, 2]]), k
    tot = ep.totals()
    assert tot["group_hist"][0, 100] >= 65 and (tot["point_hist"][:, 100] >= 1).all() and tot["group_count"][0] == 3 * 65


def test_abi_guards_and_refusals(hip_libs):
    """The C ABI with every output and the workspace inside NaN / sentinel-filled guard regions: nothing outside is written;
    every refusal returns P2M_ERR_INVALID and launches nothing."""
    from pose2mesh_release_amd import _lib
    lib = _lib.hip()
    GUARD = 64
    B, N, K, G = 3, 257, 256, 2
    t = pc.TABLES["k256"]
    pred, gt = pc.cloud(B, N, seed=18)

    def guarded(shape, dtype, fill):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        return buf, buf[GUARD:GUARD + n]

    def clean(buf, fill):
        ends = torch.cat([buf[:GUARD], buf[-GUARD:]])
        return bool(torch.isnan(ends).all()) if isinstance(fill, float) else bool((ends == fill).all())
    nan = float("nan")
    spec = {"error": ((B, N), torch.float64, nan), "mean": ((B,), torch.float64, nan), "pck": ((B, K + 1), torch.int32, -77),
            "gsum": ((G + 1,), torch.float64, nan), "gcnt": ((G + 1,), torch.int64, -77),
            "ghist": ((G + 1, K + 1), torch.int64, -77), "psum": ((N,), torch.float64, nan), "pcnt": ((N,), torch.int64, -77),
            "phist": ((N, K + 1), torch.int64, -77)}
    ws_bytes = int(lib.p2m_error_profile_workspace(B, N))
    spec["ws"] = ((ws_bytes,), torch.uint8, 0xAB)
    g = {k: guarded(*v) for k, v in spec.items()}
    for k in ("gsum", "gcnt", "ghist", "psum", "pcnt", "phist"):    # running totals start at zero; their guards stay filled
        g[k][1].zero_()
    P, Gt, T = _cu(pred), _cu(gt), torch.from_numpy(t).cuda()
    grp = torch.tensor([1, 5, 0], dtype=torch.int32, device="cuda")
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)

    def p(x):
        return None if x is None else ct.c_void_p(x.data_ptr())

    def run(**kw):
        a = dict(pred=P, gt=Gt, valid=None, B=B, B_real=B, N=N, gs=1.0, root=-1, align=0, th=T, K=K, ws=g["ws"][1],
                 ws_bytes=ws_bytes, error=g["error"][1], mean=g["mean"][1], pck=g["pck"][1], group=grp, n_groups=G,
                 gsum=g["gsum"][1], gcnt=g["gcnt"][1], ghist=g["ghist"][1], psum=g["psum"][1], pcnt=g["pcnt"][1],
                 phist=g["phist"][1])
        a.update(kw)
        rc = lib.p2m_error_profile(p(a["pred"]), p(a["gt"]), p(a["valid"]), a["B"], a["B_real"], a["N"], a["gs"], a["root"],
                                   a["align"], p(a["th"]), a["K"], p(a["ws"]), a["ws_bytes"], p(a["error"]), p(a["mean"]),
                                   p(a["pck"]), p(a["group"]), a["n_groups"], p(a["gsum"]), p(a["gcnt"]), p(a["ghist"]),
                                   p(a["psum"]), p(a["pcnt"]), p(a["phist"]), stream)
        torch.cuda.synchronize()
        return rc
    for kw in (dict(pred=None), dict(gt=None), dict(th=None), dict(ws=None), dict(error=None), dict(mean=None), dict(pck=None),
               dict(N=0), dict(B_real=B + 1), dict(B_real=-1), dict(K=1), dict(K=257), dict(root=N), dict(root=-2),
               dict(ws_bytes=ws_bytes - 1), dict(ws_bytes=0), dict(gsum=None), dict(pcnt=None), dict(phist=None),
               dict(n_groups=-1), dict(B=1 << 20, N=1 << 10)):
        assert run(**kw) == -1, kw                              # P2M_ERR_INVALID
        assert lib.p2m_last_error_string()
        assert torch.isnan(g["error"][1]).all() and (g["pck"][1] == -77).all() and (g["ws"][1] == 0xAB).all(), kw
        assert (g["gcnt"][1] == 0).all() and (g["pcnt"][1] == 0).all(), kw
    for align in (0, 1):
        assert run(align=align) == 0
        assert all(clean(g[k][0], spec[k][2]) for k in g), "a guard region was written"
    ref = pr.evaluate(pred, gt, t, align=True)
    assert np.abs(g["error"][1].view(B, N).cpu().numpy() - ref["error"]).max() <= pr.align_delta(pred, gt).max()
    assert int(g["gcnt"][1][0]) == 2 * B * N and g["gcnt"][1].tolist() == [2 * B * N, 2 * N, 2 * N]
    assert (g["pcnt"][1] == 2 * B).all() and int(g["phist"][1].sum()) == 2 * B * N and int(g["ghist"][1].sum()) == 2 * N * (B + 2)


def test_graph_capture(hip_libs):
    """One single-stream torch.cuda.graph capture of a call: three replays leave the totals of three eager calls, and the
    per-sample outputs of the eager call, bit for bit."""
    pred, gt, gs = pc.mano()
    t = pc.TABLES["k100"]
    P, G = _cu(pred), _cu(gt)
    for align in (False, True):
        eager = profile(778, t, align=align, gt_scale=gs)
        for _ in range(3):
            want = {k: v.clone() for k, v in eager(P, G).items()}
        ep = profile(778, t, align=align, gt_scale=gs)
        ep(P, G)                                                # (allocates the buffers of this size)
        ep.reset()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ep(P, G)
        ep.reset()
        for v in out.values():
            v.fill_(-1)
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        for k, v in want.items():
            assert torch.equal(out[k], v), k
        _same(ep.totals(), eager.totals(), f"capture align={align}")
        assert ep.summary()["count"] == 3 * 3 * 778
