"""CPU: the float64 restatement of the error-profile definition (tests/profile_ref.py) audited from the definition alone - the
histogram form of the PCK curve against the direct form mean(e <= t[k]), the non-strict comparison on errors that sit exactly
on a threshold, the kernel's summation order against an exact sum, the chaining of the running totals - the host-side
derivation of pose2mesh_release_amd.evaluate (profile_curves, the threshold table) against it, and the host-side checks of
evaluate.ErrorProfile."""
import math

import numpy as np
import pytest

import profile_cases as pc
import profile_ref as pr


def _same(a, b):
    """Equal bit for bit where finite, NaN where NaN; dicts and arrays alike."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), (sorted(a), sorted(b))
        for k in a:
            _same(a[k], b[k])
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), (a, b)


def test_tables_arrive_bit_for_bit():
    from pose2mesh_release_amd import evaluate
    assert np.array_equal(pc.HIT_TABLE, 0.5 * np.arange(101))
    assert np.array_equal(evaluate._threshold_table((0.0, 50.0, 101)), pc.HIT_TABLE)
    assert np.array_equal(evaluate._threshold_table((0.0, 50.0, 100)), np.linspace(0.0, 50.0, 100))
    # a sequence of three that does not end in an integer is a table of three thresholds
    assert np.array_equal(evaluate._threshold_table((5.0, 15.0, 150.0)), np.array([5.0, 15.0, 150.0]))
    assert np.array_equal(evaluate._threshold_table(pc.TABLES["steps"]), pc.TABLES["steps"])
    for bad in ((0.0, 50.0, 1), (0.0, 50.0, 257), [1.0], np.arange(257.0), [0.0, 1.0, 1.0], [2.0, 1.0], [0.0, np.inf],
                [0.0, np.nan]):
        with pytest.raises(ValueError):
            evaluate._threshold_table(bad)


@pytest.mark.parametrize("align", (False, True))
def test_histogram_form_equals_direct_form(align):
    """On the FreiHAND-size fixture with linspace(0, 50, 100): cumsum(hist) / count == mean(e <= t[k]) bit for bit, overall,
    per sample and per point; the package's host derivation agrees with the restatement's; aligned, delta is about 1.2e-4 mm,
    no error lies within delta of a threshold (the count interval has width 0) and the AUC is 0.50 - 0.54."""
    from pose2mesh_release_amd import evaluate
    pred, gt, gs = pc.mano()
    t = pc.TABLES["k100"]
    res = pr.evaluate(pred, gt, t, gt_scale=gs, align=align)
    on = res["bins"] >= 0
    st = pr.accumulate(pr.new_state(778, 100), res)
    s = pr.summary(st, t)
    assert np.array_equal(s["pck"], pr.pck_direct(res["error"], on, t))
    for b in range(3):
        assert np.array_equal(np.cumsum(res["sample_pck"][b])[:-1] / 778.0, pr.pck_direct(res["error"][b], on[b], t))
    for i in (0, 1, 389, 777):
        assert np.array_equal(s["points"]["pck"][i], pr.pck_direct(res["error"][:, i], on[:, i], t))
    assert s["count"] == 3 * 778 and 0.0 < s["pck"][10] < s["pck"][90] < 1.0
    assert abs(s["auc_points"] - s["auc"]) <= 1e-12            # every point always valid: the per-point mean is the pooled one
    for tot, cnt, hist in ((st["group_sum"], st["group_count"], st["group_hist"]),
                           (st["point_sum"], st["point_count"], st["point_hist"])):
        for a, b in zip(evaluate.profile_curves(tot, cnt, hist, t), pr.curves(tot, cnt, hist, t)):
            _same(a, b)
    if align:
        delta = pr.align_delta(pred, gt, gt_scale=gs)
        print("delta", delta, "auc", s["auc"])
        assert (delta > 1.0e-4).all() and (delta < 1.4e-4).all() and 0.50 <= s["auc"] <= 0.54
        for b in range(3):
            lo, hi = pr.count_bounds(res["error"][b], on[b], t, delta[b])
            assert np.array_equal(lo, hi)


def test_exact_hits_reject_a_strict_comparison():
    """Errors of exactly 5, 0 and 10 against t[k] = k / 2 land in bins 10, 0 and 20; 100 lands in bin K.  The same function
    with the comparison made strict puts them one bin up, and the PCK curve then misses them at their own threshold."""
    from pose2mesh_release_amd import evaluate
    pred, gt, want = pc.exact_hits()
    t = pc.HIT_TABLE
    res = pr.evaluate(pred, gt, t)
    assert res["error"][0].tolist() == [5.0, 0.0, 10.0, 100.0]
    assert res["bins"][0].tolist() == want.tolist() == [10, 0, 20, 101]
    bad = pr.evaluate(pred, gt, t, strict=True)
    assert bad["bins"][0].tolist() == [11, 1, 21, 101]
    assert not np.array_equal(bad["sample_pck"], res["sample_pck"])
    _, pck, _ = evaluate.profile_curves(res["sample_sum"], res["sample_count"], res["sample_pck"], t)
    _, pck_bad, _ = evaluate.profile_curves(bad["sample_sum"], bad["sample_count"], bad["sample_pck"], t)
    assert np.array_equal(pck[0], pr.pck_direct(res["error"][0], res["bins"][0] >= 0, t))
    assert pck[0][0] == 0.25 and pck[0][10] == 0.5 and pck[0][20] == 0.75 and pck[0][100] == 0.75
    assert pck_bad[0][0] == 0.0 and pck_bad[0][10] == 0.25 and pck_bad[0][20] == 0.5


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257, 778, 6890))
def test_kernel_order_sum_is_a_sum(n):
    """sample_sum (the kernel's order) against the exactly rounded sum: within n ulp-sized steps; a NaN poisons it."""
    e = np.abs(np.random.default_rng(n).standard_normal(n)) * 20.0
    s = pr.sample_sum(e)
    assert abs(s - math.fsum(e)) <= n * 2.0 ** -52 * math.fsum(e)
    if n == 1:
        assert s == e[0]
    e[n // 2] = np.nan
    assert np.isnan(pr.sample_sum(e))


def test_running_totals_chain_and_skip():
    """4 + 5 samples leave bitwise the state of 9; group rows; a point that is never valid has count 0, mean NaN and is left
    out of auc_points; padding rows are not counted; a NaN coordinate lands in bin K and poisons exactly the sums it enters."""
    t = pc.TABLES["k100"]
    pred, gt = pc.cloud(9, 65, seed=5)
    rng = np.random.default_rng(6)
    valid = (rng.random((9, 65)) > 0.2).astype(np.uint8)
    valid[:, 7] = 0
    group = [1, 0, 1, 7, -1, 3, 3, 0, 2]
    whole = pr.accumulate(pr.new_state(65, 100, 4), pr.evaluate(pred, gt, t, valid), group=group)
    parts = pr.new_state(65, 100, 4)
    pr.accumulate(parts, pr.evaluate(pred[:4], gt[:4], t, valid[:4]), group=group[:4])
    pr.accumulate(parts, pr.evaluate(pred[4:], gt[4:], t, valid[4:]), group=group[4:])
    _same(whole, parts)
    s = pr.summary(whole, t)
    assert s["count"] == int(valid.sum()) and sorted(s["groups"]) == [0, 1, 2, 3]
    assert s["groups"][3]["count"] == int(valid[5:7].sum()) and s["groups"][1]["count"] == int(valid[[0, 2]].sum())
    assert s["points"]["count"][7] == 0 and np.isnan(s["points"]["mean"][7]) and np.isnan(s["points"]["auc"][7])
    seen = np.arange(65) != 7
    assert np.isfinite(s["auc_points"]) and s["auc_points"] == float(np.mean(s["points"]["auc"][seen]))
    # padding
    padded = pr.evaluate(np.concatenate([pred[:3], np.full((2, 65, 3), np.nan, np.float32)]),
                         np.concatenate([gt[:3], np.full((2, 65, 3), np.nan, np.float32)]), t, B_real=3)
    real = pr.evaluate(pred[:3], gt[:3], t)
    for k in real:
        assert np.array_equal(padded[k][:3], real[k]) and (padded[k][3:] == (-1 if k == "bins" else 0)).all(), k
    _same(pr.accumulate(pr.new_state(65, 100), padded, B_real=3), pr.accumulate(pr.new_state(65, 100), real))
    # a NaN coordinate
    p2 = pred.copy()
    p2[1, 5, 2] = np.nan
    r = pr.evaluate(p2, gt, t)
    assert np.isnan(r["error"][1, 5]) and r["bins"][1, 5] == 100 and np.isnan(r["sample_mean"][1])
    assert np.isfinite(r["sample_mean"][[0, 2]]).all() and r["sample_pck"][1].sum() == 65
    s2 = pr.summary(pr.accumulate(pr.new_state(65, 100), r), t)
    assert np.isnan(s2["mean"]) and np.isfinite(s2["auc"]) and np.isnan(s2["points"]["mean"][5])
    assert np.isfinite(np.delete(s2["points"]["mean"], 5)).all()


def test_profile_host_checks(hip_libs):
    """Without a GPU: CPU tensors raise P2MError (no CPU path), bad shapes and bad constructor arguments ValueError, and the new
    entry points are in the ctypes table and exported."""
    import torch
    from pose2mesh_release_amd import _lib, evaluate
    ep = evaluate.ErrorProfile(21)
    assert ep.K == 100 and np.array_equal(ep.thresholds, np.linspace(0.0, 50.0, 100)) and ep.summary()["count"] == 0
    with pytest.raises(_lib.P2MError):
        ep(torch.zeros(2, 21, 3), torch.zeros(2, 21, 3))
    for args, kw in (((torch.zeros(2, 20, 3), torch.zeros(2, 20, 3)), {}), ((torch.zeros(2, 21, 3), torch.zeros(3, 21, 3)), {}),
                     ((torch.zeros(2, 21, 2), torch.zeros(2, 21, 2)), {}), ((torch.zeros(21, 3), torch.zeros(21, 3)), {}),
                     ((torch.zeros(2, 21, 3), torch.zeros(2, 21, 3)), dict(valid=torch.zeros(2, 20))),
                     ((torch.zeros(2, 21, 3), torch.zeros(2, 21, 3)), dict(B_real=3))):
        with pytest.raises(ValueError):
            ep(*args, **kw)
    for kw in (dict(thresholds=(0.0, 50.0, 1)), dict(thresholds=(0.0, 50.0, 257)), dict(thresholds=[3.0, 2.0]),
               dict(thresholds=[1.0]), dict(root=21), dict(root=-1), dict(n_groups=-1)):
        with pytest.raises(ValueError):
            evaluate.ErrorProfile(21, **kw)
    with pytest.raises(ValueError):
        evaluate.ErrorProfile(0)
    lib = _lib.hip()
    for n in ("p2m_error_profile", "p2m_error_profile_workspace"):
        assert n in _lib.HIP_SYMBOLS and hasattr(lib, n)
    assert len(_lib.HIP_SYMBOLS["p2m_error_profile"][1]) == 25
    assert lib.p2m_error_profile_workspace(3, 778) >= 3 * (12 + 2 * 778) and lib.p2m_error_profile_workspace(3, 778) % 16 == 0
    assert lib.p2m_error_profile_workspace(2, 0) < 0 and lib.p2m_error_profile_workspace(-1, 5) < 0
    s = {"thresholds": np.array([50.0, 100.0, 150.0]), "pck": np.array([0.25, 0.5, 0.75])}
    assert evaluate.pck_at(s, 150.0) == 0.75
    with pytest.raises(KeyError):
        evaluate.pck_at(s, 120.0)
