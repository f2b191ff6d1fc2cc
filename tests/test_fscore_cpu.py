"""CPU: the float64 restatement of the F-score definition (tests/fscore_ref.py) against scipy's k-d tree on every case of
tests/fscore_cases.py, the audit that every case's band is empty (so the GPU test may demand exact counts), an fp32 emulation
of the search kernel's arithmetic inside the derived bound, the faults a kernel of this kind can have leaving it, and the
host-side checks of pose2mesh_release_amd.evaluate's FScoreEvaluator / nearest_distances."""
import numpy as np
import pytest

import eval_ref
import fscore_cases as fc
import fscore_ref as fr


def _sets(c, b, aligned):
    P, G = fr.transformed(c["pred"][b:b + 1], c["gt"][b:b + 1], c["gt_scale"], c["regressor"], c["root"],
                          None if c["pred_root"] is None else c["pred_root"][b:b + 1],
                          None if c["gt_root"] is None else c["gt_root"][b:b + 1], aligned)
    return P[0], G[0]


def _variants(c):
    return ([("", False)] if c["centred"] else []) + ([("pa_", True)] if c["aligned"] else [])


@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_reference_agrees_with_kdtree_and_band_is_empty(name):
    """Brute force over all pairs == scipy.spatial.cKDTree (1e-9 mm), near_* and F follow from the counts, and no vertex of
    the case lies within its bound of a threshold."""
    from scipy.spatial import cKDTree
    c, r = fc.case(name), fc.reference(name)
    nv = c["pred"].shape[1]
    for pre, al in _variants(c):
        for b in range(c["pred"].shape[0]):
            P, G = _sets(c, b, al)
            assert np.abs(cKDTree(G).query(P)[0] - r[pre + "d_pred"][b]).max() <= 1e-9, (name, pre, b)
            assert np.abs(cKDTree(P).query(G)[0] - r[pre + "d_gt"][b]).max() <= 1e-9, (name, pre, b)
        for t, th in enumerate(c["thresholds"]):
            a, g = (r[pre + "d_pred"] < th).sum(1) / nv, (r[pre + "d_gt"] < th).sum(1) / nv
            assert np.array_equal(a, r[pre + "near_pred"][:, t]) and np.array_equal(g, r[pre + "near_gt"][:, t])
            with np.errstate(invalid="ignore", divide="ignore"):
                f = np.where(a + g > 0, 2 * a * g / (a + g), 0.0)
            assert np.abs(f - r[pre + "f"][:, t]).max() <= 1e-15
        assert r[pre + "band"].sum() == 0, (name, pre, r[pre + "band"])
        assert r[pre + "bound_pred"].max() < 1e-3              # and the bound is far below any threshold's spacing


def test_case_table_sits_on_the_launch_edges():
    nvs = set(fc.SHELL_NV)
    for tile in (fc.QUERY_TILE_SMALL, fc.TARGET_TILE, fc.SMALL_MAX):
        assert {tile - 1, tile, tile + 1} <= nvs
    k = fc.SMALL_MAX // fc.QUERY_TILE_LARGE + 1                 # the first multiple of the large query tile above the switch
    assert {k * fc.QUERY_TILE_LARGE - 1, k * fc.QUERY_TILE_LARGE, k * fc.QUERY_TILE_LARGE + 1} <= nvs
    assert {1, 2} <= nvs
    assert fc.case("mano778")["pred"].shape == (3, 778, 3) and fc.case("smpl6890")["pred"].shape == (2, 6890, 3)
    c = fc.five_hands()
    r = fr.evaluate(c["pred"], c["gt"], c["thresholds"], pred_root=c["pred_root"], gt_root=c["gt_root"])
    assert r["band"].sum() == 0 and r["pa_band"].sum() == 0 and 0 < r["f"].min() and r["pa_f"].max() < 1
    # non-trivial values: some F strictly between 0 and 1 in every variant that is audited
    r = fc.reference("shell1024")
    assert 0.05 < r["f"][0, 1] < 0.95 and 0.05 < r["pa_f"][0, 1] < 0.95 and (r["pa_f"] >= r["f"]).all()


EMU_CASES = [n for n in fc.CASE_NAMES if n != "smpl6890_pa"]


@pytest.mark.parametrize("name", EMU_CASES)
def test_f32_emulation_stays_inside_the_bound(name):
    """The kernel's scheme in numpy fp32 (staging about the ground truth's centroid, direct-form d^2, min, sqrt) on the
    centred (else aligned) variant of every case, both directions; the SMPL-size fixture on its first sample."""
    c, r = fc.case(name), fc.reference(name)
    pre, al = _variants(c)[0]
    worst = 0.0
    for b in range(1 if name.startswith("smpl") else c["pred"].shape[0]):
        P, G = _sets(c, b, al)
        Ps, Gs = fr.stage_f32(P, G)
        for q, t, k in ((Ps, Gs, "pred"), (Gs, Ps, "gt")):
            d = fr.emulate_search(q, t, tile=fc.TARGET_TILE).astype(np.float64)
            worst = max(worst, float((np.abs(d - r[pre + "d_" + k][b]) / r[pre + "bound_" + k][b]).max()))
    print(f"{name}: worst |emulation - float64| / bound = {worst:.3f}")
    assert worst <= 1.0


def test_planted_faults_leave_the_bound():
    """Each fault is far outside the bound on a case built to show it, and the faultless emulation is inside on the same case."""
    # a tail tile left as zeros: the staged origin wins (10 mm instead of ~90)
    c = fc.far_shells()
    r = fr.evaluate(c["pred"], c["gt"], c["thresholds"], aligned=False)
    assert r["band"].sum() == 0 and 85 < r["d_pred"].min() and r["d_pred"].max() < 95
    P, G = _sets(c, 0, False)
    Ps, Gs = fr.stage_f32(P, G)
    ok = fr.emulate_search(Ps, Gs, tile=fc.TARGET_TILE)
    assert (np.abs(ok - r["d_pred"][0]) <= r["bound_pred"][0]).all()
    bad = fr.emulate_search(Ps, Gs, tile=fc.TARGET_TILE, pad="zero")
    assert np.abs(bad - r["d_pred"][0]).min() > 70 and bad.max() < 20      # (the centroid of 1025 shell points: a few mm off)
    # a loop one target short: the vertex whose nearest target is the last one is off by millimetres
    # (on a noisy copy of the targets: shell1025, where each target is the nearest of the vertex made from it)
    c, r = fc.case("shell1025"), fc.reference("shell1025")
    Ps, Gs = fr.stage_f32(*_sets(c, 0, False))
    bad = fr.emulate_search(Ps, Gs, tile=fc.TARGET_TILE, short=1)
    assert (np.abs(bad - r["d_pred"][0]) > r["bound_pred"][0]).sum() >= 1
    assert np.abs(bad - r["d_pred"][0]).max() > 0.1
    # <= for <: a distance that is exactly a threshold in every arithmetic (3-4-5) must not count
    p, g = np.zeros((1, 3)), np.array([[3.0, 4.0, 0.0]])
    d = fr.emulate_search(*fr.stage_f32(p, g))
    assert d[0] == 5.0 and fr.nearest(p, g)[0] == 5.0
    assert fr.score(d, d, 5.0)[:2] == (0, 0) and fr.score(d, d, 5.0, strict=False)[:2] == (1, 1)
    assert fr.score(d, d, 5.0)[4] == 0.0 and fr.score(d, d, 5.0, strict=False)[4] == 1.0
    # the expansion form of d^2: cancellation at the SMPL-size fixture's extent (M ~ 1000 mm) is orders over the bound
    c, r = fc.case("smpl6890"), fc.reference("smpl6890")
    P, G = _sets(c, 0, False)
    Ps, Gs = fr.stage_f32(P, G)
    q = slice(0, 512)
    ok = fr.emulate_search(Ps[q], Gs, tile=fc.TARGET_TILE)
    bad = fr.emulate_search(Ps[q], Gs, tile=fc.TARGET_TILE, form="expansion")
    assert (np.abs(ok - r["d_pred"][0][q]) <= r["bound_pred"][0][q]).all()
    assert (np.abs(bad - r["d_pred"][0][q]) / r["bound_pred"][0][q]).max() > 5.0


def test_reference_padding_degenerates_and_summary():
    c = fc.case("shell64")
    full = fc.reference("shell64")
    pred, gt = np.concatenate([c["pred"], np.full((1, 64, 3), np.nan, np.float32)]), \
        np.concatenate([c["gt"], np.full((1, 64, 3), np.nan, np.float32)])
    r = fr.evaluate(pred, gt, c["thresholds"], B_real=2)
    for k in ("f", "pa_f", "d_pred", "pa_d_gt", "near_gt"):
        assert np.array_equal(r[k][:2], full[k]) and (r[k][2] == 0).all()
    s = fr.summary(r, c["thresholds"], B_real=2, group=[1, 40, 0], n_groups=32)
    assert s["samples"] == 2 and s["f@5"] == full["f"][:, 1].mean() and s["pa_near_gt@15"] == full["pa_near_gt"][:, 3].mean()
    assert list(s["groups"]) == [1] and s["groups"][1]["samples"] == 1 and s["groups"][1]["f@3"] == full["f"][0, 0]
    # identical meshes: all zeros, F = 1; meshes farther apart than every threshold: F = 0, not NaN
    same = fr.evaluate(c["gt"], c["gt"], (5.0,), aligned=False)
    assert (same["d_pred"] == 0).all() and (same["f"] == 1).all()
    far = fr.evaluate(c["gt"] + np.float32(500.0), c["gt"], (5.0, 15.0), aligned=False)
    assert (far["f"] == 0).all() and (far["near_pred"] == 0).all()
    # an exact similarity image with shuffled rows: the alignment over the (wrong) correspondence cannot undo it ... but with
    # the rows in order it does: pa_f = 1 at a threshold far above the bound
    g = c["gt"].astype(np.float64)
    a = np.deg2rad(25.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    img = (1.2 * g @ R.T + np.array([30.0, -20.0, 10.0])).astype(np.float32)
    ex = fr.evaluate(img, c["gt"], (0.01,))
    assert (ex["pa_f"] == 1).all() and (ex["f"] < 0.2).all()
    assert np.abs(eval_ref.rigid_align(img[0], g[0]) - g[0]).max() < 1e-3


def test_fscore_host_checks(hip_libs):
    """Without a GPU: CPU tensors raise P2MError (no CPU path), bad shapes and bad constructor arguments ValueError, and the
    new entry points are in the ctypes table and exported."""
    import torch
    from pose2mesh_release_amd import _lib, evaluate
    fs = evaluate.FScoreEvaluator(778, np.ones((21, 778), np.float32) / 778, 0)
    with pytest.raises(_lib.P2MError):
        fs(torch.zeros(2, 778, 3), torch.zeros(2, 778, 3))
    with pytest.raises(_lib.P2MError):
        evaluate.nearest_distances(torch.zeros(5, 3), torch.zeros(9, 3))
    with pytest.raises(ValueError):
        fs(torch.zeros(2, 777, 3), torch.zeros(2, 777, 3))
    with pytest.raises(ValueError):
        fs(torch.zeros(2, 778, 3), torch.zeros(3, 778, 3))
    with pytest.raises(ValueError):
        fs(torch.zeros(2, 778, 3), torch.zeros(2, 778, 3), pred_root=torch.zeros(2, 3))
    with pytest.raises(ValueError):
        fs(torch.zeros(2, 778, 3), torch.zeros(2, 778, 3), pred_root=torch.zeros(2, 3), gt_root=torch.zeros(3, 3))
    with pytest.raises(ValueError):
        fs(torch.zeros(2, 778, 3), torch.zeros(2, 778, 3), B_real=3)
    for A, B in ((torch.zeros(5, 2), torch.zeros(5, 3)), (torch.zeros(2, 5, 3), torch.zeros(3, 5, 3)),
                 (torch.zeros(5, 3), torch.zeros(1, 5, 3)), (torch.zeros(0, 3), torch.zeros(5, 3))):
        with pytest.raises(ValueError):
            evaluate.nearest_distances(A, B)
    for kw in (dict(thresholds=()), dict(thresholds=(1, 2, 3, 4, 5)), dict(thresholds=(5.0, -1.0)),
               dict(thresholds=(float("inf"),)), dict(centred=False, aligned=False), dict(regressor=np.ones((21, 777))),
               dict(regressor=np.ones((21, 778)), root=21)):
        with pytest.raises(ValueError):
            evaluate.FScoreEvaluator(778, **kw)
    assert evaluate.FScoreEvaluator(778).summary() == {"samples": 0}
    assert evaluate.FScoreEvaluator(778, thresholds=(5, 7.5), aligned=False)._columns() == \
        ["near_pred@5", "near_pred@7.5", "near_gt@5", "near_gt@7.5", "f@5", "f@7.5"]
    lib = _lib.hip()
    for n in ("p2m_mesh_fscore", "p2m_point_nn", "p2m_nn_workspace", "p2m_nn_target_tile", "p2m_nn_query_tile"):
        assert n in _lib.HIP_SYMBOLS and hasattr(lib, n)
    assert len(_lib.HIP_SYMBOLS["p2m_mesh_fscore"][1]) == 28
    # the exported tile sizes are the ones the case table was laid out for
    assert lib.p2m_nn_target_tile() == fc.TARGET_TILE
    assert lib.p2m_nn_query_tile(fc.SMALL_MAX) == fc.QUERY_TILE_SMALL and lib.p2m_nn_query_tile(1) == fc.QUERY_TILE_SMALL
    assert lib.p2m_nn_query_tile(fc.SMALL_MAX + 1) == fc.QUERY_TILE_LARGE
    assert lib.p2m_nn_workspace(2, 778, 778) >= 2 * 9 * 780 * 4 and lib.p2m_nn_workspace(2, 0, 5) < 0
