"""CPU: the yardstick of the camera kernels (tests/camfit_ref.py) against what the REAL reference recorded in
tests/golden/camfit_ref.npz (make_golden_camfit.py), and the properties the GPU tests rely on."""
import numpy as np
import pytest

import camfit_cases as cc
import camfit_ref
import sample_ref

U = 2.0 ** -24


@pytest.mark.parametrize("pose", cc.PREP_POSES)
def test_prepare_matches_the_reference(pose):
    """The float64 restatement of p2m_pose_prepare against the reference's own get_bbox / process_bbox / j2d_processing /
    standardisation.  Tolerance, from the fp32 roundings the REFERENCE makes (the yardstick makes none): get_bbox returns
    float32, process_bbox then works in float32 (about 6 operations on values up to M = the largest pixel magnitude among the
    joints and the box corners), get_center_scale rounds centre and size once more, and j2d_processing's result is cast to
    float32.  So a box value is off by at most 8 u M, the scale s relatively by 8 u, a transformed point by at most
    s 8 u M (centre) + 8 u res (scale) + u res (the cast) <= 16 u (s M + res)."""
    g = cc.golden()
    joints = g[f"prep_{pose}_joints"]
    out = camfit_ref.prepare(joints[None])
    assert out["status"][0] == 0
    box1, box2 = g[f"prep_{pose}_bbox1"].astype(np.float64), g[f"prep_{pose}_bbox2"].astype(np.float64)
    M = max(np.abs(joints).max(), np.abs(box1[:2]).max(), np.abs(box1[:2] + box1[2:]).max(), np.abs(box2[:2]).max(),
            np.abs(box2[:2] + box2[2:]).max())
    assert np.abs(out["bbox"][0] - box1).max() <= 8 * U * M
    assert np.abs(out["bbox2"][0] - box2).max() <= 8 * U * M
    assert np.abs(out["tight"][0] - g[f"prep_{pose}_tight"]).max() <= 2 * U * M
    s1, s2 = cc.CROP / box1[2], 288.0 / box2[2]
    tol_t = 16 * U * (s1 * M + cc.CROP)
    assert np.abs(out["target"][0] - g[f"prep_{pose}_target"]).max() <= tol_t
    # the standardised input z = (p - mean) / sd with p = the point / (W, H): a perturbation d of every p moves z by at most
    # 2 d / sd + |z| 2 d / sd (mean and sd move by at most d and 2 d); the reference's own division and cast add 4 u |z|
    ref = g[f"prep_{pose}_pose2d"].astype(np.float64)
    d = 16 * U * (s2 * M + 384.0) / 288.0
    p = (s2 * (joints.astype(np.float64) - (box2[:2] + box2[2:] / 2)) + np.array([144.0, 192.0])) / np.array([288.0, 384.0])
    tol_z = (2 * d / p.std(axis=0).min()) * (1 + np.abs(ref).max()) + 4 * U * np.abs(ref).max()
    assert np.abs(out["pose2d"][0] - ref).max() <= tol_z
    # the wide pose takes the other branch of process_bbox's aspect test than the demo's (width governs its bbox2)
    tight = g[f"prep_{pose}_tight"]
    if pose in ("demo", "wide"):
        assert ((tight[2] - 1) > 0.75 * (tight[3] - 1)) == (pose == "wide")


def test_prepare_fp32_mode_and_degenerate_samples():
    """The fp32 operation sequence stays within fp32 rounding of the float64 mode, and the three degenerate poses of the GPU
    test set status bit 0 with zeroed outputs."""
    g = cc.golden()
    for pose in cc.PREP_POSES:
        j = g[f"prep_{pose}_joints"][None]
        a, b = camfit_ref.prepare(j), camfit_ref.prepare(j, dtype=np.float32)
        assert np.abs(a["target"] - b["target"]).max() <= 16 * U * 2 * cc.CROP
        assert np.abs(a["pose2d"] - b["pose2d"]).max() <= 1e-4
    j = np.repeat(g["prep_demo_joints"][None], 3, 0).copy()
    j[0] = j[0, :1]                       # a single point
    j[1, 3, 1] = np.nan
    j[2, :, 1] = 240.0                    # zero height
    out = camfit_ref.prepare(j)
    assert out["status"].tolist() == [1, 1, 1]
    assert all(not out[k].any() for k in ("pose2d", "target", "bbox"))


def _fp32_spread(p, t, c0, steps, n_orders=8):
    """The largest |fp32 mode - float64 mode| of the yardstick's camera over n_orders shuffled summation orders."""
    ref, _, mar = camfit_ref.fit(p, t, None, c0, steps=steps, img_res=cc.IMG_RES)
    rng = np.random.default_rng(3)
    d = 0.0
    for _ in range(n_orders):
        cam, _, _ = camfit_ref.fit(p, t, None, c0, steps=steps, img_res=cc.IMG_RES, dtype=np.float32,
                                   order=rng.permutation(p.shape[1]))
        d = max(d, float(np.abs(cam - ref).max()))
    return ref, mar, d


def test_default_schedule_step_indices():
    """A 3-step and a 502-step run of the real reference loop from a recorded start against the float64 yardstick with the
    default schedule.  No residual of this run comes within the band, so every arithmetic takes the same signs; tolerance: 4 x
    the yardstick's own fp32-against-float64 spread over 8 summation orders.  The rate changes are pinned: first steps 500 /
    1000 (the rate lowered one step early) or 502 / 1002 (one late) miss the 502-step record."""
    g = cc.golden()
    rec = cc.fit_case("j17")
    p, t, c0 = rec["joints3d"][None], rec["target"][None], g["sched_start"][None]
    for steps, key in ((3, "sched_cam3"), (502, "sched_cam502")):
        ref, mar, spread = _fp32_spread(p, t, c0, steps)
        assert mar[0] >= cc.BAND
        err = np.abs(ref[0] - g[key].astype(np.float64)).max()
        print(f"steps {steps}: |yardstick - reference| = {err:.3e}, fp32 spread {spread:.3e}, min |residual| {mar[0]:.3e}")
        assert err <= 4 * spread + 2 * U * np.abs(g[key]).max()          # (the record itself is float32)
    for wrong in (((0, 0.1), (500, 0.05), (1000, 0.001)), ((0, 0.1), (502, 0.05), (1002, 0.001))):
        cam, _, _ = camfit_ref.fit(p, t, None, c0, steps=502, schedule=wrong, img_res=cc.IMG_RES)
        assert np.abs(cam[0] - g["sched_cam502"]).max() > 100 * (4 * spread)


@pytest.mark.parametrize("case", cc.FIT_CASES + ("outlier_w0",))
def test_full_run_bounds_are_attainable(case):
    """Conditions (a) and (b) of the GPU test hold for arithmetics that are NOT the reference's: the yardstick in float64 and in
    fp32 with two shuffled summation orders, from the same 32 starts."""
    rec = cc.fit_case(case)
    S, J = cc.N_LAUNCH, len(rec["joints3d"])
    p, t = np.repeat(rec["joints3d"][None], S, 0), np.repeat(rec["target"][None], S, 0)
    rng = np.random.default_rng(9)
    for dtype, order in ((np.float64, None), (np.float32, rng.permutation(J)), (np.float32, rng.permutation(J))):
        cam, _, _ = camfit_ref.fit(p, t, None, rec["starts"][:S], img_res=cc.IMG_RES, dtype=dtype, order=order)
        cc.check_full_run(cam, rec)


@pytest.mark.parametrize("case", cc.FIT_CASES + ("outlier_w0",))
def test_optimum_is_below_every_recorded_loss(case):
    rec = cc.fit_case(case)
    cam, loss = camfit_ref.l1_optimum(rec["joints3d"], rec["target"], None, cc.IMG_RES)
    assert abs(loss - rec["opt_loss"]) <= 1e-9 * loss
    assert (rec["losses"] >= rec["opt_loss"] - 1e-9).all()
    # dropping the outlier by weight is dropping it from the problem
    if case == "outlier_w0":
        full = cc.fit_case("outlier")
        w = np.ones(17, np.float32)
        w[cc.OUTLIER_JOINT] = 0
        assert abs(camfit_ref.l1_optimum(full["joints3d"], full["target"], w, cc.IMG_RES)[1] - loss) <= 1e-9 * loss


def test_stage_10_start_values():
    """(s, tx, ty) = (word >> 8) 2^-24 of words 0, 1, 2 of Philox at counter (index, joint 0 | 10 << 8, block 0), key = seed."""
    for seed, index in ((0, 0), (123, 5), (2 ** 40 + 17, 2 ** 33 + 3), (2 ** 64 - 1, 2 ** 64 - 2)):
        got = camfit_ref.start(seed, index, 2)
        for b in range(2):
            i = (index + b) % 2 ** 64
            w = sample_ref.philox(i & 0xFFFFFFFF, i >> 32, 10 << 8, 0, seed & 0xFFFFFFFF, seed >> 32)
            want = [float(int(w[k]) >> 8) * U for k in range(3)]
            assert got[b].tolist() == want
        assert ((got >= 0) & (got < 1)).all()
    assert len({tuple(r) for r in camfit_ref.start(123, 0, 64).tolist()}) == 64


def test_short_run_generator_leaves_out_no_case():
    """The generator of the GPU short-run test: the yardstick alone leaves out no sample (every min_abs_residual over 32 steps
    stays above the band), so the GPU test's `at most one in eight` has its whole margin."""
    kept = total = 0
    for B in cc.SHORT_B:
        for J in cc.SHORT_J:
            y = cc.short_yardstick(B, J)[32]
            kept, total = kept + int(y["keep"].sum()), total + B
    print(f"kept {kept} of {total}")
    assert kept == total
    y = cc.weight_yardstick()[32]                      # the weighted short runs start from recorded torch.rand values
    assert y["keep"].sum() * 8 >= len(y["keep"]) * 7
