"""-m gpu: the camera kernels (p2m_pose_prepare, p2m_camera_fit; camfit.prepare_pose, camfit.CameraFitter) against the float64
yardstick (tests/camfit_ref.py) and the real reference's record (tests/golden/camfit_ref.npz).

The fit's objective is piecewise linear, so two arithmetics part for good once a residual crosses zero a step apart.  Hence
two kinds of check: SHORT runs (at most 32 steps) are held step-exactly to the float64 yardstick - a sample is left out when
the yardstick met a residual within 1e-3 px of zero, at most one in eight may be -, with 4 x the yardstick's own
fp32-against-float64 spread over 8 shuffled summation orders as the tolerance (never a figure of the code under test); FULL
runs are held to the objective value they reach and to the reference's own recorded scatter (conditions (a), (b) of
camfit_cases.check_full_run).  Shapes: B in {1, 5, 67} (one wave, not a multiple of a block's four waves, more than one
block), J in {1, 2, 17, 19, 21, 64} (one lane to a full wave)."""
import numpy as np
import pytest
import torch

import camfit_cases as cc
import camfit_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def cf(hip_libs):
    from pose2mesh_release_amd import camfit
    return camfit


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def host(ns):
    torch.cuda.synchronize()
    return {k: getattr(ns, k).cpu().numpy().copy() for k in vars(ns)}


def run_fit(cf, p, t, c0=None, w=None, **kw):
    fit = cf.CameraFitter(**kw)
    return host(fit(dev(p), dev(t), None if w is None else dev(w), None if c0 is None else dev(c0)))


# ---- preparation ------------------------------------------------------------------------------------------------------------
def pixel_poses(B, J):
    rng = np.random.default_rng(31 * B + J)
    centre = rng.uniform(150, 900, (B, 1, 2))
    spread = np.where(rng.uniform(size=(B, 1, 1)) < 0.5, np.array([60.0, 160.0]), np.array([220.0, 40.0]))
    return (centre + rng.normal(0, 1, (B, J, 2)) * spread).astype(np.float32)


def prep_tolerances(joints, ref):
    """Bounds on |kernel - float64 yardstick| per sample from the kernel's fp32 operation sequence (u = 2^-24, M the largest
    pixel magnitude among joints and box corners): a box value passes at most 6 roundings of values <= M: 8 u M; a target
    s (x - c) + res / 2 carries the centre's error times s, the scale's relative 3 u and three roundings of its own:
    16 u (s M + res); the standardised input as in tests/test_camfit_cpu.py, plus the butterfly sums' 8 u on mean and sd."""
    b1, b2 = ref["bbox"], ref["bbox2"]
    M = np.maximum(np.abs(joints).max(axis=(1, 2)), np.maximum(np.abs(b1[:, :2]).max(1) + b1[:, 2], np.abs(b2[:, :2]).max(1) + b2[:, 3]))
    s1, s2 = cc.CROP / b1[:, 2], 288.0 / b2[:, 2]
    d = 16 * U * (s2 * M + 384.0) / 288.0 + 8 * U
    c2 = b2[:, :2] + b2[:, 2:] / 2
    p = (s2[:, None, None] * (joints.astype(np.float64) - c2[:, None]) + np.array([144.0, 192.0])) / np.array([288.0, 384.0])
    z = np.abs(ref["pose2d"]).max(axis=(1, 2))
    tol_z = (2 * d / p.std(axis=1).min(1)) * (1 + z) + 4 * U * z
    return 8 * U * M, 16 * U * (s1 * M + cc.CROP), tol_z


@pytest.mark.parametrize("J", cc.SHORT_J)
def test_prepare_against_the_yardstick(cf, J):
    for B in cc.SHORT_B:
        joints = pixel_poses(B, J)
        ref = camfit_ref.prepare(joints)
        out = host(cf.prepare_pose(dev(joints)))
        assert (out["status"] == ref["status"]).all()
        if J == 1:                                         # a single point has no box
            assert (out["status"] == 1).all() and not any(out[k].any() for k in ("pose2d", "target", "bbox"))
            continue
        ok = ref["status"] == 0                            # (two joints less than a pixel apart have no box either)
        assert ok.sum() * 8 >= B * 7
        with np.errstate(all="ignore"):
            tb, tt, tz = prep_tolerances(joints, ref)
        for k, tol in (("bbox", tb), ("target", tt), ("pose2d", tz)):
            err = np.abs(out[k] - ref[k]).reshape(B, -1).max(1)
            assert (err[ok] <= tol[ok]).all(), (k, B, J, err[ok].max(), tol[ok].min())
            assert not out[k][~ok].any()


def test_prepare_against_the_reference_record(cf):
    """The four recorded poses: the kernel against what the reference's own functions gave, within the sum of the two
    derived bounds (yardstick to reference: tests/test_camfit_cpu.py; kernel to yardstick: prep_tolerances)."""
    g = cc.golden()
    for pose in cc.PREP_POSES:
        joints = g[f"prep_{pose}_joints"][None]
        ref = camfit_ref.prepare(joints)
        tb, tt, tz = prep_tolerances(joints, ref)
        out = host(cf.prepare_pose(dev(joints)))
        assert out["status"][0] == 0
        assert np.abs(out["bbox"][0] - g[f"prep_{pose}_bbox1"]).max() <= 2 * tb[0]
        assert np.abs(out["target"][0] - g[f"prep_{pose}_target"]).max() <= 2 * tt[0]
        assert np.abs(out["pose2d"][0] - g[f"prep_{pose}_pose2d"]).max() <= 2 * tz[0]


def test_prepare_degenerate_samples_and_their_neighbours(cf):
    clean = pixel_poses(5, 17)
    bad = clean.copy()
    bad[1] = bad[1, :1]                  # a single point
    bad[2, 4, 0] = np.nan
    bad[3, :, 1] = 333.0                 # zero height
    a, b = host(cf.prepare_pose(dev(clean))), host(cf.prepare_pose(dev(bad)))
    assert a["status"].tolist() == [0] * 5 and b["status"].tolist() == [0, 1, 1, 1, 0]
    for k in ("pose2d", "target", "bbox"):
        assert not b[k][1:4].any()
        assert b[k][0].tobytes() == a[k][0].tobytes() and b[k][4].tobytes() == a[k][4].tobytes()


# ---- short runs -------------------------------------------------------------------------------------------------------------
def short_tolerance(steps):
    """4 x the largest |fp32 mode - float64 mode| of the yardstick over every kept sample of every shape and 8 orders."""
    ys = [cc.short_yardstick(B, J)[steps] for B in cc.SHORT_B for J in cc.SHORT_J]
    return 4 * max(y["dcam"] for y in ys), 4 * max(y["dloss"] for y in ys)


@pytest.mark.parametrize("steps", cc.SHORT_STEPS)
def test_short_runs_step_exact(cf, steps):
    tol_cam, tol_loss = short_tolerance(steps)
    kept = total = 0
    worst = [0.0, 0.0]
    for B in cc.SHORT_B:
        for J in cc.SHORT_J:
            p, t, c0 = cc.short_batch(B, J)
            y = cc.short_yardstick(B, J)[steps]
            out = run_fit(cf, p, t, c0, steps=steps)
            keep = y["keep"]
            kept, total = kept + int(keep.sum()), total + B
            assert (out["status"][keep] & 1 == 0).all()
            if steps == 0:
                assert out["cam"].tobytes() == c0.tobytes()
            ec, el = np.abs(out["cam"] - y["cam"])[keep], np.abs(out["loss"] - y["loss"])[keep]
            worst = [max(worst[0], ec.max(initial=0.0)), max(worst[1], el.max(initial=0.0))]
            assert (ec <= tol_cam).all(), (B, J, ec.max(), tol_cam)
            assert (el <= tol_loss).all(), (B, J, el.max(), tol_loss)
    print(f"steps {steps}: kept {kept} of {total}; cam err {worst[0]:.3e} (tol {tol_cam:.3e}), loss err {worst[1]:.3e} "
          f"(tol {tol_loss:.3e})")
    assert kept * 8 >= total * 7


def test_exact_fixed_point(cf):
    """Every residual exactly 0: every gradient is 0 and 1500 steps leave the camera bitwise where it was."""
    p = np.array([[[0.5, 0.5, 0.1], [-0.5, 0.5, -0.2], [0.5, -0.5, 0.3], [-0.5, -0.5, 0.0]]], np.float32)
    t = (250.0 + 250.0 * p[:, :, :2]).astype(np.float32)
    c0 = np.array([[1.0, 0.0, 0.0]], np.float32)
    out = run_fit(cf, p, t, c0)
    assert out["cam"].tobytes() == c0.tobytes() and out["loss"][0] == 0.0 and out["status"][0] == 0


# ---- full runs --------------------------------------------------------------------------------------------------------------
N_LAUNCH = cc.N_LAUNCH


def loss_bound(cam, p, t):
    J = p.shape[1]
    pred = camfit_ref.residuals64(cam, p, t, cc.IMG_RES) + t
    return (2 * J + 4) * U * (np.abs(pred).max(axis=(1, 2)) + np.abs(t).max(axis=(1, 2)))


@pytest.mark.parametrize("case", cc.FIT_CASES)
def test_full_runs_reach_the_reference_scatter(cf, case):
    rec = cc.fit_case(case)
    p, t = np.repeat(rec["joints3d"][None], N_LAUNCH, 0), np.repeat(rec["target"][None], N_LAUNCH, 0)
    out = run_fit(cf, p, t, rec["starts"][:N_LAUNCH])
    assert (out["status"] == 0).all()
    cc.check_full_run(out["cam"], rec)
    err = np.abs(out["loss"] - camfit_ref.loss64(out["cam"], p, t, None, cc.IMG_RES))
    assert (err <= loss_bound(out["cam"], p, t)).all(), (err.max(), loss_bound(out["cam"], p, t).min())


def test_weights(cf):
    """Weight 0 on the outlier joint of the fourth case: short runs against the yardstick, the full run against the optimum and
    the reference scatter recorded WITHOUT that joint; a sample whose weights sum to 0 sets status bit 0."""
    p, t, w, c0 = (a[:N_LAUNCH] for a in cc.weight_case())
    ys = cc.weight_yardstick()
    for steps in (1, 2, 8, 32):
        y = ys[steps]
        keep = y["keep"][:N_LAUNCH]
        assert keep.sum() * 8 >= len(keep) * 7
        out = run_fit(cf, p, t, c0, w, steps=steps)
        assert (np.abs(out["cam"] - y["cam"][:N_LAUNCH])[keep] <= 4 * y["dcam"]).all()
        assert (np.abs(out["loss"] - y["loss"][:N_LAUNCH])[keep] <= 4 * y["dloss"]).all()
    full = cc.fit_case("outlier")
    out = run_fit(cf, p, t, c0, w)
    cc.check_full_run(out["cam"], cc.fit_case("outlier_w0"), full["joints3d"], full["target"], w[0])
    err = np.abs(out["loss"] - camfit_ref.loss64(out["cam"], p, t, w, cc.IMG_RES))
    assert (err <= loss_bound(out["cam"], p, t)).all()
    w0 = w[:3].copy()
    w0[1] = 0.0
    out0 = run_fit(cf, p[:3], t[:3], c0[:3], w0)
    assert out0["status"].tolist() == [0, 1, 0] and not out0["cam"][1].any() and out0["loss"][1] == 0.0
    assert out0["cam"][[0, 2]].tobytes() == out["cam"][[0, 2]].tobytes()


# ---- independence, reproducibility, the stream ----------------------------------------------------------------------------------
def test_a_sample_depends_on_itself_alone(cf):
    p, t, c0 = cc.short_batch(67, 17)
    a = run_fit(cf, p, t, c0)
    b = run_fit(cf, p, t, c0)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    for i in (0, 3, 65, 66):
        one = run_fit(cf, p[i:i + 1], t[i:i + 1], c0[i:i + 1])
        assert all(one[k][0].tobytes() == a[k][i].tobytes() for k in a), i


def test_drawn_starts_and_graph_replay(cf):
    from pose2mesh_release_amd import sample
    rec = cc.fit_case("j17")
    p, t = dev(np.repeat(rec["joints3d"][None], 9, 0)), dev(np.repeat(rec["target"][None], 9, 0))
    # the start itself: steps = 0 returns it
    z = cf.CameraFitter(steps=0, seed=77)
    got = host(z(p, t))["cam"]
    assert got.tobytes() == camfit_ref.start(77, 0, 9).astype(np.float32).tobytes() and z.stream.index == 9
    # batches of 4 + 5 from one stream are the batch of 9
    f1, f2 = cf.CameraFitter(seed=77), cf.CameraFitter(seed=77)
    whole = host(f1(p, t))
    parts = [host(f2(p[:4], t[:4])), host(f2(p[4:], t[4:]))]
    for k in whole:
        assert np.concatenate([parts[0][k], parts[1][k]]).tobytes() == whole[k].tobytes()
    # a captured graph holds the fit and the state's tensor add: every replay starts from fresh values
    fg = cf.CameraFitter(stream=sample.NoiseStream(77, 0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fg(p, t)                                            # allocates the buffers; index -> 9
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fg(p, t)
    graph.replay()
    first = host(out)
    graph.replay()
    second = host(out)
    assert fg.stream.index == 27
    assert first["cam"].tobytes() != second["cam"].tobytes()
    direct = host(cf.CameraFitter(stream=sample.NoiseStream(77, 18))(p, t))
    assert second["cam"].tobytes() == direct["cam"].tobytes()
    bound_a = cc.full_run_bounds(rec)[0]
    for r in (first, second):
        L = camfit_ref.loss64(r["cam"], p.cpu().numpy(), t.cpu().numpy(), None, cc.IMG_RES)
        assert (L - rec["opt_loss"] <= bound_a).all()


# ---- status and errors ------------------------------------------------------------------------------------------------------------
def test_status_bits(cf):
    p, t, c0 = cc.short_batch(5, 19)
    clean = run_fit(cf, p, t, c0)
    tb, cb = t.copy(), c0.copy()
    tb[1, 7, 1] = np.nan
    cb[3, 2] = np.inf
    bad = run_fit(cf, p, tb, cb)
    assert bad["status"].tolist() == [0, 1, 0, 1, 0]
    assert not bad["cam"][[1, 3]].any() and not bad["loss"][[1, 3]].any()
    for k in clean:
        assert bad[k][[0, 2, 4]].tobytes() == clean[k][[0, 2, 4]].tobytes()
    mirrored = (2 * cc.IMG_RES - t).astype(np.float32)      # the target turned by 180 degrees: the optimum has s < 0
    out = run_fit(cf, p, mirrored, c0)
    assert (out["status"] == 2).all() and (out["cam"][:, 0] < 0).all()


def test_errors(cf):
    from pose2mesh_release_amd._lib import P2MError
    p, t, c0 = (dev(a) for a in cc.short_batch(5, 17))
    fit = cf.CameraFitter()
    for J in (0, 65):
        with pytest.raises(P2MError):
            fit(torch.zeros(2, J, 3, device="cuda"), torch.zeros(2, J, 2, device="cuda"), cam0=torch.zeros(2, 3, device="cuda"))
        with pytest.raises(P2MError):
            cf.prepare_pose(torch.zeros(2, J, 2, device="cuda"))
    with pytest.raises(P2MError):
        cf.CameraFitter(schedule=((0, 0.1), (900, 0.05), (500, 0.001)))(p, t, cam0=c0)
    with pytest.raises(P2MError):
        cf.CameraFitter(schedule=())(p, t, cam0=c0)
    with pytest.raises(P2MError):
        cf.CameraFitter(steps=70000)(p, t, cam0=c0)
    with pytest.raises(P2MError):
        fit(p.cpu(), t, cam0=c0)
    with pytest.raises(P2MError):
        fit(p, t.cpu(), cam0=c0)
    with pytest.raises(P2MError):
        cf.prepare_pose(p.cpu()[:, :, :2])
    out = host(fit(p, t, cam0=c0))                          # and the fitter still works
    assert (out["status"] == 0).all()


# ---- closure with the renderer ------------------------------------------------------------------------------------------------------
def test_closure_with_the_renderer(cf):
    """Pixels -> prepare_pose -> fit -> crop_cam_to_image -> p2m_mesh_project lands every joint within its own fit residual
    (taken back to image pixels) + the 1/256 px snap of the input pixel: the sign and centre conventions of the three modules."""
    from pose2mesh_release_amd import render
    H, W, J = 480, 640, 17
    rng = np.random.default_rng(12)
    p = rng.normal(0, 0.3, (1, J, 3)).astype(np.float32)
    sx, tx, ty = 0.55, 0.12, -0.08
    sy = sx * W / H                                         # isotropic in pixels, as a weak-perspective crop camera is
    pix = np.stack([W / 2 * (1 + sx * (p[0, :, 0] + tx)), H / 2 * (1 + sy * (p[0, :, 1] + ty))], 1) + rng.normal(0, 2.0, (J, 2))
    pix = pix.astype(np.float32)[None]
    prep = cf.prepare_pose(dev(pix))
    fit = cf.CameraFitter(seed=5)(dev(p), prep.target)
    cam_img = render.crop_cam_to_image(fit.cam, prep.bbox, W, H)
    xy, st = render.project_vertices(dev(p), cam_img, H, W)
    torch.cuda.synchronize()
    assert int(prep.status[0]) == 0 and int(fit.status[0]) == 0 and int(st[0]) == 0
    ref = camfit_ref.prepare(pix)
    res = np.abs(camfit_ref.residuals64(fit.cam.cpu().numpy(), p, ref["target"].astype(np.float32), cc.IMG_RES)).max()
    bound = res * ref["bbox"][0, 2] / cc.CROP + 1.0 / 256
    err = np.abs(xy.cpu().numpy()[0] / 256.0 - pix[0].astype(np.float64)).max()
    print(f"closure: max |projected - input| = {err:.4f} px, bound {bound:.4f} px (max crop residual {res:.4f} px)")
    assert err <= bound
