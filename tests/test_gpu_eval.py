"""-m gpu: evaluation on the GPU (pose2mesh_release_amd.evaluate: p2m_rigid_align, p2m_mesh_eval) against the real
reference's rigid_transform_3D / rigid_align (tests/golden/eval_*.npz) and against the float64 restatement of the
evaluation loop bodies (tests/eval_ref.py); padding, determinism, graph capture, and GraphedInference -> evaluator."""
import numpy as np
import pytest
import torch

import eval_ref
import helpers

pytestmark = pytest.mark.gpu

H36M_EVAL_JOINT = (1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15, 16)    # data/Human36M/dataset.py:62
BAR_MM = 2e-4


def _fixture_regressor(z):
    R = np.zeros(tuple(int(v) for v in z["reg_shape"]), dtype=np.float32)
    R[z["reg_rows"], z["reg_cols"]] = z["reg_vals"]
    return R


def _check_align(A, B, c, R, t, A2, rc, rR, rt, rA2, what):
    sc = float(np.abs(B).max())
    assert np.abs(R - rR).max() <= 1e-6, what
    assert (np.abs(c - rc) / np.abs(rc)).max() <= 1e-6, what
    assert np.abs(t - rt).max() <= 4e-7 * sc, what
    assert np.abs(A2 - rA2).max() <= 4e-7 * sc, what


def test_rigid_align_vs_reference_fixtures(hip_libs):
    """Every case of eval_align.npz (N = 3 .. 778, mirrored B, planar A): R 1e-6 per element, c 1e-6 relative, t and A2
    4e-7 x max|B| per element (a few fp32 ulps: holds only with fp64 internals)."""
    from pose2mesh_release_amd import evaluate
    z = helpers.golden("eval_align.npz")
    for case in [str(c) for c in z["cases"]]:
        A, B = z[f"{case}_A"], z[f"{case}_B"]
        Ag, Bg = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
        c, R, t = evaluate.rigid_transform_3D(Ag, Bg)
        A2 = evaluate.rigid_align(Ag, Bg)
        _check_align(A, B, c.cpu().numpy(), R.cpu().numpy(), t.cpu().numpy(), A2.cpu().numpy(), z[f"{case}_c"],
                     z[f"{case}_R"], z[f"{case}_t"], z[f"{case}_A2"], case)
        c1, R1, t1 = evaluate.rigid_transform_3D(Ag[0], Bg[0])           # unbatched [N, 3]
        assert c1.shape == () and R1.shape == (3, 3) and torch.equal(R1, R[0]) and torch.equal(c1, c[0])
        assert torch.equal(evaluate.rigid_align(Ag[0], Bg[0]), A2[0])


def test_exact_similarity_is_recovered(hip_libs):
    """B = c R A + t exactly (float64, then fp32): the PA error is at the fp32 rounding of mm data, <= 2e-4 mm."""
    from pose2mesh_release_amd import evaluate
    rng = np.random.default_rng(11)
    for N in (14, 6890):
        nb = 6
        A = (rng.uniform(-1, 1, (nb, N, 3)) * 600).astype(np.float32)
        Bs = np.empty((nb, N, 3))
        for i in range(nb):
            Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
            Q *= np.sign(np.linalg.det(Q))
            Bs[i] = rng.uniform(0.8, 1.25) * A[i].astype(np.float64) @ Q.T + rng.uniform(-500, 500, 3)
        assert np.abs(Bs).max() <= 2000
        B = Bs.astype(np.float32)
        A2 = evaluate.rigid_align(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()).cpu().numpy()
        assert np.linalg.norm(A2.astype(np.float64) - B, axis=-1).max() <= BAR_MM, N


def test_coincident_sample_is_non_finite_alone(hip_libs):
    """One sample whose points all coincide (varP = 0): its c, t and A2 are non-finite (the reference divides by zero),
    nothing faults, and every other sample of the batch is within the fixture bars."""
    from pose2mesh_release_amd import evaluate
    z = helpers.golden("eval_align.npz")
    for case in ("rand14", "rand778"):
        A, B = z[f"{case}_A"].copy(), z[f"{case}_B"]
        A[1] = A[1, :1]                                                   # sample 1: every point equal
        c, R, t = evaluate.rigid_transform_3D(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda())
        A2 = evaluate.rigid_align(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()).cpu().numpy()
        c, R, t = c.cpu().numpy(), R.cpu().numpy(), t.cpu().numpy()
        assert not np.isfinite(c[1]) and not np.isfinite(t[1]).any() and not np.isfinite(A2[1]).any()
        keep = [i for i in range(A.shape[0]) if i != 1]
        _check_align(A[keep], B[keep], c[keep], R[keep], t[keep], A2[keep], z[f"{case}_c"][keep], z[f"{case}_R"][keep],
                     z[f"{case}_t"][keep], z[f"{case}_A2"][keep], case)


@pytest.mark.parametrize("name", ["eval_mesh_smpl.npz", "eval_mesh_mano.npz"])
def test_evaluator_vs_reference_mesh_fixtures(hip_libs, name):
    """Stage A + E + PA-MPVPE on the reference's own loop-body results (real rigid_align; the real H36M regressor on the
    SMPL-size case), ground truth in metres read x 1000."""
    from pose2mesh_release_amd import evaluate
    z = helpers.golden(name)
    reg = _fixture_regressor(z)
    sub, root = list(z["sub"]), int(z["root"])
    ev = evaluate.MeshEvaluator(reg.shape[1], reg, root, sub_A=sub, regressor_E=reg, root_E=root, sub_E=sub, pa_mesh=True,
                                gt_mesh_scale=float(z["gt_scale"]))
    out = ev(torch.from_numpy(z["pred"]).cuda(), torch.from_numpy(z["gt"]).cuda())
    for k in eval_ref.EVAL_KEYS:
        assert np.abs(out[k].cpu().numpy().astype(np.float64) - z[k]).max() <= BAR_MM, k


def _meshes(B, nv, seed, scale_m=False):
    """Body-sized mm meshes: gt an ellipsoid hull at ~4 m, pred a perturbed similarity of it (gt in metres if scale_m)."""
    from pose2mesh_release_amd import synth
    rng = np.random.default_rng(seed)
    verts, _ = synth.hull_mesh(nv, 0)
    body = verts.astype(np.float64) * np.array([250.0, 800.0, 150.0])
    gt = body[None] @ np.stack([np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(B)]).transpose(0, 2, 1)
    gt += rng.uniform(-500, 500, (B, 1, 3)) + np.array([0, 0, 4000.0])
    pred = gt * rng.uniform(0.95, 1.05, (B, 1, 1)) + rng.uniform(-80, 80, (B, 1, 3)) + rng.standard_normal(gt.shape) * 15
    gt = (gt / 1000.0 if scale_m else gt).astype(np.float32)
    return pred.astype(np.float32), gt


CONFIGS = [
    # nv, B, stage A regressor, sub_A, stage E, gt joints given, pa_mesh, groups, gt in metres
    (6890, 64, "h36m", H36M_EVAL_JOINT, "h36m", "E", True, True, True),        # Human36M.evaluate: SMPL-like A, H36M E
    (6890, 7, "syn24", None, "h36m", None, True, False, True),
    (6890, 300, "h36m", H36M_EVAL_JOINT, None, "A", False, True, False),       # the Tester's compute_both_err
    (6890, 1, "syn24", None, "h36m", "AE", True, False, False),
    (778, 300, "syn21", None, "syn21", None, True, True, False),               # FreiHAND-like: PA-MPVPE
    (778, 7, "syn21", None, None, "A", False, False, True),
    (778, 64, "syn24", list(range(0, 24, 2)), "syn21", "E", True, False, False),
    (778, 1, "syn21", None, "syn21", "AE", True, True, False),
]


def _regressor(kind, nv):
    from pose2mesh_release_amd import synth
    if kind == "h36m":
        return helpers.golden_regressor("demo_h36m.npz")
    return synth.synthetic_regressor(int(kind[3:]), nv, seed=int(kind[3:]))


@pytest.mark.parametrize("cfg", CONFIGS, ids=[f"nv{c[0]}-B{c[1]}-{c[2]}-{c[4]}-{c[5]}" for c in CONFIGS])
def test_evaluator_vs_eval_ref(hip_libs, cfg):
    """Every per-joint and per-sample output within 2e-4 mm of eval_ref, and so are the summary and its per-group means."""
    from pose2mesh_release_amd import evaluate
    nv, B, ka, sub_A, ke, given, pa, groups, in_m = cfg
    RA, RE = _regressor(ka, nv), (_regressor(ke, nv) if ke else None)
    pred, gt = _meshes(B, nv, seed=B + nv, scale_m=in_m)
    scale = 1000.0 if in_m else 1.0
    rng = np.random.default_rng(B)
    gt_mm = gt.astype(np.float64) * scale
    gja = (np.einsum("jv,bvk->bjk", RA.astype(np.float64), gt_mm) + rng.standard_normal((B, RA.shape[0], 3)) * 5
           ).astype(np.float32) if given and "A" in given else None
    gje = (np.einsum("jv,bvk->bjk", RE.astype(np.float64), gt_mm) + rng.standard_normal((B, RE.shape[0], 3)) * 5
           ).astype(np.float32) if given and "E" in given else None
    grp = rng.integers(0, 15, B) if groups else None
    ev = evaluate.MeshEvaluator(nv, RA, 0, sub_A=sub_A, regressor_E=RE, root_E=0, sub_E=H36M_EVAL_JOINT if ke == "h36m" else None,
                                pa_mesh=pa, gt_mesh_scale=scale)

    def cu(x):
        return None if x is None else torch.from_numpy(x).cuda()
    out = ev(cu(pred), cu(gt), gt_joints_A=cu(gja), gt_joints_E=cu(gje), group=grp)
    ref = eval_ref.mesh_eval(pred, gt, RA, 0, sub_A, RE, 0, H36M_EVAL_JOINT if ke == "h36m" else None, pa, scale,
                             gt_joints_A=gja, gt_joints_E=gje)
    assert set(k for k in out if k != "sample_means") == set(ref)
    for k, v in ref.items():
        assert np.abs(out[k].cpu().numpy().astype(np.float64) - v).max() <= BAR_MM, k
    s, rs = ev.summary(), eval_ref.summary(ref, grp)
    assert s["samples"] == B
    for k in ref:
        assert abs(s[k] - rs[k]) <= BAR_MM, k
    if groups:
        assert sorted(s["groups"]) == sorted(rs["groups"])
        for g, d in rs["groups"].items():
            assert s["groups"][g]["samples"] == d["samples"]
            for k in ref:
                assert abs(s["groups"][g][k] - d[k]) <= BAR_MM, (g, k)
    ev.reset()
    assert ev.summary()["samples"] == 0


def test_compute_both_err_drop_in(hip_libs):
    """compute_both_err(pred_mesh, target_mesh, pred_joint, target_joint, eval_joint) (data/PW3D/dataset.py:273-286): the two
    floats of the numpy original, from the joints the caller passes (the Tester's J_regressor @ pred_mesh, reg_pose3d)."""
    from pose2mesh_release_amd import evaluate
    nv, B = 6890, 16
    pred, gt = _meshes(B, nv, seed=3)
    R = helpers.golden_regressor("demo_h36m.npz")
    pj = np.einsum("jv,bvk->bjk", R, pred).astype(np.float32)
    tj = (np.einsum("jv,bvk->bjk", R.astype(np.float64), gt.astype(np.float64)) + 3.0).astype(np.float32)
    j_err, s_err = evaluate.compute_both_err(*(torch.from_numpy(x).cuda() for x in (pred, gt, pj, tj)), H36M_EVAL_JOINT)
    p64, g64 = pred.astype(np.float64), gt.astype(np.float64)
    pm, tm = p64 - pj[:, :1].astype(np.float64), g64 - tj[:, :1].astype(np.float64)
    pjr, tjr = (pj - pj[:, :1]).astype(np.float64), (tj - tj[:, :1]).astype(np.float64)
    pjr, tjr = pjr[:, list(H36M_EVAL_JOINT)], tjr[:, list(H36M_EVAL_JOINT)]
    ref_s = np.sqrt(((pm - tm) ** 2).sum(2)).mean()
    ref_j = np.sqrt(((pjr - tjr) ** 2).sum(2)).mean()
    assert isinstance(j_err, float) and abs(j_err - ref_j) <= BAR_MM and abs(s_err - ref_s) <= BAR_MM


def _padded_pair(nv, B, B_real, seed):
    pred, gt = _meshes(B, nv, seed=seed, scale_m=True)
    pp, gp = pred.copy(), gt.copy()
    pp[B_real:], gp[B_real:] = np.nan, np.nan
    return pred[:B_real], gt[:B_real], pp, gp


def test_padding_and_determinism(hip_libs):
    """NaN in the padding rows with B_real < B: the real rows are bitwise the unpadded call's, padding outputs are 0, the
    summary is finite and equal to the unpadded one to 1e-12; two identical calls are bitwise equal."""
    from pose2mesh_release_amd import evaluate
    nv, B, B_real = 6890, 64, 50
    R = helpers.golden_regressor("demo_h36m.npz")
    pred, gt, pp, gp = _padded_pair(nv, B, B_real, seed=9)
    grp = np.arange(B) % 5

    def make():
        return evaluate.MeshEvaluator(nv, R, 0, sub_A=H36M_EVAL_JOINT, regressor_E=R, root_E=0, sub_E=H36M_EVAL_JOINT,
                                      pa_mesh=True, gt_mesh_scale=1000.0)
    e1, e2 = make(), make()
    o1 = {k: v.clone() for k, v in e1(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), group=grp[:B_real]).items()}
    o2 = {k: v.clone() for k, v in e2(torch.from_numpy(pp).cuda(), torch.from_numpy(gp).cuda(), B_real=B_real,
                                      group=grp).items()}
    for k in o1:
        assert torch.equal(o1[k], o2[k][:B_real]), k
        assert float(o2[k][B_real:].abs().max()) == 0.0, k
    s1, s2 = e1.summary(), e2.summary()
    assert s1["samples"] == s2["samples"] == B_real
    for k in ("mpjpe_E", "pa_mpjpe_E", "mpjpe_A", "mpvpe", "pa_mpvpe"):
        assert np.isfinite(s2[k]) and abs(s1[k] - s2[k]) <= 1e-12 * abs(s1[k]), k
        for g in s1["groups"]:
            assert abs(s1["groups"][g][k] - s2["groups"][g][k]) <= 1e-12 * abs(s1["groups"][g][k])
    o3 = e2(torch.from_numpy(pp).cuda(), torch.from_numpy(gp).cuda(), B_real=B_real, group=grp)
    for k in o2:
        assert torch.equal(o2[k], o3[k]), k
    assert e2.summary()["samples"] == 2 * B_real


def test_graph_capture_replays_bitwise(hip_libs):
    """torch.cuda.graph capture of one evaluator call (single stream) replays to the eager call's outputs bit for bit."""
    from pose2mesh_release_amd import evaluate
    nv, B = 6890, 16
    R = helpers.golden_regressor("demo_h36m.npz")
    pred, gt = _meshes(B, nv, seed=21, scale_m=True)
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    ev = evaluate.MeshEvaluator(nv, R, 0, sub_A=H36M_EVAL_JOINT, regressor_E=R, root_E=0, sub_E=H36M_EVAL_JOINT,
                                pa_mesh=True, gt_mesh_scale=1000.0)
    eager = {k: v.clone() for k, v in ev(p, g).items()}
    torch.cuda.synchronize()
    ev.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ev(p, g)
    for k in out:
        out[k].zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(out[k], eager[k]), k
    assert ev.summary()["samples"] == 2 * B


def test_graphed_inference_then_evaluator(hip_libs):
    """End to end: GraphedInference (B = 64, eval, golden H36M graphs) and the evaluator on the same stream; == eval_ref on
    the same outputs copied to the host (bar 3).  Once more with B_real = 50 (NaN-free padding from the graph's rows)."""
    from pose2mesh_release_amd import evaluate, infer, pose2mesh_net, synth
    gL, _, rev = helpers.golden_graphs("human36")
    J = int(gL[-1].shape[0])
    net = pose2mesh_net.get_model(J, gL, mano=False)
    net.load_state_dict(helpers.numpy_state(net.state_dict(), 2))
    net = net.cuda().eval()
    nv, B = 6890, 64
    R = helpers.golden_regressor("demo_h36m.npz")
    step = infer.GraphedInference(net, np.asarray(rev), nv, R, B, scale=1000.0)
    ev = evaluate.MeshEvaluator(nv, R, 0, sub_A=H36M_EVAL_JOINT, regressor_E=R, root_E=0, sub_E=H36M_EVAL_JOINT,
                                pa_mesh=True, gt_mesh_scale=1000.0)
    _, gt = _meshes(B, nv, seed=5, scale_m=True)
    gt_d = torch.from_numpy(gt).cuda()
    for B_real in (B, 50):
        mesh, joints, _ = step(synth.pose2d_batch(B, J, seed=40 + B_real).cuda())
        out = ev(mesh, gt_d, gt_joints_A=None, B_real=B_real)
        torch.cuda.synchronize()
        m = mesh.cpu().numpy()[:B_real]
        ref = eval_ref.mesh_eval(m, gt[:B_real], R, 0, H36M_EVAL_JOINT, R, 0, H36M_EVAL_JOINT, True, 1000.0)
        assert np.abs(m).max() > 10.0                                      # a real mm-scale mesh came out of the graph
        for k, v in ref.items():
            assert np.abs(out[k][:B_real].cpu().numpy().astype(np.float64) - v).max() <= BAR_MM, (B_real, k)
            assert float(out[k][B_real:].abs().max() if B_real < B else 0.0) == 0.0
    s = ev.summary()
    assert s["samples"] == B + 50
    net.set_inference(real_only=False)
