"""GPU: the body-model layer (pose2mesh_release_amd.body, csrc/body.hip) against the float64 fixtures the real
SMPL_Layer / ManoLayer produced and against tests/body_ref.py.

The bar everywhere: per-vertex and per-joint L2 <= 4 x the error of an fp32 run of the reference against its float64 run
(the factor test_bf16x3_error_is_fp32_class grants an fp32-class result over the fp32 baseline).  Fixture cases use their
stored error (the real layers' fp32 run).  Cases without one use body_ref's fp32 run of the same operator sequence - of
the case itself where it has thousands of vertices, else of a companion batch (same model kind, same input options, V =
257, B = 9): a per-vertex error class does not depend on how many vertices or samples a launch has, and the maximum over
a handful of points would be a noisy bar."""
import functools
import types

import numpy as np
import pytest
import torch

import body_cases
import body_ref
from pose2mesh_release_amd import body, synth

pytestmark = pytest.mark.gpu
TILE = body.SAMPLE_TILE


def _layer(m, center_idx=None, extra_reg=None, **kw):
    a = dict(betas=m["betas"], hands_mean=m.get("hands_mean"), tip_vertices=m.get("tip_vertices"),
             joint_order=m.get("joint_order"), scale=m.get("scale", 1.0), center_idx=center_idx, extra_regressor=extra_reg)
    a.update(kw)
    return body.BodyModel(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["weights"], m["parents"], **a)


def _cuda(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def _run(layer, pose, betas=None, trans=None):
    out = layer(_cuda(pose), _cuda(betas), _cuda(trans))
    torch.cuda.synchronize()
    return [o.cpu().numpy().copy() for o in out]


def _inputs(B, J, seed, special=True):
    """The fixture generator's input distribution: N(0, 0.6^2) poses, a zero pose and one beyond pi when B >= 5."""
    rng = np.random.default_rng(seed)
    pose = rng.standard_normal((B, J, 3)) * 0.6
    if B >= 5 and special:
        pose[1] = 0.0
        d = rng.standard_normal((J, 3))
        pose[2] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(3.0, 4.0, (J, 1))
    betas = rng.standard_normal((B, 10))
    betas[B - 1, 0] = 3.5
    trans = rng.standard_normal((B, 3)) * 0.7
    return [x.astype(np.float32) for x in (pose.reshape(B, -1), betas, trans)]


def _check(got, want, bar, what):
    for name, g, w in zip(("verts", "joints", "extra"), got, want):
        e = body_ref.max_l2(g, w)
        print(f"{what} {name}: max L2 {e:.3e}  bar {bar:.3e}")
        assert np.isfinite(g).all() and e <= bar, (what, name, e, bar)


@pytest.mark.parametrize("flavour,name", body_cases.case_ids())
def test_fixture_cases(hip_libs, flavour, name):
    c = body_cases.case(flavour, name)
    layer = _layer(c["model"], c["center_idx"], c["extra_reg"])
    got = _run(layer, c["pose"], c["betas"], c["trans"])
    want = [c["verts"], c["joints"]] + ([c["extra"]] if c["extra_reg"] is not None else [])
    assert len(got) == len(want) and all(g.shape == w.shape for g, w in zip(got, want))
    _check(got, want, 4 * c["err32"], f"{flavour}/{name}")


@functools.lru_cache(maxsize=None)
def _companion_err32(kind, with_trans, center_idx, J=None):
    m = _two_joint_model(257) if J == 2 else body_cases.model(kind, 257)
    pose, betas, trans = _inputs(9, len(m["parents"]), seed=100)
    return body_ref.err32(m, pose, betas, trans if with_trans else None, center_idx)


def _two_joint_model(V):
    m = dict(synth.body_model("smpl", V, seed=1))
    w = m["weights"][:, :2] + np.float32(0.25)
    m.update(J_regressor=m["J_regressor"][:2], weights=(w / w.sum(1, keepdims=True)).astype(np.float32),
             posedirs=np.ascontiguousarray(m["posedirs"][:, :, :9]), parents=[-1, 0])
    return m


@pytest.mark.parametrize("with_trans", [False, True])
def test_zero_pose(hip_libs, with_trans):
    """All-zero poses: the + 1e-8 of batch_rodrigues and the identity path.  verts = template + shapedirs beta (+ trans),
    joints = the rest joints (+ trans)."""
    m = body_cases.model("smpl", 257)
    _, betas, trans = _inputs(5, 24, seed=3)
    trans = trans if with_trans else None
    verts, joints = _run(_layer(m), np.zeros((5, 72), np.float32), betas, trans)
    f8 = np.float64
    want_v = m["v_template"].astype(f8) + np.einsum("vcn,bn->bvc", m["shapedirs"].astype(f8), betas.astype(f8))
    want_j = np.stack([body_ref.rest_joints(m, b) for b in betas])
    if with_trans:
        want_v, want_j = want_v + trans[:, None].astype(f8), want_j + trans[:, None].astype(f8)
    _check([verts, joints], [want_v, want_j], 4 * _companion_err32("smpl", with_trans, None), "zero pose")
    hand = body_cases.model("mano", 778)                     # MANO: zero coefficients are hands_mean, not the rest shape
    got = _run(_layer(hand), np.zeros((2, 48), np.float32))
    _check(got, body_ref.forward(hand, np.zeros((2, 48))), 4 * _companion_err32("mano", False, None), "zero coeffs")


@pytest.mark.parametrize("V", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("B", [1, TILE - 1, TILE, TILE + 1])
def test_launch_edges(hip_libs, V, B):
    """Across the 64-vertex tile and the sample tile of the skinning kernel, with a translation and an extra regressor."""
    assert body.VERTEX_TILE == 64
    m = body_cases.model("smpl", V)
    reg = synth.synthetic_regressor(3, V, seed=2) if V >= 6 else np.ones((2, V), np.float32) / V
    pose, betas, trans = _inputs(B, 24, seed=V * 100 + B)
    got = _run(_layer(m, extra_reg=reg), pose, betas, trans)
    _check(got, body_ref.forward(m, pose, betas, trans, None, reg), 4 * _companion_err32("smpl", True, None), f"V={V} B={B}")


def test_two_joints_and_last_vertex_tip(hip_libs):
    m = _two_joint_model(65)
    pose, betas, _ = _inputs(TILE + 1, 2, seed=8)
    got = _run(_layer(m, center_idx=1), pose, betas)
    _check(got, body_ref.forward(m, pose, betas, None, 1), 4 * _companion_err32("smpl", False, 1, J=2), "J=2")
    hand = body_cases.model("mano", 65)
    tips = [64, 0, 31, 63, 17]
    pose, betas, trans = _inputs(3, 16, seed=9)
    got = _run(_layer(hand, tip_vertices=tips), pose, betas, trans)
    want = body_ref.forward(hand, pose, betas, trans, tip_vertices=tips)
    _check(got, want, 4 * _companion_err32("mano", True, None), "tip = V - 1")
    assert np.array_equal(got[1][:, 4], got[0][:, 64])      # output joint 4 is tip 0: vertex V - 1 itself


@pytest.mark.parametrize("kind", ["smpl", "mano"])
def test_batch_independence(hip_libs, kind):
    """Sample i of a B = 37 call is bitwise the same sample run alone, for every output: first, last, and both sides of a
    sample-tile boundary.  Two identical calls are bitwise equal."""
    m = body_cases.model(kind, 257 if kind == "smpl" else 778)
    J = len(m["parents"])
    reg = synth.synthetic_regressor(5, m["num_vertex"], seed=4)
    pose, betas, trans = _inputs(37, J, seed=12)
    for tr, center in ((trans, None), (None, 0)):
        layer = _layer(m, center, reg)
        full = _run(layer, pose, betas, tr)
        again = _run(layer, pose, betas, tr)
        assert all(np.array_equal(a, b) for a, b in zip(full, again))
        for i in (0, TILE - 1, TILE, 36):
            one = _run(layer, pose[i:i + 1], betas[i:i + 1], None if tr is None else tr[i:i + 1])
            for name, a, b in zip(("verts", "joints", "extra"), one, full):
                assert np.array_equal(a[0], b[i]), (kind, i, name)


def test_smpl_size(hip_libs):
    m = body_cases.model("smpl", 6890)
    pose, betas, trans = _inputs(8, 24, seed=21)
    reg = synth.synthetic_regressor(17, 6890)
    got = _run(_layer(m, extra_reg=reg), pose, betas, trans)
    bar = 4 * body_ref.err32(m, pose, betas, trans)
    _check(got, body_ref.forward(m, pose, betas, trans, None, reg), bar, "V=6890 B=8")


def test_graph_capture_replays_bitwise(hip_libs):
    """One forward captured as a graph on a single stream; the static inputs are refreshed and the replay is bitwise the
    eager result, and allocates nothing."""
    m = body_cases.model("mano", 778)
    reg = synth.synthetic_regressor(21, 778, seed=6)
    B = TILE + 3
    first, second = _inputs(B, 16, seed=30), _inputs(B, 16, seed=31)
    layer, eager_layer = _layer(m, extra_reg=reg), _layer(m, extra_reg=reg)
    eager = [torch.from_numpy(o) for o in _run(eager_layer, *second)]
    static = [_cuda(x) for x in first]
    layer(*static)                                           # the buffers of this batch size exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = layer(*static)
    for s, x in zip(static, second):
        s.copy_(torch.from_numpy(x))
    for o in out:
        o.zero_()
    torch.cuda.synchronize()
    before = (torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"])
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert before == (torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"])
    for o, e in zip(out, eager):
        assert torch.equal(o.cpu(), e)


def test_buffer_reuse_does_not_alias(hip_libs):
    m = body_cases.model("smpl", 65)
    layer = _layer(m)
    p3, b3, _ = _inputs(3, 24, seed=40)
    p5, b5, _ = _inputs(5, 24, seed=41)
    v3, j3 = layer(_cuda(p3), _cuda(b3))
    keep = (v3.clone(), j3.clone())
    v5, j5 = layer(_cuda(p5), _cuda(b5))
    torch.cuda.synchronize()
    assert v3.data_ptr() != v5.data_ptr() and j3.data_ptr() != j5.data_ptr()
    assert torch.equal(v3, keep[0]) and torch.equal(j3, keep[1])           # the B = 5 call left the B = 3 buffers alone
    v3b, _ = layer(_cuda(p3[::-1].copy()), _cuda(b3))
    assert v3b.data_ptr() == v3.data_ptr() and not torch.equal(v3b, keep[0])   # same size: the buffer is reused


def test_from_layer_equals_arrays(hip_libs):
    for kind, V in (("smpl", 257), ("mano", 778)):
        m = body_cases.model(kind, V)
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32))         # noqa: E731
        stub = types.SimpleNamespace(th_betas=t(m["betas"])[None], th_shapedirs=t(m["shapedirs"]),
                                     th_posedirs=t(m["posedirs"]), th_v_template=t(m["v_template"])[None],
                                     th_J_regressor=t(m["J_regressor"]), th_weights=t(m["weights"]),
                                     kintree_parents=[4294967295] + list(m["parents"][1:]), center_idx=0)
        if kind == "mano":
            stub.th_hands_mean = t(m["hands_mean"])[None]
            stub.use_pca, stub.joint_rot_mode, stub.root_rot_mode, stub.side = False, "axisang", "axisang", "right"
        pose, betas, _ = _inputs(3, len(m["parents"]), seed=50)
        a = _run(body.BodyModel.from_layer(stub), pose, betas)
        b = _run(_layer(m, center_idx=0), pose, betas)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        _check(a, body_ref.forward(m, pose, betas, None, 0), 4 * _companion_err32(kind, False, 0), f"from_layer {kind}")


def test_inputs_that_require_grad_raise(hip_libs):
    from pose2mesh_release_amd._lib import P2MError
    layer = _layer(body_cases.model("smpl", 65))
    with pytest.raises(P2MError):
        layer(torch.zeros(1, 72, device="cuda", requires_grad=True))
    with pytest.raises(ValueError):
        layer(torch.zeros(1, 24, 3, 3, device="cuda"))
    with pytest.raises(ValueError):
        layer(torch.zeros(2, 72, device="cuda"), torch.zeros(3, 10, device="cuda"))
