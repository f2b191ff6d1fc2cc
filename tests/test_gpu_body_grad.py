"""GPU: the differentiable body-model layer (pose2mesh_release_amd.body.BodyLayer, csrc/body_bwd.hip) against the float64
autograd gradients of the real SMPL_Layer / ManoLayer (tests/golden/body_grad_*.npz) and of tests/body_grad_ref.py.

The bar everywhere: per gradient tensor (g_pose, g_betas, g_trans), the max over sample rows of |g - g64|_2 / |g64|_2 is at
most 4 x the same figure of the reference's own fp32 autograd run against its float64 run (tests/test_gpu_body.py's rule).
Fixture cases take the stored figure, as the maximum over all cases of the fixture file; cases without a fixture take
body_grad_ref's fp32 run - of a companion batch (same model kind and input options, V = 257, B = 9), or of the case itself
where it has thousands of vertices: a single row's figure would be a noisy bar.  Every gradient must be finite.

The loss is L = sum c_v verts + sum c_j joints (+ sum c_x extra) with seeded standard-normal coefficients."""
import functools

import numpy as np
import pytest
import torch

import body_cases
import body_grad_cases
import body_grad_ref
from pose2mesh_release_amd import body, synth

pytestmark = pytest.mark.gpu
TILE = body.SAMPLE_TILE
NAMES = body_grad_cases.NAMES


def _model(m, center_idx=None, extra_reg=None, **kw):
    a = dict(betas=m["betas"], hands_mean=m.get("hands_mean"), tip_vertices=m.get("tip_vertices"),
             joint_order=m.get("joint_order"), scale=m.get("scale", 1.0), center_idx=center_idx, extra_regressor=extra_reg)
    a.update(kw)
    return body.BodyModel(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["weights"], m["parents"], **a)


def _cuda(x, grad=False):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda().requires_grad_(grad)


def _np(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def _grads(layer, pose, betas, trans, coeffs, need=(True, True, True), use=None):
    """Outputs and gradients (numpy; None where the input is None or needs none) of L = sum_o (c_o out_o), o in `use`."""
    ins = [_cuda(x, n) for x, n in zip((pose, betas, trans), need)]
    out = layer(*ins)
    use = range(len(out)) if use is None else use
    loss = sum((_cuda(coeffs[o]) * out[o]).sum() for o in use)
    loss.backward()
    torch.cuda.synchronize()
    return [_np(o) for o in out], [None if x is None else _np(x.grad) for x in ins]


def _inputs(B, J, seed):
    """The fixture generator's input distribution: N(0, 0.6^2) poses, a zero pose and one beyond pi when B >= 5."""
    rng = np.random.default_rng(seed)
    pose = rng.standard_normal((B, J, 3)) * 0.6
    if B >= 5:
        pose[1] = 0.0
        d = rng.standard_normal((J, 3))
        pose[2] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(3.0, 4.0, (J, 1))
    betas = rng.standard_normal((B, 10))
    betas[B - 1, 0] = 3.5
    trans = rng.standard_normal((B, 3)) * 0.7
    return [x.astype(np.float32) for x in (pose.reshape(B, -1), betas, trans)]


def _coeffs(seed, model, B, nx=0):
    return body_grad_ref.loss_coeffs(seed, [(B, model.V, 3), (B, model.NJ, 3)] + ([(B, nx, 3)] if nx else []))[0]


def _check(got, want, bars, what):
    errs = {}
    for n, g, w in zip(NAMES, got, want):
        assert (g is None) == (w is None) and (w is None or g.shape == w.shape), (what, n)
        if w is not None:
            errs[n] = body_grad_ref.row_err(g, w)
            print(f"{what} g_{n}: max row error {errs[n]:.3e}  bar {4 * bars[n]:.3e}")
    for n, g in zip(NAMES, got):
        assert g is None or (np.isfinite(g).all() and errs[n] <= 4 * bars[n]), (what, n, errs[n], 4 * bars[n])


def _ref_bars(m, pose, betas, trans, center_idx, reg, coeffs, tips=None):
    """body_grad_ref's float64 gradients and the row errors of its fp32 run."""
    g8 = body_grad_ref.grads(m, pose, betas, trans, center_idx, reg, tips, coeffs)
    g4 = body_grad_ref.grads(m, pose, betas, trans, center_idx, reg, tips, coeffs, dtype=torch.float32)
    return g8, {n: body_grad_ref.row_err(a, b) for n, a, b in zip(NAMES, g4, g8) if b is not None}


def _two_joint_model(V):
    m = dict(synth.body_model("smpl", V, seed=1))
    w = m["weights"][:, :2] + np.float32(0.25)
    m.update(J_regressor=m["J_regressor"][:2], weights=(w / w.sum(1, keepdims=True)).astype(np.float32),
             posedirs=np.ascontiguousarray(m["posedirs"][:, :, :9]), parents=[-1, 0])
    return m


@functools.lru_cache(maxsize=None)
def _companion_bars(kind, with_trans, center_idx, nx, J=None):
    m = _two_joint_model(257) if J == 2 else body_cases.model(kind, 257)
    pose, betas, trans = _inputs(9, len(m["parents"]), seed=100)
    reg = synth.synthetic_regressor(nx, 257, seed=2) if nx else None
    NJ = len(m["joint_order"]) if m.get("joint_order") is not None else len(m["parents"])
    coeffs = body_grad_ref.loss_coeffs(77, [(9, 257, 3), (9, NJ, 3)] + ([(9, nx, 3)] if nx else []))[0]
    return _ref_bars(m, pose, betas, trans if with_trans else None, center_idx, reg, coeffs)[1]


# ---- 1. fixture cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour,name", body_cases.case_ids())
def test_fixture_cases(hip_libs, flavour, name):
    c = body_grad_cases.case(flavour, name)
    model = _model(c["model"], c["center_idx"], c["extra_reg"])
    out, got = _grads(body.BodyLayer(model), c["pose"], c["betas"], c["trans"], c["coeffs"])
    _check(got, c["grads"], body_grad_cases.file_gerr32(flavour), f"{flavour}/{name}")
    plain = model(_cuda(c["pose"]), _cuda(c["betas"]), _cuda(c["trans"]))
    assert len(plain) == len(out) and all(np.array_equal(_np(p), o) for p, o in zip(plain, out))    # bitwise the forward


# ---- 2. launch edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("B", [1, TILE - 1, TILE, TILE + 1])
def test_launch_edges(hip_libs, V, B):
    assert body.VERTEX_TILE == 64
    m = body_cases.model("smpl", V)
    reg = synth.synthetic_regressor(3, V, seed=2) if V >= 6 else np.ones((3, V), np.float32) / V
    pose, betas, trans = _inputs(B, 24, seed=V * 100 + B)
    model = _model(m, extra_reg=reg)
    coeffs = _coeffs(V * 100 + B, model, B, 3)
    _, got = _grads(body.BodyLayer(model), pose, betas, trans, coeffs)
    want = body_grad_ref.grads(m, pose, betas, trans, None, reg, coeffs=coeffs)
    _check(got, want, _companion_bars("smpl", True, None, 3), f"V={V} B={B}")


# ---- 3. small models -----------------------------------------------------------------------------------------------------------
def test_two_joints_centred(hip_libs):
    m = _two_joint_model(65)
    pose, betas, _ = _inputs(TILE + 1, 2, seed=8)
    model = _model(m, center_idx=1)
    coeffs = _coeffs(8, model, TILE + 1)
    _, got = _grads(body.BodyLayer(model), pose, betas, None, coeffs)
    want = body_grad_ref.grads(m, pose, betas, None, 1, coeffs=coeffs)
    _check(got, want, _companion_bars("smpl", False, 1, 0, J=2), "J=2")


@pytest.mark.parametrize("tips", [[64, 0, 31, 63, 17], [5, 5, 31, 63, 17]], ids=["last_vertex", "repeated"])
def test_mano_tips(hip_libs, tips):
    hand = body_cases.model("mano", 65)
    pose, betas, trans = _inputs(3, 16, seed=9)
    model = _model(hand, tip_vertices=tips)
    coeffs = _coeffs(9, model, 3)
    _, got = _grads(body.BodyLayer(model), pose, betas, trans, coeffs)
    want = body_grad_ref.grads(hand, pose, betas, trans, tip_vertices=tips, coeffs=coeffs)
    _check(got, want, _companion_bars("mano", True, None, 0), f"tips {tips}")


# ---- 4. SMPL size --------------------------------------------------------------------------------------------------------------
def test_smpl_size(hip_libs):
    """V = 6890: the fold over 108 vertex blocks."""
    m = body_cases.model("smpl", 6890)
    pose, betas, trans = _inputs(8, 24, seed=21)
    reg = synth.synthetic_regressor(17, 6890)
    model = _model(m, extra_reg=reg)
    coeffs = _coeffs(21, model, 8, 17)
    _, got = _grads(body.BodyLayer(model), pose, betas, trans, coeffs)
    want, bars = _ref_bars(m, pose, betas, trans, None, reg, coeffs)
    _check(got, want, bars, "V=6890 B=8")


# ---- 5. batch independence -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["smpl", "mano"])
def test_batch_independence(hip_libs, kind):
    """Sample i of a B = 37 call is bitwise the same sample run alone: first, last, and both sides of a sample-tile boundary;
    with trans and with a centre.  Two identical calls are bitwise equal."""
    m = body_cases.model(kind, 257 if kind == "smpl" else 778)
    J = len(m["parents"])
    reg = synth.synthetic_regressor(5, m["num_vertex"], seed=4)
    pose, betas, trans = _inputs(37, J, seed=12)
    for tr, center in ((trans, None), (None, 0)):
        model = _model(m, center, reg)
        layer = body.BodyLayer(model)
        coeffs = _coeffs(12, model, 37, 5)
        _, full = _grads(layer, pose, betas, tr, coeffs)
        _, again = _grads(layer, pose, betas, tr, coeffs)
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(full, again))
        for i in (0, TILE - 1, TILE, 36):
            _, one = _grads(layer, pose[i:i + 1], betas[i:i + 1], None if tr is None else tr[i:i + 1], [c[i:i + 1] for c in coeffs])
            for n, a, b in zip(NAMES, one, full):
                assert (a is None and b is None) or np.array_equal(a[0], b[i]), (kind, i, n)


# ---- 6. partial graphs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["smpl", "mano"])
def test_partial_graphs(hip_libs, kind):
    m = body_cases.model(kind, 257 if kind == "smpl" else 778)
    B, J = TILE + 3, len(m["parents"])
    reg = synth.synthetic_regressor(5, m["num_vertex"], seed=4)
    pose, betas, trans = _inputs(B, J, seed=60)
    model = _model(m, None, reg)
    layer = body.BodyLayer(model)
    coeffs = _coeffs(60, model, B, 5)
    _, full = _grads(layer, pose, betas, trans, coeffs)
    # inputs that need no gradient get None; the others are the full computation's
    for need in ((True, False, False), (False, True, False), (False, False, True)):
        _, got = _grads(layer, pose, betas, trans, coeffs, need=need)
        for n, g, f, k in zip(NAMES, got, full, need):
            assert (g is None and not k) or (k and np.array_equal(g, f)), (need, n)
    # one output used downstream: equal to the full computation with explicit zero gradients for the other outputs
    zeros = [np.zeros_like(c) for c in coeffs]
    for o in (0, 1, 2):
        _, got = _grads(layer, pose, betas, trans, coeffs, use=[o])
        _, want = _grads(layer, pose, betas, trans, [coeffs[i] if i == o else zeros[i] for i in range(3)])
        for n, g, w in zip(NAMES, got, want):
            assert np.isfinite(g).all() and np.abs(g).max() > 0 and np.array_equal(g, w), (o, n)
    # betas=None: the stored betas, no gradient for them; pose and trans as with the same betas passed explicitly
    stored = np.broadcast_to(m["betas"], (B, 10)).copy()
    _, got = _grads(layer, pose, None, trans, coeffs)
    _, want = _grads(layer, pose, stored, trans, coeffs)
    assert got[1] is None and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    # a non-contiguous upstream gradient
    ins = [_cuda(x, True) for x in (pose, betas, trans)]
    out = layer(*ins)
    ups = [_cuda(c) for c in coeffs]
    ups[0] = _cuda(np.ascontiguousarray(coeffs[0].transpose(2, 1, 0))).permute(2, 1, 0)
    ups[2] = _cuda(np.repeat(coeffs[2], 2, axis=2))[:, :, ::2]
    assert not ups[0].is_contiguous() and not ups[2].is_contiguous()
    got = torch.autograd.grad(out, ins, ups)
    assert all(np.array_equal(_np(g), f) for g, f in zip(got, full))


# ---- 7. capture ------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_bitwise(hip_libs):
    """Forward plus backward into static .grad tensors, captured on one stream; replayed on refreshed inputs the gradients
    are bitwise the eager ones."""
    m = body_cases.model("mano", 778)
    reg = synth.synthetic_regressor(21, 778, seed=6)
    B = TILE + 3
    first, second = _inputs(B, 16, seed=30), _inputs(B, 16, seed=31)
    model = _model(m, extra_reg=reg)
    layer = body.BodyLayer(model)
    coeffs = _coeffs(30, model, B, 21)
    _, eager = _grads(layer, *second, coeffs)
    cs = [_cuda(c) for c in coeffs]
    static = [_cuda(x, True) for x in first]

    def step():
        out = layer(*static)
        sum((c * o).sum() for c, o in zip(cs, out)).backward()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                               # tables and allocator pools exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for s in static:
        s.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    with torch.no_grad():
        for s, x in zip(static, second):
            s.copy_(torch.from_numpy(x))
            s.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for n, s, e in zip(NAMES, static, eager):
        assert np.array_equal(_np(s.grad), e), n


# ---- 8. a fit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,V", [("smpl", 257), ("mano", 778)])
def test_parameters_fit_a_target_mesh(hip_libs, kind, V):
    """60 Adam steps (lr 0.02) from zero pose, betas and trans on mean |verts - target| / scale: the gradients drive an
    optimiser (the same loop through stock torch autograd falls 13 x or more on these models) - not a tolerance."""
    m = body_cases.model(kind, V)
    J = len(m["parents"])
    rng = np.random.default_rng(5)
    pose, betas, trans = (rng.standard_normal((4, 3 * J)) * 0.3, rng.standard_normal((4, 10)), rng.standard_normal((4, 3)) * 0.2)
    model = _model(m)
    target = model(_cuda(pose), _cuda(betas), _cuda(trans))[0].clone()
    layer = body.BodyLayer(model)
    params = [torch.zeros(s, device="cuda", requires_grad=True) for s in ((4, 3 * J), (4, 10), (4, 3))]
    opt = torch.optim.Adam(params, lr=0.02)
    losses = []
    for _ in range(61):
        loss = (layer(*params)[0] - target).abs().mean() / model.scale
        losses.append(loss.detach())
        opt.zero_grad()
        loss.backward()
        opt.step()
    first, last = float(losses[0]), float(losses[60])
    print(f"{kind}: loss {first:.5f} -> {last:.5f} ({first / last:.1f} x)")
    assert np.isfinite(last) and last <= first / 4


# ---- 9. guard rails --------------------------------------------------------------------------------------------------------------
def test_guard_rails(hip_libs):
    from pose2mesh_release_amd._lib import P2MError
    model = _model(body_cases.model("smpl", 65))
    layer = body.BodyLayer(model)
    with pytest.raises(P2MError):
        model(torch.zeros(1, 72, device="cuda", requires_grad=True))        # BodyModel itself stays forward only
    with pytest.raises(P2MError):
        layer(torch.zeros(1, 72, requires_grad=True))                        # CPU tensors
    with pytest.raises(ValueError):
        layer(torch.zeros(2, 72, device="cuda"), torch.zeros(3, 10, device="cuda"))
    assert not list(layer.parameters())
    pose = torch.zeros(2, 72, device="cuda", requires_grad=True)
    a, b = layer(pose), layer(pose)
    assert a[0].data_ptr() != b[0].data_ptr() and a[0].requires_grad            # new tensors per call
    assert not layer(pose.detach())[0].requires_grad
    g, = torch.autograd.grad(a[0].sum(), pose, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()                                                  # no double backward
