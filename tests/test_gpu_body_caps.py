"""GPU: the body-model kernels (csrc/body.hip, csrc/body_bwd.hip) at their table caps and on odd skeletons - the cases of
tests/body_cap_cases.py, which tests/test_body_caps_cpu.py shows to reach the loop passes, chunk edges, LDS peaks and jslot /
regressor shapes they are named for - against tests/body_ref.py and tests/body_grad_ref.py in float64.

The bars are those of tests/test_gpu_body.py and tests/test_gpu_body_grad.py.  Forward: per-vertex and per-joint L2 <= 4 x
body_ref.err32 of the same batch (extra: times the largest absolute row sum of the regressor, which is what an error of the
vertices can grow by in extra = regressor @ verts).  Gradients: per tensor, the max over sample rows of |g - g64|_2 / |g64|_2
<= 4 x the same figure of body_grad_ref's own fp32 run of the same batch.  The one-vertex case takes both bars from a V = 65
model of the same (J, nb): the maximum over one point is a noisy bar.  The loss is L = sum c_v verts + sum c_j joints
(+ sum c_x extra) with seeded standard-normal coefficients.  Every reference is computed once and shared."""
import functools

import numpy as np
import pytest
import torch

import body_cap_cases as cc
import body_grad_ref
import body_ref
from pose2mesh_release_amd import body

pytestmark = pytest.mark.gpu
OUTS = ("verts", "joints", "extra")
GRADS = ("pose", "betas", "trans")


def _model(name, center_idx=None, regressor=True):
    c, m = cc.CASES[name], cc.case_model(name)
    return body.BodyModel(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["weights"], m["parents"],
                          betas=m["betas"], tip_vertices=m.get("tip_vertices"), joint_order=m.get("joint_order"),
                          center_idx=center_idx, extra_regressor=c["extra"] if regressor else None)


def _cuda(x, grad=False):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda().requires_grad_(grad)


def _np(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def _forward(model, pose, betas, trans):
    out = model(_cuda(pose), _cuda(betas), _cuda(trans))
    torch.cuda.synchronize()
    return [_np(o) for o in out]


def _grads(layer, pose, betas, trans, coeffs, use=None):
    """Outputs and gradients (numpy; None where the input is None) of L = sum_o (c_o out_o), o in `use`."""
    ins = [_cuda(x, True) for x in (pose, betas, trans)]
    out = layer(*ins)
    use = range(len(out)) if use is None else use
    sum((_cuda(coeffs[o]) * out[o]).sum() for o in use).backward()
    torch.cuda.synchronize()
    return [_np(o) for o in out], [None if x is None else _np(x.grad) for x in ins]


def _coeffs(name, Bn, V):
    c = cc.CASES[name]
    shapes = [(Bn, V, 3), (Bn, cc.n_joints_out(name), 3)] + ([(Bn, c["extra"].shape[0], 3)] if c["extra"] is not None else [])
    return body_grad_ref.loss_coeffs(c["seed"], shapes)[0]


def _frozen(arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _reference(name, label):
    """Float64 outputs and gradients of a run and its bars, computed once."""
    r = cc.run(name, label)
    m, reg = r["model"], r["extra_reg"]
    args = (r["pose"], r["betas"], r["trans"], r["center_idx"])
    Bn = r["pose"].shape[0]
    coeffs = _coeffs(name, Bn, m["num_vertex"])
    want = body_ref.forward(m, *args, reg)
    g8 = body_grad_ref.grads(m, *args, reg, None, coeffs)
    if name in cc.COMPANION:                                 # bars of the V = 65 model of the same (J, nb), no regressor
        k = cc.run(name, label, companion=True)
        km, kargs = k["model"], (k["pose"], k["betas"], k["trans"], k["center_idx"])
        kco = body_grad_ref.loss_coeffs(cc.CASES[name]["seed"], [(Bn, km["num_vertex"], 3), (Bn, cc.n_joints_out(name), 3)])[0]
        err32 = body_ref.err32(km, *kargs)
        b8 = body_grad_ref.grads(km, *kargs, None, None, kco)
        b4 = body_grad_ref.grads(km, *kargs, None, None, kco, dtype=torch.float32)
    else:
        err32 = body_ref.err32(m, *args)
        b8, b4 = g8, body_grad_ref.grads(m, *args, reg, None, coeffs, dtype=torch.float32)
    gbar = {n: 4 * body_grad_ref.row_err(a, b) for n, a, b in zip(GRADS, b4, b8) if b is not None and b.shape[1] > 0}
    fbar = {"verts": 4 * err32, "joints": 4 * err32}
    if reg is not None:
        fbar["extra"] = 4 * err32 * cc.row_sum_bound(reg)
    return {"run": r, "coeffs": _frozen(list(coeffs)), "want": _frozen(list(want)), "g8": _frozen(list(g8)), "fbar": fbar,
            "gbar": gbar, "pose_scale": cc.vanishing_pose_gradient_scale(name, g8)}


def _ratio(e, bar):
    return 0.0 if e == 0 else e / bar if bar > 0 else float("inf")


def _check_forward(got, ref, what):
    assert len(got) == len(ref["want"])
    for n, g, w in zip(OUTS, got, ref["want"]):
        assert g.shape == w.shape, (what, n)
        e, bar = body_ref.max_l2(g, w), ref["fbar"][n]
        print(f"{what} {n}: max L2 {e:.3e}  bar {bar:.3e}  ratio {_ratio(e, bar):.3f}")
        assert np.isfinite(g).all() and e <= bar, (what, n, e, bar)


def _check_grads(got, ref, what):
    for n, g, w in zip(GRADS, got, ref["g8"]):
        assert (g is None) == (w is None) and (w is None or g.shape == w.shape), (what, n)
        if w is None:
            continue
        assert np.isfinite(g).all(), (what, n)
        if w.shape[1] == 0:                                  # nb = 0: the gradient of [B, 0] betas is [B, 0]
            continue
        bar = ref["gbar"][n]
        if n == "pose" and ref["pose_scale"] is not None:    # a gradient that vanishes identically: against what cancels in it
            e = float((np.linalg.norm((g - w).reshape(g.shape[0], -1), axis=1) / ref["pose_scale"]).max())
        else:
            e = body_grad_ref.row_err(g, w)
        print(f"{what} g_{n}: max row error {e:.3e}  bar {bar:.3e}  ratio {_ratio(e, bar):.3f}")
        assert e <= bar, (what, n, e, bar)


# ---- 1. every case against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,label", cc.run_ids())
def test_case(hip_libs, name, label):
    """BodyModel's forward, BodyLayer's forward (bitwise the same) and backward."""
    ref = _reference(name, label)
    r = ref["run"]
    what = f"{name} {label}".strip()
    model = _model(name, r["center_idx"])
    plain = _forward(model, r["pose"], r["betas"], r["trans"])
    _check_forward(plain, ref, what)
    out, got = _grads(body.BodyLayer(model), r["pose"], r["betas"], r["trans"], ref["coeffs"])
    assert len(out) == len(plain) and all(np.array_equal(o, p) for o, p in zip(out, plain)), what
    _check_grads(got, ref, what)


# ---- 2. batch independence at the caps -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cap_both", "cap_outputs", "fold_1025"])
def test_batch_independence(hip_libs, name):
    """Samples 0, 7 and 8 of the B = 9 call (the ends of the first sample tile and the one sample of the second) are bitwise
    the same samples run alone, in every output and gradient."""
    ref = _reference(name, "")
    r, coeffs = ref["run"], ref["coeffs"]
    layer = body.BodyLayer(_model(name, r["center_idx"]))
    out, full = _grads(layer, r["pose"], r["betas"], r["trans"], coeffs)
    assert r["pose"].shape[0] == 9
    for i in (0, 7, 8):
        o1, g1 = _grads(layer, r["pose"][i:i + 1], r["betas"][i:i + 1], r["trans"][i:i + 1], [c[i:i + 1] for c in coeffs])
        for n, a, b in zip(OUTS, o1, out):
            assert np.array_equal(a[0], b[i]), (name, i, n)
        for n, a, b in zip(GRADS, g1, full):
            assert np.array_equal(a[0], b[i]), (name, i, n)


# ---- 3. a loss on the joints alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,label", [("tips_only", ""), ("drop_joints", "c3")])
def test_joints_only_loss(hip_libs, name, label):
    """With no chain joint among the outputs (tips_only) the loss still reaches the parameters through the tip vertices; with
    three of 24 kept, through both.  The gradients are non-zero and bitwise those of the full loss with explicit zero
    coefficients for the vertices."""
    ref = _reference(name, label)
    r, coeffs = ref["run"], ref["coeffs"]
    layer = body.BodyLayer(_model(name, r["center_idx"]))
    _, got = _grads(layer, r["pose"], r["betas"], r["trans"], coeffs, use=[1])
    _, want = _grads(layer, r["pose"], r["betas"], r["trans"], [np.zeros_like(coeffs[0]), coeffs[1]])
    for n, g, w in zip(GRADS, got, want):
        assert (g is None) == (w is None), n
        if g is not None:
            assert np.isfinite(g).all() and (np.abs(g).reshape(g.shape[0], -1).max(axis=1) > 0).all() and np.array_equal(g, w), n


# ---- 4. the all-zero regressor -------------------------------------------------------------------------------------------------
def test_zero_regressor(hip_libs):
    ref = _reference("reg_zero", "")
    r, coeffs = ref["run"], ref["coeffs"]
    layer = body.BodyLayer(_model("reg_zero"))
    out, full = _grads(layer, r["pose"], r["betas"], r["trans"], coeffs)
    assert out[2].shape == (9, 5, 3) and not out[2].any()                   # exactly zero
    _, only = _grads(layer, r["pose"], r["betas"], r["trans"], coeffs, use=[2])
    for n, g in zip(GRADS, only):
        assert np.isfinite(g).all() and not g.any(), n                      # an extra-only loss: exactly zero gradients
    bare = body.BodyLayer(_model("reg_zero", regressor=False))
    out2, want = _grads(bare, r["pose"], r["betas"], r["trans"], coeffs[:2])
    assert len(out2) == 2 and all(np.array_equal(a, b) for a, b in zip(out2, out[:2]))
    for n, g, w in zip(GRADS, full, want):
        assert np.array_equal(g, w), n                                      # the zero regressor adds nothing, bit for bit


# ---- 5. no shape space ---------------------------------------------------------------------------------------------------------
def test_nb0_gradients_flow(hip_libs):
    """nb = 0: [B, 0] betas and betas=None give the same outputs and the same pose / trans gradients, bitwise; the gradient of
    the [B, 0] betas is an empty [B, 0] tensor, also when nothing else needs one."""
    given, stored = _reference("nb0", "given")["run"], _reference("nb0", "stored")["run"]
    coeffs = _reference("nb0", "given")["coeffs"]
    assert given["betas"].shape == (9, 0) and stored["betas"] is None
    layer = body.BodyLayer(_model("nb0"))
    o1, g1 = _grads(layer, given["pose"], given["betas"], given["trans"], coeffs)
    o2, g2 = _grads(layer, stored["pose"], None, stored["trans"], coeffs)
    assert all(np.array_equal(a, b) for a, b in zip(o1, o2))
    assert g1[1].shape == (9, 0) and g2[1] is None
    for i in (0, 2):
        assert np.array_equal(g1[i], g2[i]) and (np.abs(g1[i]).max(axis=1) > 0).all()
    betas = _cuda(given["betas"], True)
    verts = layer(_cuda(given["pose"]), betas, _cuda(given["trans"]))[0]
    verts.sum().backward()
    assert betas.grad is not None and tuple(betas.grad.shape) == (9, 0)
