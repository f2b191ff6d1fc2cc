"""CPU: tests/body_ref.py (the float64 restatement of SMPL_Layer.forward / ManoLayer.forward) reproduces the fixtures the
real layers produced, the synthetic models regenerate, and the host side of pose2mesh_release_amd.body validates."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import body_cases
import body_ref
from pose2mesh_release_amd import body, synth
from pose2mesh_release_amd._lib import P2MError


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("flavour,name", body_cases.case_ids())
def test_body_ref_reproduces_fixture(flavour, name):
    c = body_cases.case(flavour, name)
    out = body_ref.forward(c["model"], c["pose"], c["betas"], c["trans"], c["center_idx"], c["extra_reg"])
    assert _rel(out[0], c["verts"]) <= 1e-12 and _rel(out[1], c["joints"]) <= 1e-12
    if c["extra_reg"] is not None:
        assert _rel(out[2], c["extra"]) <= 1e-12
    # the stored error is fp32-class: up to 24 chained transforms of a few roundings (6e-8 relative) each
    assert 0 < c["err32"] < 24 * 4 * 6e-8 * max(1.0, np.abs(c["verts"]).max())


def test_fixture_covers_the_issue_cases():
    ids = body_cases.case_ids()
    cs = [body_cases.case(f, n) for f, n in ids]
    assert {c["pose"].shape[0] for c in cs} == {1, 5, 37}
    assert {c["model"]["kind"] for c in cs} == {"smpl", "chain", "star", "mano"}
    for flavour in ("smpl", "mano"):
        fc = [c for (f, _), c in zip(ids, cs) if f == flavour]
        assert {c["trans"] is None for c in fc} == {True, False} and {c["center_idx"] for c in fc} == {None, 0}
        assert any(c["betas"] is None for c in fc) and any(c["extra_reg"] is not None for c in fc)
        assert any((c["pose"] == 0).all(axis=1).any() for c in fc)                                # an all-zero pose
        assert any(np.linalg.norm(c["pose"].reshape(-1, 3), axis=1).max() > np.pi for c in fc)   # beyond pi
        assert any(c["betas"] is not None and np.abs(c["betas"]).max() > 3 for c in fc)
    assert all(os.path.getsize(os.path.join(body_cases.GOLDEN, f)) < 1 << 20 for f in body_cases.FILES.values())


def test_synthetic_model_properties():
    for kind in synth.BODY_KINDS:
        m = synth.body_model(kind, 300, seed=3)
        J = len(m["parents"])
        assert J == (16 if kind == "mano" else 24) and m["posedirs"].shape == (300, 3, 9 * (J - 1))
        assert all(0 <= m["parents"][j] < j for j in range(1, J))
        assert ((m["J_regressor"] != 0).sum(1) == 12).all() and np.allclose(m["J_regressor"].sum(1), 1, atol=1e-6)
        assert ((m["weights"] != 0).sum(1) == 4).all() and np.allclose(m["weights"].sum(1), 1, atol=1e-6)
        assert m["checksum"] == synth.body_model(kind, 300, seed=3)["checksum"] != synth.body_model(kind, 300, seed=4)["checksum"]
    depth = lambda p: max(len(_chain(p, j)) for j in range(len(p)))         # noqa: E731
    assert depth(synth.body_model("chain", 30)["parents"]) == 24 and depth(synth.body_model("star", 30)["parents"]) == 2
    assert list(synth.body_model("mano", 30)["parents"]) == list(synth.MANO_PARENTS)
    with pytest.raises(ValueError):
        synth.body_model("hand")


def _chain(p, j):
    out = [j]
    while out[-1] > 0:
        out.append(p[out[-1]])
    return out


def test_zero_pose_is_the_rest_shape():
    """batch_rodrigues' + 1e-8 still gives the identity for a zero pose: verts = template + shapedirs beta, up to the sum
    of a vertex's four fp32-rounded skinning weights, which is 1 only to 4 x 2^-24 (the reference's own behaviour)."""
    m = body_cases.model("smpl", 257)
    beta = np.random.default_rng(0).standard_normal((2, 10))
    v, j = body_ref.forward(m, np.zeros((2, 72)), beta)
    want = m["v_template"].astype(np.float64) + np.einsum("vcn,bn->bvc", m["shapedirs"].astype(np.float64), beta)
    assert np.abs(v - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max()
    assert np.abs(j[1] - body_ref.rest_joints(m, beta[1])).max() <= 1e-14
    assert (body_ref.rodrigues(np.zeros((1, 3)))[0] == np.eye(3)).all()


def _args(m, **kw):
    a = dict(v_template=m["v_template"], shapedirs=m["shapedirs"], posedirs=m["posedirs"], J_regressor=m["J_regressor"],
             weights=m["weights"], parents=m["parents"])
    for k in ("betas", "hands_mean", "tip_vertices", "joint_order", "scale"):
        if k in m:
            a[k] = m[k]
    a.update(kw)
    return a


def test_host_validation():
    m = body_cases.model("smpl", 257)
    bad = list(m["parents"])
    bad[5] = 7
    with pytest.raises(ValueError, match="parents"):
        body.BodyModel(**_args(m, parents=bad))
    with pytest.raises(ValueError, match="parents"):
        body.BodyModel(**_args(m, parents=m["parents"][:-1]))
    with pytest.raises(ValueError, match="posedirs"):
        body.BodyModel(**_args(m, posedirs=m["posedirs"][:, :, :-1]))
    with pytest.raises(ValueError, match="weights"):
        body.BodyModel(**_args(m, weights=m["weights"][:-1]))
    with pytest.raises(ValueError, match="extra_regressor"):
        body.BodyModel(**_args(m, extra_regressor=np.zeros((65, 257), np.float32)))
    with pytest.raises(ValueError, match="tip_vertices"):
        body.BodyModel(**_args(m, tip_vertices=[257]))
    with pytest.raises(ValueError, match="center_idx"):
        body.BodyModel(**_args(m, center_idx=24))
    hand = body_cases.model("mano", 778)
    with pytest.raises(ValueError, match="tip"):
        body.BodyModel(**_args(hand, center_idx=4))          # output joint 4 is the thumb tip vertex
    model = body.BodyModel(**_args(m))
    assert (model.J, model.NJ, model.nb, model.V) == (24, 24, 10, 257)
    assert body.BodyModel(**_args(hand)).NJ == 21


def test_cpu_tensors_and_unsupported_modes_raise(hip_libs):
    m = body_cases.model("mano", 778)
    model = body.BodyModel(**_args(m))
    with pytest.raises(P2MError):
        model(torch.zeros(2, 48))
    with pytest.raises(P2MError):
        model(np.zeros((2, 48), np.float32))
    stub = _stub_layer(m)
    for attr, val in (("use_pca", True), ("joint_rot_mode", "rotmat"), ("root_rot_mode", "rot6d")):
        s = _stub_layer(m)
        setattr(s, attr, val)
        with pytest.raises(ValueError):
            body.BodyModel.from_layer(s)
    got = body.BodyModel.from_layer(stub)
    assert got.scale == 1000.0 and got.NJ == 21 and got.n_tips == 5
    for k, v in model._host.items():
        assert np.array_equal(v, got._host[k]), k
    from pose2mesh_release_amd import _lib
    assert _lib.hip().p2m_body_sample_tile() == body.SAMPLE_TILE and _lib.hip().p2m_body_vertex_tile() == body.VERTEX_TILE
    assert _lib.hip().p2m_body_workspace(3, 24, 10) == 3 * (220 + 288 + 4) * 4 and _lib.hip().p2m_body_workspace(1, 65, 10) < 0


def _stub_layer(m):
    """An object with the buffers and attributes of a constructed reference layer."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))             # noqa: E731
    s = types.SimpleNamespace(th_betas=t(m["betas"])[None], th_shapedirs=t(m["shapedirs"]), th_posedirs=t(m["posedirs"]),
                              th_v_template=t(m["v_template"])[None], th_J_regressor=t(m["J_regressor"]),
                              th_weights=t(m["weights"]), kintree_parents=[4294967295] + list(m["parents"][1:]),
                              center_idx=None)
    if "hands_mean" in m:
        s.th_hands_mean = t(m["hands_mean"])[None]
        s.use_pca, s.joint_rot_mode, s.root_rot_mode, s.side = False, "axisang", "axisang", "right"
    return s


def test_c_entry_rejects_bad_arguments(hip_libs):
    """No GPU needed: the checks run before any launch.  Null pointers, V / J / B < 1, J > 64, misaligned buffers."""
    import ctypes
    from pose2mesh_release_amd import _lib
    lib = _lib.hip()
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ok = dict(pose=base, pose_mean=None, betas=base, per=1, trans=None, center=-1, scale=1.0, B=1, V=1, J=2, nb=1,
              tmpl=base, dirs=base, wt=base, jt=base, js=base, parents=base, jslot=base, NJ=2, tv=None, ts=None, nt=0,
              xp=None, xi=None, xv=None, nx=0, ws=base, wsb=1 << 20, verts=base, joints=base, extra=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.p2m_body_forward(*[a[k] for k in ok])
    for kw, word in ((dict(pose=None), "null"), (dict(verts=None), "null"), (dict(ws=None), "null"), (dict(B=0), ">= 1"),
                     (dict(V=0), ">= 1"), (dict(J=0), ">= 1"), (dict(J=65), "64"), (dict(pose=base + 2), "misaligned"),
                     (dict(ws=base + 4), "misaligned"), (dict(wsb=8), "workspace"), (dict(center=2), "center_joint"),
                     (dict(nx=1), "extra"), (dict(nt=1), "tips")):
        assert call(**kw) != 0, kw
        assert word in lib.p2m_last_error_string().decode(), (kw, lib.p2m_last_error_string())


def test_dirs_repacking_round_trips():
    m = body_cases.model("smpl", 65)
    d = body.repack_dirs(m["shapedirs"], m["posedirs"])
    assert d.shape == (217, 195) and d.dtype == np.float32 and d.flags.c_contiguous
    assert d[3, 7 * 3 + 2] == m["shapedirs"][7, 2, 3] and d[10 + 100, 64 * 3 + 1] == m["posedirs"][64, 1, 100]
    sd, pd = body.unpack_dirs(d, 10)
    assert np.array_equal(sd, m["shapedirs"]) and np.array_equal(pd, m["posedirs"])


@pytest.mark.reference
@pytest.mark.parametrize("kind", ["smpl", "mano"])
def test_body_ref_matches_live_layers(kind):
    """body_ref against the real layers' forward at full size (V = 6890 / 778, B = 2), float64."""
    sys.path.insert(0, body_cases.GOLDEN)
    import make_golden_body as g
    if not os.path.isdir(g.REF_ROOT):
        pytest.skip("reference tree not present")
    m = synth.body_model(kind, 6890 if kind == "smpl" else 778, seed=9)
    pose, betas, trans = g.inputs(np.random.default_rng(4), 2, len(m["parents"]), 10)
    for tr, center in ((None, 0), (trans, None)):
        v, j = g.run_reference(m, pose, betas, tr, center, torch.float64)
        rv, rj = body_ref.forward(m, pose, betas, tr, center)
        assert _rel(rv, v) <= 1e-12 and _rel(rj, j) <= 1e-12
