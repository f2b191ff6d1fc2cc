"""CPU: the float64 yardstick of the annotation layer (tests/annot_ref.py) against scipy's rotation logarithm and against a
line-by-line transcription of the reference's Human3.6M get_smpl_coord; the host-side validation of
pose2mesh_release_amd.annot; the seeded cases hold what they promise."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import annot_cases
import annot_ref
import body_ref
from pose2mesh_release_amd import annot


def test_logarithm_agrees_with_scipy():
    """log(R . exp(root)) of annot_ref against Rotation.from_matrix(R @ exp).as_rotvec() to 1e-12 on every root of the cases
    but the exactly-pi one.  R is an exact float64 rotation here: scipy orthonormalises what it is given, the kernel's
    contract takes an fp32-rounded R as it is, and the two would differ by that rounding (1e-8)."""
    rng = np.random.default_rng(5)
    n, worst = 0, 0.0
    for i, c in enumerate(annot_cases.CASES):
        t = annot_cases.case(i)["tables"]
        R = annot_cases.random_rotations(rng, len(t["pose"]))
        for r in range(min(len(t["pose"]), 40)):
            root = t["pose"][r, :3].astype(np.float64)
            if r == annot_cases.PI_ROW and len(t["pose"]) >= annot_cases.N_SPECIAL:
                continue
            if r == 2 and len(t["pose"]) >= annot_cases.N_SPECIAL and t["cam_R"] is not None:
                # the near-pi product: rebuild it for this exact R
                ax = rng.standard_normal(3)
                root = annot_ref.log_rot(R[r].T @ annot_ref.exp_root(ax / np.linalg.norm(ax) * (np.pi - 5e-5)))
            M = R[r] @ annot_ref.exp_root(root)
            got, want = annot_ref.log_rot(M), Rotation.from_matrix(M).as_rotvec()
            assert np.linalg.norm(got) <= np.pi + 1e-12
            worst = max(worst, float(np.abs(got - want).max()))
            n += 1
    print(f"log vs scipy: {n} roots, max |diff| {worst:.3e}")
    assert n > 300 and worst <= 1e-12
    assert np.array_equal(annot_ref.log_rot(np.eye(3)), np.zeros(3))
    assert np.array_equal(annot_ref.exp_root(np.zeros(3)), np.eye(3))
    # beyond pi: the principal value is the other way round
    v = np.array([0.0, 3.7, 0.0])
    assert np.allclose(annot_ref.log_rot(annot_ref.exp_root(v)), [0.0, 3.7 - 2 * np.pi, 0.0], atol=1e-14)


def _h36m_transcription(m, pose, shape, trans, R, t):
    """data/Human36M/dataset.py:264-294 line by line in float64, the layer replaced by body_ref.forward (metres; the final
    x 1000 left out).  transforms3d's mat2axangle is replaced by scipy's rotvec: the same vector below pi."""
    f8 = np.float64
    theta = np.asarray(pose, f8).reshape(-1, 3).copy()
    beta = np.asarray(shape, f8).reshape(1, -1).copy()
    world_t, R, cam_t = np.asarray(trans, f8).reshape(3), np.asarray(R, f8).reshape(3, 3), np.asarray(t, f8).reshape(3)
    if (np.abs(beta) > 3).any():                                          # :264  far from the mean shape: the mean shape
        beta[:] = 0.0
    angle = np.linalg.norm(theta[0])                                      # :267-268
    E = Rotation.from_rotvec(theta[0] / angle * angle).as_matrix()        # :269  axis = root / angle, then axis-angle -> matrix
    M = R @ E                                                             # :270
    theta[0] = Rotation.from_matrix(M).as_rotvec()                        # :271-273  axis * angle of the product
    verts, joints = body_ref.forward(m, theta.reshape(1, -1), beta)       # :275-278  no translation: the layer's own frame
    verts, joints = verts[0], joints[0]                                   # :281-282
    shift = R @ world_t + cam_t / 1000                                    # :287-289
    root = joints[0]                                                      # :290
    shift = shift - root + R @ root                                       # :291  the rotation was about the origin, not the root
    return verts + shift, joints + shift                                  # :294


def test_human36m_preset_reproduces_the_dataset_code():
    """Verts of body_ref.forward on annot_ref's Human3.6M parameters against the transcription, to 1e-6 m.  The gap is the
    fp32 rounding of the parameters plus the folded-J0 difference (the root tables are fp32), printed on its own."""
    i = annot_cases.CASES.index(("human36m", "smpl", 1000, 37, 3))
    c = annot_cases.case(i)
    assert c["flags"] == dict(rotate_root=True, beta_reset=True, compensate_root=True, t_scale=1e-3)
    models = annot_cases.model_dicts("smpl", 31, 3)
    rt, rs = annot_ref.root_tables(models)
    assert np.allclose(rt, c["root_template"], rtol=0, atol=1e-7) and np.allclose(rs, c["root_shapedirs"], rtol=0, atol=1e-8)
    o = annot_cases.reference(c)
    t = c["tables"]
    worst = worst_j0 = 0.0
    n = 0
    for b, r in enumerate(c["idx"]):
        if r in (0, annot_cases.PI_ROW) or o["status"][b] & annot_ref.BAD_GENDER:
            continue                       # the reference's 0 / 0; the undefined axis sign; a gender the reference cannot index
        m = models[o["gender"][b]]
        want_v, want_j = _h36m_transcription(m, t["pose"][r], t["betas"][r], t["trans"][r], t["cam_R"][r], t["cam_t"][r])
        got_v, got_j = body_ref.forward(m, o["pose"][b:b + 1], o["betas"][b:b + 1], o["trans"][b:b + 1])
        worst = max(worst, body_ref.max_l2(got_v[0], want_v), body_ref.max_l2(got_j[0], want_j))
        J0 = body_ref.rest_joints(m, o["betas"][b])[0]
        J0_folded = c["root_template"][o["gender"][b]].astype(np.float64) + c["root_shapedirs"][o["gender"][b]].astype(np.float64) @ o["betas"][b]
        worst_j0 = max(worst_j0, float(np.abs(J0 - J0_folded).max()))
        n += 1
    print(f"human36m preset vs transcription: {n} samples, max vertex / joint L2 {worst:.3e} m; folded J0 vs the float64 rest "
          f"root {worst_j0:.3e} m")
    assert n >= 30 and worst <= 1e-6
    assert (o["status"] & annot_ref.BETA_RESET).any() and not (o["status"][5] & annot_ref.BETA_RESET)
    assert o["status"][6] & annot_ref.BETA_RESET and not o["betas"][6].any() and o["betas"][5, 3] == 3.0


def test_cases_hold_what_they_promise():
    seen = set()
    for i, (preset, kind, N, B, G) in enumerate(annot_cases.CASES):
        c = annot_cases.case(i)
        seen.add(preset)
        idx, t = c["idx"], c["tables"]
        assert len(idx) == B and idx.min() >= 0 and idx.max() < N
        if B == 37 and N == 1000:
            assert set(range(annot_cases.N_SPECIAL)) <= set(idx.tolist()) and N - 1 in idx and len(set(idx.tolist())) < B
            assert not t["pose"][0, :3].any() and np.linalg.norm(t["pose"][1, :3]) > np.pi
            assert abs(np.linalg.norm(t["pose"][4, :3]) - 1e-7) < 1e-9
            assert t["betas"][5, 3] == 3.0 and abs(t["betas"][6]).max() > 3.0 and abs(t["betas"][6]).max() < 3.000001
    assert seen == set(annot.PRESETS) and len(annot.PRESETS) == 7
    assert {c[2] for c in annot_cases.CASES} == {1, 1000} and {c[3] for c in annot_cases.CASES} == {1, 5, 37}
    assert {c[4] for c in annot_cases.CASES} == {1, 3} and {c[1] for c in annot_cases.CASES} == {"smpl", "mano"}


def test_reference_defined_behaviour():
    """Out-of-range indices, a gender of G and non-finite roots in the yardstick itself."""
    c = annot_cases.case(0)
    o = annot_cases.reference(c, np.asarray([-1, 3, c["N"], 7]))
    assert o["status"][0] == o["status"][2] == annot_ref.BAD_INDEX
    for k in ("pose", "betas", "trans", "focal", "princpt", "given_cam", "given_img", "gender"):
        assert not o[k][0].any() and not o[k][2].any(), k
    assert o["status"][3] & annot_ref.BAD_GENDER and o["gender"][3] == 0
    srcs = [np.full((4, 2, 3), g, np.float32) for g in range(3)]
    assert annot_ref.select(srcs, [2, 0, 3, -1])[:, 0, 0].tolist() == [2.0, 0.0, 0.0, 0.0]
    assert annot_ref.ulp_diff(np.float32([1.0, -0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0])).tolist() == [1, 0]


def test_presets():
    p = annot.PRESETS
    assert p["human36m"] == dict(rotate_root=True, beta_reset=True, compensate_root=True, t_scale=1e-3)
    for k in ("amass", "freihand"):
        assert p[k] == dict(rotate_root=True, beta_reset=False, compensate_root=False, t_scale=1.0)
    for k in ("pw3d", "surreal"):
        assert p[k] == dict(rotate_root=False, beta_reset=False, compensate_root=False, t_scale=1.0)
    for k in ("muco", "coco"):
        assert p[k] == dict(rotate_root=False, beta_reset=True, compensate_root=False, t_scale=1.0)


def test_host_side_validation_raises():
    """Everything below is decided on the host, before any device memory is touched."""
    N = 6
    z = lambda *sh: np.zeros(sh, np.float32)  # noqa: E731
    ok = dict(pose=z(N, 72), betas=z(N, 10), focal=z(N, 2), princpt=z(N, 2))
    with pytest.raises(ValueError, match="preset"):
        annot.AnnotationSource(**ok, preset="h36m")
    for bad in (dict(pose=z(N, 71)), dict(betas=z(N + 1, 10)), dict(focal=z(N, 3)), dict(princpt=z(N - 1, 2)),
                dict(trans=z(N, 2)), dict(cam_R=z(N, 3, 2)), dict(cam_t=z(N, 4)), dict(gender=np.zeros(N + 1, np.uint8)),
                dict(given_cam=z(N, 17, 2)), dict(given_cam=z(N, 17, 3), given_img=z(N, 16, 2)), dict(given_cam=z(N, 33, 3))):
        with pytest.raises(ValueError):
            annot.AnnotationSource(**{**ok, **bad})
    with pytest.raises(ValueError, match="focal"):
        annot.AnnotationSource(z(N, 72), z(N, 10))
    with pytest.raises(ValueError, match="compensate_root"):
        annot.AnnotationSource(**ok, preset="human36m")
    bank = annot_cases.bank("smpl", 31, 3)
    with pytest.raises(ValueError, match="root_shapedirs"):
        annot.AnnotationSource(**{**ok, "betas": z(N, 8)}, models=bank, preset="human36m")
    with pytest.raises(ValueError, match="joints"):
        annot.AnnotationSource(**{**ok, "pose": z(N, 48)}, models=bank)
    a, b = (annot_cases.body_model(m) for m in (annot_cases.model_dicts("smpl", 31, 1)[0], annot_cases.model_dicts("smpl", 300, 1)[0]))
    with pytest.raises(ValueError, match="unequal V"):
        annot.GenderedBody([a, b])
    with pytest.raises(ValueError):
        annot.GenderedBody([])
    with pytest.raises(ValueError):
        annot.GenderedBody([a] * 5)
    with pytest.raises(TypeError):
        annot.GenderedBody([a, "female"])
    named = annot.GenderedBody({"male": a, "female": a})
    assert named.names == ["male", "female"] and named.G == 2
    rt, rs = named.root_tables()
    assert rt.shape == (2, 3) and rs.shape == (2, 3, 10) and rt.dtype == rs.dtype == np.float32
