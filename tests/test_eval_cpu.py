"""CPU: the float64 restatement of the evaluation loop bodies (tests/eval_ref.py) against the eval_* fixtures that
tests/golden/make_golden_eval.py produced with the real reference's rigid_transform_3D / rigid_align, against the live
reference where its tree is present, and the host-side checks of pose2mesh_release_amd.evaluate."""
import numpy as np
import pytest

import eval_ref
import helpers

H36M_EVAL_JOINT = (1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15, 16)


def _align_cases():
    z = helpers.golden("eval_align.npz")
    return z, [str(c) for c in z["cases"]]


def fixture_regressor(z):
    R = np.zeros(tuple(int(v) for v in z["reg_shape"]), dtype=np.float32)
    R[z["reg_rows"], z["reg_cols"]] = z["reg_vals"]
    return R


def test_fixtures_cover_the_issue_cases():
    z, cases = _align_cases()
    sizes = {z[f"{c}_A"].shape[1] for c in cases}
    assert {3, 14, 17, 21, 778} <= sizes
    assert any(c.startswith("mirror") for c in cases) and any(c.startswith("planar") for c in cases)
    for c in cases:
        assert z[f"{c}_A"].dtype == np.float32 and z[f"{c}_B"].dtype == np.float32
        assert z[f"{c}_R"].dtype == np.float64 and z[f"{c}_A2"].dtype == np.float64
    # the mirrored cases do take the reference's det < 0 branch: c uses s1 + s2 - s3 and R stays proper
    for c in cases:
        assert np.allclose(np.linalg.det(z[f"{c}_R"]), 1.0, atol=1e-9)
    m = z["mirror14_A"].astype(np.float64), z["mirror14_B"].astype(np.float64)
    H = [(a - a.mean(0)).T @ (b - b.mean(0)) for a, b in zip(*m)]
    assert all(np.linalg.det(h) < 0 for h in H)
    for name in ("eval_mesh_smpl.npz", "eval_mesh_mano.npz"):
        mz = helpers.golden(name)
        assert mz["pred"].dtype == np.float32 and mz["gt"].dtype == np.float32
    assert fixture_regressor(helpers.golden("eval_mesh_smpl.npz")).shape == (17, 6890)
    assert np.array_equal(fixture_regressor(helpers.golden("eval_mesh_smpl.npz")), helpers.golden_regressor("demo_h36m.npz"))


def test_eval_ref_reproduces_the_alignment_fixtures():
    z, cases = _align_cases()
    for c in cases:
        A, B = z[f"{c}_A"], z[f"{c}_B"]
        sc = float(np.abs(B).max())
        cc, R, t, A2 = eval_ref.batch_rigid(A, B)
        assert np.abs(R - z[f"{c}_R"]).max() <= 1e-10, c
        assert (np.abs(cc - z[f"{c}_c"]) / np.abs(z[f"{c}_c"])).max() <= 1e-10, c
        assert np.abs(t - z[f"{c}_t"]).max() <= 1e-10 * sc, c
        assert np.abs(A2 - z[f"{c}_A2"]).max() <= 1e-10 * sc, c
        for i in range(A.shape[0]):                                   # the single-set functions agree with the batch
            assert np.abs(eval_ref.rigid_align(A[i], B[i]) - A2[i]).max() <= 1e-12 * sc


@pytest.mark.parametrize("name,sub", [("eval_mesh_smpl.npz", H36M_EVAL_JOINT), ("eval_mesh_mano.npz", None)])
def test_eval_ref_reproduces_the_mesh_fixtures(name, sub):
    z = helpers.golden(name)
    reg = fixture_regressor(z)
    assert list(z["sub"]) == list(sub if sub is not None else range(reg.shape[0]))
    out = eval_ref.mesh_eval(z["pred"], z["gt"], reg, int(z["root"]), list(z["sub"]), reg, int(z["root"]), list(z["sub"]),
                             pa_mesh=True, gt_scale=float(z["gt_scale"]))
    sc = float(np.abs(z["gt"]).max()) * float(z["gt_scale"])
    for k in eval_ref.EVAL_KEYS:
        assert out[k].shape == z[k].shape, k
        assert np.abs(out[k] - z[k]).max() <= 1e-10 * sc, k
    # plausible magnitudes (mm): the prediction is a perturbed similarity of the truth
    assert 1.0 < out["mpvpe"].min() and out["pa_mpvpe"].max() < out["mpvpe"].min()
    assert (out["pa_mpjpe_E"].mean(1) <= out["mpjpe_E"].mean(1) + 1e-9).all()


def test_eval_ref_degenerate_and_exact_cases():
    rng = np.random.default_rng(4)
    A = rng.standard_normal((17, 3)) * 300
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    Q *= np.sign(np.linalg.det(Q))
    B = 1.3 * A @ Q.T + np.array([10.0, -400.0, 2000.0])
    c, R, t = eval_ref.rigid_transform_3D(A, B)
    assert abs(c - 1.3) < 1e-12 and np.abs(R - Q).max() < 1e-12
    assert np.abs(eval_ref.rigid_align(A, B) - B).max() < 1e-9
    same = np.tile(A[:1].astype(np.float32), (17, 1)).astype(np.float64)   # all points coincide (fp32 values, as the
    # kernels see them: their mean is exact, so varP = 0 exactly) -> non-finite
    assert not np.isfinite(eval_ref.rigid_align(same, B)).any()


def test_summary_groups():
    per = {"mpjpe_A": np.array([[1.0, 3.0], [5.0, 7.0], [2.0, 2.0]]), "mpvpe": np.array([1.0, 2.0, 3.0])}
    s = eval_ref.summary(per, group=[0, 1, 0])
    assert s["samples"] == 3 and s["mpjpe_A"] == 20.0 / 6 and s["mpvpe"] == 2.0
    assert s["groups"][0] == {"mpjpe_A": 2.0, "mpvpe": 2.0, "samples": 2}
    assert s["groups"][1]["mpjpe_A"] == 6.0


_LIVE = """
import sys, numpy as np
sys.path[:0] = [sys.argv[2]]
import ref_loader
cu = ref_loader.load_aug().coord_utils
z = dict(np.load(sys.argv[1]))
for k in [k for k in z if k.endswith("_A")]:
    c, R, t = cu.rigid_transform_3D(z[k], z[k[:-2] + "_B"])
    z[k[:-2] + "_c"], z[k[:-2] + "_R"], z[k[:-2] + "_t"] = np.float64(c), R, np.asarray(t).reshape(3)
    z[k[:-2] + "_A2"] = cu.rigid_align(z[k], z[k[:-2] + "_B"])
np.savez(sys.argv[1], **z)
"""


@pytest.mark.reference
def test_eval_ref_vs_live_reference(tmp_path):
    """eval_ref's restatement against the real lib/coord_utils.py on fresh sets (random, mirrored, planar; 3 .. 778
    points).  The reference runs in a child process: loading it installs its global config, which no other test should
    inherit."""
    import os
    import subprocess
    import sys
    import ref_loader
    if not ref_loader.available():
        pytest.skip("reference tree not present")
    rng = np.random.default_rng(99)
    sets = {}
    for N in (3, 14, 17, 778):
        for kind in range(3):
            A = rng.standard_normal((N, 3)) * 200 + 500
            if kind == 2:
                A[:, 2] = 0.3 * A[:, 0] - A[:, 1]
            B = A @ np.linalg.qr(rng.standard_normal((3, 3)))[0].T * 0.9 + 100 + rng.standard_normal((N, 3)) * 10
            if kind == 1:
                B[:, 1] = -B[:, 1]
            sets[f"s{N}_{kind}_A"], sets[f"s{N}_{kind}_B"] = A, B
    path = str(tmp_path / "live.npz")
    np.savez(path, **sets)
    oracle_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
    r = subprocess.run([sys.executable, "-c", _LIVE, path, oracle_dir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(path)
    for k in [k[:-2] for k in sets if k.endswith("_A")]:
        A, B = sets[k + "_A"], sets[k + "_B"]
        c1, R1, t1 = eval_ref.rigid_transform_3D(A, B)
        sc = np.abs(B).max()
        assert abs(c1 - z[k + "_c"]) <= 1e-12 * abs(z[k + "_c"]) and np.abs(R1 - z[k + "_R"]).max() <= 1e-12, k
        assert np.abs(t1 - z[k + "_t"]).max() <= 1e-12 * sc, k
        assert np.abs(eval_ref.rigid_align(A, B) - z[k + "_A2"]).max() <= 1e-12 * sc, k


def test_evaluate_host_checks():
    """pose2mesh_release_amd.evaluate without a GPU: CPU tensors raise (no CPU fallback), bad regressors / subsets are
    rejected at construction, and the ctypes prototypes of the two entry points are in the table."""
    import torch
    from pose2mesh_release_amd import _lib, evaluate
    with pytest.raises(_lib.P2MError):
        evaluate.rigid_align(torch.zeros(14, 3), torch.zeros(14, 3))
    ev = evaluate.MeshEvaluator(778, np.ones((21, 778), np.float32) / 778, 0, pa_mesh=True)
    with pytest.raises(_lib.P2MError):
        ev(torch.zeros(2, 778, 3), torch.zeros(2, 778, 3))
    with pytest.raises(ValueError):
        evaluate.MeshEvaluator(778, np.ones((21, 777), np.float32), 0)
    with pytest.raises(ValueError):
        evaluate.MeshEvaluator(778, np.ones((65, 778), np.float32), 0)
    with pytest.raises(ValueError):
        evaluate.MeshEvaluator(778, np.ones((21, 778), np.float32), 0, sub_A=[0, 21])
    with pytest.raises(ValueError):
        evaluate.MeshEvaluator(778, np.ones((21, 778), np.float32), 0, regressor_E=np.ones((17, 778)), root_E=17)
    assert "p2m_rigid_align" in _lib.HIP_SYMBOLS and "p2m_mesh_eval" in _lib.HIP_SYMBOLS
    assert len(_lib.HIP_SYMBOLS["p2m_mesh_eval"][1]) == 34
    assert evaluate.MeshEvaluator(778, None, 0).summary() == {"samples": 0}
