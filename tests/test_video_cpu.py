"""CPU: the yardsticks of pose2mesh_release_amd.video and everything of it that needs no GPU.  tests/video_ref.py (the fp32
op-by-op filter, the float64 metrics) against the fixture that tests/golden/make_golden_video.py recorded from the real
reference, and against the live reference where its tree exists; the C entries' argument checks; the host-side tables."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import helpers
import video_ref


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_filter_restatement_equals_fixture_bitwise():
    z = helpers.golden("video_ref.npz")
    x, ptr = z["flt_x"], z["flt_seq_ptr"]
    flat = x.reshape(len(x), -1)
    assert x.dtype == np.float32 and len(z["flt_params"]) == 4
    for k, (mc, b) in enumerate(z["flt_params"]):
        y = video_ref.one_euro_seqs(flat, ptr, mc, b)
        assert np.array_equal(_bits(y), _bits(z[f"flt_y{k}"].reshape(flat.shape))), (mc, b)
    # chunked through the carried state = one shot (the contract the GPU's streaming form is held to)
    one, _ = video_ref.one_euro(flat[:40], 0.004, 0.7)
    st, parts = None, []
    for a, e in ((0, 1), (1, 6), (6, 40)):
        y, st = video_ref.one_euro(flat[a:e], 0.004, 0.7, state=st)
        parts.append(y)
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(one))


def test_metric_restatement_equals_fixture():
    """float64 against float64: the reference's SVD alignment and eval_ref's differ by rounding only."""
    z = helpers.golden("video_ref.npz")
    rows, ptr = video_ref.tables(z["ev_masks"])
    sm = video_ref.one_euro_seqs(z["ev_pred"].reshape(130, -1), ptr, 0.004, 0.005, rows=rows).reshape(130, 14, 3)
    assert np.array_equal(_bits(sm), _bits(z["ev_smoothed"]))
    r = video_ref.video_eval(sm, z["ev_gt"][rows], ptr)
    assert np.allclose(r["seq_stats"][:, 2], z["ev_accel_error"], rtol=1e-12, atol=0)
    assert np.allclose(r["seq_stats"][:, 3], z["ev_mpjpe_list"], rtol=1e-12, atol=0)
    assert np.abs(r["pa_mpjpe"] - z["ev_pa_mpjpe"]).max() <= 1e-9
    assert np.allclose(r["totals"][:3], z["ev_totals"], rtol=1e-12, atol=0)
    assert r["totals"][3:].tolist() == [2, 0, 2, 0, 130]
    g, p = z["ev_gt"][z["ev_masks"][1]], z["ev_pred"][z["ev_masks"][1]]
    a, v = video_ref.error_accel(g, p)
    assert v[:38].all() and not v[38:].any() and np.allclose(a[:38], z["acc_plain"], rtol=1e-12, atol=0)
    a, v = video_ref.error_accel(g, p, z["acc_vis_mask"])
    assert np.allclose(a[v], z["acc_vis"], rtol=1e-12, atol=0) and v.sum() == len(z["acc_vis"]) == 26
    # every frame of the fixture is well posed for the alignment
    assert (z["ev_smoothed"].astype(np.float64).var(axis=1).sum(axis=1) > 1.0).all()


@pytest.mark.reference
def test_filter_restatement_equals_live_reference_bitwise():
    import ref_loader
    path = os.path.join(ref_loader.REF_ROOT, "lib", "smooth_utils.py")
    if not os.path.exists(path):
        pytest.skip("reference tree not present")
    spec = importlib.util.spec_from_file_location("smooth_utils_live", path)      # needs only numpy
    sm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sm)
    rng = np.random.default_rng(5)
    x = (np.cumsum(rng.standard_normal((300, 14, 3)) * 6.0, axis=0) + rng.standard_normal((300, 14, 3)) * 15.0
         + rng.uniform(-900, 900, (1, 14, 3))).astype(np.float32)
    for mc, b in ((0.004, 0.7), (0.004, 0.005), (1.0, 0.0), (0.05, 3.0)):
        ref = sm.smooth_pose(x, min_cutoff=mc, beta=b)
        assert ref.dtype == np.float32
        mine = video_ref.one_euro(x.reshape(300, -1), mc, b)[0].reshape(x.shape)
        assert np.array_equal(_bits(mine), _bits(ref)), (mc, b)


def test_one_euro_entry_rejects_bad_arguments(hip_libs):
    from pose2mesh_release_amd import _lib
    lib = _lib.hip()
    assert lib.p2m_one_euro_lookahead() >= 1
    buf = (ctypes.c_float * 1024)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ok = dict(x=base, seq_ptr=base, rows=None, N=4, S=1, C=3, mc=0.004, beta=0.7, dc=1.0, dt=1.0, sx=None, sdx=None,
              started=None, y=base + 2048, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.p2m_one_euro(*[a[k] for k in ok])
    inf, nan = float("inf"), float("nan")
    for kw, word in ((dict(x=None), "null"), (dict(seq_ptr=None), "null"), (dict(y=None), "null"), (dict(S=0), "S >= 1"),
                     (dict(C=0), "C >= 1"), (dict(N=-1), "N >= 0"), (dict(N=1 << 30, C=2), "2^31"),
                     (dict(S=1 << 30, C=2), "2^31"), (dict(mc=nan), "non-finite"), (dict(beta=inf), "non-finite"),
                     (dict(dc=-inf), "non-finite"), (dict(dt=nan), "non-finite"), (dict(dt=0.0), "dt > 0"),
                     (dict(dt=-1.0), "dt > 0"), (dict(mc=-1e-9), "min_cutoff >= 0"), (dict(dc=-1.0), "d_cutoff >= 0"),
                     (dict(dt=1e-60), "fp32 range"), (dict(beta=1e300), "fp32 range"), (dict(dc=1e39), "fp32 range"),
                     (dict(sx=base), "all three"), (dict(sx=base, sdx=base), "all three"), (dict(started=base), "all three"),
                     (dict(sdx=base, started=base), "all three"), (dict(rows=base, y=base), "alias")):
        assert call(**kw) == -1, kw
        assert word in lib.p2m_last_error_string().decode(), (kw, lib.p2m_last_error_string())


def test_video_eval_entry_rejects_bad_arguments(hip_libs):
    from pose2mesh_release_amd import _lib
    lib = _lib.hip()
    buf = (ctypes.c_float * 1024)()
    base = ctypes.addressof(buf)
    ok = dict(pred=base, gt=base, seq_ptr=base, vis=None, N=4, S=1, J=14, pa=1, accel=base, valid=base, mpjpe=base, pam=base,
              fs=base, ss=base, tot=base, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.p2m_video_eval(*[a[k] for k in ok])
    for kw, word in ((dict(pred=None), "null"), (dict(gt=None), "null"), (dict(seq_ptr=None), "null"), (dict(accel=None), "null"),
                     (dict(valid=None), "null"), (dict(mpjpe=None), "null"), (dict(fs=None), "null"), (dict(ss=None), "null"),
                     (dict(tot=None), "null"), (dict(pam=None), "want_pa"), (dict(S=0), "S >= 1"), (dict(N=-1), "N >= 0"),
                     (dict(J=0), "1..64"), (dict(J=65), "1..64"), (dict(N=1 << 28, J=3), "2^31")):
        assert call(**kw) == -1, kw
        assert word in lib.p2m_last_error_string().decode(), (kw, lib.p2m_last_error_string())


def test_sequence_tables():
    from pose2mesh_release_amd import video
    m = np.zeros((3, 12), bool)
    m[0, :3] = m[0, 8:] = True                      # a two-run video, as a two-person video after the sort by person_id
    m[1, 3:8] = True                                # a contiguous one;  video 2 is empty
    rows, ptr, n = video.sequence_tables(list(m))
    assert rows.dtype == np.int32 and ptr.dtype == np.int32 and n == 12
    assert rows.tolist() == [0, 1, 2, 8, 9, 10, 11, 3, 4, 5, 6, 7] and ptr.tolist() == [0, 7, 12, 12]
    r2, p2 = video_ref.tables(list(m))
    assert np.array_equal(rows, r2) and np.array_equal(ptr, p2)
    # index arrays keep their own order; n defaults to the largest position + 1
    rows, ptr, n = video.sequence_tables([np.array([5, 4, 9]), [], np.arange(2)])
    assert rows.tolist() == [5, 4, 9, 0, 1] and ptr.tolist() == [0, 3, 3, 5] and n == 10
    assert video.sequence_tables([np.array([1, 0])], n=40)[2] == 40
    # the reference's construction (dataset.py:157-163): names sorted by person first
    names = np.array(["b", "a", "a", "b", "b", "a"])
    vi = [names == u for u in np.unique(names)]
    rows, ptr, n = video.sequence_tables(vi)
    assert rows.tolist() == [1, 2, 5, 0, 3, 4] and ptr.tolist() == [0, 3, 6] and n == 6
    for bad in ([np.array([0, 12])], [m[0], np.zeros(5, bool)], [np.array([-1])], [np.array([0.5])], []):
        with pytest.raises(ValueError):
            video.sequence_tables(bad, n=12 if len(bad) == 1 else None)


def test_cpu_tensors_raise():
    import torch
    from pose2mesh_release_amd import video
    from pose2mesh_release_amd._lib import P2MError
    x = torch.zeros(5, 14, 3)
    with pytest.raises(P2MError):
        video.smooth_pose(x)
    with pytest.raises(P2MError):
        video.OneEuroFilter()(x)
    with pytest.raises(P2MError):
        video.error_accel(x, x)
    with pytest.raises(P2MError):
        video.VideoEvaluator([np.ones(5, bool)], 14).put(0, x, x)
    with pytest.raises(ValueError):
        video.VideoEvaluator([np.ones(5, bool)], 65)
    with pytest.raises(ValueError):
        video.OneEuroFilter(dt=0.0)
