"""-m gpu: F-scores on the GPU (p2m_mesh_fscore, p2m_point_nn; evaluate.FScoreEvaluator, nearest_distances) against the
float64 restatement of the definition (tests/fscore_ref.py) on the case table of tests/fscore_cases.py: every distance within
the derived per-vertex bound, and - the bands of all cases being empty (tests/test_fscore_cpu.py) - counts exact, near_* and F
to 1e-12.  Through the C ABI with every output pre-filled with NaN inside guard regions, and through the public classes,
which must agree with it bit for bit.  Then the shell case, degenerate meshes, alignment, padding, batch independence,
repeatability, group totals, graph capture and the refusals."""
import ctypes as ct

import numpy as np
import pytest
import torch

import fscore_cases as fc
import fscore_ref as fr

pytestmark = pytest.mark.gpu

GUARD = 64


class Guarded:
    """A device array of `shape` inside a buffer with GUARD sentinel elements on both sides, everything pre-filled."""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + n].view(*shape)
        self.fill = fill

    def ptr(self):
        return ct.c_void_p(self.view.data_ptr())

    def untouched(self, t):
        return bool(torch.isnan(t).all()) if isinstance(self.fill, float) else bool((t == self.fill).all())

    def guards_ok(self):
        return self.untouched(self.buf[:GUARD]) and self.untouched(self.buf[-GUARD:])


def _p(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


def _cu(x, dtype=torch.float32):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to("cuda", dtype)


def abi_fscore(c, B_real=None, group=None, n_groups=0, want_totals=False, ws_short=0, expect_rc=0, **over):
    """p2m_mesh_fscore on a case dict (fscore_cases) with guarded, NaN-filled outputs -> (rc, dict of numpy results, guarded)."""
    from pose2mesh_release_amd import _lib
    from pose2mesh_release_amd import loss as _loss
    lib = _lib.hip()
    c = dict(c, **over)
    pred, gt = _cu(c["pred"]), _cu(c["gt"])
    B, nv = int(pred.shape[0]), int(pred.shape[1])
    B_real = B if B_real is None else B_real
    th = tuple(c["thresholds"])
    T = len(th)
    variants = (1 if c["centred"] else 0) | (2 if c["aligned"] else 0)
    pres = ([""] if c["centred"] else []) + (["pa_"] if c["aligned"] else [])
    nvar = len(pres)
    tabs = {}
    J = 0
    if c["regressor"] is not None:
        t = _loss._regressor_tables(np.asarray(c["regressor"], np.float32), nv)
        tabs = {k: _cu(t["jr_" + k], torch.float32 if k == "val" else torch.int32) for k in ("ptr", "idx", "val")}
        J = int(c["regressor"].shape[0])
    pr, gr = _cu(c["pred_root"]), _cu(c["gt_root"])
    g = {pre + k: Guarded((B, nv), torch.float32, float("nan")) for pre in pres for k in ("d_pred", "d_gt")}
    g["counts"] = Guarded((B, nvar, 2, T), torch.int32, -77)
    g["scores"] = Guarded((B, nvar, 3, T), torch.float64, float("nan"))
    ws_bytes = int(lib.p2m_nn_workspace(B, nv, nv))
    g["ws"] = Guarded((max(ws_bytes, 16),), torch.uint8, 0xAB)
    totals = torch.zeros((n_groups + 1, 1 + nvar * 3 * T), device="cuda", dtype=torch.float64) if want_totals else None
    grp = _cu(group, torch.int32)
    th_arr = (ct.c_float * max(T, 1))(*th)
    rc = lib.p2m_mesh_fscore(_p(pred), _p(gt), B, B_real, nv, float(c["gt_scale"]), _p(tabs.get("ptr")), _p(tabs.get("idx")),
                             _p(tabs.get("val")), J, int(c["root"]), _p(pr), _p(gr), variants, th_arr, T, g["ws"].ptr(),
                             ws_bytes - ws_short, *(g[k].ptr() if k in g else None for k in ("d_pred", "d_gt", "pa_d_pred",
                                                                                           "pa_d_gt")),
                             g["counts"].ptr(), g["scores"].ptr(), _p(grp), n_groups, _p(totals),
                             ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, lib.p2m_last_error_string())
    assert all(v.guards_ok() for v in g.values()), "a guard region was written"
    out = {k: v.view.cpu().numpy() for k, v in g.items() if k != "ws"}
    for v, pre in enumerate(pres):
        out[pre + "near_pred"], out[pre + "near_gt"], out[pre + "f"] = (out["scores"][:, v, k] for k in range(3))
        out[pre + "count_pred"], out[pre + "count_gt"] = out["counts"][:, v, 0], out["counts"][:, v, 1]
    if totals is not None:
        out["totals"] = totals.cpu().numpy()
    return rc, out, g


def evaluator_for(c, **kw):
    from pose2mesh_release_amd import evaluate
    return evaluate.FScoreEvaluator(c["pred"].shape[1], c["regressor"], c["root"], c["thresholds"], c["centred"], c["aligned"],
                                    c["gt_scale"], **kw)


def run_class(c, fs=None, **kw):
    fs = fs or evaluator_for(c)
    out = fs(_cu(c["pred"]), _cu(c["gt"]), _cu(c["pred_root"]), _cu(c["gt_root"]), **kw)
    return fs, {k: v.cpu().numpy() for k, v in out.items()}


def check_against(out, ref, c, what):
    """Distances within the per-vertex bound; counts exact (empty band); near_* and F to 1e-12.  Returns the worst error / bound."""
    worst = 0.0
    for pre in ([""] if c["centred"] else []) + (["pa_"] if c["aligned"] else []):
        assert ref[pre + "band"].sum() == 0, what
        for k in ("pred", "gt"):
            err = np.abs(out[pre + "d_" + k].astype(np.float64) - ref[pre + "d_" + k])
            ratio = float((err / ref[pre + "bound_" + k]).max())
            print(f"{what} {pre}d_{k}: worst error {err.max():.3e}, worst error / bound {ratio:.3f}")
            worst = max(worst, ratio)
            assert ratio <= 1.0, (what, pre, k, ratio)
            if pre + "count_" + k in out:
                assert np.array_equal(out[pre + "count_" + k], ref[pre + "count_" + k]), (what, pre, k)
        for k in ("near_pred", "near_gt", "f"):
            assert np.abs(out[pre + k] - ref[pre + k]).max() <= 1e-12, (what, pre, k)
    return worst


@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_case_table(hip_libs, name):
    """nv = 1, 2, every tile size - 1 / exact / + 1, the queries-per-lane switch, 778 with B = 3 and 6890 with B = 2 (the
    reference-made fixtures): the C ABI with guarded NaN-filled outputs, and FScoreEvaluator bit for bit the same."""
    c, ref = fc.case(name), fc.reference(name)
    _, out, _ = abi_fscore(c)
    check_against(out, ref, c, name)
    _, cls = run_class(c)
    for k, v in cls.items():
        assert np.array_equal(v, out[k]), (name, k)


@pytest.mark.parametrize("shape", fc.NN_SHAPES)
def test_point_nn_unequal_sizes(hip_libs, shape):
    """p2m_point_nn with nA != nB (guarded outputs) and nearest_distances: both directions within the bound, staged about
    the centroid of B."""
    from pose2mesh_release_amd import _lib, evaluate
    lib = _lib.hip()
    nb, nA, nB = shape
    A, B = fc.nn_pair(nb, nA, nB, seed=nA + nB)
    Ag, Bg = _cu(A), _cu(B)
    gab, gba = Guarded((nb, nA), torch.float32, float("nan")), Guarded((nb, nB), torch.float32, float("nan"))
    n = int(lib.p2m_nn_workspace(nb, nA, nB))
    ws = Guarded((n,), torch.uint8, 0xAB)
    rc = lib.p2m_point_nn(_p(Ag), _p(Bg), nb, nA, nB, gab.ptr(), gba.ptr(), ws.ptr(), n,
                          ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and gab.guards_ok() and gba.guards_ok() and ws.guards_ok()
    dab, dba = gab.view.cpu().numpy(), gba.view.cpu().numpy()
    for b in range(nb):
        _, M = fr.staged(A[b].astype(np.float64), B[b].astype(np.float64))
        for d, q, t, k in ((dab[b], A[b], B[b], "ab"), (dba[b], B[b], A[b], "ba")):
            ref = fr.nearest(q, t)
            ratio = float((np.abs(d - ref) / fr.bound(M, ref)).max())
            print(f"point_nn {shape} sample {b} d_{k}: worst error / bound {ratio:.3f}")
            assert ratio <= 1.0
    c_ab, c_ba = evaluate.nearest_distances(Ag, Bg)
    assert torch.equal(c_ab.cpu(), gab.view.cpu()) and torch.equal(c_ba.cpu(), gba.view.cpu())
    s_ab, s_ba = evaluate.nearest_distances(Ag[0], Bg[0])                  # unbatched [N, 3], [M, 3]
    assert s_ab.shape == (nA,) and s_ba.shape == (nB,) and torch.equal(s_ab, c_ab[0]) and torch.equal(s_ba, c_ba[0])
    # one direction only: the other buffer is not needed and the one asked for is the same
    gab2 = Guarded((nb, nA), torch.float32, float("nan"))
    rc = lib.p2m_point_nn(_p(Ag), _p(Bg), nb, nA, nB, gab2.ptr(), None, ws.ptr(), n,
                          ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(gab2.view, gab.view) and gab2.guards_ok()


def test_far_shells(hip_libs):
    """The true nearest target is farther than the staging origin (prediction on a 10 mm shell inside a 100 mm one, nv one
    past a target tile): a tail tile left as zeros would report ~10 mm instead of ~90."""
    c = fc.far_shells()
    ref = fr.evaluate(c["pred"], c["gt"], c["thresholds"], aligned=False)
    _, out, _ = abi_fscore(c)
    check_against(out, ref, c, "far_shells")
    assert out["d_pred"].min() > 85 and (out["count_pred"][:, 0] == 0).all() and (out["count_pred"][:, 1] == c["pred"].shape[1]).all()


def test_degenerate_meshes(hip_libs):
    c = fc.case("mano778")
    # identical meshes: the staged sets are bitwise equal, every centred distance is exactly 0 and F = 1
    same = dict(c, pred=(c["gt"].astype(np.float64) * c["gt_scale"]).astype(np.float32), gt_scale=1.0)
    same["gt"] = same["pred"]
    _, out, _ = abi_fscore(same)
    assert (out["d_pred"] == 0).all() and (out["d_gt"] == 0).all() and (out["f"] == 1.0).all()
    ref = fr.evaluate(same["pred"], same["gt"], same["thresholds"], 1.0, same["regressor"], same["root"])
    assert (np.abs(out["pa_d_pred"] - ref["pa_d_pred"]) <= ref["pa_bound_pred"]).all() and (out["pa_f"] == 1.0).all()
    # farther apart than every threshold (no centring: compared where they are): F = 0, not NaN
    far = dict(c, pred=same["pred"] + np.float32(5000.0), gt=same["pred"], gt_scale=1.0, regressor=None, aligned=False)
    _, out, _ = abi_fscore(far)
    assert (out["f"] == 0.0).all() and (out["near_pred"] == 0.0).all() and (out["counts"] == 0).all()
    assert out["d_pred"].min() > 1000.0 and np.isfinite(out["d_pred"]).all()


def test_alignment_recovers_an_exact_similarity(hip_libs):
    """The prediction is an exact similarity image (25 degrees, x 1.2, a shift) of the ground truth, rows of the pair in a
    shuffled order: pa_f = 1 at 0.01 mm, far above the bound, while the centred F is small.  (The alignment is PA-MPVPE's,
    over the index correspondence, so the shuffle is applied to both meshes alike; the search itself never uses the order.)"""
    g = fc.case("shell1024")["gt"].astype(np.float64)
    rng = np.random.default_rng(3)
    g = np.stack([x[rng.permutation(x.shape[0])] for x in g])
    a = np.deg2rad(25.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    c = dict(fc.case("shell1024"), pred=(1.2 * g @ R.T + np.array([30.0, -20.0, 10.0])).astype(np.float32),
             gt=g.astype(np.float32), thresholds=(0.01,))
    ref = fr.evaluate(c["pred"], c["gt"], c["thresholds"])
    assert ref["pa_bound_pred"].max() < 0.002 and ref["pa_d_pred"].max() < 0.002
    _, out, _ = abi_fscore(c)
    assert (out["pa_f"] == 1.0).all() and (out["f"] < 0.2).all()
    assert (np.abs(out["pa_d_pred"] - ref["pa_d_pred"]) <= ref["pa_bound_pred"]).all()


def _five():
    """Five 778-point shell clouds (a small similarity apart, centres given), three thresholds; band empty (asserted where
    counts are compared with the reference)."""
    return fc.five_hands()


def test_padding_rows(hip_libs):
    """B_real < B with NaN in the padding rows' inputs: their outputs are 0, the real rows are bitwise those of the unpadded
    call, and the summary equals the unpadded one to 1e-12."""
    c = _five()
    pad = dict(c, pred=c["pred"].copy(), gt=c["gt"].copy())
    pad["pred"][3:] = np.nan
    pad["gt"][3:] = np.nan
    real = dict(c, pred=c["pred"][:3], gt=c["gt"][:3], pred_root=c["pred_root"][:3], gt_root=c["gt_root"][:3])
    _, out, _ = abi_fscore(pad, B_real=3)
    _, ref, _ = abi_fscore(real)
    for k in ("d_pred", "d_gt", "pa_d_pred", "pa_d_gt", "counts", "scores"):
        assert (out[k][3:] == 0).all(), k
        assert np.array_equal(out[k][:3], ref[k]), k
    fs_p, _ = run_class(pad, B_real=3)
    fs_r, _ = run_class(real)
    sp, sr = fs_p.summary(), fs_r.summary()
    assert sp["samples"] == sr["samples"] == 3 and set(sp) == set(sr)
    assert all(abs(sp[k] - sr[k]) <= 1e-12 for k in sr)


def test_batch_independence_and_repeatability(hip_libs):
    """A sample alone at B = 1 and at position 3 of B = 5 is bitwise the same; two identical calls are bitwise equal."""
    c = _five()
    _, full, _ = abi_fscore(c)
    _, again, _ = abi_fscore(c)
    alone = dict(c, pred=c["pred"][3:4], gt=c["gt"][3:4], pred_root=c["pred_root"][3:4], gt_root=c["gt_root"][3:4])
    _, one, _ = abi_fscore(alone)
    for k in ("d_pred", "d_gt", "pa_d_pred", "pa_d_gt", "counts", "scores"):
        assert np.array_equal(full[k], again[k]), k
        assert np.array_equal(full[k][3:4], one[k]), k
    assert 0 < full["f"].min() and full["f"].max() < 1 and not np.array_equal(full["scores"][3], full["scores"][2])


def test_group_totals(hip_libs):
    """Running totals over two calls, per group, against fscore_ref.summary; ids outside [0, n_groups) count overall only."""
    c = _five()
    group = [1, 0, 1, 7, -1]
    fs = evaluator_for(c, n_groups=4)
    run_class(c, fs, group=group)
    run_class(c, fs, group=torch.tensor(group, device="cuda"), B_real=4)
    ref = fr.evaluate(c["pred"], c["gt"], c["thresholds"], pred_root=c["pred_root"], gt_root=c["gt_root"])
    assert ref["band"].sum() == 0 and ref["pa_band"].sum() == 0
    both = {k: np.concatenate([v, v[:4]]) for k, v in ref.items()}
    want = fr.summary(both, c["thresholds"], group=group + group[:4], n_groups=4)
    got = fs.summary()
    assert got["samples"] == 9 and sorted(got["groups"]) == [0, 1] and got["groups"][1]["samples"] == 4

    def same(a, b):
        assert set(a) == set(b), (set(a) ^ set(b))
        for k in a:
            if k != "groups":
                assert abs(a[k] - b[k]) <= 1e-12, k
    same(got, want)
    for gid in got["groups"]:
        same(got["groups"][gid], want["groups"][gid])
    assert "f@3" in got and "pa_f@8" in got and "near_pred@5" in got and "pa_near_gt@3" in got
    fs.reset()
    assert fs.summary()["samples"] == 0


def test_graph_capture_replays_bitwise(hip_libs):
    """One single-stream torch.cuda.graph capture of an evaluator call replays to the eager outputs bit for bit."""
    c = fc.case("mano778")
    fs = evaluator_for(c)
    pred, gt = _cu(c["pred"]), _cu(c["gt"])
    eager = {k: v.clone() for k, v in fs(pred, gt).items()}                 # (also allocates the buffers of this size)
    tot = fs.totals.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fs(pred, gt)
    fs.reset()
    for v in out.values():
        v.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(out[k], v), k
    assert torch.equal(fs.totals, tot)


def test_refusals(hip_libs):
    """Every refusal returns P2M_ERR_INVALID and launches nothing: the NaN-filled outputs stay untouched."""
    from pose2mesh_release_amd import _lib
    lib = _lib.hip()
    c = dict(fc.case("shell64"), thresholds=(5.0, 15.0))

    err = -1                                                             # P2M_ERR_INVALID
    for kw in (dict(thresholds=(5.0, 0.0)), dict(thresholds=(-5.0,)), dict(thresholds=(float("inf"),)),
               dict(thresholds=(float("nan"),)), dict(ws_short=1), dict(centred=False, aligned=False), dict(B_real=3)):
        rc, _, g = abi_fscore(c, expect_rc=err, **kw)
        assert all(v.untouched(v.view) for v in g.values()), kw
        assert lib.p2m_last_error_string()
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    pred, gt = _cu(c["pred"]), _cu(c["gt"])
    n = int(lib.p2m_nn_workspace(2, 64, 64))
    ws = Guarded((n,), torch.uint8, 0xAB)
    d = Guarded((2, 64), torch.float32, float("nan"))
    th = (ct.c_float * 5)(1, 2, 3, 4, 5)

    def call(pred=_p(pred), gt=_p(gt), B=2, nv=64, thp=th, T=2, wsp=ws.ptr(), wsn=n):
        rc = lib.p2m_mesh_fscore(pred, gt, B, B, nv, 1.0, None, None, None, 0, 0, None, None, 1, thp, T, wsp, wsn, d.ptr(), None,
                                 None, None, None, None, None, 0, None, stream)
        torch.cuda.synchronize()
        return rc
    assert call() == 0 and not d.untouched(d.view)
    d.view.fill_(float("nan"))
    ws.view.fill_(0xAB)
    for kw in (dict(pred=None), dict(gt=None), dict(thp=None), dict(wsp=None), dict(nv=0), dict(T=0), dict(T=5),
               dict(B=1 << 20, nv=1 << 10), dict(wsn=n - 1), dict(wsn=0)):
        assert call(**kw) == err, kw
        assert d.untouched(d.view) and ws.untouched(ws.view) and d.guards_ok(), kw
    # p2m_point_nn: the same kinds
    for args in ((None, _p(gt), 2, 64, 64, d.ptr(), None, ws.ptr(), n), (_p(pred), _p(gt), 2, 0, 64, d.ptr(), None, ws.ptr(), n),
                 (_p(pred), _p(gt), 2, 64, 64, None, None, ws.ptr(), n), (_p(pred), _p(gt), 2, 64, 64, d.ptr(), None, None, n),
                 (_p(pred), _p(gt), 2, 64, 64, d.ptr(), None, ws.ptr(), n - 1),
                 (_p(pred), _p(gt), 1 << 20, 1 << 10, 4, d.ptr(), None, ws.ptr(), n)):
        assert lib.p2m_point_nn(*args, stream) == err
        torch.cuda.synchronize()
        assert d.untouched(d.view) and ws.untouched(ws.view)
