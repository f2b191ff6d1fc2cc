"""-m gpu: the evaluation kernels (csrc/eval.hip: k_rigid_align, k_mesh_eval, k_eval_fold; the solve of csrc/p2m_eval.h) on
the case tables of tests/eval_cases.py, against the float64 restatement tests/eval_ref.py: degenerate alignments (zero and
tiny eigenvalue gaps, the early exits of the Jacobi sweeps), the launch edges of the wave / block kernels, the joint-fill
loops and the stage-E wave of the evaluator at their trip counts, roots that tell stage A from stage E, the fold's second
trip and out-of-range group ids; guard rows, full writes, position independence, repeatability and the refusals of the C ABI.
Each group prints its worst error / bar before it asserts (pytest -s shows it).  tests/test_eval_edges_cpu.py audits the
tables without a GPU."""

import numpy as np
import pytest
import torch

import eval_cases as ec
import eval_ref

pytestmark = pytest.mark.gpu

R_BAR, C_BAR, T_BAR = 1e-6, 1e-6, 4e-7           # tests/test_gpu_eval.py: R per element, c relative, t / A2 x max|B|
BAR_MM = ec.BAR_MM


def _cu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- alignment ---------------------------------------------------------------------------------------------------------------
_align_out = {}


def _align(name):
    """c, R, t, A2 of a case: rigid_transform_3D and rigid_align (two launches), and once more in one launch with A2; the
    two runs must agree bit for bit.  Kept per session (the classes' tests and the summary share them)."""
    from pose2mesh_release_amd import evaluate
    if name not in _align_out:
        k = ec.align_case(name)
        A, B = _cu(k["A"]), _cu(k["B"])
        c, R, t = evaluate.rigid_transform_3D(A, B)
        first = [x.cpu().numpy() for x in (c, R, t, evaluate.rigid_align(A, B))]
        again = [x.cpu().numpy() for x in evaluate._rigid(A, B, True)]
        for q, x, y in zip("cRtA", first, again):
            assert x.shape == y.shape and _same(x, y), (name, q, "two runs differ")
        _align_out[name] = first
    return _align_out[name]


def _unique_shares(k, ref, out, keep):
    """Worst error / bar of the sets `keep` against eval_ref.batch_rigid."""
    c, R, t, A2 = (x[keep] for x in out)
    sc = float(np.abs(k["B"][keep]).max())
    sh = {"t": np.abs(t - ref["t"][keep]).max() / (T_BAR * sc), "A2": np.abs(A2 - ref["A2"][keep]).max() / (T_BAR * sc)}
    if k["compare_R"]:
        sh["R"] = np.abs(R - ref["R"][keep]).max() / R_BAR
        sh["c"] = (np.abs(c - ref["c"][keep]) / np.abs(ref["c"][keep])).max() / C_BAR
    else:
        # constant B: the reference's c is exactly 0, so the relative bar has nothing to refer to; c is a ratio of the two
        # sets' spreads (order 1 for any other B of this size), and the bar is taken absolute
        sh["c"] = np.abs(c - ref["c"][keep]).max() / C_BAR
    return sh


def _report(title, rows):
    print(f"\n{title}: worst error / bar")
    for name, sh in rows:
        print(f"  {name:24s} " + " ".join(f"{q} {v:9.2e}" for q, v in sh.items()))


def _assert_shares(rows):
    for name, sh in rows:
        for q, v in sh.items():
            assert v <= 1.0, (name, q, v)                      # (NaN fails too)


def test_unique_alignments_vs_eval_ref(hip_libs):
    """Every `unique` case at the bars of tests/test_gpu_eval.py; constant B (H = 0): c = 0 and every row of A2 is cB."""
    rows = []
    for name in ec.align_names("unique"):
        k, out = ec.align_case(name), _align(name)
        assert all(np.isfinite(x).all() for x in out), name
        rows.append((name, _unique_shares(k, ec.align_reference(name), out, np.arange(k["A"].shape[0]))))
        if not k["compare_R"]:
            cB = k["B"][:, :1].astype(np.float64)
            assert np.abs(out[3] - cB).max() <= T_BAR * np.abs(k["B"]).max(), name
        Rg = out[1].astype(np.float64)
        assert np.abs(Rg @ Rg.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6 and (np.linalg.det(Rg) > 0).all(), name
    _report("unique", rows)
    _assert_shares(rows)


def test_free_alignments_reach_the_optimum(hip_libs):
    """Gap 0 or nearly 0 (or data 1e6 from the origin): R is not compared.  c within 1e-6 of the optimum's, R orthogonal to
    1e-6 and proper, the RMS residual of A2 within 4e-7 max|B| of the optimum's; A2 itself where A is (nearly) collinear."""
    rows = []
    for name in ec.align_names("free"):
        k, out, ref = ec.align_case(name), _align(name), ec.align_reference(name)
        c, R, t, A2 = out
        assert all(np.isfinite(x).all() for x in out), name
        sc = float(np.abs(k["B"]).max())
        Rg = R.astype(np.float64)
        rms = np.sqrt(np.mean(np.sum((A2.astype(np.float64) - k["B"].astype(np.float64)) ** 2, axis=-1), axis=-1))
        sh = {"c": (np.abs(c - ref["copt"]) / np.abs(ref["copt"])).max() / C_BAR,
              "RRt": np.abs(Rg @ Rg.transpose(0, 2, 1) - np.eye(3)).max() / 1e-6,
              "rms": np.abs(rms - ref["rms"]).max() / (T_BAR * sc)}
        if k["a2_unique"]:
            sh["A2"] = np.abs(A2 - ref["A2"]).max() / (T_BAR * sc)
        assert (np.linalg.det(Rg) > 0).all(), name
        rows.append((name, sh))
    _report("free", rows)
    _assert_shares(rows)


def test_nonfinite_sets_stay_alone(hip_libs):
    """N = 1, a coincident set, a NaN, an inf: that set's c, t and A2 are non-finite, nothing faults, and every other set of
    the batch meets the `unique` bars."""
    rows = []
    for name in ec.align_names("nonfinite"):
        k, out = ec.align_case(name), _align(name)
        c, R, t, A2 = out
        for i in k["bad"]:
            assert not np.isfinite(c[i]) and not np.isfinite(t[i]).any() and not np.isfinite(A2[i]).any(), (name, i)
        keep = np.array([i for i in range(k["A"].shape[0]) if i not in k["bad"]], dtype=np.int64)
        if keep.size:
            assert all(np.isfinite(x[keep]).all() for x in out), name
            rows.append((name, _unique_shares(k, ec.align_reference(name), out, keep)))
    _report("nonfinite (the other sets)", rows)
    _assert_shares(rows)
    assert len(rows) == 6


@pytest.mark.parametrize("N", [17, 257])
def test_alignment_is_position_independent(hip_libs, N):
    """One set copied to all 7 positions of a batch (every wave of a block, both blocks of the wave kernel; 7 blocks of the
    block kernel): c, R, t and A2 are bitwise the same at every position, and the same as the set alone."""
    from pose2mesh_release_amd import evaluate
    k = ec.align_case(f"generic{N}" if N == 257 else "tail17_nb7")
    A, B = np.repeat(k["A"][2:3], 7, axis=0), np.repeat(k["B"][2:3], 7, axis=0)
    out = [x.cpu().numpy() for x in evaluate._rigid(_cu(A), _cu(B), True)]
    one = [x.cpu().numpy() for x in evaluate._rigid(_cu(A[0]), _cu(B[0]), True)]
    for q, x, o in zip("cRtA", out, one):
        assert np.isfinite(x).all()
        for i in range(7):
            assert np.array_equal(x[i], x[0]), (q, i)
        assert np.array_equal(x[0], o), q


def _abi_rigid(A, B, nb, N, c, R, t, A2):
    from pose2mesh_release_amd import _lib, evaluate
    return _lib.hip().p2m_rigid_align(evaluate._p(A), evaluate._p(B), nb, N, evaluate._p(c), evaluate._p(R), evaluate._p(t),
                                      evaluate._p(A2), evaluate._stream())


@pytest.mark.parametrize("nb,N", [(7, 17), (5, 3), (2, 255), (1, 256), (3, 257), (6, 1)])
def test_alignment_writes_its_rows_and_no_more(hip_libs, nb, N):
    """Outputs prefilled with NaN and two more rows than the batch: every element of the nb rows is written, the rows past the
    end are untouched (N = 1: written, with non-finite c, t, A2 and a finite R)."""
    rng = np.random.default_rng(nb * 1000 + N)
    A = ec._generic(rng, nb, N)
    A_d, B_d = _cu(A.astype(np.float32)), _cu(ec._similar(A, rng).astype(np.float32))
    nan = float("nan")
    c = torch.full((nb + 2,), nan, device="cuda")
    R = torch.full((nb + 2, 9), nan, device="cuda")
    t = torch.full((nb + 2, 3), nan, device="cuda")
    A2 = torch.full((nb + 2, N, 3), nan, device="cuda")
    assert _abi_rigid(A_d, B_d, nb, N, c, R, t, A2) == 0
    torch.cuda.synchronize()
    for q, x in (("c", c), ("R", R), ("t", t), ("A2", A2)):
        assert bool(torch.isnan(x[nb:]).all()), (q, "guard rows written")
        if N > 1 or q == "R":
            assert bool(torch.isfinite(x[:nb]).all()), (q, "not every element written")
    if N == 1:
        assert not bool(torch.isfinite(c[:nb]).any()) and not bool(torch.isfinite(A2[:nb]).any())
    # nb = 0 is a no-op
    assert _abi_rigid(A_d, B_d, 0, N, c[nb:], R[nb:], t[nb:], A2[nb:]) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(c[nb:]).all()) and bool(torch.isnan(A2[nb:]).all())


# ---- evaluator ---------------------------------------------------------------------------------------------------------------
def _evaluator(name, n_groups=4):
    from pose2mesh_release_amd import evaluate
    k, z = ec.eval_case(name), ec.eval_inputs(name)
    return evaluate.MeshEvaluator(k["nv"], z["RA"], k["root_A"], sub_A=k["sub_A"], regressor_E=z["RE"], root_E=k["root_E"],
                                  sub_E=k["sub_E"], pa_mesh=k["pa_mesh"], gt_mesh_scale=z["scale"], n_groups=n_groups)


_eval_out = {}


def _run_eval(name):
    """Outputs of an evaluator case as float64 numpy (plus the summary after the first call); a second call into the same
    evaluator must reproduce them bit for bit.  Kept per session."""
    if name not in _eval_out:
        z = ec.eval_inputs(name)
        ev = _evaluator(name)
        args = (_cu(z["pred"]), _cu(z["gt"]))
        kw = dict(gt_joints_A=_cu(z["gja"]), gt_joints_E=_cu(z["gje"]), pred_joints_A=_cu(z["pja"]))
        first = {q: v.cpu().numpy().copy() for q, v in ev(*args, **kw).items()}
        summary = ev.summary()
        again = {q: v.cpu().numpy() for q, v in ev(*args, **kw).items()}
        for q in first:
            assert _same(first[q], again[q]), (name, q, "two runs differ")
        assert ev.summary()["samples"] == 2 * ec.EVAL_B
        _eval_out[name] = (first, summary)
    return _eval_out[name]


def _miss(x, ref):
    """Largest |x - ref| over the entries where the reference is finite, in bars; inf if the two disagree on finiteness."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    if x.shape != ref.shape or not np.array_equal(np.isfinite(x), np.isfinite(ref)):
        return float("inf")
    fin = np.isfinite(ref)
    return float(np.abs(x[fin] - ref[fin]).max() / BAR_MM) if fin.any() else 0.0


@pytest.mark.parametrize("name", [k["name"] for k in ec.EVAL_CASES])
def test_evaluator_edges_vs_eval_ref(hip_libs, name):
    """Every per-joint, per-sample and summary value of a case within 2e-4 mm of eval_ref.mesh_eval / summary; where the
    reference is non-finite (one stage-E joint: 0 / 0) the kernel's value is non-finite too, and only there."""
    out, summary = _run_eval(name)
    ref = ec.eval_reference(name)
    assert set(q for q in out if q != "sample_means") == set(ref)
    sh = {q: _miss(out[q], v) for q, v in ref.items()}
    sh["sample_means"] = _miss(out["sample_means"], ec.sample_means(ref))
    if ref["mpvpe"].min() >= 4096.0:
        # ground-truth joints 10 m away: MPVPE carries the shift (~ 17.7 m), and from 4096 mm on half an fp32 ulp (2.4e-4 mm
        # and more) is wider than the bar, so the fp32 output cannot be held to it.  The fp64 column of sample_means is (above),
        # and the fp32 output must be exactly its rounding.
        assert np.array_equal(out["mpvpe"], out["sample_means"][:, 3].astype(np.float32))
        del sh["mpvpe"]
    with np.errstate(all="ignore"):
        rs = eval_ref.summary(ref)
    assert summary["samples"] == ec.EVAL_B and "groups" not in summary
    for q in ref:
        sh["summary " + q] = _miss(summary[q], rs[q])
    _report("evaluator", [(name, sh)])
    for q, v in sh.items():
        assert v <= 1.0, (name, q, v)
    k = ec.eval_case(name)
    assert out["mpjpe_A"].shape == (ec.EVAL_B, len(k["sub_A"]) if k["sub_A"] is not None else k["JA"])
    assert out["mpjpe_E"].shape == (ec.EVAL_B, len(k["sub_E"]) if k["sub_E"] is not None else k["JE"])


def test_evaluator_degenerate_subsets(hip_libs):
    """One stage-E joint: pa_mpjpe_E and its column of sample_means are non-finite, every other output is finite.  Two
    joints: the alignment is exact, the PA error is at most the bar."""
    out, summary = _run_eval("subE1")
    assert not np.isfinite(out["pa_mpjpe_E"]).any() and not np.isfinite(out["sample_means"][:, 1]).any()
    assert not np.isfinite(summary["pa_mpjpe_E"])
    for q, v in out.items():
        if q == "sample_means":
            assert np.isfinite(v[:, [0, 2, 3, 4]]).all()
        elif q != "pa_mpjpe_E":
            assert np.isfinite(v).all(), q
    assert all(np.isfinite(summary[q]) for q in ("mpjpe_E", "mpjpe_A", "mpvpe", "pa_mpvpe"))
    out2, _ = _run_eval("subE2")
    assert out2["pa_mpjpe_E"].max() <= BAR_MM and out2["mpjpe_E"].max() > 1.0


def test_evaluator_roots_and_shift(hip_libs):
    """(root_A, root_E) = (3, 9) against (9, 3) on the same data: the outputs differ by more than 100 bars (each is within one
    bar of its own reference: test_evaluator_edges_vs_eval_ref).  Ground-truth joints 10.24 m from the mesh frame: the joint
    metrics and PA-MPVPE are those of the unshifted joints to a bar (the shift is exact in fp32), MPVPE carries the shift."""
    a, b = _run_eval("roots_3_9")[0], _run_eval("roots_9_3")[0]
    for q in ("mpjpe_A", "mpvpe", "mpjpe_E"):
        assert np.abs(a[q].astype(np.float64) - b[q]).max() > 100 * BAR_MM, q
    s, u = _run_eval("shifted_gt_joints")[0], _run_eval("unshifted_gt_joints")[0]
    for q in ("mpjpe_A", "mpjpe_E", "pa_mpjpe_E", "pa_mpvpe"):
        assert np.abs(s[q].astype(np.float64) - u[q]).max() <= BAR_MM, q
    assert (s["mpvpe"] > 10000.0).all() and (u["mpvpe"] < 200.0).all()


# ---- totals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_groups", ec.TOTALS_N_GROUPS)
def test_totals_over_calls_and_group_ids(hip_libs, n_groups):
    """Three calls of B = 5, 3 and 5 (the last all padding, NaN meshes) into one evaluator: the counts per group are exact,
    ids outside [0, n_groups) count in row 0 only, group means are within 2e-4 mm of eval_ref, rows of groups that received
    nothing stay exactly 0 ((n_groups + 1) * 6 > 256 from n_groups = 42: the fold's second trip)."""
    from pose2mesh_release_amd import evaluate
    calls, RA, RE = ec.totals_inputs()
    ids = ec.totals_groups(n_groups)
    ev = evaluate.MeshEvaluator(ec.TOTALS_NV, RA, ec.TOTALS_ROOT_A, regressor_E=RE, root_E=ec.TOTALS_ROOT_E, pa_mesh=True,
                                n_groups=n_groups)
    refs, before = [], None
    for (pred, gt), (B, B_real), g in zip(calls, ec.TOTALS_CALLS, ids):
        if B_real == 0:
            before = ev.totals.clone()
        out = ev(_cu(pred), _cu(gt), B_real=B_real, group=g)
        if B_real:
            refs.append(ec.sample_means(eval_ref.mesh_eval(pred, gt, RA, ec.TOTALS_ROOT_A, None, RE, ec.TOTALS_ROOT_E, None, True)))
            assert _miss(out["sample_means"].cpu().numpy(), refs[-1]) <= 1.0
        else:
            assert all(float(v.abs().max()) == 0.0 for v in out.values())           # padding rows: 0, inputs never read
    tot = ev.totals.cpu().numpy()
    assert tot.shape == (n_groups + 1, 6) and np.array_equal(tot, before.cpu().numpy())
    means = np.concatenate(refs)
    gid = np.array(ids[0] + ids[1], dtype=np.int64)
    assert tot[0, 0] == len(gid) == 8
    worst = np.abs(tot[0, 1:] / 8 - means.mean(axis=0)).max() / BAR_MM
    valid = sorted({int(g) for g in gid if 0 <= g < n_groups})
    assert n_groups == 0 or n_groups - 1 in valid
    for g in range(n_groups):
        m = gid == g
        assert tot[g + 1, 0] == m.sum(), g
        if m.any():
            worst = max(worst, np.abs(tot[g + 1, 1:] / m.sum() - means[m].mean(axis=0)).max() / BAR_MM)
        else:
            assert not tot[g + 1].any(), g
    assert tot[1:, 0].sum() == sum(1 for g in gid if 0 <= g < n_groups) < 8            # the other ids: row 0 only
    print(f"\ntotals n_groups = {n_groups}: worst group mean error / bar {worst:.2e}")
    assert worst <= 1.0
    s = ev.summary()
    assert s["samples"] == 8 and sorted(s.get("groups", {})) == valid
    for g in valid:
        assert s["groups"][g]["samples"] == int((gid == g).sum())


# ---- the C ABI: guard rows, full writes, refusals ---------------------------------------------------------------------------
class _Abi:
    """One p2m_mesh_eval call assembled from an evaluator case: device tensors by name, overridable before call()."""

    def __init__(self, name, B=ec.EVAL_B, B_real=3, n_groups=3, stage_E=True, pa_mesh=True, rows=1, slack=0):
        from pose2mesh_release_amd import loss
        k, z = ec.eval_case(name), ec.eval_inputs(name)
        self.B, self.B_real, self.nv, self.scale, self.n_groups = B, B_real, k["nv"], z["scale"], n_groups
        self.JA, self.root_A, self.JE, self.root_E = k["JA"], k["root_A"], k["JE"] if stage_E else 0, k["root_E"]
        self.pa_mesh = int(pa_mesh)
        self.t = {"pred": _cu(z["pred"]), "gt": _cu(z["gt"]), "pja": _cu(z["pja"]), "gja": _cu(z["gja"]), "gje": _cu(z["gje"])}
        for pre, Rg in (("ra", z["RA"]), ("re", z["RE"] if stage_E else None)):
            tab = loss._regressor_tables(Rg, k["nv"]) if Rg is not None else None
            for q in ("ptr", "idx", "val"):
                self.t[f"{pre}_{q}"] = _cu(tab["jr_" + q]) if tab else None
        self.sub_A, self.sub_E = k["sub_A"], k["sub_E"] if stage_E else None
        self.t["sub_A"] = _cu(np.asarray(k["sub_A"], np.int32)) if k["sub_A"] is not None else None
        self.t["sub_E"] = _cu(np.asarray(self.sub_E, np.int32)) if self.sub_E is not None else None
        self.nsA = len(k["sub_A"]) if k["sub_A"] is not None else k["JA"]
        self.nsE = (len(self.sub_E) if self.sub_E is not None else self.JE) if stage_E else 0
        nan = float("nan")

        def f(*shape, dtype=torch.float32):
            return torch.full(shape, nan, device="cuda", dtype=dtype)
        R = B + rows                                           # `rows` guard rows past the end, `slack` guard columns' worth
        self.o = {"mpjpe_A": f(R, self.nsA + slack), "mpvpe": f(R), "mpjpe_E": f(R, max(self.nsE, 1) + slack),
                  "pa_mpjpe_E": f(R, max(self.nsE, 1) + slack), "pa_mpvpe": f(R),
                  "sample_means": f(R, 5, dtype=torch.float64),
                  "totals": torch.zeros((n_groups + 1 + rows, 6), device="cuda", dtype=torch.float64)}
        self.o["totals"][n_groups + 1:] = nan
        self.t["group"] = _cu(np.array([0, n_groups - 1, 1, 2, 0][:B] + [0] * max(B - 5, 0), np.int32))
        self.nsub_A = len(k["sub_A"]) if k["sub_A"] is not None else 0
        self.nsub_E = len(self.sub_E) if self.sub_E is not None else 0

    def call(self, **over):
        from pose2mesh_release_amd import _lib, evaluate
        a = dict(self.t)
        a.update(self.o)
        v = dict(B=self.B, B_real=self.B_real, nv=self.nv, JA=self.JA, root_A=self.root_A, nsub_A=self.nsub_A, JE=self.JE,
                 root_E=self.root_E, nsub_E=self.nsub_E, pa_mesh=self.pa_mesh, n_groups=self.n_groups)
        for q, x in over.items():
            (v if q in v else a)[q] = x
        p = evaluate._p
        return _lib.hip().p2m_mesh_eval(
            p(a["pred"]), p(a["gt"]), v["B"], v["B_real"], v["nv"], self.scale, p(a["ra_ptr"]), p(a["ra_idx"]), p(a["ra_val"]),
            v["JA"], v["root_A"], p(a["sub_A"]), v["nsub_A"], p(a["pja"]), p(a["gja"]), p(a["re_ptr"]), p(a["re_idx"]),
            p(a["re_val"]), v["JE"], v["root_E"], p(a["sub_E"]), v["nsub_E"], p(a["gje"]), v["pa_mesh"], p(a["mpjpe_A"]),
            p(a["mpvpe"]), p(a["mpjpe_E"]), p(a["pa_mpjpe_E"]), p(a["pa_mpvpe"]), p(a["sample_means"]), p(a["group"]),
            v["n_groups"], p(a["totals"]), evaluate._stream())

    def untouched(self):
        torch.cuda.synchronize()
        tot = self.o["totals"]
        return all(bool(torch.isnan(x).all()) for q, x in self.o.items() if q != "totals") and \
            float(tot[:self.n_groups + 1].abs().max()) == 0.0 and bool(torch.isnan(tot[self.n_groups + 1:]).all())


@pytest.mark.parametrize("name,stage_E,pa_mesh", [("full64", True, True), ("long_subsets", True, False), ("nv6", False, False),
                                                  ("given_A64", True, True)])
def test_evaluator_writes_its_rows_and_no_more(hip_libs, name, stage_E, pa_mesh):
    """p2m_mesh_eval with NaN-prefilled outputs of one row more than the batch and B_real = 3 of B = 5: every element the
    contract names is written (rows >= B_real as 0; all five columns of sample_means, 0 for a metric not computed), the rows
    past the end and the outputs of a stage that is off are untouched, the totals' guard row too."""
    x = _Abi(name, stage_E=stage_E, pa_mesh=pa_mesh)
    assert x.call() == 0
    torch.cuda.synchronize()
    B, Br = x.B, x.B_real
    ref = ec.eval_reference(name)
    on = {"mpjpe_A": True, "mpvpe": True, "mpjpe_E": stage_E, "pa_mpjpe_E": stage_E, "pa_mpvpe": pa_mesh, "sample_means": True}
    for q, is_on in on.items():
        o = x.o[q]
        assert bool(torch.isnan(o[B:]).all()), (q, "guard row written")
        if is_on:
            assert bool(torch.isfinite(o[:B]).all()), (q, "not every element written")
            assert float(o[Br:B].abs().max()) == 0.0, (q, "padding rows must be 0")
            if q in ref:
                assert _miss(o[:Br].cpu().numpy(), ref[q][:Br]) <= 1.0, q
        else:
            assert bool(torch.isnan(o).all()), (q, "written although its stage is off")
    sm = x.o["sample_means"][:Br]
    for col, is_on in enumerate((stage_E, stage_E, True, True, pa_mesh)):
        assert bool((sm[:, col] > 0).all()) if is_on else float(sm[:, col].abs().max()) == 0.0, col
    tot = x.o["totals"]
    assert bool(torch.isnan(tot[x.n_groups + 1:]).all()) and float(tot[0, 0]) == Br
    assert tot[1:x.n_groups + 1, 0].tolist() == [1.0, 1.0, 1.0]                      # groups 0, n_groups - 1 = 2, 1 of the real rows


def test_empty_batch_is_a_no_op(hip_libs):
    """B = 0 (valid pointers): status 0, no output and no total is touched.  B_real = 0 of B = 5: outputs 0, totals unchanged."""
    x = _Abi("nv256")
    assert x.call(B=0, B_real=0) == 0
    assert x.untouched()
    assert x.call(B_real=0) == 0
    torch.cuda.synchronize()
    assert all(float(x.o[q][:x.B].abs().max()) == 0.0 for q in x.o if q != "totals")
    assert float(x.o["totals"][:x.n_groups + 1].abs().max()) == 0.0 and bool(torch.isnan(x.o["totals"][x.n_groups + 1:]).all())


def test_refusals_leave_the_outputs_alone(hip_libs):
    """Arguments the C ABI refuses (beyond those of the Python layer): a non-zero status, a message, and every output still
    at its sentinel.  The buffers are sized for the refused shape, so nothing depends on the refusal for its bounds."""
    from pose2mesh_release_amd import _lib, loss, synth
    lib = _lib.hip()

    def refused(x, **over):
        rc = x.call(**over)
        assert rc != 0 and lib.p2m_last_error_string(), over
        assert x.untouched(), over
    x = _Abi("full64", slack=1)                                # JA = 64 -> 65: a 65-row regressor, outputs of 65 columns
    tab = loss._regressor_tables(synth.synthetic_regressor(65, x.nv, 3), x.nv)
    refused(x, JA=65, ra_ptr=_cu(tab["jr_ptr"]), ra_idx=_cu(tab["jr_idx"]), ra_val=_cu(tab["jr_val"]))
    refused(x, JE=65, re_ptr=_cu(tab["jr_ptr"]), re_idx=_cu(tab["jr_idx"]), re_val=_cu(tab["jr_val"]))
    refused(x, root_A=64)
    refused(x, root_E=64)
    refused(x, root_A=-1)
    sub65 = _cu(np.arange(65, dtype=np.int32) % 64)
    refused(x, sub_A=sub65, nsub_A=65)
    refused(x, sub_E=sub65, nsub_E=65)
    refused(x, sub_A=sub65, nsub_A=0)
    refused(x, re_ptr=None)                                    # JE > 0 with a null regressor
    refused(x, re_val=None)
    refused(x, pa_mpvpe=None)                                  # pa_mesh without its output
    refused(x, sample_means=None)                              # totals without sample_means
    refused(x, n_groups=-1)
    refused(x, B_real=x.B + 1)
    refused(x, B_real=-1)
    refused(x, nv=0)
    refused(x, ra_ptr=None)                                    # stage A: no regressor and no joints
    refused(x, mpvpe=None)
    assert x.call() == 0 and not x.untouched()                 # (the same call without an override is accepted)
    # p2m_rigid_align
    A = _cu(ec.align_case("tail17_nb7")["A"])
    nan = float("nan")
    c, R, t, A2 = (torch.full(s, nan, device="cuda") for s in ((7,), (7, 9), (7, 3), (7, 17, 3)))
    for bad in (dict(N=0), dict(N=-1), dict(nb=-1), dict(c=None), dict(R=None), dict(t=None), dict(A=None), dict(B=None)):
        a = dict(A=A, B=A, nb=7, N=17, c=c, R=R, t=t, A2=A2)
        a.update(bad)
        assert _abi_rigid(**a) != 0 and lib.p2m_last_error_string(), bad
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in (c, R, t, A2)), bad
    assert _abi_rigid(A, A, 7, 17, c, R, t, None) == 0         # A2 is optional
    torch.cuda.synchronize()
    assert bool(torch.isfinite(c).all()) and bool(torch.isnan(A2).all())
