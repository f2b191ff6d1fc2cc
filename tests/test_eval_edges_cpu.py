"""CPU: the audit of tests/eval_cases.py, the tables that tests/test_gpu_eval_edges.py runs through csrc/eval.hip.

  - the tables do hold the sizes at which the kernels change path (second trips of the joint-fill and fold loops, the
    stage-E wave full / nearly empty, the wave kernel's tails, the dispatch boundary), with roots that tell A from E;
  - every alignment case's class agrees with its spectrum (eval_ref.alignment_spectrum);
  - the float64 reference alone stays inside the bars of the `unique` class when every input moves by one fp32 ulp (a bar
    the reference cannot hold against its own input rounding would test nothing);
  - faults planted in a copy of the restatement (roots swapped, root after the subset, no det-sign fix, sample variance,
    mean over J) leave the bars on the cases meant to catch them."""
import numpy as np
import pytest

import eval_cases as ec
import eval_ref

R_BAR, C_BAR, T_BAR = 1e-6, 1e-6, 4e-7           # tests/test_gpu_eval.py: R per element, c relative, t / A2 x max|B|


def test_tables_hold_the_launch_edges():
    ev = ec.EVAL_CASES
    nsE = [len(k["sub_E"]) if k["sub_E"] is not None else k["JE"] for k in ev]
    assert any(k["JA"] >= 43 for k in ev) and any(k["JA"] == 43 for k in ev)       # 2 * 43 * 3 = 258: the first second trip
    assert any(k["JE"] == 42 for k in ev) and any(k["JE"] >= 43 for k in ev)
    assert {64, 1, 2, 3} <= set(nsE)
    assert any(k["sub_A"] is not None and len(k["sub_A"]) == 64 > k["JA"] for k in ev)
    for k in ev:
        assert k["root_A"] != k["root_E"] and k["root_A"] > 0 and k["root_E"] > 0, k["name"]
        assert 0 <= k["root_A"] < k["JA"] and 0 <= k["root_E"] < k["JE"]
        for sub, J in ((k["sub_A"], k["JA"]), (k["sub_E"], k["JE"])):
            assert sub is None or (1 <= len(sub) <= 64 and min(sub) >= 0 and max(sub) < J)
    for name in ("subE1", "subE2", "subE3"):
        k = ec.eval_case(name)
        assert k["root_E"] not in k["sub_E"]
    k = ec.eval_case("long_subsets")
    assert len(set(k["sub_A"])) < len(k["sub_A"]) and len(set(k["sub_E"])) < len(k["sub_E"])
    assert k["sub_E"][k["root_E"]] != k["root_E"]             # (a root taken after the subset is another joint)
    assert {k["nv"] for k in ev} == {6, 63, 256, 257, 600}
    assert any(not k["reg_A"] and k["JA"] == 64 for k in ev)
    al = ec.align_cases()
    assert set(ec.ALIGN_N) <= {k["A"].shape[1] for k in al if k["cls"] == "unique"}
    assert {1, 2, 3} <= {k["A"].shape[0] % 4 for k in al if k["A"].shape[1] <= 256 and k["cls"] == "unique"}
    assert any(k["A"].shape == (3, 257, 3) for k in al)
    assert {1, 2} <= {k["A"].shape[1] for k in al}
    assert len({k["name"] for k in al}) == len(al)
    for k in al:
        assert k["A"].dtype == np.float32 and k["A"].shape == k["B"].shape
        fin = np.isfinite(k["A"]) & np.isfinite(k["B"])
        if not k["big"]:
            assert max(np.abs(k["A"][fin]).max(), np.abs(k["B"][fin]).max()) <= ec.COORD_MAX, k["name"]
    assert max(ec.TOTALS_N_GROUPS) >= 42 and {0, 41, 42} <= set(ec.TOTALS_N_GROUPS)   # (41 + 1) * 6 = 252, (42 + 1) * 6 = 258
    for G in ec.TOTALS_N_GROUPS:
        ids = ec.totals_groups(G)
        flat = [g for call in ids[:2] for g in call]
        assert [len(c) for c in ids] == [B for B, _ in ec.TOTALS_CALLS]
        assert -1 in flat and G in flat and ec.INT32_MAX in flat                    # (n_groups itself is out of range)
        assert G == 0 or G - 1 in flat                                              # the highest valid group


def test_classes_match_their_spectra():
    for k in ec.align_cases():
        spec = [eval_ref.alignment_spectrum(a, b) for a, b in zip(k["A"], k["B"])]
        for i, s in enumerate(spec):
            what = (k["name"], i, s["gap"])
            if i in k["bad"]:
                assert k["cls"] == "nonfinite" and (s["varP"] == 0.0 or not np.isfinite(s["gap"])), what
            elif k["cls"] in ("unique", "nonfinite"):
                if k["compare_R"]:
                    assert s["gap"] >= ec.UNIQUE_GAP_MIN and s["varP"] > 0, what
                else:                                          # constant B: H = 0 exactly
                    assert s["s"][0] == 0.0 and s["varP"] > 0, what
            else:
                assert s["varP"] > 0 and (k["big"] or s["gap"] <= ec.FREE_GAP_MAX), what
        if k["cls"] == "nonfinite":
            assert len(k["bad"]) >= 1
    by = {k["name"]: k for k in ec.align_cases()}
    spec = [eval_ref.alignment_spectrum(a, b) for a, b in zip(by["mirrored_cube"]["A"], by["mirrored_cube"]["B"])]
    assert all(s["sign"] < 0 and abs(s["s"][1] - s["s"][2]) <= 1e-7 * s["s"][0] for s in spec)   # (fp32 rounding of the turned ones)
    assert spec[0]["gap"] == 0.0                               # (the integer one: exactly)
    for name in ("mirrored64", "mirrored257", "near_mirrored_cube"):
        assert all(eval_ref.alignment_spectrum(a, b)["sign"] < 0 for a, b in zip(by[name]["A"], by[name]["B"])), name
    assert all(eval_ref.alignment_spectrum(a, b)["gap"] < 1e-12 for n in ("collinearA17", "collinear_both257", "collinearB17",
               "two_points") for a, b in zip(by[n]["A"], by[n]["B"]))
    assert all(1e-9 < eval_ref.alignment_spectrum(a, b)["gap"] < 1e-5
               for a, b in zip(by["near_collinearA17"]["A"], by["near_collinearA17"]["B"]))


def test_spectrum_and_optimum_on_known_sets():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((40, 3)) * np.array([300.0, 200.0, 100.0])
    Q = ec._rot(rng)
    B = 1.25 * A @ Q.T + np.array([5.0, -7.0, 11.0])
    s = eval_ref.alignment_spectrum(A, B)
    ev = np.sort(np.linalg.eigvalsh(np.cov(A.T, bias=True)))[::-1] * 1.25
    assert np.allclose(s["s"], ev, rtol=1e-12) and s["sign"] == 1.0 and abs(s["varP"] - np.var(A, axis=0).sum()) < 1e-9
    assert abs(s["gap"] - 2 * (ev[1] + ev[2]) / ev[0]) < 1e-12
    c, rms = eval_ref.optimum(A, B)
    assert abs(c - 1.25) < 1e-12 and rms < 1e-9
    assert eval_ref.alignment_spectrum(A, B * np.array([1.0, 1.0, -1.0]))["sign"] == -1.0
    # the residual does not depend on which optimal rotation is taken: a collinear A turned about its line
    k = ec.align_case("collinearA17")
    a, b = k["A"][0].astype(np.float64), k["B"][0].astype(np.float64)
    c, R, t = eval_ref.rigid_transform_3D(a, b)
    d = a[1] - a[0]
    d /= np.linalg.norm(d)
    K = np.array([[0, -d[2], d[1]], [d[2], 0, -d[0]], [-d[1], d[0], 0]])
    R2 = R @ (np.eye(3) + np.sin(1.0) * K + (1 - np.cos(1.0)) * K @ K)
    res = [np.sqrt(np.mean(np.sum(((c * r @ (a - a.mean(0)).T).T + b.mean(0) - b) ** 2, axis=1))) for r in (R, R2)]
    assert abs(res[0] - res[1]) < 1e-9 and abs(res[0] - eval_ref.optimum(a, b)[1]) < 1e-9 and np.abs(R - R2).max() > 0.1


def _ulp_moved(x, rng):
    up = rng.integers(0, 2, x.shape).astype(bool)
    return np.where(up, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))).astype(np.float32)


def test_reference_holds_the_unique_bars_against_one_input_ulp(capsys):
    """Every coordinate of every `unique` case moved by one fp32 ulp (seeded signs): eval_ref's R, c, t, A2 move by at most
    half their bar.  The kernels see exactly the fp32 inputs, so this is no error of theirs; it shows that the bars are
    coarser than the conditioning of the cases, so that a miss is the kernel's.  A case over 0.5 belongs in `free`."""
    worst = {"R": (0.0, ""), "c": (0.0, ""), "t": (0.0, ""), "A2": (0.0, "")}
    lines = []
    for k in ec.align_cases():
        if k["cls"] != "unique":
            continue
        rng = np.random.default_rng(5)
        ref = ec.align_reference(k["name"])
        c, R, t, A2 = eval_ref.batch_rigid(_ulp_moved(k["A"], rng), _ulp_moved(k["B"], rng))
        sc = float(np.abs(k["B"]).max())
        share = {"t": np.abs(t - ref["t"]).max() / (T_BAR * sc), "A2": np.abs(A2 - ref["A2"]).max() / (T_BAR * sc)}
        if k["compare_R"]:
            share["R"] = np.abs(R - ref["R"]).max() / R_BAR
            share["c"] = (np.abs(c - ref["c"]) / np.abs(ref["c"])).max() / C_BAR
        else:
            share["c"] = np.abs(c - ref["c"]).max() / C_BAR      # constant B: c = 0, the bar is absolute
        lines.append(f"{k['name']:24s} " + " ".join(f"{q} {share[q]:6.3f}" for q in ("R", "c", "t", "A2") if q in share))
        for q, v in share.items():
            if v > worst[q][0]:
                worst[q] = (float(v), k["name"])
            assert v <= 0.5, (k["name"], q, v)
    with capsys.disabled():
        print("\nshare of the bar moved by one input ulp (eval_ref alone):")
        print("\n".join(lines))
        print("largest: " + ", ".join(f"{q} {v:.3f} ({n})" for q, (v, n) in worst.items()))


def test_weakly_fixed_cases_are_not_in_unique():
    """The cases the sensitivity rule moved to `free` although their gap is not 0: one input ulp moves eval_ref's R by more
    than its bar, so R is no yardstick there (the nearly symmetric mirrored cube, the sets 1e6 from the origin)."""
    for name in ("near_mirrored_cube", "offset1e6_17", "offset1e6_257", "near_collinearA17"):
        k = ec.align_case(name)
        assert k["cls"] == "free"
        rng = np.random.default_rng(5)
        R = eval_ref.batch_rigid(_ulp_moved(k["A"], rng), _ulp_moved(k["B"], rng))[1]
        assert np.abs(R - ec.align_reference(name)["R"]).max() > R_BAR, name


# ---- planted faults --------------------------------------------------------------------------------------------------------
def _rigid_faulty(A, B, fault):
    """eval_ref.rigid_transform_3D with one planted fault."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    cA, cB = A.mean(axis=0), B.mean(axis=0)
    H = (A - cA).T @ (B - cB) / A.shape[0]
    U, s, V = np.linalg.svd(H)
    R = V.T @ U.T
    if np.linalg.det(R) < 0 and fault != "no_det_fix":
        s[-1] = -s[-1]
        V[2] = -V[2]
        R = V.T @ U.T
    varP = np.var(A, axis=0, ddof=1 if fault == "sample_variance" else 0).sum()
    c = np.sum(s) / varP
    return c, R, cB - (c * R) @ cA


def _mesh_eval_faulty(name, fault):
    """eval_ref.mesh_eval on an evaluator case with one planted fault -> (per-sample dict, sample means [B, 5])."""
    k, z = ec.eval_case(name), ec.eval_inputs(name)
    root_A, root_E = (k["root_E"], k["root_A"]) if fault == "roots_swapped" else (k["root_A"], k["root_E"])
    pred, gt = z["pred"].astype(np.float64), z["gt"].astype(np.float64) * z["scale"]
    res = {q: [] for q in eval_ref.EVAL_KEYS}

    def align(a, b):
        c, R, t = eval_ref.rigid_transform_3D(a, b)
        return (c * R @ a.T).T + t
    for n in range(pred.shape[0]):
        mo, mg = pred[n], gt[n]
        jo = z["pja"][n].astype(np.float64) if z["pja"] is not None else z["RA"].astype(np.float64) @ mo
        jg = z["gja"][n].astype(np.float64) if z["gja"] is not None else z["RA"].astype(np.float64) @ mg
        mo, mg = mo - jo[root_A], mg - jg[root_A]
        po, pg = jo - jo[root_A], jg - jg[root_A]
        if k["sub_A"] is not None:
            po, pg = po[k["sub_A"]], pg[k["sub_A"]]
        res["mpjpe_A"].append(np.linalg.norm(po - pg, axis=-1))
        res["mpvpe"].append(np.linalg.norm(mo - mg, axis=-1).mean())
        res["pa_mpvpe"].append(np.linalg.norm(align(mo, mg) - mg, axis=-1).mean())
        RE = z["RE"].astype(np.float64)
        eo = RE @ mo
        eg = z["gje"][n].astype(np.float64) if z["gje"] is not None else RE @ mg
        if fault == "root_after_subset" and k["sub_E"] is not None:
            eo, eg = eo[k["sub_E"]], eg[k["sub_E"]]
            eo, eg = eo - eo[root_E], eg - eg[root_E]
        else:
            eo, eg = eo - eo[root_E], eg - eg[root_E]
            if k["sub_E"] is not None:
                eo, eg = eo[k["sub_E"]], eg[k["sub_E"]]
        res["mpjpe_E"].append(np.linalg.norm(eo - eg, axis=-1))
        res["pa_mpjpe_E"].append(np.linalg.norm(align(eo, eg) - eg, axis=-1))
    res = {q: np.array(v) for q, v in res.items()}
    means = ec.sample_means(res)
    if fault == "mean_over_J":
        means[:, 0] = res["mpjpe_E"].sum(axis=1) / k["JE"]
        means[:, 1] = res["pa_mpjpe_E"].sum(axis=1) / k["JE"]
        means[:, 2] = res["mpjpe_A"].sum(axis=1) / k["JA"]
    return res, means


def _eval_miss(name, fault):
    """Largest distance of the faulty copy from eval_ref over every per-joint, per-sample and mean value, in bars."""
    res, means = _mesh_eval_faulty(name, fault)
    ref = ec.eval_reference(name)
    worst = max(np.abs(res[q] - ref[q]).max() for q in ref)
    return max(worst, np.abs(means - ec.sample_means(ref)).max()) / ec.BAR_MM


def test_the_copy_without_a_fault_is_the_reference():
    for k in ec.EVAL_CASES:
        if k["name"] != "subE1":
            assert _eval_miss(k["name"], None) <= 1e-6, k["name"]
    for name in ("generic3", "mirrored64", "generic600"):
        k = ec.align_case(name)
        for i in range(k["A"].shape[0]):
            c, R, t = _rigid_faulty(k["A"][i], k["B"][i], None)
            assert abs(c - ec.align_reference(name)["c"][i]) <= 1e-14 * abs(c) and np.array_equal(R, ec.align_reference(name)["R"][i])


def test_planted_faults_leave_the_bars():
    # roots swapped: every case has root_A != root_E; the discriminator pair is the one built for it
    for name in ("roots_3_9", "roots_9_3", "full64", "nv256"):
        assert _eval_miss(name, "roots_swapped") > 100.0, name
    # root taken after the subset: a 64-entry subset whose entry root_E is another joint
    assert _eval_miss("long_subsets", "root_after_subset") > 100.0
    # mean over J instead of over the subset: subsets longer and shorter than the joint count
    for name in ("long_subsets", "subE2", "subE3"):
        assert _eval_miss(name, "mean_over_J") > 100.0, name
    # the alignment's own faults, on the alignment table
    for name in ec.align_names("unique"):
        k, ref = ec.align_case(name), ec.align_reference(name)
        if not k["compare_R"]:
            continue
        N = k["A"].shape[1]
        for i in range(k["A"].shape[0]):
            c = _rigid_faulty(k["A"][i], k["B"][i], "sample_variance")[0]
            assert abs(c - ref["c"][i]) / abs(ref["c"][i]) > 100 * C_BAR, name        # (N - 1) / N, N <= 600
            assert N <= 600
    for name in ("mirrored64", "mirrored257", "near_mirrored_cube"):
        k, ref = ec.align_case(name), ec.align_reference(name)
        for i in range(k["A"].shape[0]):
            c, R, t = _rigid_faulty(k["A"][i], k["B"][i], "no_det_fix")
            assert np.linalg.det(R) < 0 and abs(c - ref["c"][i]) / ref["c"][i] > 1000 * C_BAR, name
            assert np.abs(R - ref["R"][i]).max() > 1000 * R_BAR, name


def test_roots_discriminate():
    """The same data with (root_A, root_E) = (3, 9) and (9, 3): the two references differ by more than 100 bars in every
    metric that depends on a root, so a kernel reading one root for the other cannot pass both."""
    a, b = ec.eval_reference("roots_3_9"), ec.eval_reference("roots_9_3")
    for q in ("mpjpe_A", "mpvpe", "mpjpe_E"):
        assert np.abs(a[q] - b[q]).max() > 100 * ec.BAR_MM, q
    za, zb = ec.eval_inputs("roots_3_9"), ec.eval_inputs("roots_9_3")
    assert np.array_equal(za["pred"], zb["pred"]) and np.array_equal(za["RE"], zb["RE"])


def test_reference_of_the_degenerate_evaluator_cases():
    ref = ec.eval_reference("subE1")
    assert not np.isfinite(ref["pa_mpjpe_E"]).any()            # one joint: varP = 0, the reference's 0 / 0
    assert all(np.isfinite(ref[q]).all() for q in ref if q != "pa_mpjpe_E")
    assert ec.eval_reference("subE2")["pa_mpjpe_E"].max() <= ec.BAR_MM              # two points align exactly
    assert ec.eval_reference("subE3")["pa_mpjpe_E"].max() > ec.BAR_MM
    # 10.24 m on the given ground-truth joints: the joint metrics and the aligned mesh error do not see it, MPVPE does (the
    # ground-truth mesh is centred on the given root joint, data/PW3D/dataset.py:275)
    a, b = ec.eval_reference("shifted_gt_joints"), ec.eval_reference("unshifted_gt_joints")
    for q in ("mpjpe_A", "mpjpe_E", "pa_mpjpe_E", "pa_mpvpe"):
        assert np.abs(a[q] - b[q]).max() <= 1e-6 * ec.BAR_MM, q
    assert (a["mpvpe"] > 10000.0).all() and (b["mpvpe"] < 200.0).all()
    za, zb = ec.eval_inputs("shifted_gt_joints"), ec.eval_inputs("unshifted_gt_joints")
    assert np.array_equal(za["gja"].astype(np.float64) - 10240.0, zb["gja"].astype(np.float64))      # exact in fp32
    assert np.array_equal(za["gje"].astype(np.float64) + 10240.0, zb["gje"].astype(np.float64))
