"""CPU: the case table of tests/test_gpu_body_caps.py (tests/body_cap_cases.py), audited with the restatements alone - that
every case reaches the loop pass, chunk edge, cap or table shape it is named for, that the host side of BodyModel builds the
tables the kernels expect for it, and that the float64 yardsticks are well conditioned on it, so that a bar of 4 x their fp32
error is a tight one.  A GPU test that passes on a case which never reached the arm it names would pin nothing."""
import functools

import numpy as np
import pytest
import torch

import body_cap_cases as cc
import body_grad_ref
import body_ref
from pose2mesh_release_amd import body, synth

# case -> K, kpad == K, nfold, passes of the fold (1024 threads), of the g_coef loop (192), of the nb loops (64), 3 ntip, 3 JX,
# g_A chunks, dropped chain joints, longest regressor column
EXPECT = {
    "cap_both":    (640, True, 1420, 2, 4, 2, 0, 0, 9, 0, 0),
    "cap_chain":   (640, True, 1420, 2, 4, 2, 0, 0, 9, 0, 0),
    "cap_shape":   (640, True, 676, 1, 4, 10, 0, 0, 1, 0, 0),
    "cap_outputs": (640, True, 1420, 2, 4, 2, 192, 192, 9, 0, 63),
    "fold_1024":   (436, True, 1024, 1, 3, 1, 0, 0, 7, 0, 0),
    "fold_1025":   (437, False, 1025, 2, 3, 1, 0, 0, 7, 0, 0),
    "coef_192":    (192, True, 228, 1, 1, 3, 0, 0, 1, 0, 0),
    "coef_193":    (193, False, 229, 1, 2, 3, 0, 0, 1, 0, 0),
    "j1":          (5, False, 29, 1, 1, 1, 0, 0, 1, 0, 0),
    "k1":          (1, False, 25, 1, 1, 1, 0, 0, 1, 0, 0),
    "j7":          (57, False, 153, 1, 1, 1, 0, 0, 1, 0, 0),
    "j8":          (64, True, 172, 1, 1, 1, 0, 0, 2, 0, 0),
    "drop_joints": (217, False, 517, 1, 2, 1, 6, 0, 4, 21, 0),
    "tips_only":   (217, False, 517, 1, 2, 1, 9, 0, 4, 24, 0),
    "tail_22":     (145, False, 349, 1, 1, 1, 66, 66, 3, 0, None),
    "reg_zero":    (217, False, 517, 1, 2, 1, 0, 15, 4, 0, 0),
    "reg_rows":    (217, False, 517, 1, 2, 1, 0, 12, 4, 0, 2),
    "col_64":      (19, False, 55, 1, 1, 1, 0, 192, 1, 0, 64),
    "nb0":         (9, False, 45, 1, 1, 0, 0, 0, 1, 0, 0),
}


def _body_model(name, **kw):
    c, m = cc.CASES[name], cc.case_model(name)
    a = dict(betas=m["betas"], tip_vertices=m.get("tip_vertices"), joint_order=m.get("joint_order"), extra_regressor=c["extra"])
    a.update(kw)
    return body.BodyModel(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["weights"], m["parents"], **a)


def test_table_is_complete():
    assert set(EXPECT) == set(cc.NAMES)
    assert cc.B == body.SAMPLE_TILE + 1 and all(c["B"] == cc.B for c in cc.CASES.values())
    assert (cc.VT, cc.TB, cc.JMAX, cc.KMAX) == (body.VERTEX_TILE, body.SAMPLE_TILE, body.MAX_JOINTS, body.MAX_COEFFS)


@pytest.mark.parametrize("name", cc.NAMES)
def test_case_reaches_its_arm(name):
    c = cc.CASES[name]
    J, nb, V = c["J"], c["nb"], c["V"]
    K = cc.n_coef(J, nb)
    ntip, JX = len(c["tips"] or ()), 0 if c["extra"] is None else c["extra"].shape[0]
    slots = cc.jslot(name)
    col = 0 if c["extra"] is None else int(np.count_nonzero(c["extra"], axis=0).max())
    got = (K, cc.kpad(K) == K, cc.n_fold(J, K), cc.passes(cc.n_fold(J, K), cc.FOLD_THREADS), cc.passes(K, cc.NT),
           cc.passes(nb, 64), 3 * ntip, 3 * JX, cc.n_chunks(J), int((slots < 0).sum()), col)
    want = EXPECT[name]
    assert got[:10] == want[:10] and (want[10] is None or got[10] == want[10]), (got, want)
    assert 1 <= J <= cc.JMAX and 1 <= K <= cc.KMAX and ntip <= cc.JMAX and JX <= cc.JMAX
    assert cc.skin_lds(J, K) <= 65536 and cc.bwd_lds(J, K) <= 65536


def test_caps_and_edges():
    """What the table's figures mean for the loops they are about."""
    K = 640
    # both skin kernels at their LDS peak: the byte counts body_skin_lds and body_bwd_lds give at the caps
    for name in ("cap_both", "cap_chain", "cap_outputs"):
        assert (cc.CASES[name]["J"], cc.n_coef(cc.CASES[name]["J"], cc.CASES[name]["nb"])) == (cc.JMAX, cc.KMAX)
    assert cc.skin_lds(64, K) == 51328 and cc.bwd_lds(64, K) == 63872
    assert cc.skin_lds(2, K) < 51328 and cc.bwd_lds(2, K) < 63872        # cap_shape: K alone does not reach the peak
    # the g_coef loop at K = 640: three full passes of 192 and a fourth of 64
    assert K - 3 * cc.NT == 64
    # the fold: SMPL (nfold 517) stays in the first pass; fold_1024 fills it exactly, fold_1025 puts one element - a g_coef
    # one, index nfold - 1 >= nA - into the second; the cap cases put g_coef elements only there (nA = 780 < 1024)
    assert cc.n_fold(24, 217) == 517
    assert cc.n_fold(48, 436) == cc.FOLD_THREADS and cc.n_fold(48, 437) - cc.FOLD_THREADS == 1 and 12 * 49 < 1024
    assert 12 * 65 == 780 and cc.n_fold(64, 640) - cc.FOLD_THREADS == 396
    # the tail: 63 elements (JX = 21) were one short of a second pass of its 64 threads; 22 put 2 elements there, 64 make
    # exactly three passes
    assert 3 * 21 < 64 < 3 * 22 == 66 and 3 * 64 == 3 * 64
    # the g_A chunk walk (8 rows a chunk, J + 1 rows): J = 7 has the weight-1 row as the last of chunk 0, J = 8 alone in
    # chunk 1 (an odd chunk: threads 96..191), J = 64 as the first of chunk 8, the ninth
    assert divmod(7, 8) == (0, 7) and cc.n_chunks(7) == 1
    assert divmod(8, 8) == (1, 0) and cc.n_chunks(8) == 2
    assert divmod(64, 8) == (8, 0) and cc.n_chunks(64) == 9
    # J = 1: no chain step, no pose directions, K = nb
    for name in ("j1", "k1"):
        c = cc.CASES[name]
        assert c["J"] == 1 and cc.n_coef(1, c["nb"]) == c["nb"] and cc.case_model(name)["posedirs"].shape[2] == 0
    assert cc.CASES["k1"]["V"] == 1 and cc.COMPANION["k1"] == (1, 1, 65)
    # the chain of depth 63, centred on its deepest joint
    m = cc.case_model("cap_chain")
    assert m["parents"] == [-1] + list(range(63)) and cc.CASES["cap_chain"]["runs"] == (("", "given", False, 63),)
    assert cc.case_model("cap_both")["parents"] != m["parents"]
    # nb loops beyond one wave
    assert cc.CASES["cap_shape"]["nb"] == 631 and cc.CASES["coef_192"]["nb"] == 183 and cc.CASES["cap_both"]["nb"] == 73


def test_output_tables():
    # cap_outputs: 64 tips with the last vertex, the first and a repeated one; all 128 outputs, shuffled; 64 extra joints with
    # an empty row, a full row and one vertex in every other row
    c = cc.CASES["cap_outputs"]
    V = c["V"]
    assert len(c["tips"]) == 64 and c["tips"][:4] == [V - 1, 0, 5, 5] and all(0 <= t < V for t in c["tips"])
    assert sorted(c["order"]) == list(range(128)) and c["order"] != list(range(128)) and cc.n_joints_out("cap_outputs") == 128
    s = cc.jslot("cap_outputs")
    assert (s >= 0).all() and (s != np.arange(64)).any()
    n = np.count_nonzero(c["extra"], axis=1)
    assert c["extra"].shape == (64, V) and n[10] == 0 and n[20] == V and (np.delete(n, [10, 20]) <= 7).all()
    assert np.count_nonzero(c["extra"][:, 77]) == 63                        # every row but the empty one
    # col_64: a vertex used by all 64 extra joints, the longest column walk of the vertex stage
    assert np.count_nonzero(cc.CASES["col_64"]["extra"][:, 7]) == 64
    # drop_joints: 3 of 24 chain joints kept, chain joint 5 in slot 0, a tip in slot 1; output 3 is chain joint 23, output 0
    # is chain joint 5 and not the root
    s = cc.jslot("drop_joints")
    assert {j: int(s[j]) for j in np.flatnonzero(s >= 0)} == {0: 2, 5: 0, 23: 3}
    assert cc.CASES["drop_joints"]["order"] == [5, 24, 0, 23, 25] and cc.n_joints_out("drop_joints") == 5
    assert [(r[3], r[2]) for r in cc.CASES["drop_joints"]["runs"]] == [(3, False), (0, False)]
    for label, joint in (("c3", 23), ("c0", 5)):
        r = cc.run("drop_joints", label)
        assert _body_model("drop_joints", center_idx=r["center_idx"]).center_joint == joint and r["trans"] is None
    # tips_only: no chain joint is an output
    assert (cc.jslot("tips_only") == -1).all() and cc.n_joints_out("tips_only") == 3
    # tail_22
    c = cc.CASES["tail_22"]
    assert len(c["tips"]) == 22 and c["extra"].shape == (22, 65) and cc.n_joints_out("tail_22") == 16 + 22
    # reg_zero, reg_rows
    assert not cc.CASES["reg_zero"]["extra"].any()
    R = cc.CASES["reg_rows"]["extra"]
    assert np.count_nonzero(R, axis=1).tolist() == [0, 1, 65, 3] and R[1, 64] == 1 and (R[3] < 0).sum() == 1
    assert cc.row_sum_bound(R) == pytest.approx(1.6) and cc.row_sum_bound(cc.CASES["reg_zero"]["extra"]) == 0.0


@pytest.mark.parametrize("name", cc.NAMES)
def test_host_tables(name):
    """BodyModel constructs on the host; the coefficient-major table is [K, 3 V], the backward's vertex-major copy
    [3 V, kpad] with zero padding, and the column table rebuilds the regressor."""
    c = cc.CASES[name]
    J, nb, V = c["J"], c["nb"], c["V"]
    K = cc.n_coef(J, nb)
    model = _body_model(name)
    assert (model.J, model.nb, model.V, model.NJ) == (J, nb, V, cc.n_joints_out(name))
    assert model.n_tips == len(c["tips"] or ()) and model.JX == (0 if c["extra"] is None else c["extra"].shape[0])
    assert model._host["dirs"].shape == (K, 3 * V) and np.array_equal(model._host["jslot"], cc.jslot(name))
    g = model._grad_tables(torch.device("cpu"))
    dt = g["dirs_t"].numpy()
    assert dt.shape == (3 * V, cc.kpad(K)) and np.array_equal(dt[:, :K], model._host["dirs"].T) and not dt[:, K:].any()
    if c["extra"] is not None:
        ptr, idx, val = (g[k].numpy() for k in ("xc_ptr", "xc_idx", "xc_val"))
        R = np.zeros_like(c["extra"])
        for v in range(V):
            assert (np.diff(idx[ptr[v]:ptr[v + 1]]) > 0).all()                      # joints ascending
            R[idx[ptr[v]:ptr[v + 1]], v] = val[ptr[v]:ptr[v + 1]]
        assert ptr.shape == (V + 1,) and np.array_equal(R, c["extra"])
        assert int(np.diff(ptr).max()) == int(np.count_nonzero(c["extra"], axis=0).max())
        # the row table of the forward: never empty, row lengths those of the regressor
        assert model._host["xr_idx"].size >= 1 and model._host["xr_val"].size >= 1
        assert np.array_equal(np.diff(model._host["xr_ptr"]), np.count_nonzero(c["extra"], axis=1))


def test_nb0_constructs_and_uploads_no_empty_table():
    """A model without a shape space is accepted: the host tables that have no element (the stored betas, the rest joints'
    shape directions) stay empty on the host and reach the device as one-element dummies, so that no kernel argument is a
    null pointer; [B, 0] betas are accepted as an input."""
    model = _body_model("nb0")
    assert model.nb == 0 and model._host["betas"].shape == (0,) and model._host["js"].shape == (2, 3, 0)
    assert model._host["dirs"].shape == (9, 3 * 65)
    dev = model._device_tables(torch.device("cpu"))
    assert dev["betas"].numel() == 1 and dev["js"].numel() == 1 and dev["dirs"].shape == (9, 3 * 65)
    assert all(t.numel() >= 1 for t in dev.values())
    assert int(body._lib.hip().p2m_body_workspace(cc.B, 2, 0)) == cc.B * (12 + 24 + 4) * 4
    with pytest.raises(ValueError):
        _body_model("nb0", betas=np.zeros(1, np.float32))
    # K = 0 stays out: J = 1 without a shape space has no coefficient at all
    m = cc.model(1, 0, 65)
    with pytest.raises(ValueError):
        body.BodyModel(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["weights"], m["parents"])


@functools.lru_cache(maxsize=None)
def _conditioning(name, label):
    r = cc.run(name, label, companion=name in cc.COMPANION)
    m, reg = r["model"], r["extra_reg"]
    args = (r["pose"], r["betas"], r["trans"], r["center_idx"])
    fwd = body_ref.err32(m, *args)
    Bn, V = r["pose"].shape[0], m["num_vertex"]
    NJ = cc.n_joints_out(name)
    shapes = [(Bn, V, 3), (Bn, NJ, 3)] + ([(Bn, reg.shape[0], 3)] if reg is not None else [])
    coeffs = body_grad_ref.loss_coeffs(cc.CASES[name]["seed"], shapes)[0]
    g8 = body_grad_ref.grads(m, *args, reg, None, coeffs)
    g4 = body_grad_ref.grads(m, *args, reg, None, coeffs, dtype=torch.float32)
    return m, fwd, g8, g4


@pytest.mark.parametrize("name,label", cc.run_ids())
def test_references_are_well_conditioned(name, label):
    """The fp32 run of both restatements against their float64 run: finite, the forward's worst per-vertex L2 under 1e-4 of
    the model's extent, every gradient row error under 1e-4 - so 4 x these figures is a bar an fp32-class kernel can be held
    to and a wrong one cannot meet."""
    m, fwd, g8, g4 = _conditioning(name, label)
    extent = float(np.ptp(np.asarray(m["v_template"], np.float64), axis=0).max())
    print(f"{name} {label}: forward fp32 error {fwd:.3e} of extent {extent:.2f}")
    assert np.isfinite(fwd) and extent > 0.5 and fwd <= 1e-4 * extent
    for n, a, b in zip(("pose", "betas", "trans"), g4, g8):
        assert (a is None) == (b is None)
        if b is None:
            continue
        assert np.isfinite(a).all() and np.isfinite(b).all()
        if b.shape[1] == 0:                                                 # nb = 0: an empty gradient
            assert n == "betas" and a.shape == b.shape
            continue
        e = body_grad_ref.row_err(a, b)
        print(f"{name} {label} g_{n}: fp32 row error {e:.3e}")
        assert np.abs(b).reshape(b.shape[0], -1).max(axis=1).min() > 0 and e <= 1e-4, (n, e)


def test_one_vertex_pose_gradient_vanishes():
    """k1: one joint regressed from one vertex is that vertex, so no output depends on the pose and the float64 pose gradient
    is zero to rounding (1e-12 of the moment that cancels in it); the betas and trans gradients are live.  No other case has
    such a gradient: all of them take the row error relative to |g64|, which test_references_are_well_conditioned shows to
    be non-zero in every row."""
    r = cc.run("k1", "")
    m = r["model"]
    assert m["J_regressor"].tolist() == [[1.0]] and m["weights"].tolist() == [[1.0]]
    coeffs = body_grad_ref.loss_coeffs(cc.CASES["k1"]["seed"], [(cc.B, 1, 3), (cc.B, 1, 3)])[0]
    g8 = body_grad_ref.grads(m, r["pose"], r["betas"], r["trans"], None, None, None, coeffs)
    scale = cc.vanishing_pose_gradient_scale("k1", g8)
    assert scale.shape == (cc.B,) and (scale > 0.1).all()
    assert (np.linalg.norm(g8[0], axis=1) <= 1e-12 * scale).all()
    assert (np.abs(g8[1]).max(axis=1) > 0).all() and (np.abs(g8[2]).max(axis=1) > 0).all()
    assert all(cc.vanishing_pose_gradient_scale(n, g8) is None for n in cc.NAMES if n != "k1")


def test_no_fixture_drift():
    """The general builder is a separate generator: synth.body_model still makes the model the committed fixtures were made
    with (the checksum tests/golden/body_smpl.npz stores for V = 257, seed 0)."""
    import body_cases
    want = float(body_cases.fixture("smpl")["checksum_smpl"])
    assert int(body_cases.fixture("smpl")["num_vertex"]) == 257 and int(body_cases.fixture("smpl")["seed"]) == 0
    got = synth.body_model("smpl", 257)["checksum"]
    assert abs(got - want) <= 1e-9 * abs(want)
