"""CPU: the case table of tests/test_gpu_posenet_edges.py (tests/posenet_ref.py), audited with the restatements alone - that the
closed-form backward is the float64 autograd of the forward, that every case reaches the trip of pass 1, the clamp pattern, the
tile pass and the column quads it is named for, and that the float64 reference alone keeps the ReLU kink out of the comparison
(at most KINK_CAP elements per case, nch and variant, with the seeds recorded in posenet_ref.EDGE_SEEDS).  A GPU test that
passes on a case which never reached the arm it names would pin nothing.  Every figure is printed (pytest -s / -rP)."""
import pytest
import torch

import posenet_ref as pr

# case -> trips of pass 1, row groups that make the last trip, live rows per thread on it, clamped loads on it, padding rows on
# it, tile passes, rows of the last pass, blocks, live quads of the last block, B odd
EXPECT = {
    (128, 0, 32):    (1, 32, {4}, 0, 0, 1, 128, 1, 8, False),
    (129, 0, 36):    (2, 1, {1}, 3, 0, 1, 129, 2, 1, True),
    (132, 129, 36):  (2, 4, {1}, 12, 3, 1, 132, 2, 1, False),
    (256, 0, 32):    (2, 32, {4}, 0, 0, 1, 256, 1, 8, False),
    (257, 0, 4):     (3, 1, {1}, 3, 0, 2, 1, 1, 1, True),
    (260, 257, 68):  (3, 4, {1}, 12, 3, 2, 4, 3, 1, False),
    (516, 513, 36):  (5, 4, {1}, 12, 3, 3, 4, 2, 1, False),
    (64, 0, 28):     (1, 32, {2}, 64, 0, 1, 64, 1, 7, False),
    (40, 37, 4):     (1, 32, {1, 2}, 88, 3, 1, 40, 1, 1, False),
}


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def test_table_is_complete():
    assert set(EXPECT) == set(pr.EDGE_CASES) and len(pr.EDGE_CASES) == 9
    assert set(pr.ARM_SHAPES) <= set(pr.EDGE_CASES) and pr.NCH == (1, 3) and len(pr.PN_VARIANTS) == 5
    assert (pr.PN_COLS, pr.PN_RG, pr.PN_TROWS, pr.TRIP_ROWS) == (32, 32, 256, 128)
    for B, Br, F in pr.EDGE_CASES:
        assert F % 4 == 0 and 0 <= Br <= B and 4 * B * F < 150 * 1024          # every [B, F] tensor under 150 KB
    # no shape of the direct tests of tests/test_gpu_amax.py makes a second trip or a second tile pass; the whole-network
    # tests stop at exactly two trips and one pass
    for B in (32, 36, 64):
        assert pr.trips(B, 0) == 1 and pr.tile_passes(B)[0] == 1
    assert pr.trips(256, 0) == 2 and pr.tile_passes(256) == (1, 256)


@pytest.mark.parametrize("B,B_real,F", pr.EDGE_CASES)
def test_case_reaches_its_arm(B, B_real, F):
    Br = B_real or B
    t, groups, live, clamped, pad = pr.last_trip(B, Br)
    npass, last_rows = pr.tile_passes(B)
    nblk, live_q, dead_q = pr.quads(F)
    got = (t, groups, live, clamped, pad, npass, last_rows, nblk, live_q, B % 2 == 1)
    print(f"({B}, {B_real}, {F}): {t} trips ({groups} row groups make the last, {sorted(live)} live rows, {clamped} clamped loads, "
          f"{pad} padding rows on it), {npass} tile passes (last {last_rows} rows), {nblk} blocks, {live_q} live / {dead_q} dead "
          f"quads in the last")
    assert got == EXPECT[(B, B_real, F)], (got, EXPECT[(B, B_real, F)])
    assert t == -(-B // pr.TRIP_ROWS) and npass == -(-B // pr.PN_TROWS) and live_q + dead_q == pr.PN_Q
    # the padding is the tail of the last trip and of the last tile pass
    assert B - Br <= 3 and B - Br <= last_rows


def test_arms_the_table_is_named_for():
    """What the figures mean for the loops they are about."""
    # the second and later trips: only u = 0 is live there in every case that makes one past a full trip
    assert pr.last_trip(129, 129)[2] == {1} and pr.last_trip(128, 128)[2] == {4} and pr.last_trip(256, 256)[2] == {4}
    # (129, 0, 36) and (132, 129, 36): the same 129 samples
    a, b = pr.case_inputs(129, 0, 36, 3), pr.case_inputs(132, 129, 36, 3)
    for k in pr.ROW_TENSORS:
        assert torch.equal(a[k], b[k][..., :129, :]) and (b[k][..., 129:, :] == 0.75).all()
    for k in ("bias", "gamma", "beta", "rm", "rv"):
        assert torch.equal(a[k], b[k])
    # the tile: 256 fills it exactly, 257 puts one row - 260 four, one of them real - into a second pass, 516 four into a third
    assert pr.tile_passes(256) == (1, 256) and pr.tile_passes(257) == (2, 1) and pr.tile_passes(260) == (2, 4)
    assert pr.tile_passes(516) == (3, 4) and 257 - 256 == 1 and 513 - 512 == 1
    # dead quads next to live ones: F = 4 (7 dead), 28 (1 dead), 36 and 68 (a full block first)
    assert [pr.quads(F) for F in (4, 28, 32, 36, 68)] == [(1, 1, 7), (1, 7, 1), (1, 8, 0), (2, 1, 7), (3, 1, 7)]
    # odd B: an odd row stride of aT (no 8-byte alignment of its rows)
    assert [B for B, _, _ in pr.EDGE_CASES if B % 2] == [129, 257]


def _cases():
    return [(B, Br, F, nch) for B, Br, F in pr.EDGE_CASES for nch in pr.NCH]


@pytest.mark.parametrize("B,B_real,F,nch", _cases())
def test_backward_is_the_autograd_of_the_forward(B, B_real, F, nch):
    """bwd_ref against torch's float64 autograd of act_ref, every variant, with and without gamma / beta: 1e-12 relative."""
    Br = B_real or B
    d = pr.case_inputs(B, B_real, F, nch)
    for bias, resid, bn, p_drop in pr.PN_VARIANTS:
        for affine in (True, False):
            z = pr.z_ref(d["P"], Br, d["bias"] if bias else None, d["resid"] if resid else None).requires_grad_(True)
            gam = d["gamma"].double().requires_grad_(True) if affine else None
            bet = d["beta"].double().requires_grad_(True) if affine else None
            rnd = d["rnd"] if (bn and p_drop > 0) else None
            a = pr.act_ref(z, bn, gam, bet, d["rm"], d["rv"], rnd, p_drop)[0]
            ga = d["G"].double().sum(0)[:Br]
            (a * ga).sum().backward()
            add = d["addend"] if resid else None
            gz, dg, db, dbias, _ = pr.bwd_ref(z.detach(), ga, bn, gam, bet, d["rm"], d["rv"], rnd, p_drop, add)
            want = z.grad + (add.double()[:Br] if resid else 0.0)
            errs = {"gz": _rel(gz, want), "dbias": _rel(dbias, want.sum(0))}
            if bn is not None and affine:
                errs["dgamma"], errs["dbeta"] = _rel(dg, gam.grad), _rel(db, bet.grad)
            assert (dg is None) == (bn is None) and (db is None) == (bn is None)
            assert max(errs.values()) <= 1e-12, (bias, resid, bn, p_drop, affine, errs)


@pytest.mark.parametrize("B,B_real,F,nch", _cases())
def test_kink_counts_and_conditioning(B, B_real, F, nch):
    """Per variant: the elements within KINK of the ReLU kink (at most KINK_CAP, from the float64 restatement alone), and the
    error of torch's own fp32 evaluation of the same lines on z and a - what the GPU test's 1e-5 is measured against."""
    Br = B_real or B
    d = pr.case_inputs(B, B_real, F, nch)
    seed = pr.EDGE_SEEDS.get((Br, F, nch), 1)
    for bias, resid, bn, p_drop in pr.PN_VARIANTS:
        r = pr.stage_ref(d, Br, bias, resid, bn, p_drop)
        r32 = pr.stage_ref(d, Br, bias, resid, bn, p_drop, dtype=torch.float32)
        n = int(r["near"].sum())
        ez, ea = float((r32["z"].double() - r["z"]).abs().max()), float((r32["a"].double() - r["a"]).abs().max())
        print(f"({B}, {B_real}, {F}) nch {nch} seed {seed} bias {bias} resid {resid} bn {bn} p_drop {p_drop}: {n} elements within "
              f"{pr.KINK} of the kink; fp32 restatement: z {ez:.2e}, a {ea:.2e}")
        assert n <= pr.KINK_CAP
        assert all(torch.isfinite(v).all() for v in r.values() if torch.is_tensor(v) and v.dtype.is_floating_point)
        assert ez <= 1e-5 and ea <= 1e-5
        if bn == "train":
            # the batch is well conditioned: no column whose samples nearly agree
            assert float(r["invstd"].max()) < 10.0


@pytest.mark.parametrize("B,B_real,F", pr.ARM_SHAPES)
def test_arm_kink_counts(B, B_real, F):
    """The arms of posenet_ref.ARMS at their two shapes: the same cap on the elements at the ReLU kink, from float64 alone."""
    assert B_real > 1 and B > B_real
    for name in pr.ARMS:
        d, Br = pr.arm_inputs(name, B, B_real, F)
        r = pr.arm_ref(name, d, Br)
        n = int(r["near"].sum())
        print(f"({B}, {B_real}, {F}) {name}: {Br} rows, {n} elements within {pr.KINK} of the kink")
        assert n <= pr.KINK_CAP and d["P"].shape[0] == pr.ARMS[name][0]
        assert all(torch.isfinite(v).all() for v in r.values() if torch.is_tensor(v) and v.dtype.is_floating_point)
    # one sample in train mode: variance 0, the pre-activation is beta itself
    d, Br = pr.arm_inputs("one_sample_train", B, B_real, F)
    r = pr.arm_ref("one_sample_train", d, Br)
    assert Br == 1 and torch.equal(r["mean"], r["z"][0]) and float((r["invstd"] - pr.EPS ** -0.5).abs().max()) < 1e-9
    assert torch.equal(r["pre"][0], d["beta"].double())
