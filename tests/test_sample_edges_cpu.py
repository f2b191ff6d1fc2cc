"""CPU: the case tables of tests/test_gpu_sample_edges.py, audited with the restatement (tests/sample_ref.py) alone - that the
mesh-arm table reaches what it claims to reach, that the cases at the joint-table caps are sane and show what they are meant
to show, and that the late-zeroing input takes the restatement's fp32 `bad` branch.  A GPU test that passes on a case which
never reached the arm it names would pin nothing; these conditions are on the seeds of tests/sample_cases.py."""
import numpy as np
import pytest

import sample_cases
import sample_ref

OUTS = ("pose2d", "mesh", "lift_pose3d", "reg_pose3d")


def _ref(c, dtype=np.float64, **kw):
    args = dict(rot=c["rot"], flip=c["flip"])
    args.update(kw)
    with np.errstate(all="ignore"):
        return sample_ref.chain(c["verts"], c["focal"], c["princpt"], dtype=dtype, **args, **sample_cases.chain_kwargs(c))


def test_mesh_arm_predictor():
    """Hand-worked lines of the kernel's arm selection: n = 21 floats per sample (nv = 7)."""
    arm = sample_cases.mesh_arm
    assert arm(0x1000, 0x2000, 0, 7) == (True, 0, 5, 1)           # both on a line: no head, 5 float4, 1 left
    assert arm(0x1000, 0x2000, 1, 7) == (True, 3, 4, 2)           # sample 1 starts 84 bytes in: offset 4 -> head 3
    assert arm(0x1004, 0x2004, 0, 7) == (True, 3, 4, 2)
    assert arm(0x1008, 0x2008, 0, 7) == (True, 2, 4, 3)
    assert arm(0x100c, 0x200c, 0, 7) == (True, 1, 5, 0)
    assert arm(0x1004, 0x2008, 0, 7) == (False, 21, 0, 0)         # offsets differ: the scalar loop
    assert arm(0x1004, 0x2004, 0, 1) == (True, 3, 0, 0)           # n <= head
    assert arm(0x100c, 0x200c, 0, 2) == (True, 1, 1, 1)
    assert arm(0x1004, 0x2004, 0, 2) == (True, 3, 0, 3)           # n4 == 0 with a tail
    assert arm(0x1004, 0x2004, 0, 345) == (True, 3, 258, 0)       # n4 > 256


def test_mesh_table_coverage():
    """The evidence that the vec arm is compared with a reference: over every (case, sample) of the mesh-arm tests the table
    reaches the vec arm with every head and tail in 0..3, n <= head, n4 == 0 < n - head, n4 > 256, and the scalar arm, with
    at least half of the pairs on the vec arm.

    The placed views alone give 120 of 260 pairs on the vec arm (4 of 16 offset pairs for nv in {7, 63}, 4 of 5 for the other
    four vertex counts); the batch-split runs in plain buffers (9 + 1 + 8 + 3 + 6 samples, all on the vec arm and all
    compared with the restatement) bring it to 147 of 287."""
    rows = sample_cases.mesh_table()
    assert [3 * nv % 4 for nv in sample_cases.MESH_NV] == [3, 2, 0, 1, 1, 3]
    assert len(rows) == (2 * 16 + 4 * 5) * sample_cases.MESH_B + 27
    for nv in sample_cases.MESH_NV:
        pairs = sample_cases.mesh_pairs(nv)
        assert pairs[0] == (0, 0) and len(set(pairs)) == len(pairs) == (16 if nv in sample_cases.MESH_ALL_PAIRS_NV else 5)
        assert sum(i != o for i, o in pairs) == (12 if nv in sample_cases.MESH_ALL_PAIRS_NV else 1)
    share = sample_cases.check_mesh_coverage((r[0],) + r[4:] for r in rows)
    print(f"mesh table: {len(rows)} (case, sample) pairs, {share:.3f} on the vec arm")
    # slot parity: at nv = 63 the samples of one launch sit on different heads
    assert {r[5] for r in rows if r[0] == 63 and (r[1], r[2]) == (0, 0)} == {0, 1, 2, 3}
    # the batch splits move samples to another head than they have in the whole batch
    whole = [sample_cases.mesh_arm(0, 0, b, 63)[1] for b in range(9)]
    for parts in sample_cases.MESH_SPLITS[1:]:
        split = [sample_cases.mesh_arm(0, 0, b, 63)[1] for B in parts for b in range(B)]
        assert sum(a != b for a, b in zip(whole, split)) >= 6, parts


@pytest.mark.parametrize("nv", sample_cases.MESH_NV)
def test_mesh_cases_are_live(nv):
    """nv = 1 is the degenerate box (status 1, zero mesh); every other case is live with a mesh worth comparing, and as well
    conditioned as the case the bar is measured on: the restatement's own fp32 run errs by at most half the bar (4 x its
    error on the 65 x 257 case) on every output, so at least half of it is the kernel's."""
    big = sample_cases.chain_case(65, 257, 50, "coco")
    bar = {k: 4.0 * float(np.abs(_ref(big, np.float32)[k].astype(np.float64) - _ref(big)[k]).max()) for k in OUTS}
    for c in (sample_cases.mesh_case(nv), sample_cases.mesh_split_case()):
        r, r32 = _ref(c), _ref(c, np.float32)
        dead = nv == 1 and c["verts"].shape[1] == 1
        assert (r["status"] == (1 if dead else 0)).all() and np.array_equal(r["status"], r32["status"])
        if dead:
            assert (r["mesh"] == 0).all()
            continue
        assert (np.abs(r["mesh"]).max(axis=(1, 2)) > 0.05).all()
        for k in OUTS:
            e = float(np.abs(r32[k].astype(np.float64) - r[k]).max())
            print(f"nv={c['verts'].shape[1]} {k}: fp32 restatement {e:.3e}  bar {bar[k]:.3e}")
            assert e <= 0.5 * bar[k], k


def test_cap32_tables():
    """The set at the kernel's caps: Jr = 32, J = 28 + 4 = 32, 16 disjoint pairs over all 32 joints with joint 31 in one, both
    roots joint 31, regressor rows of 1, 6, 64, 65 and 257 entries."""
    c = sample_cases.cap32_case(5)
    assert c["reg_R"].shape == (32, 257) and c["in_R"].shape == (28, 257) and len(c["midpoints"]) == 4
    assert c["reg_root"] == 31 and c["input_root"] == 31 and c["input_root"] >= c["in_R"].shape[0]
    flat = [j for p in c["flip_pairs"] for j in p]
    assert len(c["flip_pairs"]) == 16 and sorted(flat) == list(range(32)) and any(31 in p for p in c["flip_pairs"])
    for R in (c["reg_R"], c["in_R"]):
        n = np.count_nonzero(R, axis=1)
        assert n[:5].tolist() == [1, 6, 64, 65, 257] and (n[5:] == 6).all() and (R >= 0).all()
        assert np.abs(R.sum(axis=1) - 1).max() <= 1e-6


@pytest.mark.parametrize("B,seed", [(1, 61), (5, 65), (65, 50)])
def test_cap32_cases_are_live(B, seed):
    """Live samples, decided alike in fp32; with B = 5 some samples flipped and some not, and the pair permutation visible:
    the restatement without the pairs differs from the one with them by far more than any bar."""
    c = sample_cases.cap32_case(B, seed)
    r64, r32 = _ref(c), _ref(c, np.float32)
    assert (r64["status"] == 0).all() and (r32["status"] == 0).all()
    if B == 5:
        f = c["flip"] != 0
        assert f.any() and not f.all()
        plain = _ref(dict(c, flip_pairs=()))
        for k in ("lift_pose3d", "pose2d"):
            d = np.abs(plain[k] - r64[k]).max(axis=(1, 2))
            print(f"cap32 B=5 {k}: without the pair permutation off by {d[f].min():.3e} .. {d[f].max():.3e} on flipped samples")
            assert (d[f] > 1e-2).all() and (d[~f] == 0).all()
        # joint 31 is both roots and sits in pair (0, 31): the permutation moves the root's own row
        assert (np.abs(r64["lift_pose3d"][f, 0]).max(axis=1) == 0).all() and (np.abs(r64["lift_pose3d"][f, 31]).max(axis=1) > 0).all()


def test_cap32_noise_case():
    """Table noise at J = 32, rot / flip drawn: every one of the 65 samples is live and decided alike by the fp32 run (mask,
    flip, the rot = 0 pattern), so all of them are compared - the share the existing table-noise case keeps; among the first
    CAP32_NOISE_B, which the GPU runs, both flips and both rot patterns occur and the mask has both values."""
    c, kw = sample_cases.cap32_noise_case()
    r64, r32 = _ref(c, **kw), _ref(c, np.float32, **kw)
    n = sample_cases.CAP32_NOISE_B
    assert (r64["status"] == 0).all() and (r32["status"] == 0).all()
    assert np.array_equal(r64["mask"], r32["mask"]) and np.array_equal(r64["flip"], r32["flip"])
    assert np.array_equal(r64["rot"] == 0, r32["rot"] == 0)
    assert r64["mask"].shape == (65, 32) and not r64["mask"][:, 0].any() and r64["mask"][:, 31].all()
    for v in (r64["flip"][:n], r64["rot"][:n] == 0, r64["mask"][:n]):
        assert v.any() and not v.all()
    same = np.ones(65, bool)
    print(f"cap32 table noise: samples compared {same.sum()} of 65")
    assert same.mean() >= 0.6


def test_tiny_set_and_empty_row():
    """Jr = 1, Ji = 2: live, reg_pose3d exactly 0 and, with the regressed joint given back, fit_err exactly 0 in either
    precision.  An empty regressor row: the joint sits at the origin, z = 0, the projection is 0 / 0 - status bit 0 and
    everything zero."""
    c = sample_cases.tiny_set_case()
    for dt in (np.float64, np.float32):
        base = _ref(c, dt)
        assert (base["status"] == 0).all() and (base["reg_pose3d"] == 0).all()
        given = sample_cases.tiny_given(c)
        assert given.shape == (4, 1, 3)
        r = _ref(c, dt, given_cam=given)
        assert (r["status"] == 0).all() and (r["fit_err"] == 0).all() and (r["reg_pose3d"] == 0).all()
        assert (np.abs(r["pose2d"]) > 0).all() and (r["lift_valid"] == 1).all()
    c = sample_cases.empty_row_case()
    assert np.count_nonzero(c["in_R"][3]) == 0
    for dt in (np.float64, np.float32):
        r = _ref(c, dt)
        assert (r["status"] == 1).all()
        assert all((r[k] == 0).all() for k in ("pose2d", "mesh", "lift_pose3d", "reg_pose3d", "mesh_valid", "lift_valid", "reg_valid"))


@pytest.mark.parametrize("variant", ["trans_none", "mm", "rot_edges"])
def test_option_cases_are_live(variant):
    c = sample_cases.option_case(variant)
    r64, r32 = _ref(c), _ref(c, np.float32)
    assert (r64["status"] == 0).all() and (r32["status"] == 0).all()
    if variant != "rot_edges":       # the same scene as the plain case, said another way
        plain = _ref(sample_cases.option_case())
        assert np.abs(r64["mesh"] - plain["mesh"]).max() <= 1e-5 and np.abs(r64["pose2d"] - plain["pose2d"]).max() <= 1e-3


def test_option_drawn_halves():
    """The stream state of the half-drawn cases draws both flips, a zeroed and a kept rotation among its 4 samples; with
    rot_factor 0 every drawn rotation is exactly zero."""
    a = sample_cases.OPTION_AUG
    rot, flip = sample_ref.draw_aug(a["seed"], a["first"], 4, a["rot_factor"], True)
    assert flip.any() and not flip.all() and (rot == 0).any() and (rot != 0).any()
    for dt in (np.float64, np.float32):
        assert (sample_ref.draw_aug(a["seed"], a["first"], 4, 0.0, True, dt)[0] == 0).all()


def test_late_zero_case_takes_the_bad_branch():
    """x = +-3e38 on two joints of the middle sample: finite, so the early checks pass in fp32 (the box width overflows to
    inf, inf * th > 0, inf - 1 >= 0), the scale is W / inf = 0, the crop coordinates are 0 * inf = NaN, and the
    standardisation fails - status bit 0 through the restatement's late `bad` branch (its px is kept, not zeroed, which only
    a sample alive after the early checks has).  In float64 nothing overflows and the sample stays live: the expected status
    is an exact fact of the fp32 operation sequence."""
    c = sample_cases.late_zero_chain_case()
    gcam, sane, bad = sample_cases.late_zero_case(_ref(c))
    assert np.isfinite(bad).all() and np.abs(bad[1, :, 1]).max() < 1e4
    r32 = _ref(c, np.float32, given_cam=gcam, given_img=bad)
    assert r32["status"].tolist() == [0, 1, 0]
    assert np.isnan(r32["px"][1]).any(), "dead before the standardisation: not the late branch"
    for k in ("pose2d", "mesh", "lift_pose3d", "reg_pose3d", "mesh_valid", "lift_valid", "reg_valid"):
        assert (r32[k][1] == 0).all() and np.abs(r32[k][[0, 2]]).max() > 0, k
    assert _ref(c, np.float64, given_cam=gcam, given_img=bad)["status"].tolist() == [0, 0, 0]
    s32 = _ref(c, np.float32, given_cam=gcam, given_img=sane)
    assert s32["status"].tolist() == [0, 0, 0]
    for k in ("pose2d", "mesh", "lift_pose3d", "reg_pose3d"):
        assert np.array_equal(s32[k][[0, 2]], r32[k][[0, 2]]), k
