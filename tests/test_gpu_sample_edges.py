"""GPU: the edges of the training-sample chain (csrc/sample.hip, p2m_train_sample / TrainSampleBuilder) against the float64
restatement tests/sample_ref.py::chain, under the rules of tests/test_gpu_sample.py (its _chain_bar: 4 x the error of the
restatement's fp32 run against its float64 run over 65 samples x 257 vertices of the joint set).

A  both arms of k_sample_main's mesh stream - 16 bytes per lane where a sample's input and output are aligned alike, one
   scalar loop otherwise - at every head and tail, in views placed at float offsets 0..3 inside sentinel-filled tensors;
B  the joint tables at their caps (Jr = J = 32, 4 midpoints, 16 flip pairs, CSR rows of 1, 6, 64, 65 and 257 entries), at
   their smallest (Jr = 1, Ji = 2) and with an empty row;
C  the options no other test sets;
D  the late zeroing of k_sample_finish.

tests/test_sample_edges_cpu.py audits the case tables with the restatement alone."""
import numpy as np
import pytest
import torch

import sample_cases
import sample_ref
import test_gpu_sample as base
from pose2mesh_release_amd import sample

pytestmark = pytest.mark.gpu
OUTS, MASKS = base.OUTS, base.MASKS
SENT = base.GUARD
PAD = sample_cases.MESH_PAD


def _ref(c, dtype=np.float64, **kw):
    with np.errstate(all="ignore"):
        return base._ref_chain(c, dtype, **kw)


def _placed(B, nv, k, fill):
    """(flat, view): a contiguous [B, nv, 3] view that starts PAD + k floats into a flat tensor filled with `fill`."""
    flat = torch.full((sample_cases.mesh_flat_len(B, nv),), fill, dtype=torch.float32, device="cuda")
    return flat, flat[PAD + k:PAD + k + 3 * B * nv].view(B, nv, 3)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run(c, b, k_in=None, k_out=None, first=0, rot="case", flip="case", given=None, plain=False):
    """One builder call.  k_in / k_out: verts / mesh as placed views at that float offset (verts surrounded by NaN, mesh by
    the sentinel, which must survive); None: a fresh tensor / a guarded output like every other output (plain: the builder's
    own fresh buffers, unguarded).  Returns the outputs as numpy arrays and the arm of every sample's mesh stream, from the
    addresses the kernel was given."""
    B, nv = c["verts"].shape[:2]
    out, wholes = b.buffers(B), {}
    for k, t in ([] if plain else list(vars(out).items())):
        wholes[k], view = base._guarded(tuple(t.shape), t.dtype)
        setattr(out, k, view)
    verts = base._cuda(c["verts"])
    if k_in is not None:
        _, v = _placed(B, nv, k_in, float("nan"))
        v.copy_(verts)
        verts = v
    if k_out is not None:
        mflat, out.mesh = _placed(B, nv, k_out, SENT)
        wholes.pop("mesh", None)
    assert verts.is_contiguous() and out.mesh.is_contiguous()
    b.stream.seek(first)
    got = b(verts, base._cuda(c["focal"]), base._cuda(c["princpt"]), trans=None if c["trans"] is None else base._cuda(c["trans"]),
            mesh_scale=c["mesh_scale"], out=out, rot=base._cuda(c["rot"]) if isinstance(rot, str) else rot,
            flip=base._cuda(c["flip"], np.int32) if isinstance(flip, str) else flip, given=given)
    torch.cuda.synchronize()
    assert got is out and b.stream.index == first + B
    for k, w in wholes.items():
        if k == "kind" and b.noise_mode != 1:
            continue
        assert base._guards_intact(w), f"a guard row of {k} was written"
    if k_out is not None:
        m = mflat.cpu().numpy()
        s, e = PAD + k_out, PAD + k_out + 3 * B * nv
        assert (m[:s] == np.float32(SENT)).all() and (m[e:] == np.float32(SENT)).all(), "the mesh stream wrote outside its view"
    arms = [sample_cases.mesh_arm(verts.data_ptr(), out.mesh.data_ptr(), i, nv) for i in range(B)]
    return {k: getattr(out, k).cpu().numpy().copy() for k in vars(out)}, arms


def _compare(tag, got, want, bar, outs=OUTS):
    assert np.array_equal(got["status"], want["status"]), tag
    for k in MASKS:
        assert np.array_equal(got[k], want[k]), (tag, k)
    worst = {}
    for k in outs:
        worst[k] = float(np.abs(got[k] - want[k]).max())
        assert np.isfinite(got[k]).all() and worst[k] <= bar[k], (tag, k, worst[k], bar[k])
    return worst


# ---- A: both arms of the mesh stream ---------------------------------------------------------------------------------------
def test_mesh_table_coverage_on_device(hip_libs):
    """The coverage assertion of test_sample_edges_cpu.py::test_mesh_table_coverage, from the addresses this allocator
    gives: the same rows as the CPU table (which takes every allocation to start on a 16-byte line)."""
    rows = []
    for nv in sample_cases.MESH_NV:
        for k_in, k_out in sample_cases.mesh_pairs(nv):
            (_, v), (_, m) = _placed(sample_cases.MESH_B, nv, k_in, 0.0), _placed(sample_cases.MESH_B, nv, k_out, 0.0)
            rows += [(nv, k_in, k_out, b) + sample_cases.mesh_arm(v.data_ptr(), m.data_ptr(), b, nv) for b in range(sample_cases.MESH_B)]
    for parts in sample_cases.MESH_SPLITS:
        for B in parts:
            v, m = torch.empty(B, 63, 3, device="cuda"), torch.empty(B, 63, 3, device="cuda")
            rows += [(63, 0, 0, b) + sample_cases.mesh_arm(v.data_ptr(), m.data_ptr(), b, 63) for b in range(B)]
    assert rows == sample_cases.mesh_table()
    share = sample_cases.check_mesh_coverage((r[0],) + r[4:] for r in rows)
    print(f"mesh table on the device: {len(rows)} (case, sample) pairs, {share:.3f} on the vec arm")


@pytest.mark.parametrize("nv", sample_cases.MESH_NV)
def test_mesh_arms_against_restatement(hip_libs, nv):
    """Noise off, rot / flip given, B = 5, the coco set; verts and mesh as views at every listed pair of float offsets.  Every
    run: the arm of each sample is the CPU table's (so that table's coverage holds here), nothing outside the mesh view is
    written, every output against the float64 restatement (mesh under _chain_bar, the worst error printed per arm), and the
    mesh bit for bit the (0, 0) run's - an element is one thread's same operation sequence whichever loop handles it.
    nv = 1 is the degenerate box: status 1 and an all-zero mesh in both arms."""
    c = sample_cases.mesh_case(nv)
    want, bar = _ref(c), base._chain_bar("coco")
    assert (want["status"] == (1 if nv == 1 else 0)).all()
    b = base._builder(c, noise=None)
    table = {r[:4]: r[4:] for r in sample_cases.mesh_table()[:-27]}
    first, worst, count = None, {True: 0.0, False: 0.0}, {True: 0, False: 0}
    for k_in, k_out in sample_cases.mesh_pairs(nv):
        got, arms = _run(c, b, k_in, k_out)
        assert arms == [table[(nv, k_in, k_out, i)] for i in range(sample_cases.MESH_B)], (k_in, k_out, arms)
        _compare((nv, k_in, k_out), got, want, bar)
        assert np.array_equal(got["rot_flip"], np.stack([c["rot"], c["flip"].astype(np.float32)], axis=1))
        if nv == 1:
            assert (got["mesh"] == 0).all()
        for i, a in enumerate(arms):
            worst[a[0]] = max(worst[a[0]], float(np.abs(got["mesh"][i] - want["mesh"][i]).max()))
            count[a[0]] += 1
        if first is None:
            assert (k_in, k_out) == (0, 0)
            first = got["mesh"]
        assert np.array_equal(_bits(got["mesh"]), _bits(first)), f"mesh at offsets {(k_in, k_out)} differs bitwise from (0, 0)"
    print(f"nv={nv} mesh vs float64: vec arm worst {worst[True]:.3e} over {count[True]} samples, scalar arm worst "
          f"{worst[False]:.3e} over {count[False]} samples, bar {bar['mesh']:.3e}")
    assert count[True] and count[False]


def test_mesh_batch_splits(hip_libs):
    """Plain buffers, nv = 63: a batch of 9 as 1 + 8 and as 3 + 6, every part in fresh tensors, equals the whole batch bit
    for bit.  A sample's head is (4 - slot) % 4 here, so the parts put most samples on another head than the whole batch
    does (the 4 + 5 split of test_chain_stream_properties keeps every head).  Every run is on the vec arm and is compared
    with the restatement as well."""
    c = sample_cases.mesh_split_case()
    want, bar = _ref(c), base._chain_bar("coco")
    b = base._builder(c, noise=None)
    runs = {}
    for parts in sample_cases.MESH_SPLITS:
        outs, arms, s0 = [], [], 0
        for B in parts:
            part = {k: (v[s0:s0 + B].copy() if k in ("verts", "trans", "focal", "princpt", "rot", "flip") else v) for k, v in c.items()}
            g, a = _run(part, b, first=s0, plain=True)
            outs.append(g)
            arms += a
            s0 += B
        assert all(a[0] for a in arms), "a plain-buffer run left the vec arm"
        runs[parts] = ({k: np.concatenate([o[k] for o in outs]) for k in OUTS + MASKS + ("status",)}, [a[1] for a in arms])
        worst = _compare(parts, runs[parts][0], want, bar)
        print(f"split {parts}: heads {runs[parts][1]}, mesh worst {worst['mesh']:.3e}  bar {bar['mesh']:.3e}")
    whole, heads = runs[(9,)]
    for parts in sample_cases.MESH_SPLITS[1:]:
        got, h = runs[parts]
        assert sum(x != y for x, y in zip(h, heads)) >= 6
        for k in whole:
            assert np.array_equal(_bits(got[k].astype(np.float32)), _bits(whole[k].astype(np.float32))), (parts, k)


# ---- B: the table caps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,seed", [(1, 61), (5, 65)])
def test_cap32_against_restatement(hip_libs, B, seed):
    """Jr = 32, J = 28 + 4 = 32, 16 flip pairs over all 32 joints, both roots joint 31, CSR rows of 1, 6, 64, 65 and 257
    entries: every output against the restatement, under the bar of this set (65 x 257).  With B = 5 some samples are
    flipped (test_sample_edges_cpu.py shows that the pair permutation is then far outside the bar if it is wrong)."""
    c = sample_cases.cap32_case(B, seed)
    want, bar = _ref(c), base._chain_bar("cap32")
    got, _ = _run(c, base._builder(c, noise=None))
    assert (want["status"] == 0).all()
    worst = _compare(("cap32", B), got, want, bar)
    for k in OUTS:
        print(f"cap32 B={B} {k}: worst {worst[k]:.3e}  bar {bar[k]:.3e}")
    assert np.array_equal(got["rot_flip"], np.stack([c["rot"], c["flip"].astype(np.float32)], axis=1))


def test_cap32_table_noise(hip_libs):
    """Table noise at J = 32, rot and flip drawn: flip and the rot = 0 pattern equal the restatement's exactly, rot within
    _rot_bar, pose2d within 4 x the fp32 restatement's error over the 65 samples of the case (the GPU runs the first 9; a
    sample depends on its global index alone).  The Bernoulli mask is exact: one wrong bit moves a joint by its table
    entry, a pixel or more, against a bar of 1e-5 (p2m_pose_noise_table's own mask at J = 32 is compared directly by
    test_gpu_sample.py::test_noise_table)."""
    c65, kw = sample_cases.cap32_noise_case()
    r64, r32 = _ref(c65, **kw), _ref(c65, np.float32, **kw)
    assert np.array_equal(r64["mask"], r32["mask"]) and (r64["status"] == 0).all()
    n = sample_cases.CAP32_NOISE_B
    c = sample_cases.head_of(c65, n)
    b = base._builder(c, noise="table", table=kw["table"], rotate_factor=30.0, flip=True, seed=kw["seed"])
    got, _ = _run(c, b, first=kw["first_index"], rot=None, flip=None)
    assert (got["status"] == 0).all()
    assert np.array_equal(got["rot_flip"][:, 1] != 0, r64["flip"][:n]) and r64["flip"][:n].any() and not r64["flip"][:n].all()
    assert np.array_equal(got["rot_flip"][:, 0] == 0, r64["rot"][:n] == 0) and (r64["rot"][:n] != 0).any()
    assert np.abs(got["rot_flip"][:, 0] - r64["rot"][:n]).max() <= base._rot_bar()
    bar = 4.0 * float(np.abs(r32["pose2d"].astype(np.float64) - r64["pose2d"]).max())
    err = float(np.abs(got["pose2d"] - r64["pose2d"][:n]).max())
    print(f"cap32 table noise: samples compared {n} of {n}, masked {r64['mask'][:n].sum()} of {r64['mask'][:n].size}, "
          f"pose2d worst {err:.3e}  bar {bar:.3e}")
    assert np.isfinite(got["pose2d"]).all() and err <= bar
    lbar = max(base._chain_bar("cap32")["lift_pose3d"], 4.0 * float(np.abs(r32["lift_pose3d"].astype(np.float64) - r64["lift_pose3d"]).max()))
    lerr = float(np.abs(got["lift_pose3d"] - r64["lift_pose3d"][:n]).max())
    print(f"cap32 table noise: lift_pose3d worst {lerr:.3e}  bar {lbar:.3e}")
    assert lerr <= lbar


def test_smallest_tables(hip_libs):
    """Jr = 1, Ji = 2, no midpoints: live; reg_pose3d is exactly 0 and, with given=, fit_err exactly 0 (one joint equals its
    own mean); everything else against the restatement under the coco bar."""
    c = sample_cases.tiny_set_case()
    bar = base._chain_bar("coco")
    b = base._builder(c, noise=None)
    for given in (None, sample_cases.tiny_given(c)):
        want = _ref(c) if given is None else _ref(c, given_cam=given)
        got, _ = _run(c, b, given=None if given is None else (base._cuda(given), None))
        worst = _compare("tiny", got, want, bar)
        print(f"Jr=1 Ji=2 given={given is not None}: " + ", ".join(f"{k} worst {worst[k]:.3e} bar {bar[k]:.3e}" for k in OUTS))
        assert (got["status"] == 0).all() and (got["reg_pose3d"] == 0).all() and (got["fit_err"] == 0).all()
        assert (got["lift_valid"] == 1).all() and (got["reg_valid"] == 1).all()


def test_empty_regressor_row(hip_libs):
    """An empty row of the input regressor: the CSR loop does not run, the joint sits at the origin, z = 0 and the projection
    is 0 / 0 - status bit 0 and everything zero, as the restatement says (asserted on the CPU first)."""
    c = sample_cases.empty_row_case()
    want = _ref(c)
    assert (want["status"] == 1).all() and all((want[k] == 0).all() for k in OUTS + MASKS)
    got, _ = _run(c, base._builder(c, noise=None))
    assert (got["status"] == 1).all()
    for k in OUTS + MASKS:
        assert (got[k] == 0).all(), k


# ---- C: the options --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["trans_none", "mm"])
def test_option_trans_and_scale(hip_libs, variant):
    """trans=None (the translation in the vertices) and mesh_scale=1 (vertices in mm) against the restatement."""
    c = sample_cases.option_case(variant)
    want, bar = _ref(c), base._chain_bar("coco")
    got, _ = _run(c, base._builder(c, noise=None))
    assert (want["status"] == 0).all()
    worst = _compare(variant, got, want, bar)
    print(f"{variant}: " + ", ".join(f"{k} worst {worst[k]:.3e} bar {bar[k]:.3e}" for k in OUTS))


def test_option_fit_thr_zero(hip_libs):
    """given= with fit_thr = 0: fit_err as in test_chain_given_joints (up to 200 mm here), and no status bit 1 whatever it is."""
    c = sample_cases.option_case()
    given = sample_cases.given_joints(c, _ref(c))
    want = _ref(c, given_cam=given, fit_thr=0.0)
    got, _ = _run(c, base._builder(c, noise=None, fit_thr=0.0), given=(base._cuda(given), None))
    C = 1000.0 * (float(np.abs(c["trans"]).max()) + 2.0)
    err = float(np.abs(got["fit_err"] - want["fit_err"]).max())
    print(f"fit_thr=0: fit_err {got['fit_err'].tolist()}, worst {err:.3e}  bar {64 * 2.0 ** -24 * C:.3e}")
    assert got["fit_err"].max() > 100.0 and err <= 64 * 2.0 ** -24 * C
    assert (got["status"] == 0).all() and (want["status"] == 0).all()
    _compare("fit_thr=0", got, want, base._chain_bar("coco"))
    assert all((got[k] == 1).all() for k in MASKS)


def test_option_given_img_is_ignored_with_an_input_regressor(hip_libs):
    """given_img passed to the coco set, which projects its own input joints: every output is bitwise the run without it."""
    c = sample_cases.option_case()
    r = _ref(c)
    given = sample_cases.given_joints(c, r)
    gimg = (r["img"][:, :17] + 40.0).astype(np.float32)
    b = base._builder(c, noise=None)
    a, _ = _run(c, b, given=(base._cuda(given), None))
    g, _ = _run(c, b, given=(base._cuda(given), base._cuda(gimg)))
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), g[k].view(np.uint8)), k
    _compare("given_img", g, _ref(c, given_cam=given, given_img=gimg), base._chain_bar("coco"))


def test_option_half_drawn_augmentation(hip_libs):
    """rot given with flip drawn, and the reverse, at a fixed stream index: the given half is what was given, the drawn half
    is the restatement's draw and the all-drawn run's."""
    c, a = sample_cases.option_case(), sample_cases.OPTION_AUG
    b = base._builder(c, noise=None, rotate_factor=a["rot_factor"], flip=True, seed=a["seed"])
    drot, dflip = sample_ref.draw_aug(a["seed"], a["first"], 4, a["rot_factor"], True)
    both, _ = _run(c, b, first=a["first"], rot=None, flip=None)
    grot, _ = _run(c, b, first=a["first"], flip=None)
    gflip, _ = _run(c, b, first=a["first"], rot=None)
    bar = base._rot_bar()
    print(f"drawn rot {both['rot_flip'][:, 0].tolist()} flip {both['rot_flip'][:, 1].tolist()}, rot worst "
          f"{np.abs(both['rot_flip'][:, 0] - drot).max():.3e}  bar {bar:.3e}")
    for r in (both, gflip):
        assert np.array_equal(r["rot_flip"][:, 0] == 0, drot == 0) and np.abs(r["rot_flip"][:, 0] - drot).max() <= bar
    for r in (both, grot):
        assert np.array_equal(r["rot_flip"][:, 1] != 0, dflip)
    assert np.array_equal(_bits(gflip["rot_flip"][:, 0]), _bits(both["rot_flip"][:, 0]))
    assert np.array_equal(_bits(grot["rot_flip"][:, 1]), _bits(both["rot_flip"][:, 1]))
    assert np.array_equal(_bits(grot["rot_flip"][:, 0]), _bits(c["rot"]))
    assert np.array_equal(gflip["rot_flip"][:, 1], c["flip"].astype(np.float32))
    cb = base._chain_bar("coco")
    _compare("rot given", grot, _ref(c, flip=dflip), cb)
    _compare("flip given", gflip, _ref(c, rot=None, rot_factor=a["rot_factor"], flip_enabled=True, seed=a["seed"],
                                       first_index=a["first"]), cb)


def test_option_zero_rotate_factor(hip_libs):
    """Drawn rot with rotate_factor = 0: every rot is exactly 0, the `rot != 0` skip is taken, and lift_pose3d is bitwise the
    run with rot given as zeros."""
    c = sample_cases.option_case()
    b = base._builder(c, noise=None, rotate_factor=0.0, flip=False, seed=sample_cases.OPTION_AUG["seed"])
    drawn, _ = _run(c, b, first=sample_cases.OPTION_AUG["first"], rot=None)
    given, _ = _run(c, b, first=sample_cases.OPTION_AUG["first"], rot=torch.zeros(4, device="cuda"))
    assert (drawn["rot_flip"][:, 0] == 0).all() and np.array_equal(drawn["rot_flip"][:, 1], c["flip"].astype(np.float32))
    assert np.array_equal(_bits(drawn["lift_pose3d"]), _bits(given["lift_pose3d"]))
    _compare("rotate_factor=0", drawn, _ref(c, rot=np.zeros(4, np.float32)), base._chain_bar("coco"))


def test_option_rot_edges(hip_libs):
    """rot = 180, 360, -0.0 (and 0.0), given: against the restatement under _chain_bar; a batch of -0.0 is bitwise the batch
    of 0.0 (rot_flip itself keeps the sign it was given)."""
    c = sample_cases.option_case("rot_edges")
    want, bar = _ref(c), base._chain_bar("coco")
    b = base._builder(c, noise=None)
    got, _ = _run(c, b)
    worst = _compare("rot edges", got, want, bar)
    print("rot 180, 360, -0.0, 0.0: " + ", ".join(f"{k} worst {worst[k]:.3e} bar {bar[k]:.3e}" for k in OUTS))
    assert np.array_equal(_bits(got["rot_flip"][:, 0]), _bits(c["rot"]))
    zp, _ = _run(c, b, rot=torch.zeros(4, device="cuda"))
    zm, _ = _run(c, b, rot=-torch.zeros(4, device="cuda"))
    assert np.signbit(zm["rot_flip"][:, 0]).all() and not np.signbit(zp["rot_flip"][:, 0]).any()
    for k in OUTS + MASKS + ("status",):
        assert np.array_equal(zp[k].view(np.uint8), zm[k].view(np.uint8)), k


# ---- D: the late zeroing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_in,k_out", [(0, 0), (0, 1)])
def test_late_zeroing(hip_libs, k_in, k_out):
    """The middle of three samples passes k_sample_main's checks and fails the standardisation of k_sample_finish (given 2D
    joints with x = +-3e38 on two joints: see test_sample_edges_cpu.py; the expected status is the restatement's fp32 run's,
    an exact fact of the fp32 operation sequence).  status == [0, 1, 0]; every output and mask of sample 1 is zero, the mesh
    included, and nothing outside the mesh view is written; samples 0 and 2 are bitwise what they are with a sane middle
    sample.  Once with the mesh on the vec arm, once on the scalar arm."""
    c = sample_cases.late_zero_chain_case()
    gcam, sane, bad = sample_cases.late_zero_case(_ref(c))
    want = _ref(c, np.float32, given_cam=gcam, given_img=bad)
    assert want["status"].tolist() == [0, 1, 0] and np.isnan(want["px"][1]).any()
    b = base._builder(c, noise=None)
    got, arms = _run(c, b, k_in, k_out, given=(base._cuda(gcam), base._cuda(bad)))
    ok, arms_ok = _run(c, b, k_in, k_out, given=(base._cuda(gcam), base._cuda(sane)))
    assert arms == arms_ok and all(a[0] == (k_in == k_out) for a in arms), arms
    print(f"late zeroing, mesh arms {['vec' if a[0] else 'scalar' for a in arms]}: status {got['status'].tolist()}")
    assert got["status"].tolist() == [0, 1, 0] and ok["status"].tolist() == [0, 0, 0]
    for k in OUTS + MASKS:
        assert (got[k][1] == 0).all(), k
        assert np.array_equal(got[k][[0, 2]].view(np.uint8), ok[k][[0, 2]].view(np.uint8)), k
        assert np.abs(ok[k][1]).max() > 0, k
    _compare("late zeroing, sane", ok, _ref(c, given_cam=gcam, given_img=sane), base._chain_bar("human36"))
