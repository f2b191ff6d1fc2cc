"""GPU: the sample kernels (pose2mesh_release_amd.sample, csrc/sample.hip) - the two noise kernels and the whole chain
(TrainSampleBuilder / p2m_train_sample) - against the float64 restatement tests/sample_ref.py run on the same stream state.

On robust units (sample_ref's audit: no deciding candidate inside the fp32 band) `kind` is equal exactly and the
coordinates agree to the project's fp32-class bar: 4 x the error of an fp32 numpy run of the restatement against its float64
run (tests/test_gpu_body.py's rule), taken over the 65 x 17 points of the companion case `all_valid` - a per-point error
class does not depend on how many samples a launch has, and the maximum over a handful of points would be a noisy bar.
On non-robust units (and on pairs that coincide: margin 0 by construction): finite values and a legal kind."""
import functools

import numpy as np
import pytest
import torch

import sample_cases
import sample_ref
from pose2mesh_release_amd import _lib, sample

pytestmark = pytest.mark.gpu
GUARD = 7.0
UNIT_OF = (np.arange(17) + 1) // 2


def _cuda(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def _guarded(shape, dtype):
    """A tensor with one guard row before and after: (whole, view of the middle)."""
    whole = torch.full((shape[0] + 2,) + tuple(shape[1:]), GUARD, dtype=dtype, device="cuda")
    return whole, whole[1:-1]


def _guards_intact(whole):
    w = whole.cpu().numpy()
    return (w[0] == w.dtype.type(GUARD)).all() and (w[-1] == w.dtype.type(GUARD)).all()


def _run_coco(joints, area, seed, first):
    B = joints.shape[0]
    st = sample.NoiseStream(seed, first)
    ow, out = _guarded((B, 17, 3), torch.float32)
    kw, kind = _guarded((B, 17), torch.int8)
    o, k = sample.noise_coco(_cuda(joints), _cuda(area), st, out=out, kind=kind)
    torch.cuda.synchronize()
    assert o.data_ptr() == out.data_ptr() and k.data_ptr() == kind.data_ptr()
    assert _guards_intact(ow) and _guards_intact(kw), "a guard row was written"
    assert st.index == (first + B) & 0xFFFFFFFFFFFFFFFF
    return out.cpu().numpy().copy(), kind.cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def _coco_bar():
    c = sample_cases.noise_cases()["all_valid"]
    a = [c["joints"], c["area"], sample_ref.COCO_SIGMAS, c["seed"], c["first_index"]]
    o64, k64, rb = sample_ref.noise_coco(*a)
    o32, k32, _ = sample_ref.noise_coco(*a, dtype=np.float32)
    same = rb[:, UNIT_OF] & (k64 == k32)
    return 4.0 * float(np.abs(o32[same] - o64[same]).max())


def _all_cases():
    cases = dict(sample_cases.noise_cases())
    cases["zeroed_lower"] = sample_cases.zeroed_lower_case()
    return cases


@pytest.mark.parametrize("name", list(_all_cases()))
def test_noise_coco_against_restatement(hip_libs, name):
    c = _all_cases()[name]
    want, wkind, robust = sample_ref.noise_coco(c["joints"], c["area"], sample_ref.COCO_SIGMAS, c["seed"], c["first_index"])
    got, kind = _run_coco(c["joints"], c["area"], c["seed"], c["first_index"])
    robust[:, list(c["coincident"])] = False
    rj = robust[:, UNIT_OF]
    bar = _coco_bar()
    err = float(np.abs(got[rj] - want[rj]).max()) if rj.any() else 0.0
    print(f"{name}: robust joints {rj.sum()} of {rj.size}, kinds {np.bincount(kind.ravel() + 1, minlength=6).tolist()}, "
          f"worst |x - ref| {err:.3e}  bar {bar:.3e}")
    assert np.isfinite(got).all() and set(np.unique(kind).tolist()) <= {-1, 0, 1, 2, 4}
    zero = kind == -1
    assert (got[zero] == 0).all() and (got[~zero][:, 2] == 1).all()
    assert np.array_equal(kind[rj], wkind[rj])
    assert err <= bar


def test_zeroed_lower_joint_feeds_partner(hip_libs):
    """Area 0 and a coincident pair: nothing passes for the lower joint (0 > 0 is false, exactly, in any precision), it is
    zeroed, and the higher joint sees the partner at (0, 0) and keeps its own position (every radius is 0)."""
    c = sample_cases.zeroed_lower_case()
    got, kind = _run_coco(c["joints"], c["area"], c["seed"], c["first_index"])
    assert (kind[:, [1, 11]] == -1).all() and (got[:, [1, 11]] == 0).all()
    assert (kind[:, [2, 12]] >= 0).all() and np.array_equal(got[:, [2, 12], :2], c["joints"][:, [2, 12], :2])


def _table_case(B, J):
    rng = np.random.default_rng(B * 100 + J)
    pose = (rng.uniform(0, 1, (B, J, 2)) * [288, 384]).astype(np.float32)
    return pose, sample_cases.table(J, seed=J), 4242 + J, (1 << 40) + B


@functools.lru_cache(maxsize=None)
def _table_bar():
    pose, tab, seed, first = _table_case(65, 32)
    want, _ = sample_ref.noise_table(pose, *tab, 288, 384, seed, first)
    w32, _ = sample_ref.noise_table(pose, *tab, 288, 384, seed, first, dtype=np.float32)
    return 4.0 * float(np.abs(w32 - want).max())


@pytest.mark.parametrize("B,J", [(1, 1), (3, 17), (9, 19), (65, 32)])
def test_noise_table(hip_libs, B, J):
    """The Bernoulli mask is exact; the values are within 4 x the fp32 restatement's error, taken over the 65 x 32 points of
    the largest case (as _coco_bar does: a handful of points would give a noisy bar)."""
    pose, (mean, std, weight), seed, first = _table_case(B, J)
    want, mask = sample_ref.noise_table(pose, mean, std, weight, 288, 384, seed, first)
    w32, m32 = sample_ref.noise_table(pose, mean, std, weight, 288, 384, seed, first, dtype=np.float32)
    assert np.array_equal(mask, m32)
    st = sample.NoiseStream(seed, first)
    ow, out = _guarded((B, J, 2), torch.float32)
    sample.noise_table(_cuda(pose), _cuda(mean), _cuda(std), _cuda(weight), st, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert _guards_intact(ow) and st.index == first + B
    changed = (got != pose).any(axis=2)
    assert np.array_equal(changed, mask), "Bernoulli mask differs"
    bar = _table_bar()
    assert mask.any()
    err = float(np.abs(got - want).max())
    print(f"table B={B} J={J}: masked {mask.sum()} of {mask.size}, worst {err:.3e}  bar {bar:.3e}")
    assert np.isfinite(got).all() and err <= bar
    # in place
    p = _cuda(pose)
    sample.noise_table(p, _cuda(mean), _cuda(std), _cuda(weight), sample.NoiseStream(seed, first), out=p)
    assert torch.equal(p, out)


def test_stream_properties(hip_libs):
    """The same state twice is bitwise equal; samples [0, 9) as one batch equal batches 4 + 5 with the index advanced by the
    calls themselves; another seed or index gives other numbers."""
    c = sample_cases.noise_cases()["valid_le10"]
    j, a = _cuda(c["joints"]), _cuda(c["area"])

    def run(seed, first, parts):
        st = sample.NoiseStream(seed, first)
        outs = [sample.noise_coco(j[s], a[s], st) for s in parts]
        return torch.cat([o for o, _ in outs]), torch.cat([k for _, k in outs])
    whole = [slice(0, 9)]
    o1, k1 = run(c["seed"], c["first_index"], whole)
    o2, k2 = run(c["seed"], c["first_index"], whole)
    o3, k3 = run(c["seed"], c["first_index"], [slice(0, 4), slice(4, 9)])
    assert torch.equal(o1, o2) and torch.equal(k1, k2)
    assert torch.equal(o1, o3) and torch.equal(k1, k3)
    assert not torch.equal(o1, run(c["seed"] + 1, c["first_index"], whole)[0])
    assert not torch.equal(o1, run(c["seed"], c["first_index"] + 9, whole)[0])


def test_graph_capture_replays_with_fresh_numbers(hip_libs):
    """A call, the index advance included, captured in a torch.cuda.graph: replay r gives the eager result for indices
    first + r B."""
    c = sample_cases.noise_cases()["valid_le10"]
    B = c["joints"].shape[0]
    j, a = _cuda(c["joints"]), _cuda(c["area"])
    pose = j[:, :, :2].contiguous()
    mean, std, weight = (_cuda(x) for x in sample_cases.table(17, seed=5))
    eager = []
    st = sample.NoiseStream(c["seed"], 100)
    for _ in range(2):
        o, k = sample.noise_coco(j, a, st, advance=False)
        t = sample.noise_table(pose, mean, std, weight, st)
        eager.append((o.clone(), k.clone(), t.clone()))
    st = sample.NoiseStream(c["seed"], 100)
    out, kind, tab = torch.empty(B, 17, 3, device="cuda"), torch.empty(B, 17, dtype=torch.int8, device="cuda"), torch.empty(B, 17, 2, device="cuda")
    sample.noise_coco(j, a, sample.NoiseStream(1, 0), out=out, kind=kind)             # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sample.noise_coco(j, a, st, out=out, kind=kind, advance=False)
        sample.noise_table(pose, mean, std, weight, st, out=tab)
    for r in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[r][0]) and torch.equal(kind, eager[r][1]) and torch.equal(tab, eager[r][2]), r
    assert st.index == 100 + 2 * B


def test_kind_frequencies(hip_libs):
    """4096 samples of one pose: the share of each kind per joint sits within 5 binomial sigmas of the restatement's own
    renormalised table when every type is available (all joints valid, a pose with room around every joint)."""
    n = 4096
    joints, area = sample_cases.histogram_poses()["all_valid"]
    _, kind = sample.noise_coco(_cuda(np.repeat(joints[None], n, 0)), _cuda(np.full(n, area)), sample.NoiseStream(99, 0))
    kind = kind.cpu().numpy()
    assert (kind >= 0).all()
    for jn in range(17):
        pj, pm, pi = sample_ref.probabilities(jn, 17)
        want = {0: pj, 1: pm, 2: pi if jn else 0.0, 4: 1 - pj - pm - pi}
        tot = sum(want.values())
        for k, p in want.items():
            p = p / tot
            assert abs((kind[:, jn] == k).mean() - p) <= 5 * np.sqrt(p * (1 - p) / n) + 1e-12, (jn, k)


def test_refusals(hip_libs):
    lib = _lib.hip()
    z = torch.zeros(4096, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    p, n = z.data_ptr(), None
    out = torch.zeros(4096, device="cuda").data_ptr()
    assert lib.p2m_pose_noise_coco(p, p, p, n, out, n, 1, n) == -1 and b"state" in lib.p2m_last_error_string()
    assert lib.p2m_pose_noise_table(p, p, p, p, 17, 288.0, 384.0, n, out, 1, n) == -1 and b"state" in lib.p2m_last_error_string()
    assert lib.p2m_pose_noise_table(p, p, p, p, 33, 288.0, 384.0, st.data_ptr(), out, 1, n) == -1
    assert b"J outside" in lib.p2m_last_error_string()
    assert lib.p2m_pose_noise_table(p, p, p, p, 0, 288.0, 384.0, st.data_ptr(), out, 1, n) == -1
    assert lib.p2m_pose_noise_coco(p, p, p, st.data_ptr(), out, n, 0, n) == -1
    assert lib.p2m_pose_noise_coco(p, p, p, st.data_ptr(), p, n, 1, n) == -1 and b"alias" in lib.p2m_last_error_string()
    assert lib.p2m_pose_noise_coco(n, p, p, st.data_ptr(), out, n, 1, n) == -1
    # a shifted view of the same buffer overlaps without sharing its base pointer
    assert lib.p2m_pose_noise_coco(p, p, p, st.data_ptr(), p + 4 * 17, n, 2, n) == -1 and b"overlap" in lib.p2m_last_error_string()
    assert lib.p2m_pose_noise_coco(p + 4 * 17, p, p, st.data_ptr(), p, n, 2, n) == -1
    torch.cuda.synchronize()
    assert (z == 0).all()
    with pytest.raises(_lib.P2MError):
        sample.noise_coco(torch.zeros(2, 17, 3), torch.ones(2), sample.NoiseStream(1))
    with pytest.raises(_lib.P2MError):
        sample.noise_table(torch.zeros(2, 17, 2), z[:34].view(17, 2), z[:34].view(17, 2), z[:17], sample.NoiseStream(1))
    with pytest.raises(_lib.P2MError):
        sample.NoiseStream(1, device="cpu")


# ---- the chain: TrainSampleBuilder / p2m_train_sample --------------------------------------------------------------------
OUTS = ("pose2d", "mesh", "lift_pose3d", "reg_pose3d")
MASKS = ("mesh_valid", "lift_valid", "reg_valid")


def _builder(c, **kw):
    return sample.TrainSampleBuilder(c["reg_R"], c["in_R"], c["midpoints"], (c["reg_root"], c["input_root"]), c["flip_pairs"],
                                     input_shape=(c["H"], c["W"]), **kw)


def _run_chain(c, b, first=0, rot="case", flip="case", given=None):
    """One builder call into guarded outputs; returns dict of numpy arrays."""
    B = c["verts"].shape[0]
    plain = b.buffers(B)
    wholes, out = {}, plain
    for k, t in vars(plain).items():
        wholes[k], view = _guarded(tuple(t.shape), t.dtype)
        setattr(out, k, view)
    b.stream.seek(first)
    got = b(_cuda(c["verts"]), _cuda(c["focal"]), _cuda(c["princpt"]), trans=_cuda(c["trans"]), mesh_scale=c["mesh_scale"], out=out,
            rot=_cuda(c["rot"]) if isinstance(rot, str) else rot, flip=_cuda(c["flip"], np.int32) if isinstance(flip, str) else flip,
            given=given)
    torch.cuda.synchronize()
    assert got is out and b.stream.index == first + B
    for k, w in wholes.items():
        if k == "kind" and b.noise_mode != 1:
            continue
        assert _guards_intact(w), f"a guard row of {k} was written"
    return {k: getattr(out, k).cpu().numpy().copy() for k in wholes}


def _ref_chain(c, dtype=np.float64, **kw):
    args = dict(rot=c["rot"], flip=c["flip"])
    args.update(kw)
    return sample_ref.chain(c["verts"], c["focal"], c["princpt"], dtype=dtype, **args, **sample_cases.chain_kwargs(c))


@functools.lru_cache(maxsize=None)
def _chain_bar(joint_set):
    """Per output: 4 x the error of an fp32 numpy run of the restatement against its float64 run (tests/test_gpu_body.py's
    rule), over the 65 samples x 257 vertices of the largest small case of the joint set."""
    c = sample_cases.chain_case(65, 257, 50, joint_set)
    r64, r32 = _ref_chain(c), _ref_chain(c, np.float32)
    assert np.array_equal(r64["status"], r32["status"])
    return {k: 4.0 * float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) for k in OUTS}


@pytest.mark.parametrize("B,nv,joint_set", [(1, 63, "coco"), (3, 1, "coco"), (9, 257, "human36"), (65, 257, "coco"),
                                            (3, 63, "human36"), (2, 6890, "coco")])
def test_chain_against_restatement(hip_libs, B, nv, joint_set):
    """Given rot / flip, noise off: every output against the float64 restatement.  nv = 1: the degenerate bbox."""
    c = sample_cases.chain_case(B, nv, 50 if (B, nv) == (65, 257) else 60 + B + nv, joint_set)
    want = _ref_chain(c)
    got = _run_chain(c, _builder(c, noise=None))
    bar = _chain_bar(joint_set)
    assert np.array_equal(got["status"], want["status"]) and (want["status"] == (1 if nv == 1 else 0)).all()
    for k in MASKS:
        assert np.array_equal(got[k], want[k]), k
    for k in OUTS:
        err = float(np.abs(got[k] - want[k]).max())
        print(f"B={B} nv={nv} {joint_set} {k}: worst {err:.3e}  bar {bar[k]:.3e}")
        assert np.isfinite(got[k]).all() and err <= bar[k], k
    assert np.array_equal(got["rot_flip"], np.stack([c["rot"], c["flip"].astype(np.float32)], axis=1))


def test_chain_degenerate_sample_in_a_batch(hip_libs):
    """A sample whose vertices coincide, between two sane ones, with coco noise on: status bit 0, all outputs zero, all masks
    0, and its neighbours as if it were not there."""
    c = sample_cases.chain_case(3, 63, 70, "coco")
    c["verts"][1] = c["verts"][1][:1]
    got = _run_chain(c, _builder(c, noise="coco", seed=5))
    want = _ref_chain(c, noise=sample_ref.NOISE_COCO, sigmas=sample_ref.COCO_SIGMAS, seed=5)
    assert got["status"].tolist() == want["status"].tolist() == [0, 1, 0]
    assert all((got[k][1] == 0).all() for k in OUTS + MASKS)
    assert all((got[k][[0, 2]] == 1).all() for k in MASKS) and np.isfinite(got["pose2d"]).all()


@functools.lru_cache(maxsize=None)
def _rot_bar():
    """4 x the fp32 restatement's error of the drawn rotation (rot_factor 30), over 4096 draws."""
    r64, r32 = (sample_ref.draw_aug(17, 0, 4096, 30.0, True, dt)[0] for dt in (np.float64, np.float32))
    return 4.0 * float(np.abs(r32.astype(np.float64) - r64).max())


@functools.lru_cache(maxsize=None)
def _noise_chain_case(mode):
    c = sample_cases.chain_case(65, 63, 80 + mode, "coco" if mode == sample_ref.NOISE_COCO else "human36")
    kw = dict(rot=None, flip=None, rot_factor=30.0, flip_enabled=True, noise=mode, seed=777, first_index=(1 << 33) + 3)
    if mode == sample_ref.NOISE_COCO:
        kw["sigmas"] = sample_ref.COCO_SIGMAS
    else:
        kw["table"] = sample_cases.table(17, seed=9)
    r64, r32 = _ref_chain(c, **kw), _ref_chain(c, np.float32, **kw)
    return c, kw, r64, r32


@pytest.mark.parametrize("mode", [sample_ref.NOISE_COCO, sample_ref.NOISE_TABLE])
def test_chain_with_noise_and_drawn_augmentation(hip_libs, mode):
    """rot and flip drawn from the stream, noise on: flip, the rot = 0 pattern, kind (on robust units) and the table's
    Bernoulli mask equal the restatement's exactly; rot and, for samples whose nine units are all robust, pose2d agree to
    4 x the fp32 restatement's error over the same 65 samples (those it decides like the float64 run).

    The seed is a condition of this test.  sample_ref's robustness band is derived for IDENTICAL fp32 inputs; here the
    kernel's noise step starts from the pixel coordinates and the area its own first launch computed, which differ from
    the restatement's (float64, rounded once) by the chain's fp32 error, 1e-5 .. 1e-4 px.  A candidate within that distance
    of its threshold but outside the band could be decided differently: the band's factor 2 covers most of it, the fixed
    seed (chain_case 81, stream seed 777) the rest.  Another seed may need another look, not a wider bar.  At most 5 % of
    the units may be non-robust (the audit's cap), so at least 0.95^9 = 63 % of the samples keep all nine: 60 % is asserted."""
    c, kw, r64, r32 = _noise_chain_case(mode)
    b = _builder(c, noise="coco" if mode == sample_ref.NOISE_COCO else "table", table=kw.get("table"), rotate_factor=30.0,
                 flip=True, seed=777)
    got = _run_chain(c, b, first=kw["first_index"], rot=None, flip=None)
    assert (got["status"] == 0).all() and (r64["status"] == 0).all()
    assert np.array_equal(got["rot_flip"][:, 1] != 0, r64["flip"]) and r64["flip"].any() and not r64["flip"].all()
    assert np.array_equal(got["rot_flip"][:, 0] == 0, r64["rot"] == 0) and (r64["rot"] != 0).any()
    assert np.abs(got["rot_flip"][:, 0] - r64["rot"]).max() <= _rot_bar()
    if mode == sample_ref.NOISE_COCO:
        ok = r64["robust"].all(axis=1)
        rj = r64["robust"][:, UNIT_OF]
        assert np.array_equal(got["kind"][rj], r64["kind"][rj]) and ok.mean() >= 0.6
        same = ok & (r32["kind"] == r64["kind"]).all(axis=1)
    else:
        ok = same = np.ones(65, bool)
    bar = 4.0 * float(np.abs(r32["pose2d"][same].astype(np.float64) - r64["pose2d"][same]).max())
    err = float(np.abs(got["pose2d"][ok] - r64["pose2d"][ok]).max())
    print(f"noise mode {mode}: samples compared {ok.sum()} of 65, pose2d worst {err:.3e}  bar {bar:.3e}")
    assert np.isfinite(got["pose2d"]).all() and err <= bar
    lbar = _chain_bar(c["joint_set"])["lift_pose3d"]
    assert np.abs(got["lift_pose3d"] - r64["lift_pose3d"]).max() <= max(lbar, 4.0 * float(
        np.abs(r32["lift_pose3d"].astype(np.float64) - r64["lift_pose3d"]).max()))


def test_chain_stream_properties(hip_libs):
    """Same state twice: bitwise equal.  Samples [0, 9) as one batch equal batches 4 + 5, per sample and bitwise, with the index
    advanced by the builder itself.  Over 4096 samples the drawn flips and the rot = 0 share sit within 5 binomial sigmas
    of 0.5, and both equal the restatement's draws."""
    c = sample_cases.chain_case(9, 63, 90, "coco")
    b = _builder(c, noise="coco", rotate_factor=30.0, flip=True, seed=31)
    v, f, p, t = (_cuda(c[k]) for k in ("verts", "focal", "princpt", "trans"))

    def run(first, parts):
        b.stream.seek(first)
        outs = [b(v[s], f[s], p[s], trans=t[s], out=b.buffers(s.stop - s.start)) for s in parts]
        return {k: torch.cat([getattr(o, k) for o in outs]) for k in OUTS + ("kind", "rot_flip", "status")}
    a1, a2, a3 = run(1000, [slice(0, 9)]), run(1000, [slice(0, 9)]), run(1000, [slice(0, 4), slice(4, 9)])
    for k in a1:
        assert torch.equal(a1[k], a2[k]) and torch.equal(a1[k], a3[k]), k
    assert not torch.equal(a1["pose2d"], run(1009, [slice(0, 9)])["pose2d"])
    n = 4096
    big = sample_cases.chain_case(n, 8, 91, "human36")
    bb = _builder(big, noise=None, rotate_factor=30.0, flip=True, seed=17)
    o = bb(_cuda(big["verts"]), _cuda(big["focal"]), _cuda(big["princpt"]), trans=_cuda(big["trans"]))
    rf = o.rot_flip.cpu().numpy()
    rot, flip = sample_ref.draw_aug(17, 0, n, 30.0, True)
    assert np.array_equal(rf[:, 1] != 0, flip) and np.array_equal(rf[:, 0] == 0, rot == 0)
    assert np.abs(rf[:, 0] - rot).max() <= _rot_bar()
    assert np.abs(rf[:, 0]).max() <= 60.0
    for share in ((rf[:, 1] != 0).mean(), (rf[:, 0] == 0).mean()):
        assert abs(share - 0.5) <= 5 * np.sqrt(0.25 / n)


def test_chain_graph_capture(hip_libs):
    """A builder call, the index advance included, captured in a torch.cuda.graph and replayed twice gives the eager
    results for indices i and i + B."""
    c = sample_cases.chain_case(9, 63, 95, "coco")
    b = _builder(c, noise="coco", rotate_factor=30.0, flip=True, seed=3)
    v, f, p, t = (_cuda(c[k]) for k in ("verts", "focal", "princpt", "trans"))
    b.stream.seek(500)
    eager = []
    for _ in range(2):
        o = b(v, f, p, trans=t)
        eager.append({k: getattr(o, k).clone() for k in OUTS + MASKS + ("kind", "rot_flip", "status")})
    out = b.buffers(9)
    b(v, f, p, trans=t, out=out)              # warm-up outside the capture
    torch.cuda.synchronize()
    b.stream.seek(500)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b(v, f, p, trans=t, out=out)
    for r in range(2):
        g.replay()
        torch.cuda.synchronize()
        for k, e in eager[r].items():
            assert torch.equal(getattr(out, k), e), (r, k)
    assert b.stream.index == 500 + 18


def test_chain_given_joints(hip_libs):
    """Human36M's annotated reg joints: fit_err against the restatement, status bit 1 and the masks of :396-400 over the
    threshold, reg_pose3d from the given joints."""
    c = sample_cases.chain_case(4, 63, 42, "coco")
    given = sample_cases.given_joints(c, _ref_chain(c))
    want = _ref_chain(c, given_cam=given, fit_thr=30.0)
    got = _run_chain(c, _builder(c, noise=None, fit_thr=30.0), given=(_cuda(given), None))
    assert got["status"].tolist() == want["status"].tolist() == [0, 0, 2, 2]
    # fit_err in fp32, C = the largest coordinate (the regressed joints are absolute: the cloud, within 2 m of trans): a mean
    # of 17 terms errs by <= 17 u C, each of the two centred sets by <= 18 u C, their difference by <= 37 u C per component,
    # a distance over three components by <= 64 u C
    C = 1000.0 * (float(np.abs(c["trans"]).max()) + 2.0)
    assert np.abs(got["fit_err"] - want["fit_err"]).max() <= 64 * 2.0 ** -24 * C
    for k in MASKS:
        assert np.array_equal(got[k], want[k]), k
    assert (got["mesh_valid"][2:] == 0).all() and (got["lift_valid"][2:] == 0).all() and (got["reg_valid"] == 1).all()
    bar = _chain_bar("coco")
    for k in OUTS:
        assert np.abs(got[k] - want[k]).max() <= bar[k], k
    # the human36 input set takes the given 2D joints too
    h = sample_cases.chain_case(4, 63, 43, "human36")
    base = _ref_chain(h)
    gcam, gimg = sample_cases.given_joints(h, base), (base["img"] + 3.0).astype(np.float32)
    want = _ref_chain(h, given_cam=gcam, given_img=gimg, fit_thr=30.0)
    got = _run_chain(h, _builder(h, noise=None, fit_thr=30.0), given=(_cuda(gcam), _cuda(gimg)))
    assert got["status"].tolist() == [0, 0, 2, 2] and (got["lift_valid"] == 1).all() and (got["mesh_valid"][2:] == 0).all()
    assert np.abs(got["pose2d"] - want["pose2d"]).max() <= _chain_bar("human36")["pose2d"]


def test_chain_refusals(hip_libs):
    """J > 32 chain joints, midpoints > 4, NULL state, unknown noise_mode: P2M_ERR_INVALID, nothing launched."""
    lib = _lib.hip()
    z = torch.zeros(1 << 16, device="cuda")
    iz = torch.zeros(64, dtype=torch.int32, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    mids = np.zeros((5, 2), np.int32)
    import ctypes
    order = ("verts trans mesh_scale focal princpt B nv rr_ptr rr_idx rr_val Jr reg_root ir_ptr ir_idx ir_val Ji midpoints n_mid "
             "input_root given_cam given_img fit_thr rot flip rot_factor flip_enabled noise_mode sigmas tab_mean tab_std tab_weight "
             "flip_pairs n_pairs W H state workspace workspace_bytes pose2d mesh lift reg mesh_valid lift_valid reg_valid status "
             "fit_err kind rot_flip stream").split()
    p, ip = z.data_ptr(), iz.data_ptr()
    base = dict(verts=p, trans=None, mesh_scale=1000.0, focal=p, princpt=p, B=1, nv=8, rr_ptr=ip, rr_idx=ip, rr_val=p, Jr=17,
                reg_root=0, ir_ptr=ip, ir_idx=ip, ir_val=p, Ji=17, midpoints=mids.ctypes.data_as(ctypes.c_void_p), n_mid=2,
                input_root=17, given_cam=None, given_img=None, fit_thr=0.0, rot=None, flip=None, rot_factor=0.0, flip_enabled=0,
                noise_mode=0, sigmas=p, tab_mean=p, tab_std=p, tab_weight=p, flip_pairs=None, n_pairs=0, W=288.0, H=384.0,
                state=st.data_ptr(), workspace=p, workspace_bytes=1 << 16, pose2d=p, mesh=p, lift=p, reg=p, mesh_valid=p,
                lift_valid=p, reg_valid=p, status=ip, fit_err=None, kind=None, rot_flip=None, stream=None)

    def refused(word, **over):
        a = dict(base, **over)
        assert lib.p2m_train_sample(*[a[k] for k in order]) == -1
        assert word in lib.p2m_last_error_string(), lib.p2m_last_error_string()
    refused(b"J = Ji + midpoints", Ji=31)
    refused(b"Jr outside", Jr=33)
    refused(b"midpoints outside", n_mid=5)
    refused(b"state", state=None)
    refused(b"noise_mode", noise_mode=3)
    refused(b"noise_mode", noise_mode=-1)
    refused(b"coco noise", noise_mode=1, Ji=10, input_root=0)
    refused(b"workspace", workspace_bytes=16)
    refused(b"input_root", input_root=19)
    torch.cuda.synchronize()
    assert (z == 0).all() and (iz == 0).all()
    with pytest.raises(_lib.P2MError):
        c = sample_cases.chain_case(2, 8, 1, "human36")
        _builder(c, noise=None)(torch.from_numpy(c["verts"]), _cuda(c["focal"]), _cuda(c["princpt"]))
    with pytest.raises(ValueError):
        _builder(sample_cases.chain_case(2, 8, 1, "human36"), noise="gaussian")
