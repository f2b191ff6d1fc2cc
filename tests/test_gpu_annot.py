"""GPU: the annotation layer (pose2mesh_release_amd.annot, csrc/annot.hip) against its float64 yardstick tests/annot_ref.py
on the seeded cases of tests/annot_cases.py.

Bars.  Row copies are bitwise.  pose_out[:3] and trans_out are within ONE fp32 ulp of the yardstick's fp32 value: both
sides round the same float64 quantity, and the device's float64 sin / cos / atan2 / sqrt (and its fused multiply-adds) differ
from numpy's by ~1e-16, so the two can differ only across a rounding boundary.  The exactly-pi row compares rotation
matrices to 1e-6 instead (its axis sign is undefined).  The chain through the body models takes the forward's own bar from
tests/test_gpu_body.py: 4 x the fp32-vs-float64 error of the companion batch."""
import ctypes

import numpy as np
import pytest
import torch

import annot_cases
import annot_ref
import body_ref
import test_gpu_body as forward_tests
from pose2mesh_release_amd import _lib, annot, sample, synth

pytestmark = pytest.mark.gpu
KEYS = ("pose", "betas", "trans", "focal", "princpt", "gender", "given_cam", "given_img", "status")


def _source(c, models="tables"):
    t = c["tables"]
    if models == "tables":
        models = (c["root_template"], c["root_shapedirs"])
    R = None if t["cam_R"] is None else t["cam_R"].reshape(-1, 3, 3)
    return annot.AnnotationSource(t["pose"], t["betas"], t["trans"], R, t["cam_t"], focal=t["focal"], princpt=t["princpt"],
                                  gender=t["gender"], given_cam=t["given_cam"], given_img=t["given_img"], models=models,
                                  preset=c["preset"])


def _idx(a, dtype=torch.int64):
    return torch.from_numpy(np.asarray(a, np.int64)).to(dtype).cuda()


def _np(batch):
    torch.cuda.synchronize()
    return {k: None if getattr(batch, k) is None else getattr(batch, k).cpu().numpy().copy() for k in KEYS}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _compare(got, want, c, idx, what):
    """The bars of the module docstring, for the samples of one call."""
    t = c["tables"]
    for k in ("betas", "focal", "princpt", "gender", "status", "given_cam", "given_img"):
        assert (got[k] is None) == (want[k] is None), (what, k)
        if want[k] is not None:
            assert got[k].dtype == want[k].dtype and _same_bits(got[k], want[k]), (what, k)
    assert _same_bits(got["pose"][:, 3:], want["pose"][:, 3:]), what
    d_t = annot_ref.ulp_diff(got["trans"], want["trans"])
    d_p = annot_ref.ulp_diff(got["pose"][:, :3], want["pose"][:, :3])
    pi_rows = [b for b, r in enumerate(idx) if r == annot_cases.PI_ROW and c["N"] >= annot_cases.N_SPECIAL and c["flags"]["rotate_root"]]
    for b in pi_rows:
        r = idx[b]
        R = np.eye(3) if t["cam_R"] is None else t["cam_R"][r].astype(np.float64).reshape(3, 3)
        M = R @ annot_ref.exp_root(t["pose"][r, :3])
        e = float(np.abs(annot_ref.exp_root(got["pose"][b, :3]) - M).max())
        print(f"{what}: exactly-pi sample {b}: max |exp(pose_out) - R exp(root)| {e:.3e}")
        assert e <= 1e-6, (what, b, e)
        assert abs(np.linalg.norm(got["pose"][b, :3].astype(np.float64)) - np.pi) < 1e-6
        d_p[b] = 0
    print(f"{what}: max ulp distance pose[:3] {int(d_p.max())}, trans {int(d_t.max())}; status bits {sorted(set(want['status'].tolist()))}")
    assert np.isfinite(got["pose"]).all() and np.isfinite(got["trans"]).all(), what
    if not c["flags"]["rotate_root"]:
        assert _same_bits(got["pose"][:, :3], want["pose"][:, :3]), what
    assert d_p.max() <= 1 and d_t.max() <= 1, (what, int(d_p.max()), int(d_t.max()))


@pytest.mark.parametrize("i", range(len(annot_cases.CASES)), ids=annot_cases.case_ids())
def test_gather_and_glue(hip_libs, i):
    c = annot_cases.case(i)
    src = _source(c)
    want = annot_cases.reference(c)
    got = _np(src(_idx(c["idx"], torch.int64 if i % 2 == 0 else torch.int32)))
    _compare(got, want, c, c["idx"], annot_cases.case_ids()[i])
    if c["flags"]["beta_reset"] and c["N"] >= annot_cases.N_SPECIAL and c["B"] == 37:
        st = dict(zip(c["idx"][:8].tolist(), want["status"][:8].tolist()))
        assert st[6] & annot_ref.BETA_RESET and not st[5] & annot_ref.BETA_RESET
    if c["G"] > 1 and c["N"] >= annot_cases.N_SPECIAL and c["B"] == 37:
        assert want["status"][7] & annot_ref.BAD_GENDER and got["gender"][7] == 0


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_out_of_range_indices_and_genders(hip_libs, dtype):
    """idx = -1 and N: status bit 0, every output of the sample zero (the buffers are pre-filled), the other samples of the
    batch bitwise what they are without them.  Row 7 carries gender = G: bit 1, model 0, gender_out 0."""
    c = annot_cases.case(0)
    N = c["N"]
    src = _source(c)
    clean = [5, 9, 7, 0, N - 1]
    mixed = [5, -1, 9, N, 7, 0, N - 1, -(2 ** 31) if dtype == torch.int32 else -(2 ** 40), 2 ** 31 - 1 if dtype == torch.int32 else 2 ** 40]
    keep, bad = [0, 2, 4, 5, 6], [1, 3, 7, 8]
    base = _np(src(_idx(clean, dtype)))
    out = src.buffers(len(mixed))
    for k in KEYS:
        getattr(out, k).fill_(float("nan") if getattr(out, k).dtype == torch.float32 else 77)
    got = _np(src(_idx(mixed, dtype), out=out))
    assert got["status"][bad].tolist() == [annot_ref.BAD_INDEX] * 4
    for k in KEYS[:-1]:
        assert not _bits(got[k][bad]).any(), k
        assert _same_bits(got[k][keep], base[k]), k
    assert np.array_equal(got["status"][keep], base["status"])
    assert got["status"][4] & annot_ref.BAD_GENDER and got["gender"][4] == 0
    _compare(got, annot_cases.reference(c, mixed), c, mixed, f"mixed {dtype}")


def _select(srcs, gender, B, V, NJ, JX, outs):
    G = len(srcs[0])
    arrs = [(ctypes.c_void_p * G)(*[s.data_ptr() for s in group]) if group else None for group in srcs]
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    return _lib.hip().p2m_body_select(arrs[0], arrs[1], arrs[2], G, p(gender), B, V, NJ, JX, p(outs[0]), p(outs[1]), p(outs[2]),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("V", [31, 300, 301])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_select(hip_libs, V, offset):
    """G = 3 sources of distinct patterns, B = 37 with every gender present (and two out of range, which count as 0) and one
    batch of a single gender; 3 V floats per sample is a multiple of 4 only for V = 300, so vectors straddle samples.  The
    outputs start `offset` floats into their allocations (a sliced tensor): the unaligned heads and tails, with guard words
    around them."""
    B, NJ, JX, G = 37, 24, 17 if V != 300 else 0, 3
    rng = np.random.default_rng(V)
    sizes = [n for n in (V, NJ, JX) if n]
    srcs = [[torch.from_numpy((rng.standard_normal((B, n, 3)) + 10 * (g + 1)).astype(np.float32)).cuda() for g in range(G)]
            for n in sizes] + [[]] * (3 - len(sizes))
    mixed = np.concatenate([[0, 1, 2, 5, -1, 2, 2, 1], rng.integers(0, G, B - 8)]).astype(np.int32)
    for gender in (mixed, np.full(B, 1, np.int32), np.full(B, 2, np.int32)):
        flat = [torch.full((B * n * 3 + 8,), -7.0, device="cuda") for n in sizes]
        outs = [f[offset:offset + B * n * 3].view(B, n, 3) for f, n in zip(flat, sizes)] + [None] * (3 - len(sizes))
        assert all(o.data_ptr() % 16 == 4 * offset for o in outs if o is not None)
        rc = _select(srcs, torch.from_numpy(gender).cuda(), B, V, NJ, JX, outs)
        torch.cuda.synchronize()
        assert rc == 0, _lib.hip().p2m_last_error_string()
        for group, o, f, n in zip(srcs, outs, flat, sizes):
            want = annot_ref.select([s.cpu().numpy() for s in group], gender)
            assert _same_bits(o.cpu().numpy(), want), (V, offset, n)
            guard = f.cpu().numpy()
            assert (guard[:offset] == -7.0).all() and (guard[offset + B * n * 3:] == -7.0).all(), (V, offset, n)


def _chain(c, bank, idx):
    src = _source(c, models=bank)
    batch = src(idx)
    out = bank(batch.pose, batch.betas, batch.trans, batch.gender)
    torch.cuda.synchronize()
    return batch, [o.cpu().numpy().copy() for o in out]


@pytest.mark.parametrize("V", [31, 300, 301])
@pytest.mark.parametrize("kind", ["smpl", "mano"])
def test_chain_against_float64(hip_libs, kind, V):
    """bank(src(idx)) against body_ref.forward on the yardstick's parameters, each sample with its own model."""
    c = annot_cases.chain_case(kind, V)
    bank = annot_cases.bank(kind, V, 3, True)
    models = annot_cases.model_dicts(kind, V, 3)
    reg = synth.synthetic_regressor(annot_cases.JR, V, seed=7)
    want_p = annot_cases.reference(c)
    batch, got = _chain(c, bank, _idx(c["idx"]))
    _compare(_np(batch), want_p, c, c["idx"], f"chain {kind} V={V} parameters")
    want = [np.zeros_like(g, dtype=np.float64) for g in got]
    for b in range(c["B"]):
        m = models[want_p["gender"][b]]
        for w, o in zip(want, body_ref.forward(m, want_p["pose"][b:b + 1], want_p["betas"][b:b + 1], want_p["trans"][b:b + 1], None, reg)):
            w[b] = o[0]
    assert len(set(want_p["gender"].tolist())) == 3
    forward_tests._check(got, want, 4 * forward_tests._companion_err32(kind, True, None), f"chain {kind} V={V}")


def test_single_model_bank_returns_the_models_buffers(hip_libs):
    m = annot_cases.body_model(annot_cases.model_dicts("smpl", 31, 1)[0])
    bank = annot.GenderedBody([m])
    c = annot_cases.case(annot_cases.CASES.index(("human36m", "smpl", 1000, 5, 1)))
    batch = _source(c, models=bank)(_idx(c["idx"]))
    v, j = bank(batch.pose, batch.betas, batch.trans, batch.gender)
    v2, j2 = m(batch.pose, batch.betas, batch.trans)
    assert v.data_ptr() == v2.data_ptr() and j.data_ptr() == j2.data_ptr() and not bank._bufs


def test_batch_independence(hip_libs):
    """A sample's parameters and meshes are bitwise the same at B = 1 and inside B = 37."""
    c = annot_cases.chain_case("smpl", 301)
    bank = annot_cases.bank("smpl", 301, 3, True)
    batch, full = _chain(c, bank, _idx(c["idx"]))
    full_p = _np(batch)
    for b in (0, 2, 7, 8, 36):
        one_b, one = _chain(c, bank, _idx(c["idx"][b:b + 1], torch.int32))
        one_p = _np(one_b)
        for k in KEYS:
            assert _same_bits(one_p[k][0], full_p[k][b]), (b, k)
        for name, a, f in zip(("verts", "joints", "extra"), one, full):
            assert _same_bits(a[0], f[b]), (b, name)


def test_capture_replays_bitwise(hip_libs):
    """src + bank + TrainSampleBuilder (no noise, rot / flip given) captured on one stream; after idx.copy_(other) the replay
    is bitwise the eager chain, and allocates nothing."""
    V, B = 301, 37
    c = annot_cases.chain_case("smpl", V)
    reg = synth.synthetic_regressor(annot_cases.JR, V, seed=7)
    rot = torch.linspace(-20, 20, B, device="cuda")
    flip = (torch.arange(B, device="cuda") % 2).to(torch.int32)
    pairs = ((1, 4), (2, 5), (3, 6), (14, 11), (15, 12), (16, 13))

    def make():
        bank = annot.GenderedBody([annot_cases.body_model(m, reg) for m in annot_cases.model_dicts("smpl", V, 3)])
        return _source(c, models=bank), bank, sample.TrainSampleBuilder(reg, None, (), (0, 0), pairs, noise=None)

    def chain(parts, idx):
        src, bank, build = parts
        batch = src(idx)
        verts, joints, j_h36m = bank(batch.pose, batch.betas, batch.trans, batch.gender)
        s = build(verts, batch.focal, batch.princpt, given=(batch.given_cam, batch.given_img), rot=rot, flip=flip)
        return [batch.pose, batch.betas, batch.trans, batch.gender, batch.status, verts, joints, j_h36m, s.pose2d, s.mesh,
                s.lift_pose3d, s.reg_pose3d, s.mesh_valid, s.lift_valid, s.reg_valid, s.status]

    first = _idx(c["idx"])
    other = _idx(np.random.default_rng(3).integers(0, c["N"], B))
    eager = [o.clone() for o in chain(make(), other)]
    parts = make()
    static = first.clone()
    chain(parts, static)                                     # the buffers of this batch size exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain(parts, static)
    static.copy_(other)
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    before = (torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"])
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert before == (torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"])
    assert float(eager[9].abs().max()) > 0 and int((eager[15] == 0).sum()) > 0
    for k, (o, e) in enumerate(zip(outs, eager)):
        assert torch.equal(o.cpu(), e.cpu()), k


def test_cpu_tensors_raise(hip_libs):
    c = annot_cases.case(0)
    src = _source(c)
    with pytest.raises(_lib.P2MError):
        src(torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        src(torch.zeros(4, device="cuda"))
    bank = annot_cases.bank("smpl", 31, 3)
    batch = src(_idx(c["idx"]))
    with pytest.raises(_lib.P2MError):
        bank(batch.pose, batch.betas, batch.trans, batch.gender.cpu())


def test_c_entry_errors(hip_libs):
    """P2M_ERR_INVALID without a launch: the outputs keep their fill."""
    c = annot_cases.case(0)
    t = {k: None if v is None else torch.from_numpy(v).cuda() for k, v in c["tables"].items()}
    rt, rs = torch.from_numpy(c["root_template"]).cuda(), torch.from_numpy(c["root_shapedirs"]).cuda()
    B, N, J, nb = 4, c["N"], 24, 10
    idx = _idx([0, 1, 2, 3], torch.int32)
    o = {k: torch.full(sh, -5, device="cuda", dtype=dt) for k, sh, dt in (
        ("pose", (B, 72), torch.float32), ("betas", (B, nb), torch.float32), ("trans", (B, 3), torch.float32),
        ("focal", (B, 2), torch.float32), ("princpt", (B, 2), torch.float32), ("gender", (B,), torch.int32),
        ("given_cam", (B, 17, 3), torch.float32), ("given_img", (B, 17, 2), torch.float32), ("status", (B,), torch.int32))}
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731

    def call(**kw):
        a = dict(pose=p(t["pose"]), betas=p(t["betas"]), idx=p(idx), rt=p(rt), rs=p(rs), G=3, J=J, nb=nb, Jr=17, B=B, N=N,
                 compensate=1, status=p(o["status"]), pose_out=p(o["pose"]))
        a.update(kw)
        return _lib.hip().p2m_annot_gather(
            a["pose"], a["betas"], p(t["trans"]), p(t["cam_R"]), p(t["cam_t"]), p(t["focal"]), p(t["princpt"]), p(t["gender"]),
            p(t["given_cam"]), p(t["given_img"]), a["N"], a["J"], a["nb"], a["Jr"], a["idx"], 0, a["B"], a["rt"], a["rs"], a["G"],
            1, 1, a["compensate"], 3.0, 1e-3, a["pose_out"], p(o["betas"]), p(o["trans"]), p(o["focal"]), p(o["princpt"]),
            p(o["gender"]), p(o["given_cam"]), p(o["given_img"]), a["status"], None)

    bad = (dict(pose=None), dict(idx=None), dict(status=None), dict(pose_out=None), dict(betas=None), dict(G=5), dict(G=0),
           dict(rt=None), dict(rs=None), dict(J=0), dict(J=65), dict(nb=65), dict(nb=-1), dict(Jr=33), dict(B=0), dict(N=0),
           dict(pose=ctypes.c_void_p(t["pose"].data_ptr() + 2)))
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"p2m_annot_gather" in _lib.hip().p2m_last_error_string()
    torch.cuda.synchronize()
    assert all(bool((x == -5).all()) for x in o.values())
    assert call(compensate=0, rt=None, rs=None) == 0        # the root tables are optional without the compensation
    torch.cuda.synchronize()
    want = annot_ref.gather(c["tables"], [0, 1, 2, 3], 3, rotate_root=True, beta_reset=True, t_scale=1e-3)
    assert o["status"].tolist() == want["status"].tolist() and _same_bits(o["betas"].cpu().numpy(), want["betas"])
    srcs = [[torch.zeros(B, n, 3, device="cuda") for _ in range(3)] for n in (31, 24)] + [[]]
    outs = [torch.full((B, n, 3), -5.0, device="cuda") for n in (31, 24)] + [None]
    g = torch.zeros(B, dtype=torch.int32, device="cuda")
    assert _select(srcs, g, B, 31, 24, 0, outs) == 0
    assert _select([s + s[:1] * 2 for s in srcs], g, B, 31, 24, 0, outs) == -1                  # G = 5
    assert _select(srcs, None, B, 31, 24, 0, outs) == -1
    assert _select(srcs, g, B, 31, 24, 0, [srcs[0][1], outs[1], None]) == -1                    # an output that is a source
    assert _select(srcs, g, 0, 31, 24, 0, outs) == -1
