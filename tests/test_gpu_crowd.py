"""-m gpu: the crowd kernels (p2m_crowd_select, p2m_person_colours; crowd.CrowdFilter, crowd.person_colours) against the float64
yardstick (tests/crowd_ref.py) on the cases of tests/crowd_cases.py.  Everything is compared EXACTLY: integer outputs equal,
float outputs bit for bit (NaN slots as NaN).  tests/test_crowd_cpu.py shows that each hand-made case is decided by the rule
it names and that the random crowds keep clear of both thresholds, so the order of a float64 sum decides nothing here."""
import numpy as np
import pytest
import torch

import camfit_ref
import crowd_cases as cc
import crowd_ref
import render_cases

pytestmark = pytest.mark.gpu

CASES = cc.cases()
OUTPUTS = ("keep", "reason", "dup_of", "count", "index", "score", "joints")


@pytest.fixture(scope="module")
def cr(hip_libs):
    from pose2mesh_release_amd import crowd
    return crowd


@pytest.fixture(scope="module")
def yard():
    """The yardstick's outputs, computed once per case."""
    return {n: crowd_ref.select(c["dets"], c["num"], **c["kw"]) for n, c in CASES.items()}


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def host(ns):
    torch.cuda.synchronize()
    return {k: getattr(ns, k).cpu().numpy().copy() for k in vars(ns)}


def same(a, b):
    """Equal integers; equal bits for floats, with NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def run_case(cr, c):
    sel = cr.CrowdFilter(**c["kw"])
    return host(sel(dev(c["dets"]), None if c["num"] is None else dev(c["num"], torch.int32)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_against_the_yardstick(cr, yard, name):
    out, ref = run_case(cr, CASES[name]), yard[name]
    for k in OUTPUTS:
        assert same(out[k], ref[k]), (name, k, out[k], ref[k])
    for k, want in CASES[name]["expect"].items():
        assert np.array_equal(out[k][0], np.asarray(want, out[k].dtype).reshape(out[k][0].shape)), (name, k)


def test_an_image_depends_on_itself_alone(cr):
    dets, num = CASES["random_crowds"]["dets"], np.array([32, 17, 0, 32, 5, 31, 32, 1], np.int32)
    sel = cr.CrowdFilter()
    alone = host(sel(dev(dets[:1]), dev(num[:1], torch.int32)))
    alone17 = host(sel(dev(dets[1:2]), dev(num[1:2], torch.int32)))
    for pos in range(5):
        order = [2, 3, 4, 5, 6]
        order[pos] = 0
        order[(pos + 2) % 5] = 1
        out = host(sel(dev(dets[order]), dev(num[order], torch.int32)))
        for k in OUTPUTS:
            assert same(out[k][pos], alone[k][0]), (pos, k)
            assert same(out[k][(pos + 2) % 5], alone17[k][0]), (pos, k)
    again = host(sel(dev(dets[:1]), dev(num[:1], torch.int32)))
    assert all(same(again[k], alone[k]) for k in OUTPUTS)


# ---- colours ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, seed, first", cc.COLOUR_RUNS)
def test_colours_against_the_yardstick(cr, n, seed, first):
    from pose2mesh_release_amd import sample
    for s, v in cc.TIE_SV:
        st = sample.NoiseStream(seed, first)
        out = host(cr.person_colours(n, stream=st, s=s, v=v))
        rgb, u8 = crowd_ref.colours(seed, first, n, s, v)
        assert same(out["rgb"], rgb) and same(out["u8"], u8), (n, seed, first, s, v)
        assert st.index == (first + n) & 0xFFFFFFFFFFFFFFFF
    if n == 256:                                           # every sector of the hue circle is hit
        sector = (crowd_ref.hues(seed, first, n) * 6.0).astype(int) % 6
        assert set(sector) == set(range(6))


def test_stream_contract(cr):
    from pose2mesh_release_amd import camfit, sample
    st = sample.NoiseStream(77, 0)
    a = host(cr.person_colours(4, stream=st))
    assert st.index == 4
    b = host(cr.person_colours(4, stream=st))
    assert st.index == 8 and a["rgb"].tobytes() != b["rgb"].tobytes()
    st.seek(0)
    again = host(cr.person_colours(8, stream=st))
    assert again["rgb"].tobytes() == np.concatenate([a["rgb"], b["rgb"]]).tobytes()
    assert again["u8"].tobytes() == np.concatenate([a["u8"], b["u8"]]).tobytes()
    seeded = host(cr.person_colours(4, seed=77))
    assert seeded["rgb"].tobytes() == a["rgb"].tobytes()
    # shared with the camera fit: the fitter draws stage 10 at the indices that follow, as documented, and stage 11 at an
    # index is not stage 10's word at that index
    st.seek(0)
    cr.person_colours(4, stream=st)
    fit = camfit.CameraFitter(steps=0, stream=st)
    cam = host(fit(torch.zeros(3, 17, 3, device="cuda"), torch.zeros(3, 17, 2, device="cuda")))["cam"]
    assert cam.tobytes() == camfit_ref.start(77, 4, 3).astype(np.float32).tobytes() and st.index == 7
    assert not np.isin(crowd_ref.hues(77, 0, 8), camfit_ref.start(77, 0, 8)).any()
    after = host(cr.person_colours(2, stream=st))
    assert same(after["rgb"], crowd_ref.colours(77, 7, 2)[0])


def test_capture_and_replay(cr):
    from pose2mesh_release_amd import sample
    dets = CASES["random_crowds"]["dets"]
    static = dev(dets[:4])
    sel, st = cr.CrowdFilter(), sample.NoiseStream(5, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = sel(static)                                   # allocates the buffers
        col = cr.person_colours(32, stream=st)              # index -> 32
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = host(out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = sel(static)
        col_g = cr.person_colours(32, stream=st, out=col)
    assert out_g is out and col_g is col
    graph.replay()
    first, first_col = host(out_g), host(col_g)
    assert all(same(first[k], eager[k]) for k in OUTPUTS)
    static.copy_(dev(dets[4:]))                             # new detections in the static input
    graph.replay()
    second, second_col = host(out_g), host(col_g)
    ref = crowd_ref.select(dets[4:])
    assert all(same(second[k], ref[k]) for k in OUTPUTS)
    assert not same(second["keep"], first["keep"])
    assert st.index == 96
    assert same(first_col["rgb"], crowd_ref.colours(5, 32, 32)[0]) and same(second_col["rgb"], crowd_ref.colours(5, 64, 32)[0])
    assert same(second_col["u8"], crowd_ref.colours(5, 64, 32)[1]) and first_col["rgb"].tobytes() != second_col["rgb"].tobytes()


# ---- absent people through the existing chain ---------------------------------------------------------------------------------
VIS_SKELETON = ((0, 1), (0, 2), (2, 4), (1, 3), (5, 7), (7, 9), (12, 14), (14, 16), (11, 13), (13, 15), (5, 17), (6, 17), (11, 18),
                (12, 18), (17, 18), (17, 0), (6, 8), (8, 10))


def test_absent_people_ride_through_the_chain(cr):
    """CrowdFilter -> prepare_pose -> CameraFitter -> crop_cam_to_image -> MeshRenderer(scene) -> PoseOverlay.coco_skeleton with
    4 slots, 2 of them empty, gives bit for bit the picture of the chain run on the two accepted people alone.  The fitter
    learns of an empty slot through its weights, (prep.status == 0): prepare_pose zeroes such a sample's target, which is
    finite, and weights summing to 0 are what makes p2m_camera_fit return cam = 0 with status bit 0."""
    from pose2mesh_release_amd import camfit, overlay, render
    H = W = 64
    rng = np.random.default_rng(9)
    j3 = rng.normal(0, 0.25, (17, 3)).astype(np.float32)
    base = np.zeros((17, 3), np.float32)
    base[:, :2] = np.array([20.0, 22.0]) + 28.0 * j3[:, :2]
    base[:, 2] = 0.875
    weak, twin, other = base.copy(), base.copy(), base.copy()
    weak[:, :2] += (9.0, -4.0)
    weak[:, 2] = 0.05                                       # score 0.85
    twin[:, :2] += rng.normal(0, 2.0, (17, 2)).astype(np.float32)
    other[:, :2] += (25.0, 21.0)                            # mean distance 23 >= 20
    dets = np.stack([base, weak, twin, other])[None]
    ref = crowd_ref.select(dets)
    assert ref["reason"][0].tolist() == [0, 1, 2, 0]
    verts, faces = render_cases.hull(64)
    mesh = dev(0.3 * verts[None] + rng.normal(0, 0.02, (4, 1, 3)).astype(np.float32))
    joints3d = dev(np.concatenate([j3[None]] * 4) + rng.normal(0, 0.01, (4, 17, 3)).astype(np.float32))
    joints3d = torch.cat([joints3d, joints3d[:, [11, 5]]], 1)                          # 19 joints, as the regressor gives
    cam0 = dev(rng.uniform(0.3, 0.9, (4, 3)))
    colours = cr.person_colours(4, seed=3)
    background = dev(render_cases.background(H, W, 4), torch.uint8)
    swap = torch.tensor(list(range(17)) + [18, 17], device="cuda")                     # run.py:322, pelvis <-> thorax

    def chain(people, n):
        """people [1, n, 19, 3] as CrowdFilter returns them."""
        px = people[0]
        prep = camfit.prepare_pose(px)
        weight = (prep.status == 0).to(torch.float32)[:, None].expand(n, 19)
        fit = camfit.CameraFitter(steps=300)(joints3d[:n], prep.target, weight=weight, cam0=cam0[:n])
        cam_img = render.crop_cam_to_image(fit.cam, prep.bbox, W, H)
        out = render.MeshRenderer(faces, H, W, mode="scene")(mesh[:n], cam_img, colours.rgb[:n], background=background)
        skel = overlay.PoseOverlay.coco_skeleton(VIS_SKELETON, H, W)
        img = skel(out["image"], people[:, :, swap], colours=colours.u8[None, :n])["image"]
        torch.cuda.synchronize()
        return prep, fit, out, img.cpu().numpy().copy()

    sel = cr.CrowdFilter()(dev(dets))
    assert same(host(sel)["joints"], ref["joints"]) and int(sel.count[0]) == 2
    prep, fit, out, img = chain(sel.joints, 4)
    assert prep.status.tolist() == [0, 0, 1, 1]
    assert (fit.status.cpu() & 1).tolist() == [0, 0, 1, 1] and not fit.cam[2:].any() and fit.cam[:2].all()
    ids = set(out["mesh_id"].unique().tolist())
    print(f"chain: cam {fit.cam.tolist()}, render status {out['status'].tolist()}, mesh ids {sorted(ids)}, "
          f"pixels per mesh {[int((out['mesh_id'] == k).sum()) for k in range(4)]}")
    assert ids - {-1} == {0, 1}, ids
    two = dev(dets[:, [0, 3]])
    sel2 = cr.CrowdFilter()(two)
    assert int(sel2.count[0]) == 2
    _, fit2, out2, img2 = chain(sel2.joints, 2)
    assert fit2.cam.cpu().numpy().tobytes() == fit.cam[:2].cpu().numpy().tobytes()
    assert same(out2["mesh_id"].cpu().numpy(), out["mesh_id"].cpu().numpy())
    assert img.tobytes() == img2.tobytes() and (img != background.cpu().numpy()[None]).any()


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_argument_errors(cr):
    from pose2mesh_release_amd import _lib, sample
    from pose2mesh_release_amd._lib import P2MError
    good = dev(CASES["greedy_chain"]["dets"])
    z = lambda *sh: torch.zeros(sh, device="cuda")         # noqa: E731
    bad_calls = [
        lambda: cr.CrowdFilter()(good.cpu()),                                          # no CPU path
        lambda: cr.CrowdFilter()(good, num=torch.zeros(1, dtype=torch.int32)),
        lambda: cr.CrowdFilter()(z(0, 3, 17, 3)),                                      # B < 1
        lambda: cr.CrowdFilter()(z(1, 0, 17, 3)),                                      # P outside [1, 64]
        lambda: cr.CrowdFilter()(z(1, 65, 17, 3)),
        lambda: cr.CrowdFilter()(z(1, 3, 63, 3)),                                      # Jo = 65
        lambda: cr.CrowdFilter(midpoints=())(z(1, 3, 65, 3)),
        lambda: cr.CrowdFilter(midpoints=((0, 1),) * 9)(z(1, 3, 17, 3)),               # more than 8 midpoints
        lambda: cr.CrowdFilter(midpoints=((11, 17),))(good),                           # a midpoint index outside [0, J)
        lambda: cr.CrowdFilter(midpoints=((-1, 5),))(good),
        lambda: cr.CrowdFilter()(z(1, 3, 11, 3)),                                      # the default midpoints need J >= 13
        lambda: cr.CrowdFilter(pose_thr=float("nan"))(good),                           # thresholds that are not finite
        lambda: cr.CrowdFilter(score_thr=float("inf"))(good),
        lambda: cr.CrowdFilter(min_diff=float("-inf"))(good),
        lambda: cr.person_colours(0, seed=1),
        lambda: cr.person_colours(4, seed=1, s=1.5),
        lambda: cr.person_colours(4, seed=1, v=float("nan")),
        lambda: cr.person_colours(4, device="cpu"),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(P2MError):
            call()
            pytest.fail(f"call {k} did not raise")
    lib, i32 = _lib.hip(), torch.int32
    o = dict(j=z(1, 3, 19, 3), c=torch.zeros(1, dtype=i32, device="cuda"), i=torch.zeros(1, 3, dtype=i32, device="cuda"),
             r=torch.zeros(1, 3, dtype=torch.int8, device="cuda"), d=torch.zeros(1, 3, dtype=i32, device="cuda"),
             s=torch.zeros(1, 3, dtype=torch.float64, device="cuda"), k=torch.zeros(1, 3, dtype=torch.bool, device="cuda"))
    import ctypes
    mid = (ctypes.c_int32 * 4)(11, 12, 5, 6)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    args = [ptr(good), None, 1, 3, 17, mid, 2, 0.1, 1.5, 20.0] + [ptr(o[k]) for k in "jcirdsk"] + [None]
    for k in (0, 5, 10, 11, 12, 13, 14, 15, 16):           # each required pointer NULL in turn
        a = list(args)
        a[k] = None
        assert lib.p2m_crowd_select(*a) == -1, k
    st = sample.NoiseStream(1, 0)
    assert lib.p2m_person_colours(None, 4, 0.5, 1.0, ptr(o["j"]), None, None) == -1
    assert lib.p2m_person_colours(ptr(st.state), 4, 0.5, 1.0, None, None, None) == -1
    # and the module still works
    out = host(cr.CrowdFilter()(good))
    assert out["reason"][0].tolist() == [0, 2, 0]
    assert same(host(cr.person_colours(7, seed=123))["u8"], crowd_ref.colours(123, 0, 7)[1])
