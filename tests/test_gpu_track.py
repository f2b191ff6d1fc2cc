"""-m gpu: the tracker (p2m_pose_track; track.PoseTracker, track.identity_colours) and OneEuroFilter.reset(mask=) against the
float64 yardstick (tests/track_ref.py) on the cases of tests/track_cases.py.  Everything is compared EXACTLY: integer outputs
equal, float outputs bit for bit (NaN slots as NaN), the state after the last frame included.  tests/test_track_cpu.py shows
that each hand-made case is decided by the rule it names."""
import ctypes

import numpy as np
import pytest
import torch

import track_cases as tc
import track_ref

pytestmark = pytest.mark.gpu

CASES = tc.cases()
OUTPUTS, STATE = track_ref.OUTPUTS, track_ref.STATE
VIEWS = (("alive", tc.A), ("present", tc.Pn), ("born", tc.B), ("fresh", tc.Fr), ("retired", tc.R))


@pytest.fixture(scope="module")
def tk(hip_libs):
    from pose2mesh_release_amd import track
    return track


@pytest.fixture(scope="module")
def yard():
    """The yardstick's outputs and final state, computed once per case."""
    return {n: tc.run_ref(c) for n, c in CASES.items()}


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def host(ns, keys=OUTPUTS):
    torch.cuda.synchronize()
    return {k: getattr(ns, k).cpu().numpy().copy() for k in keys}


def state_of(trk):
    return host(trk, STATE)


def same(a, b):
    """Equal integers; equal bits for floats, with NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def run_gpu(tk, c, chunk=None):
    trk = tk.PoseTracker(c["slots"], **c["kw"])
    out = tc.drive(c, lambda x: host(trk(dev(x))), lambda m: trk.reset(None if m is None else dev(m, torch.bool)), chunk)
    return out, state_of(trk)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_against_the_yardstick(tk, yard, name):
    c = CASES[name]
    (out, st), (ref, ref_st) = run_gpu(tk, c), yard[name]
    for k in OUTPUTS:
        assert same(out[k], ref[k]), (name, k, out[k], ref[k])
    for k in STATE:
        assert same(st[k], ref_st[k]), (name, k, st[k], ref_st[k])
    for f, k, want in c["expect"]:
        assert same(out[k][f, 0], np.asarray(want, out[k].dtype).reshape(out[k][f, 0].shape)), (name, f, k)


def test_views_and_the_one_frame_form(tk, yard):
    c = CASES["streams"]
    ref, _ = yard["streams"]
    trk = tk.PoseTracker(c["slots"], **c["kw"])
    for f in range(4):
        ns = trk(dev(c["people"][f]))                      # [S, P, Jo, 3] -> [S, T, ...]
        out = host(ns)
        assert all(same(out[k], ref[k][f]) for k in OUTPUTS), f
        for name, bit in VIEWS:
            v = getattr(ns, name)
            assert v.dtype == torch.bool and same(v.cpu().numpy(), (ref["flags"][f] & bit) != 0), (f, name)
    assert trk(dev(c["people"][4])) is ns                  # static buffers per input shape


def test_a_stream_depends_on_itself_alone(tk, yard):
    c = CASES["streams"]
    ref, ref_st = yard["streams"]
    for order in ([3, 0, 4], [1], [4, 3, 2, 1, 0, 2]):
        out, st = run_gpu(tk, dict(c, people=c["people"][:, order]))
        for pos, s in enumerate(order):
            assert all(same(out[k][:, pos], ref[k][:, s]) for k in OUTPUTS), (order, pos)
            assert all(same(st[k][pos], ref_st[k][s]) for k in STATE), (order, pos)


@pytest.mark.parametrize("name", ["walkers", "streams", "retired_slot_waits_a_frame"])
def test_one_call_of_f_frames_equals_f_calls_of_one(tk, name):
    c = CASES[name]
    whole, whole_st = run_gpu(tk, c)
    for chunk in (1, 7):
        out, st = run_gpu(tk, c, chunk=chunk)
        assert all(same(out[k], whole[k]) for k in OUTPUTS), (name, chunk)
        assert all(same(st[k], whole_st[k]) for k in STATE), (name, chunk)


def test_capture_and_replay(tk):
    c = CASES["streams"]
    x = c["people"]
    trk, eager = (tk.PoseTracker(c["slots"], **c["kw"]) for _ in range(2))
    static = dev(x[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        trk(static)                                        # allocates the state and the buffers
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    trk.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = trk(static)
    st = track_ref.new_state(x.shape[1], c["slots"], x.shape[3])
    track_ref.track(x[:1], st, **c["kw"])
    track_ref.reset(st)
    eager(dev(x[0]))
    eager.reset()
    for f in range(8):
        static.copy_(dev(x[f]))
        graph.replay()
        got, ref, eag = host(out_g), track_ref.track(x[f:f + 1], st, **c["kw"]), host(eager(dev(x[f])))
        assert all(same(got[k], ref[k][0]) for k in OUTPUTS), f
        assert all(same(got[k], eag[k]) for k in OUTPUTS), f
        assert same(out_g.fresh.cpu().numpy(), (ref["flags"][0] & tc.Fr) != 0)
    assert all(same(state_of(trk)[k], st[k]) for k in STATE)
    assert int(st["next_uid"].min()) > 5                   # the ids went on counting over the reset


def test_argument_errors(tk):
    from pose2mesh_release_amd import _lib
    from pose2mesh_release_amd._lib import P2MError
    good = dev(CASES["overflow"]["people"])
    z = lambda *sh: torch.zeros(sh, device="cuda")         # noqa: E731
    bad_calls = [
        lambda: tk.PoseTracker()(good.cpu()),                                          # no CPU path
        lambda: tk.PoseTracker()(z(0, 1, 3, 4, 3)),                                    # F < 1
        lambda: tk.PoseTracker()(z(0, 3, 4, 3)),                                       # S < 1
        lambda: tk.PoseTracker()(z(1, 0, 4, 3)),                                       # P outside [1, 64]
        lambda: tk.PoseTracker()(z(1, 65, 4, 3)),
        lambda: tk.PoseTracker(slots=0)(good),                                         # T outside [1, 64]
        lambda: tk.PoseTracker(slots=65)(good),
        lambda: tk.PoseTracker()(z(1, 3, 65, 3)),                                      # Jo outside [1, 64]
        lambda: tk.PoseTracker(min_common=0)(good),                                    # min_common outside [1, Jo]
        lambda: tk.PoseTracker(min_common=5)(good),
        lambda: tk.PoseTracker(max_missed=-1)(good),
        lambda: tk.PoseTracker(pose_thr=float("nan"))(good),                           # thresholds that are not finite
        lambda: tk.PoseTracker(gate=float("inf"))(good),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(P2MError):
            call()
            pytest.fail(f"call {k} did not raise")
    trk = tk.PoseTracker(2)
    trk(good)
    with pytest.raises(P2MError):
        trk.reset(torch.zeros(1, dtype=torch.bool))                                    # a CPU mask
    with pytest.raises(ValueError):
        trk(z(2, 2, 3, 4, 3))                                                          # another S than the state's
    lib, i32 = _lib.hip(), torch.int32
    zi = lambda *sh: torch.zeros(sh, dtype=i32, device="cuda")                         # noqa: E731
    o = dict(p=z(1, 2, 4, 3), u=zi(1, 2), m=zi(1, 2), n=zi(1), j=z(2, 1, 2, 4, 3), s=zi(2, 1, 3), q=zi(2, 1, 2), i=zi(2, 1, 2),
             f=torch.zeros(2, 1, 2, dtype=torch.uint8, device="cuda"), c=torch.zeros(2, 1, 3, dtype=torch.float64, device="cuda"),
             d=zi(2, 1))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    args = [ptr(good), 2, 1, 3, 2, 4, 0.1, 0.3, 3, 10] + [ptr(o[k]) for k in "pumnjsqifcd"] + [None]
    for k in (0, 10, 11, 12, 13):                          # each required pointer NULL in turn
        a = list(args)
        a[k] = None
        assert lib.p2m_pose_track(*a) == -1, k
    a = list(args)
    a[19] = ctypes.c_void_p(o["c"].data_ptr() + 4)         # misaligned cost
    assert lib.p2m_pose_track(*a) == -1
    for k in range(14, 21):                                # every output may be NULL
        a = list(args)
        a[k] = None
        o["u"].fill_(-1)
        assert lib.p2m_pose_track(*a) == 0, k
    torch.cuda.synchronize()
    assert o["u"].tolist() == [[12, 13]] and o["n"].tolist() == [14]       # 7 calls, 2 births each: the ids go on counting
    # and the module still works
    out, _ = run_gpu(tk, CASES["overflow"])
    assert out["slot_of"][1, 0].tolist() == [0, 1, -2]


# ---- OneEuroFilter.reset(mask=) ---------------------------------------------------------------------------------------------
MC, BETA = 0.5, 0.25


def test_filter_reset_by_mask_equals_reset_by_ids_and_is_capturable():
    from pose2mesh_release_amd import video
    rng = np.random.default_rng(3)
    x = dev(rng.normal(0, 1, (9, 4, 5, 3)))
    a, b, g = (video.OneEuroFilter(MC, BETA) for _ in range(3))
    masks = {3: [False, True, True, False], 4: [False] * 4, 6: [True, False, False, True]}
    static_in, static_mask = x[0].clone(), torch.zeros(4, dtype=torch.bool, device="cuda")
    g.reset(mask=static_mask)                              # before the first call: nothing to reset yet
    g(static_in)
    torch.cuda.synchronize()
    g.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.reset(mask=static_mask)
        y_g = g(static_in)
    restarted = False
    for f in range(9):
        m = masks.get(f, [False] * 4)
        if any(m):
            a.reset([k for k in range(4) if m[k]])
        b.reset(mask=torch.tensor(m).cuda())
        static_in.copy_(x[f])
        static_mask.copy_(torch.tensor(m))
        graph.replay()
        ya, yb = a(x[f]).cpu().numpy(), b(x[f]).cpu().numpy()
        assert ya.tobytes() == yb.tobytes() == y_g.cpu().numpy().tobytes(), f
        if f == 3:
            restarted = ya[1].tobytes() == x[f, 1].cpu().numpy().tobytes() and ya[0].tobytes() != x[f, 0].cpu().numpy().tobytes()
    assert restarted
    with pytest.raises(ValueError):
        a.reset(mask=torch.zeros(3, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError):
        a.reset([1], mask=torch.zeros(4, dtype=torch.bool, device="cuda"))


# ---- the chain: detections -> people -> tracks -> filter, no network in it ------------------------------------------------------
def test_the_crowd_video_chain(tk):
    """Two people, 12 frames; the detector's list order swaps from frame to frame, person 1 is not detected in frames 5 and 6.
    CrowdFilter -> PoseTracker -> OneEuroFilter.reset(mask=fresh) -> OneEuroFilter on out.joints: the filtered rows of an
    identity's slot are bit for bit smooth_pose of that person's own frames, restarted after the gap.  The same frames fed to
    the filter in list order are not."""
    from pose2mesh_release_amd import crowd, video
    F, T = 12, 4
    rng = np.random.default_rng(5)
    shape = rng.uniform(0, 1, (2, 17, 2)) * np.array([40.0, 100.0])
    dets = np.zeros((F, 3, 17, 3), np.float32)             # the third detection is always too weak to be a person
    dets[:, 2, :, :2] = 500.0
    where = np.zeros((F, 2), np.int64)                     # list slot of person i in frame f
    for f in range(F):
        for i in range(2):
            pose = np.array([30.0 + 250.0 * i + 3.0 * f, 40.0 + 2.0 * f]) + shape[i] + rng.normal(0, 1.5, (17, 2))
            slot = (i + f) % 2
            where[f, i] = slot
            dets[f, slot, :, :2] = pose
            dets[f, slot, :, 2] = 0.0 if (i == 1 and f in (5, 6)) else rng.uniform(0.5, 1.0, 17)
    sel = crowd.CrowdFilter()(dev(dets))
    people = sel.joints.clone()                            # [F, 3, 19, 3]
    count = sel.count.cpu().tolist()
    assert count == [2] * 5 + [1, 1] + [2] * 5
    gap = np.isin(np.arange(F), (5, 6))                    # there the filter's list is person 0 alone, then NaN slots
    frames = torch.arange(F, device="cuda")
    own = [people[frames, torch.from_numpy(np.where(gap, 0, where[:, 0])).cuda()],      # person 0's own frames [F, 19, 3]
           people[frames, torch.from_numpy(np.where(gap, 2, where[:, 1])).cuda()]]
    assert torch.isfinite(own[0]).all() and torch.isnan(own[1][5:7]).all() and torch.isfinite(own[1][[0, 4, 7, 11]]).all()
    want = [video.smooth_pose(own[0], MC, BETA).cpu().numpy(),
            np.concatenate([video.smooth_pose(own[1][:5], MC, BETA).cpu().numpy(), np.full((2, 19, 3), np.nan, np.float32),
                            video.smooth_pose(own[1][7:], MC, BETA).cpu().numpy()])]
    table = crowd.person_colours(8, seed=3).rgb
    trk, flt, naive = tk.PoseTracker(T), video.OneEuroFilter(MC, BETA), video.OneEuroFilter(MC, BETA)
    got, colours, uids, listed = [], [], [], []
    for f in range(F):
        out = trk(people[f][None])                         # one frame of one stream
        flt.reset(mask=out.fresh.reshape(-1))
        got.append(flt(out.joints.reshape(T, 19, 3)).cpu().numpy().copy())
        colours.append(tk.identity_colours(out.uid, table).cpu().numpy().copy())
        uids.append(out.uid.cpu().numpy().copy())
        listed.append(naive(people[f, :2]).cpu().numpy().copy())
    got, colours, uids, listed = np.stack(got), np.stack(colours), np.stack(uids), np.stack(listed)
    assert (uids[:, 0, :2] == [0, 1]).all() and (uids[:, 0, 2:] == -1).all()      # slot i is person i throughout
    seen = ~gap
    assert got[:, 0].tobytes() == want[0].tobytes()
    assert got[seen, 1].tobytes() == want[1][seen].tobytes()
    table_h = table.cpu().numpy()
    for i in range(2):
        assert (colours[:, 0, i] == table_h[i]).all()      # one colour per identity in all frames
    assert listed[:, 0].tobytes() != want[0].tobytes() and listed[seen, 1].tobytes() != want[1][seen].tobytes()
    assert listed[0, 0].tobytes() == want[0][0].tobytes()  # (frame 0 is in person order: the list order is what breaks it)
