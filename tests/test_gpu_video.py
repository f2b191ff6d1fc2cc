"""-m gpu: pose2mesh_release_amd.video on the GPU.  The One-Euro filter (p2m_one_euro) is held BITWISE to the real
reference's float32 output (tests/golden/video_ref.npz) and to the fp32 op-by-op restatement (tests/video_ref.py) over the
kernel's shape edges, the carried state, graph replay and isolation; the per-video metrics (p2m_video_eval) to the float64
restatement and to the reference's recorded numbers.  Every shape is kilobytes, except the two batches that reach the
kernel's wide-access threshold (a few megabytes)."""
import numpy as np
import pytest
import torch

import helpers
import video_ref

pytestmark = pytest.mark.gpu

ONE_ROUNDING = 6e-8            # 2^-24 = 5.96e-8: an fp64 value stored once as fp32
MC, BETA = 0.004, 0.7


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(gpu, ref, what=""):
    g = gpu.cpu().numpy() if isinstance(gpu, torch.Tensor) else gpu
    assert g.shape == ref.shape and np.array_equal(_bits(g), _bits(ref)), what


def _signal(T, C, seed):
    """mm-scale coordinates: a random walk plus jitter, float32 [T, C]."""
    rng = np.random.default_rng([seed, T, C])
    return (np.cumsum(rng.standard_normal((T, C)) * 5.0, axis=0) + rng.standard_normal((T, C)) * 12.0
            + rng.uniform(-800, 800, (1, C))).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_filter_equals_reference_record_bitwise(hip_libs):
    from pose2mesh_release_amd import video
    z = helpers.golden("video_ref.npz")
    x, ptr = _dev(z["flt_x"]), z["flt_seq_ptr"]
    for k, (mc, b) in enumerate(z["flt_params"]):
        _same(video.smooth_pose(x, float(mc), float(b), seq_ptr=ptr), z[f"flt_y{k}"], (mc, b))
    a, e = int(ptr[1]), int(ptr[2])                                     # one sequence, the drop-in call
    _same(video.smooth_pose(x[a:e], 0.004, 0.005), z["flt_y1"][a:e])


def test_filter_shape_edges_bitwise(hip_libs):
    """C around a wave, around a block of 256 lanes at 4-, 8- and 16-byte lane accesses (256, 512, 1024 coordinates), an odd
    C and a misaligned base that defeat wide accesses; T around the prefetch ring."""
    from pose2mesh_release_amd import video
    la = video.lookahead()
    Cs = (1, 63, 64, 65, 255, 256, 257, 510, 514, 1020, 1028, 1031)
    Ts = (1, 2, la - 1, la, la + 1, 2 * la + 3)
    for C in Cs:
        full = _signal(max(Ts), C, 1)
        xg = _dev(full)
        for T in Ts:
            _same(video.smooth_pose(xg[:T], MC, BETA), video_ref.one_euro(full[:T], MC, BETA)[0], (C, T))
    T, C = 2 * la + 3, 64
    full = _signal(T, C, 2)
    off = torch.empty(T * C + 1, device="cuda")[1:].view(T, C)          # rows start 4 bytes off a 16-byte boundary
    off.copy_(_dev(full))
    assert off.data_ptr() % 8 == 4
    _same(video.smooth_pose(off, MC, BETA), video_ref.one_euro(full, MC, BETA)[0], "misaligned")


def test_filter_other_dt_and_cutoffs_bitwise(hip_libs):
    """dt != 1 keeps the division of the difference (dt == 1 runs a kernel without it); d_cutoff and beta < 0 enter too."""
    from pose2mesh_release_amd import video
    la = video.lookahead()
    T, B, C = la + 5, 2, 65
    xs = np.stack([_signal(T, C, 40 + b) for b in range(B)], axis=1)
    for mc, beta, dc, dt in ((0.004, 0.7, 1.0, 1.0 / 30.0), (0.5, 0.01, 2.5, 0.5), (0.0, -0.02, 0.0, 3.0), (1.0, 0.0, 1.0, 1.0)):
        f = video.OneEuroFilter(mc, beta, dc, dt)
        got = torch.cat([f(_dev(xs[:3]), chunk=True).clone(), f(_dev(xs[3:]), chunk=True).clone()])
        ref = np.stack([video_ref.one_euro(xs[:, b], mc, beta, dc, dt)[0] for b in range(B)], axis=1)
        _same(got, ref, (mc, beta, dc, dt))


@pytest.mark.parametrize("C,width", [(8194, 8), (16388, 16)])
def test_filter_wide_accesses_bitwise(hip_libs, C, width):
    """The kernel moves to 8- and 16-byte lane accesses only once the narrower width has 2^19 lanes in flight (64 sequences x C
    coordinates here: the smallest batch that gets there; a few megabytes).  4097 lanes per sequence: a block edge.  Ragged
    lengths around the prefetch ring, through the carried state, in place."""
    from pose2mesh_release_amd import video
    la = video.lookahead()
    S = 64
    assert S * C // (width // 8) > 1 << 19 and C % (width // 4) == 0 and C % (width // 2) != 0
    lens = [1] * S
    lens[0], lens[5], lens[17], lens[63] = 2 * la + 3, 0, la + 1, la - 1
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    N = int(ptr[-1])
    x = _signal(N, C, 50)
    first = np.stack([_signal(1, C, 60 + s)[0] for s in range(S)])               # the frame before, fed in a call of its own
    ref = np.empty_like(x)
    for s in range(S):
        st = video_ref.one_euro(first[s:s + 1], MC, BETA)[1]
        ref[ptr[s]:ptr[s + 1]] = video_ref.one_euro(x[ptr[s]:ptr[s + 1]], MC, BETA, state=st)[0]
    state = (torch.zeros((S, C), device="cuda"), torch.zeros((S, C), device="cuda"),
             torch.zeros(S, device="cuda", dtype=torch.int32))
    fg = _dev(first)
    video._one_euro(fg, _dev(np.arange(S + 1, dtype=np.int32)), None, S, S, C, MC, BETA, 1.0, 1.0, state, fg)
    _same(fg, first, "first frames pass through")
    xg = _dev(x)
    video._one_euro(xg, _dev(ptr), None, N, S, C, MC, BETA, 1.0, 1.0, state, xg)
    _same(xg, ref, "wide, carried state, in place")
    # a fresh start, out of place
    y = video.smooth_pose(_dev(x), MC, BETA, seq_ptr=ptr)
    _same(y, video_ref.one_euro_seqs(x, ptr, MC, BETA), "wide, fresh")


@pytest.mark.parametrize("C", [64, 65, 42])
def test_filter_ragged_rows_in_place_bitwise(hip_libs, C):
    from pose2mesh_release_amd import video
    la = video.lookahead()
    lens = (la + 3, 0, 1, 2 * la + 5)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    N = int(ptr[-1])
    x = _signal(N, C, 3)
    ref = video_ref.one_euro_seqs(x, ptr, MC, BETA)
    xg = _dev(x)
    _same(video.smooth_pose(xg, MC, BETA, seq_ptr=ptr), ref, "ragged")
    _same(video.smooth_pose(xg, MC, BETA, seq_ptr=_dev(ptr)), ref, "device seq_ptr")
    # a row table: the input lies permuted in a larger array
    perm = np.random.default_rng(4).permutation(N + 9)[:N].astype(np.int32)
    big = _signal(N + 9, C, 5)
    big[perm] = x
    y = torch.empty((N, C), device="cuda")
    video._one_euro(_dev(big), _dev(ptr), _dev(perm), N, len(lens), C, MC, BETA, 1.0, 1.0, None, y)
    _same(y, ref, "rows")
    assert np.array_equal(video_ref.one_euro_seqs(big, ptr, MC, BETA, rows=perm), ref)
    # in place
    assert video.smooth_pose(xg, MC, BETA, seq_ptr=ptr, out=xg) is xg
    _same(xg, ref, "in place")


def test_chunked_state_equals_one_shot_bitwise(hip_libs):
    """T = 37 as chunks of 1, 5 and 31 frames through the carried state; two tracks, ragged per call."""
    from pose2mesh_release_amd import video
    T, C = 37, 65
    xs = [_signal(T, C, 6), _signal(T, C, 7)]
    ref = [video_ref.one_euro(x, MC, BETA) for x in xs]
    state = (torch.zeros((2, C), device="cuda"), torch.zeros((2, C), device="cuda"),
             torch.zeros(2, device="cuda", dtype=torch.int32))
    got = [[], []]
    for (a, e), (a2, e2) in (((0, 1), (0, 5)), ((1, 6), (5, 5)), ((6, 37), (5, 37))):      # track 1: 5, 0 and 32 frames
        n1, n2 = e - a, e2 - a2
        x = _dev(np.concatenate([xs[0][a:e], xs[1][a2:e2]]))
        y = torch.empty_like(x)
        video._one_euro(x, _dev(np.array([0, n1, n1 + n2], np.int32)), None, n1 + n2, 2, C, MC, BETA, 1.0, 1.0, state, y)
        got[0].append(y[:n1].cpu().numpy())
        got[1].append(y[n1:].cpu().numpy())
        assert state[2].tolist() == [1, 1]
    for k in range(2):
        _same(np.concatenate(got[k]), ref[k][0], k)
        _same(state[0][k], ref[k][1][0])
        _same(state[1][k], ref[k][1][1])


def test_one_euro_filter_stream_chunks_graph_and_reset(hip_libs):
    from pose2mesh_release_amd import video
    T, B, shape = 37, 3, (7, 3)
    C = 21
    xs = np.stack([_signal(T, C, 10 + b) for b in range(B)], axis=1)               # [T, B, C]
    ref = np.stack([video_ref.one_euro(xs[:, b], MC, BETA)[0] for b in range(B)], axis=1)
    xg = _dev(xs).view(T, B, *shape)
    # chunks of 1 (the frame form), 5 and 31
    f = video.OneEuroFilter(MC, BETA)
    parts = [f(xg[0]).clone().view(1, B, C), f(xg[1:6], chunk=True).clone().reshape(5, B, C),
             f(xg[6:], chunk=True).clone().reshape(31, B, C)]
    _same(torch.cat(parts), ref, "chunks")
    # frame by frame under graph replay
    g = video.OneEuroFilter(MC, BETA)
    static_in = xg[0].clone()
    g(static_in)                                                                # allocates the buffers of this shape
    torch.cuda.synchronize()
    g.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = g(static_in)
    g.reset()
    outs = []
    for t in range(T):
        static_in.copy_(xg[t])
        graph.replay()
        outs.append(y.clone().view(B, C))
    _same(torch.stack(outs), ref, "graph replay")
    # reset of track 1 after frame 20: it restarts from frame 21 on, its neighbours continue
    h = video.OneEuroFilter(MC, BETA)
    first = h(xg[:21], chunk=True).clone().reshape(21, B, C)
    h.reset([1])
    rest = h(xg[21:], chunk=True).clone().reshape(T - 21, B, C)
    want = ref.copy()
    want[21:, 1] = video_ref.one_euro(xs[21:, 1], MC, BETA)[0]
    _same(torch.cat([first, rest]), want, "reset one track")
    h.reset()
    _same(h(xg[:3], chunk=True).reshape(3, B, C), ref[:3], "reset all")
    with pytest.raises(ValueError):
        h(xg[0, :2])


def test_filter_isolation_nan_and_guards(hip_libs):
    from pose2mesh_release_amd import video
    la = video.lookahead()
    C, lens, G = 66, (la + 2, 2 * la + 1, 9), 3
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    N, S = int(ptr[-1]), len(lens)
    x = _signal(N, C, 20)
    sentinel = -12345.5
    ybuf = torch.full((N + 2 * G, C), sentinel, device="cuda")
    sbuf = [torch.full((S + 2 * G, C), sentinel, device="cuda") for _ in range(2)]
    started = torch.zeros(S + 2 * G, device="cuda", dtype=torch.int32)
    state = (sbuf[0][G:G + S], sbuf[1][G:G + S], started[G:G + S])
    video._one_euro(_dev(x), _dev(ptr), None, N, S, C, MC, BETA, 1.0, 1.0, state, ybuf[G:G + N])
    batch = ybuf[G:G + N].cpu().numpy()
    _same(batch, video_ref.one_euro_seqs(x, ptr, MC, BETA), "batch")
    for t in (ybuf, sbuf[0], sbuf[1]):                                      # guard rows untouched
        n = t.shape[0] - 2 * G
        assert bool((t[:G] == sentinel).all()) and bool((t[G + n:] == sentinel).all())
    assert started.tolist() == [0] * G + [1] * S + [0] * G
    # a sequence filtered alone == itself inside the batch
    a, e = int(ptr[1]), int(ptr[2])
    _same(video.smooth_pose(_dev(x[a:e]), MC, BETA), batch[a:e], "alone")
    # a NaN in one coordinate of one frame: exactly that coordinate's tail in that sequence
    xn = x.copy()
    f_nan, c_nan = a + 4, 37
    xn[f_nan, c_nan] = np.nan
    yn = video.smooth_pose(_dev(xn), MC, BETA, seq_ptr=ptr).cpu().numpy()
    changed = _bits(yn) != _bits(batch)
    want = np.zeros_like(changed)
    want[f_nan:e, c_nan] = True
    assert np.array_equal(changed, want) and np.isnan(yn[f_nan:e, c_nan]).all()


def _joints(N, J, seed, noise=25.0):
    rng = np.random.default_rng([seed, N, J])
    gt = (rng.standard_normal((1, J, 3)) * 250.0 + np.cumsum(rng.standard_normal((N, J, 3)) * 6.0, axis=0)).astype(np.float32)
    pred = (gt + rng.standard_normal((N, J, 3)) * noise).astype(np.float32)
    return pred, gt


def _check_eval(out, S, ref, scale, J):
    acc, val = out["accel"].cpu().numpy().astype(np.float64), out["valid"].cpu().numpy().astype(bool)
    assert np.array_equal(val, ref["valid"]) and not acc[~val].any()
    assert (np.abs(acc - ref["accel"]) <= ONE_ROUNDING * np.abs(ref["accel"])).all()
    mp = out["mpjpe"].cpu().numpy().astype(np.float64)
    assert (np.abs(mp - ref["mpjpe"]) <= ONE_ROUNDING * np.abs(ref["mpjpe"])).all()
    stats = out["stats"].cpu().numpy()
    seq, tot = stats[:S], stats[S]
    if J > 1:
        pa = out["pa_mpjpe"].cpu().numpy().astype(np.float64)
        assert pa.shape == ref["pa_mpjpe"].shape and (np.abs(pa - ref["pa_mpjpe"]) <= 4e-7 * scale).all()
        np.testing.assert_allclose(seq, ref["seq_stats"], rtol=1e-10, atol=0, equal_nan=True)
        np.testing.assert_allclose(tot, ref["totals"], rtol=1e-10, atol=0, equal_nan=True)
    else:       # one joint has no extent: the alignment divides 0 by 0, here as in the reference - every PA value is NaN
        assert np.isnan(out["pa_mpjpe"].cpu().numpy()).all() and np.isnan(ref["pa_mpjpe"]).all()
        assert np.isnan(seq[seq[:, 0] > 0, 4]).all() and np.isnan(tot[2])
        cols = [0, 1, 2, 3, 5]
        np.testing.assert_allclose(seq[:, cols], ref["seq_stats"][:, cols], rtol=1e-10, atol=0, equal_nan=True)
        np.testing.assert_allclose(np.delete(tot, 2), np.delete(ref["totals"], 2), rtol=1e-10, atol=0, equal_nan=True)
    return tot


@pytest.mark.parametrize("J", [1, 14, 64])
def test_video_eval_vs_float64_restatement(hip_libs, J):
    """Sequences of 0, 1, 2 and 3 frames, a longer one with vis gaps, and one whose vis leaves no valid triple: that one is
    left out of the acceleration total, counted, and NaN in its per-video value."""
    from pose2mesh_release_amd import video
    lens = (0, 1, 2, 3, 41, 7, 0)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    N, S = int(ptr[-1]), len(lens)
    pred, gt = _joints(N, J, 30)
    vis = np.ones(N, np.uint8)
    vis[int(ptr[4]) + np.array([0, 9, 10, 22, 40])] = 0
    vis[int(ptr[5]) + np.array([2, 5])] = 0                                   # 7 frames, no three visible in a row
    ref = video_ref.video_eval(pred, gt, ptr, vis, True)
    assert ref["totals"][3:].tolist() == [2, 5, 5, 2, N] and np.isnan(ref["seq_stats"][5, 2]) and ref["seq_stats"][5, 0] == 7
    pg, gg, sp, vg = _dev(pred), _dev(gt), _dev(ptr), _dev(vis)
    out = video._video_eval(pg, gg, sp, S, vg, True)
    tot = _check_eval(out, S, ref, float(np.abs(gt).max()), J)
    again = video._video_eval(pg, gg, sp, S, vg, True)["stats"].cpu().numpy()
    assert np.array_equal(again.view(np.uint64), out["stats"].cpu().numpy().view(np.uint64))     # bitwise, NaNs included
    assert np.array_equal(tot.view(np.uint64), again[S].view(np.uint64))
    # without vis and without PA; a sequence's results do not depend on its neighbours
    ref2 = video_ref.video_eval(pred, gt, ptr, None, False)
    out2 = video._video_eval(pg, gg, sp, S, None, False)
    st2 = out2["stats"].cpu().numpy()
    np.testing.assert_allclose(st2[:S], ref2["seq_stats"], rtol=1e-10, atol=0, equal_nan=True)
    np.testing.assert_allclose(st2[S], ref2["totals"], rtol=1e-10, atol=0, equal_nan=True)
    a, e = int(ptr[4]), int(ptr[5])
    alone = video._video_eval(pg[a:e].contiguous(), gg[a:e].contiguous(), _dev(np.array([0, e - a], np.int32)), 1,
                              vg[a:e].contiguous(), True)
    assert torch.equal(alone["stats"][0].view(torch.int64), out["stats"][4].view(torch.int64))
    assert torch.equal(alone["accel"], out["accel"][a:e])
    assert torch.equal(alone["pa_mpjpe"].view(torch.int32), out["pa_mpjpe"][a:e].view(torch.int32))     # (J = 1: NaNs)


def test_drop_ins_reproduce_the_reference_record(hip_libs):
    """VideoEvaluator on the fixture's two-run video_indices, fed in Tester batches, against the numbers the reference's
    loop printed from; compute_error_accel with and without vis on exactly the recorded inputs."""
    from pose2mesh_release_amd import video
    z = helpers.golden("video_ref.npz")
    pred, gt, masks = _dev(z["ev_pred"]), _dev(z["ev_gt"]), z["ev_masks"]
    ve = video.VideoEvaluator(list(masks), 14)                                    # the protocol's 0.004 / 0.005
    for first in range(0, 130, 32):
        ve.put(first, pred[first:first + 32], gt[first:first + 32])
    res = ve.summary()
    _same(ve.last["pred"], z["ev_smoothed"], "smoothed")
    for key, want in zip(("accel_error", "mpjpe", "pa_mpjpe"), z["ev_totals"]):
        assert abs(res[key] - want) <= 1e-10 * abs(want), (key, res[key], want)
    np.testing.assert_allclose(res["per_video"]["accel_error"], z["ev_accel_error"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(res["per_video"]["mpjpe"], z["ev_mpjpe_list"], rtol=1e-10, atol=0)
    assert res["per_video"]["frames"].tolist() == [90, 40] and res["per_video"]["accel_frames"].tolist() == [88, 38]
    assert (res["videos"], res["videos_without_accel"], res["empty_videos"], res["frames"]) == (2, 0, 0, 130)
    pa = ve.last["pa_mpjpe"].cpu().numpy().astype(np.float64)
    assert (np.abs(pa - z["ev_pa_mpjpe"]) <= 4e-7 * float(np.abs(z["ev_gt"]).max())).all()
    # smooth=False evaluates the raw predictions
    raw = video.VideoEvaluator([np.flatnonzero(m) for m in masks], 14, smooth=False, pa=False)
    raw.put(0, pred, gt)
    rows, ptr = video_ref.tables(masks)
    r = video_ref.video_eval(z["ev_pred"][rows], z["ev_gt"][rows], ptr, None, False)
    rr = raw.summary()
    assert abs(rr["accel_error"] - r["totals"][0]) <= 1e-10 * r["totals"][0] and np.isnan(rr["pa_mpjpe"])
    assert abs(rr["mpjpe"] - r["totals"][1]) <= 1e-10 * r["totals"][1]
    # compute_error_accel
    g, p = gt[50:90], pred[50:90]
    plain = video.compute_error_accel(g, p).cpu().numpy().astype(np.float64)
    assert plain.shape == z["acc_plain"].shape and (np.abs(plain - z["acc_plain"]) <= ONE_ROUNDING * z["acc_plain"]).all()
    wv = video.compute_error_accel(g, p, z["acc_vis_mask"]).cpu().numpy().astype(np.float64)
    assert wv.shape == z["acc_vis"].shape and (np.abs(wv - z["acc_vis"]) <= ONE_ROUNDING * z["acc_vis"]).all()
    acc, valid = video.error_accel(g, p, _dev(z["acc_vis_mask"]))
    assert acc.shape == (40,) and int(valid.sum()) == 26 and not bool(valid[38:].any())
    assert video.compute_error_accel(g[:2], p[:2]).shape == (0,)


def test_errors(hip_libs):
    from pose2mesh_release_amd import video
    from pose2mesh_release_amd._lib import P2MError
    cpu = torch.zeros(4, 14, 3)
    gpu = cpu.cuda()
    for call in (lambda: video.smooth_pose(cpu), lambda: video.OneEuroFilter()(cpu), lambda: video.error_accel(cpu, gpu),
                 lambda: video.compute_error_accel(gpu, cpu)):
        with pytest.raises(P2MError):
            call()
    ve = video.VideoEvaluator([np.ones(6, bool)], 14)
    with pytest.raises(P2MError):
        ve.put(0, cpu, cpu)
    with pytest.raises(ValueError):
        ve.put(0, gpu[:, :13], gpu[:, :13])                                   # wrong J
    with pytest.raises(ValueError):
        ve.put(3, gpu, gpu)                                                   # positions 3 .. 6 of 6
    with pytest.raises(ValueError):
        ve.put(-1, gpu, gpu)
    with pytest.raises(ValueError):
        video.error_accel(gpu, gpu[:3])
    with pytest.raises(ValueError):
        video.smooth_pose(gpu, seq_ptr=[0, 2, 3])
    with pytest.raises(ValueError):
        video.smooth_pose(gpu, out=torch.zeros(4, 14, 3, device="cuda", dtype=torch.float64))
