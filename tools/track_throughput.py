#!/usr/bin/env python3
"""Tracker throughput (GPU).  Prints one JSON line: ms per call of track.PoseTracker (cuda events around back-to-back calls,
median of --repeats windows) on walkers of tests/track_cases.py - about 5/8 of the list slots filled, shuffled list order, 10 %
missed detections, 19 joints - at
  (S, P, T, F) = (1, 8, 16, 1)   one video, frame by frame     (64, 16, 16, 1)   a batch of videos, frame by frame
                 (1, 8, 16, 64)  one video, 64 frames a call   (64, 64, 64, 1)   the largest slots (P = T = 64, Jo = 19)
`call_ms` is the whole call (the kernel and the two elementwise ops of the boolean views), `kernel_ms` the launch of
p2m_pose_track alone through the same binding, `per_frame_ms` = call_ms / F.  Beside each: `host_ms`, the same frames by the
numpy loop of tests/track_ref.py on the host (`host_frames` frames of one stream timed, scaled to S F); `floor_ms`, a launch
with next to nothing to do through the same binding (p2m_person_colours, n = 1): the cost of a launch in this process.  The
device's decisions are compared with the yardstick's before anything is timed.
Usage: python tools/track_throughput.py [--steps 2000] [--warmup 50] [--repeats 5] [--no-host] [--only S,P,T,F]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = ((1, 8, 16, 1), (64, 16, 16, 1), (1, 8, 16, 64), (64, 64, 64, 1))
ROUND = 8                        # the timed calls cycle through this many different inputs, so that the state keeps moving


def event_ms(body, steps, warmup, repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        body()
    times = []
    for _ in range(repeats):
        e0.record()
        for _ in range(steps):
            body()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / steps)
    return float(np.median(times)), float(min(times)), float(max(times))


def leg(S, P, T, F, args):
    import track_cases as tc
    import track_ref
    from pose2mesh_release_amd import _lib, crowd, track
    frames = ROUND * F
    people_h, _ = tc.walkers(seed=100 + S + P + F, n=max(1, P * 5 // 8), F=frames, P=P, S=S)
    calls = [torch.from_numpy(people_h[k * F:(k + 1) * F] if F > 1 else people_h[k]).cuda() for k in range(ROUND)]
    trk = track.PoseTracker(T)
    flags = [trk(x).flags.cpu().numpy().reshape(F, S, T) for x in calls]
    torch.cuda.synchronize()
    flags = np.concatenate(flags)
    res = {"S": S, "P": P, "T": T, "F": F, "Jo": 19,
           "share": {k: round(float(((flags & v) != 0).mean()), 3) for k, v in (("present", 2), ("fresh", 8))}}
    if not args.no_host:
        nh = min(frames, args.host_frames)
        st = track_ref.new_state(1, T, 19)
        t0 = time.perf_counter()
        ref = track_ref.track(people_h[:nh, :1], st)
        dt = time.perf_counter() - t0
        res["host_frames"], res["host_ms"] = nh, round(1e3 * dt * S * F / nh, 3)
        assert np.array_equal(ref["flags"][:, 0], flags[:nh, 0]), "the device's decisions differ from the yardstick's"
    st = crowd.NoiseStream(1, 0)
    one = crowd.person_colours(1, stream=st)
    turn = [0]

    def call():
        turn[0] = (turn[0] + 1) % ROUND
        trk(calls[turn[0]])

    buf = trk(calls[0])
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    lib, stream = _lib.hip(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fixed = [F, S, P, T, 19, trk.pose_thr, trk.gate, trk.min_common, trk.max_missed] + \
        [ptr(t) for t in (trk.pose, trk.uid, trk.missed, trk.next_uid, buf.joints, buf.slot_of, buf.person_of, buf.uid, buf.flags,
                          buf.cost, buf.dropped)] + [stream]
    inputs = [ptr(x) for x in calls]

    def kernel():
        turn[0] = (turn[0] + 1) % ROUND
        lib.p2m_pose_track(inputs[turn[0]], *fixed)

    ms = {"call": event_ms(call, args.steps, args.warmup, args.repeats),
          "kernel": event_ms(kernel, args.steps, args.warmup, args.repeats),
          "floor": event_ms(lambda: crowd.person_colours(1, stream=st, out=one, advance=False), args.steps, args.warmup,
                            args.repeats)}
    for k, (med, lo, hi) in ms.items():
        res[f"{k}_ms"], res[f"{k}_ms_range"] = round(med, 5), [round(lo, 5), round(hi, 5)]
    res["per_frame_ms"] = round(ms["call"][0] / F, 5)
    res["stream_frames_per_s"] = round(1e3 * S * F / ms["call"][0], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=8, help="frames of one stream the host loop is timed on (scaled to S F)")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--only", help="S,P,T,F: one size alone (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "track_throughput needs the GPU"
    sizes = SIZES if args.only is None else (tuple(int(v) for v in args.only.split(",")),)
    line = {"steps": args.steps, "repeats": args.repeats}
    for S, P, T, F in sizes:
        line[f"{S}x{P}x{T}x{F}"] = leg(S, P, T, F, args)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
