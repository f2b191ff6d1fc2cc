#!/usr/bin/env python3
"""Crowd filter throughput (GPU).  Prints one JSON line: ms per launch of crowd.CrowdFilter (cuda events around back-to-back
launches, median of --repeats windows) on crowds of which about half the people are duplicates of an earlier one, at
  (B, P) = (1, 30)   one image of the demo's size        (64, 32)   a batch of frames        (256, 64)   the largest slots
J = 17 detections + pelvis and neck.  Beside each: `host_ms`, the same work by the numpy loop of tests/crowd_ref.py on the host
(the reference's own form, run.py:281-306; `host_images` images timed, scaled to B); `floor_ms`, a launch with next to
nothing to do through the same binding (p2m_person_colours, n = 1): the cost of a launch in this process; `colours_ms`,
person_colours for B x P people.  The device's decisions are compared with the yardstick's before anything is timed.
Usage: python tools/crowd_throughput.py [--steps 2000] [--warmup 50] [--repeats 5] [--no-host] [--only B,P]"""
import argparse
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

SIZES = ((1, 30), (64, 32), (256, 64))


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


def leg(B, P, args):
    import crowd_cases as cc
    import crowd_ref
    from pose2mesh_release_amd import crowd
    dets_h = cc.random_crowds(1000 + B, B=B, P=P, n_proto=max(1, P * 5 // 16))
    dets = torch.from_numpy(dets_h).cuda()
    sel = crowd.CrowdFilter()
    out = sel(dets)
    torch.cuda.synchronize()
    res = {"B": B, "P": P, "J": 17}
    reason = out.reason.cpu().numpy()
    res["share"] = {k: round(float((reason == v).mean()), 3) for k, v in (("accepted", 0), ("low", 1), ("duplicate", 2))}
    if not args.no_host:
        nh = min(B, args.host_images)
        t0 = time.perf_counter()
        ref = crowd_ref.select(dets_h[:nh])
        dt = time.perf_counter() - t0
        res["host_images"], res["host_ms"] = nh, round(1e3 * dt * B / nh, 3)
        assert np.array_equal(ref["reason"], reason[:nh]) and np.array_equal(ref["dup_of"], out.dup_of.cpu().numpy()[:nh]), \
            "the device's decisions differ from the yardstick's"
    st = crowd.NoiseStream(1, 0)
    one = crowd.person_colours(1, stream=st)
    many = crowd.person_colours(B * P, stream=st)
    ms = {"select": event_ms(lambda: sel(dets), args.steps, args.warmup, args.repeats),
          "floor": event_ms(lambda: crowd.person_colours(1, stream=st, out=one, advance=False), args.steps, args.warmup, args.repeats),
          "colours": event_ms(lambda: crowd.person_colours(B * P, stream=st, out=many), args.steps, args.warmup, args.repeats)}
    for k, (med, lo, hi) in ms.items():
        res[f"{k}_ms"], res[f"{k}_ms_range"] = round(med, 5), [round(lo, 5), round(hi, 5)]
    res["images_per_s"] = round(1e3 * B / ms["select"][0], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=8, help="images the host loop is timed on (scaled to B)")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--only", help="B,P: one size alone (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "crowd_throughput needs the GPU"
    sizes = SIZES if args.only is None else (tuple(int(v) for v in args.only.split(",")),)
    line = {"steps": args.steps, "repeats": args.repeats}
    for B, P in sizes:
        line[f"{B}x{P}"] = leg(B, P, args)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
