#!/usr/bin/env python3
"""Error-profile throughput, B = 64 (GPU).  Prints one JSON line: ms per call of evaluate.ErrorProfile (cuda events around
back-to-back calls, the median of --repeats windows, all in one process) for N = 21 (the joints of a hand), 778 (MANO) and
6890 (SMPL), each raw and similarity-aligned, 100 thresholds, per-point totals on.  Beside each, measured the same way:
  floor_ms      an empty launch: p2m_error_profile on one point of one sample without totals, through the same binding - the cost
                of a launch in this process (a profile call is three launches)
  mesh_eval_ms  a MeshEvaluator call (stage A with a synthetic 21-joint regressor, pa_mesh as the profile's align) on the same
                point sets
  copy_ms       a device-to-device copy of the bytes a call reads (pred and gt) and writes (error), as one tensor
  host_ms       the numpy restatement on the host (tests/profile_ref.py: evaluate + accumulate), --host-steps calls timed
The device's totals are compared with the restatement's before anything is timed (raw: bit for bit; aligned: the counts of
the overall histogram within the interval the alignment tolerance allows).
Usage: python tools/profile_throughput.py [--steps 200] [--warmup 20] [--repeats 5] [--host-steps 1] [--no-host]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B = 64
SIZES = (21, 778, 6890)


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
    return [round(float(np.median(times)), 5), round(float(min(times)), 5), round(float(max(times)), 5)]


def floor_call():
    """One launch with next to nothing to do, through the same binding."""
    from pose2mesh_release_amd import _lib
    lib = _lib.hip()
    one = torch.zeros((1, 1, 3), device="cuda")
    th = torch.tensor([0.0, 1.0], device="cuda", dtype=torch.float64)
    ws = torch.zeros(64, device="cuda", dtype=torch.uint8)
    err, mean = torch.zeros(1, device="cuda", dtype=torch.float64), torch.zeros(1, device="cuda", dtype=torch.float64)
    pck = torch.zeros(3, device="cuda", dtype=torch.int32)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    args = [ptr(one), ptr(one), None, 1, 1, 1, 1.0, -1, 0, ptr(th), 2, ptr(ws), 64, ptr(err), ptr(mean), ptr(pck), None, 0,
            None, None, None, None, None, None]
    keep = (one, th, ws, err, mean, pck)

    def body(keep=keep):
        rc = lib.p2m_error_profile(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
    return body


def leg(N, align, args, floor):
    import profile_cases as pc
    import profile_ref as pr
    from pose2mesh_release_amd import evaluate, synth
    t = np.linspace(0.0, 50.0, 100)
    pred_h, gt_h = pc.cloud(B, N, seed=N)
    pred, gt = torch.from_numpy(pred_h).cuda(), torch.from_numpy(gt_h).cuda()
    ep = evaluate.ErrorProfile(N, t, align=align)
    ep(pred, gt)
    tot = ep.totals()
    t0 = time.perf_counter()
    ref = pr.evaluate(pred_h, gt_h, t, align=align)
    state = pr.accumulate(pr.new_state(N, 100), ref)
    host_first = time.perf_counter() - t0
    if align:
        delta = pr.align_delta(pred_h, gt_h)
        on = np.ones(N, bool)
        lo, hi = (sum(x) for x in zip(*(pr.count_bounds(ref["error"][b], on, t, delta[b]) for b in range(B))))
        cum = np.cumsum(tot["group_hist"][0])[:-1]
        assert (lo <= cum).all() and (cum <= hi).all(), "the device's counts leave the alignment tolerance"
    else:
        for k in state:
            assert np.array_equal(tot[k], state[k], equal_nan=True), f"the device's {k} differs from the restatement's"
    res = {"N": N, "align": align, "mean_error": round(float(ep.summary()["mean"]), 3), "auc": round(float(ep.summary()["auc"]), 4)}
    res["call_ms"] = event_ms(lambda: ep(pred, gt), args.steps, args.warmup, args.repeats)
    res["floor_ms"] = event_ms(floor, args.steps, args.warmup, args.repeats)
    ev = evaluate.MeshEvaluator(N, synth.synthetic_regressor(21, N) if N > 21 else np.eye(21, dtype=np.float32), 0,
                                pa_mesh=align)
    res["mesh_eval_ms"] = event_ms(lambda: ev(pred, gt), args.steps, args.warmup, args.repeats)
    src = torch.zeros(B * N * (3 * 4 * 2 + 8), device="cuda", dtype=torch.uint8)
    dst = torch.empty_like(src)
    res["copy_ms"] = event_ms(lambda: dst.copy_(src), args.steps, args.warmup, args.repeats)
    res["copy_bytes"] = int(src.numel())
    if not args.no_host:
        times = [host_first]
        for _ in range(args.host_steps):
            t0 = time.perf_counter()
            pr.accumulate(state, pr.evaluate(pred_h, gt_h, t, align=align))
            times.append(time.perf_counter() - t0)
        res["host_ms"] = round(1e3 * float(np.median(times)), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "profile_throughput needs the GPU"
    floor = floor_call()
    line = {"B": B, "K": 100, "steps": args.steps, "repeats": args.repeats, "ms": "[median, min, max] of the windows"}
    for N in SIZES:
        for align in (False, True):
            line[f"N{N}_{'aligned' if align else 'raw'}"] = leg(N, align, args, floor)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
