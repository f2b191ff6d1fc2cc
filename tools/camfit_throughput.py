#!/usr/bin/env python3
"""Camera-fit throughput (GPU).  Prints one JSON line:
  fit       for B = 1, 8, 64, 4096 people of J = 17 joints: ms per launch of CameraFitter with the default schedule (1500 steps)
            - the median of `--repeats` launches timed one by one with device events after `--warmup` launches, with the
            fastest and slowest beside it - and fits per second at the median
  prepare   the same for prepare_pose at B = 64
  stock     the form a user of the reference runs today, in the same process on the same device: a three-parameter torch
            module under torch.nn.L1Loss and torch.optim.Adam for 1500 iterations with the two rate changes, ONE person, wall
            time around a synchronise, `--stock-repeats` runs after one warm-up run
  condition the batched launch for B = 64 takes less time than the stock loop takes for one person
Usage: python tools/camfit_throughput.py [--repeats 30] [--warmup 5] [--stock-repeats 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

J, CROP = 17, 500
BATCHES = (1, 8, 64, 4096)


def people(B, seed=0):
    """Joints in metres, a camera per person, the target a few pixels off its projection, and pixel joints for prepare."""
    rng = np.random.default_rng(seed)
    p = rng.normal(0, 0.3, (B, J, 3)).astype(np.float32)
    cam = np.stack([rng.uniform(0.6, 1.4, B), rng.uniform(-0.2, 0.2, B), rng.uniform(-0.2, 0.2, B)], 1)
    t = (p[:, :, :2] + cam[:, None, 1:]) * cam[:, None, :1] * (CROP / 2) + CROP / 2 + rng.normal(0, 4.0, (B, J, 2))
    return torch.from_numpy(p).cuda(), torch.from_numpy(t.astype(np.float32)).cuda()


def launches_ms(body, repeats, warmup):
    for _ in range(warmup):
        body()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(repeats)]
    for a, b in ev:
        a.record()
        body()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


class StockCamera(torch.nn.Module):
    """Three parameters (s, tx, ty): joints [1, J, 3] -> crop pixels [1, J, 2]."""

    def __init__(self, img_res):
        super().__init__()
        self.img_res = img_res
        self.cam = torch.nn.Parameter(torch.rand((1, 3)))

    def forward(self, joints):
        return (joints[:, :, :2] + self.cam[None, :, 1:]) * self.cam[None, :, :1] * self.img_res + self.img_res


def stock_fit(p, t):
    layer = StockCamera(CROP / 2).cuda()
    l1, adam = torch.nn.L1Loss(), torch.optim.Adam(layer.parameters(), lr=0.1)
    for it in range(1500):
        adam.zero_grad()
        l1(layer(p), t).backward()
        adam.step()
        if it in (500, 1000):
            for group in adam.param_groups:
                group["lr"] = 0.05 if it == 500 else 0.001
    return layer.cam.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stock-repeats", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "camfit_throughput needs the GPU"
    from pose2mesh_release_amd import camfit
    line = {"J": J, "steps": camfit.DEFAULT_STEPS, "repeats": args.repeats, "fit": {}}
    for B in BATCHES:
        p, t = people(B)
        fit = camfit.CameraFitter(crop=CROP, seed=1)
        r = launches_ms(lambda: fit(p, t), args.repeats, args.warmup)
        r["fits_per_s"] = round(1e3 * B / r["median_ms"], 1)
        line["fit"][str(B)] = r
    pix = torch.rand(64, J, 2, device="cuda") * 400 + 100
    out = camfit.prepare_pose(pix)
    line["prepare"] = {"64": launches_ms(lambda: camfit.prepare_pose(pix, out=out), args.repeats, args.warmup)}
    p, t = people(1)
    stock_fit(p, t)
    torch.cuda.synchronize()
    runs = []
    for _ in range(args.stock_repeats):
        t0 = time.perf_counter()
        stock_fit(p, t)
        torch.cuda.synchronize()
        runs.append(1e3 * (time.perf_counter() - t0))
    runs.sort()
    line["stock"] = {"people": 1, "median_ms": round(runs[len(runs) // 2], 2), "min_ms": round(runs[0], 2),
                     "max_ms": round(runs[-1], 2), "runs": len(runs)}
    line["condition_b64_faster_than_stock_one_person"] = line["fit"]["64"]["max_ms"] < line["stock"]["min_ms"]
    print(json.dumps(line), flush=True)
    assert line["condition_b64_faster_than_stock_one_person"], "the batched fit is slower than the stock loop: wrong shape"


if __name__ == "__main__":
    main()
