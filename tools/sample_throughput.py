#!/usr/bin/env python3
"""Throughput of the sample-noise kernels (pose2mesh_release_amd.sample) on the GPU, by HIP events: samples/s at B = 256 of
  coco_typical   p2m_pose_noise_coco, a standing figure in a 288 x 384 crop with all joints valid: every left / right pair is
                 close enough to need the miss counts (2 x 2000 candidates per joint)
  coco_far       the same with every pair far apart (area / 400): the counts are skipped
  table          p2m_pose_noise_table, 17 joints
  chain_coco / chain_table / chain_none   p2m_train_sample (TrainSampleBuilder) at SMPL size (6890 vertices), drawn rot / flip:
                 17 + 2 coco input joints with the coco noise; the human36 input set with the table noise; and without noise
  chain_none_small   chain_none on 64 vertices: the per-sample joint section alone, next to no mesh to stream
each call advancing the stream index, as in training.  Prints one JSON line.  Each leg runs in a child process of its own
under `timeout`; the first leg that fails ends the run.
Usage: python tools/sample_throughput.py [--steps 200] [--warmup 20] [--leg-timeout 120]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B = 256
LEGS = ("coco_typical", "coco_far", "table", "chain_coco", "chain_table", "chain_none", "chain_none_small")
NV, NV_SMALL = 6890, 64


def leg(name, steps, warmup):
    import numpy as np
    import torch
    from pose2mesh_release_amd import sample, synth
    assert torch.cuda.is_available(), "sample_throughput needs the GPU"
    rng = np.random.default_rng(0)
    if name.startswith("chain"):
        return chain_leg(name, steps, warmup, rng)
    xy = np.asarray(synth.COCO_STANDING_POSE, np.float32)[None] + rng.normal(0, 3, (B, 17, 2)).astype(np.float32)
    joints = torch.from_numpy(np.concatenate([xy, np.ones((B, 17, 1), np.float32)], axis=2)).cuda()
    area = torch.full((B,), 104.0 * 291.0 / (400.0 if name == "coco_far" else 1.0), device="cuda")
    st = sample.NoiseStream(123)
    if name == "table":
        pose = joints[:, :, :2].contiguous()
        mean = torch.from_numpy(rng.normal(0, 2, (17, 2)).astype(np.float32)).cuda()
        std = torch.from_numpy(rng.uniform(0.5, 6, (17, 2)).astype(np.float32)).cuda()
        weight = torch.from_numpy(rng.uniform(0.05, 0.95, 17).astype(np.float32)).cuda()
        out = torch.empty_like(pose)

        def call():
            sample.noise_table(pose, mean, std, weight, st, out=out)
    else:
        out, kind = torch.empty_like(joints), torch.empty((B, 17), dtype=torch.int8, device="cuda")

        def call():
            sample.noise_coco(joints, area, st, out=out, kind=kind)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        call()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    res = {"B": B, "ms_per_call": round(ms, 4), "samples_per_s": round(B / ms * 1e3, 1), "us_per_sample": round(ms * 1e3 / B, 3)}
    if name != "table":
        res["kind_share"] = {k: round(float((kind == v).float().mean()), 4)
                             for k, v in (("jitter", 0), ("miss", 1), ("inversion", 2), ("good", 4), ("zeroed", -1))}
    return res


def chain_leg(name, steps, warmup, rng):
    import numpy as np
    import torch
    from pose2mesh_release_amd import sample, synth
    nv = NV_SMALL if name.endswith("_small") else NV
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    verts = cu(rng.normal(0, 1, (B, nv, 3)) * [0.25, 0.5, 0.15])
    trans = cu(np.stack([rng.uniform(-0.4, 0.4, B), rng.uniform(-0.4, 0.4, B), rng.uniform(3, 6, B)], axis=1))
    focal, princpt = cu(rng.uniform(1000, 1500, (B, 2))), cu(rng.uniform(400, 600, (B, 2)))
    reg = synth.synthetic_regressor(17, nv, seed=5)
    coco_pairs = [(a, a + 1) for a in range(1, 17, 2)]
    if name == "chain_coco":
        b = sample.TrainSampleBuilder(reg, synth.synthetic_regressor(17, nv, seed=6), ((11, 12), (5, 6)), (0, 17), coco_pairs,
                                      noise="coco", rotate_factor=30, flip=True)
    else:
        table = (rng.normal(0, 2, (17, 2)), rng.uniform(0.5, 6, (17, 2)), rng.uniform(0.05, 0.95, 17))
        b = sample.TrainSampleBuilder(reg, None, (), (0, 0), ((1, 4), (2, 5), (3, 6), (14, 11), (15, 12), (16, 13)),
                                      noise="table" if name == "chain_table" else None, table=table if name == "chain_table" else None,
                                      rotate_factor=30, flip=True)
    out = b.buffers(B)
    for _ in range(warmup):
        b(verts, focal, princpt, trans=trans, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.pose2d).all()) and int(out.status.max()) == 0
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        b(verts, focal, princpt, trans=trans, out=out)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    return {"B": B, "nv": nv, "ms_per_call": round(ms, 4), "samples_per_s": round(B / ms * 1e3, 1),
            "mesh_GB_per_s": round(2 * B * nv * 12 / ms / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--leg-timeout", type=int, default=120)
    ap.add_argument("--leg", choices=LEGS)
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(args.leg, args.steps, args.warmup)), flush=True)
        return 0
    res = {}
    for name in LEGS:
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"sample_throughput: leg {name} ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps({"sample_throughput": res, "steps": args.steps}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
