#!/usr/bin/env python3
"""Throughput of the video module (pose2mesh_release_amd.video) on the GPU, by HIP events:
  joints   the filter at joint size: 37 sequences, 35 515 frames in all (3DPW's test split), C = 42
  mesh     the filter at mesh size: 8 tracks x 256 frames x 20 670 coordinates
  stream   the streaming call OneEuroFilter()(x) at x [64, 6890, 3]: one new frame for each of 64 tracks
  eval     VideoEvaluator.summary() at the 3DPW size (37 videos, 35 515 frames, 14 joints): gather, filter, metrics, one sync
each beside two yardsticks measured in the same run: a device-to-device copy of the filter's algorithmic bytes (8 per
element: every input read once, every output written once; the streaming call moves 24 per element, its state included) and
the reference's numpy loop on the host (tests/video_ref.py, which restates lib/smooth_utils.py and the loop of
data/PW3D/dataset.py:391-414 operation by operation).  Prints one JSON line.  Each leg runs in a child process of its own
under `timeout`; the first leg that fails ends the run.
Usage: python tools/video_throughput.py [--steps 100] [--warmup 10] [--leg-timeout 240]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

LEGS = ("joints", "mesh", "stream", "eval")
PW3D_VIDEOS, PW3D_FRAMES = 37, 35515


def event_ms(step, steps, warmup):
    import torch
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def copy_ms(elements, steps, warmup):
    """A device-to-device copy of `elements` floats: 8 bytes moved per element."""
    import torch
    a = torch.randn(elements, device="cuda")
    b = torch.empty_like(a)
    return event_ms(lambda: b.copy_(a), steps, warmup)


def pw3d_lengths():
    base, rem = divmod(PW3D_FRAMES, PW3D_VIDEOS)
    return [base + (1 if s < rem else 0) for s in range(PW3D_VIDEOS)]


def leg(name, steps, warmup):
    import numpy as np
    import torch
    import video_ref
    from pose2mesh_release_amd import video
    assert torch.cuda.is_available(), "video_throughput needs the GPU"
    rng = np.random.default_rng(0)
    res = {"lookahead": video.lookahead()}
    if name in ("joints", "mesh"):
        lens, C = (pw3d_lengths(), 42) if name == "joints" else ([256] * 8, 20670)
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        N = int(ptr[-1])
        x = (np.cumsum(rng.standard_normal((N, C), dtype=np.float32) * 5, axis=0) % 2000).astype(np.float32)
        xg, sp = torch.from_numpy(x).cuda(), torch.from_numpy(ptr).cuda()
        out = torch.empty_like(xg)
        ms = event_ms(lambda: video.smooth_pose(xg, 0.004, 0.005, seq_ptr=sp, out=out), steps, warmup)
        t = time.perf_counter()
        ref = video_ref.one_euro_seqs(x, ptr, 0.004, 0.005)
        host_ms = (time.perf_counter() - t) * 1e3
        assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32)), "the kernel and the numpy loop disagree"
        cms = copy_ms(N * C, steps, warmup)
        res.update(sequences=len(lens), frames=N, C=C, ms_per_call=round(ms, 4), algorithmic_MB=round(8 * N * C / 1e6, 2),
                   GBps=round(8 * N * C / ms / 1e6, 1), copy_ms=round(cms, 4), copy_GBps=round(8 * N * C / cms / 1e6, 1),
                   copy_ceiling_fraction=round(cms / ms, 4), numpy_loop_ms=round(host_ms, 1),
                   speedup_over_numpy_loop=round(host_ms / ms, 1))
    elif name == "stream":
        B, shape = 64, (6890, 3)
        frames = [torch.randn((B,) + shape, device="cuda") * 100 for _ in range(4)]
        f = video.OneEuroFilter(0.004, 0.005)
        k = [0]

        def step():
            f(frames[k[0] & 3])
            k[0] += 1
        ms = event_ms(step, steps, warmup)
        n = B * shape[0] * shape[1]
        xs = [fr.reshape(B, -1).cpu().numpy() for fr in frames]
        t = time.perf_counter()
        st = None
        for i in range(8):
            _, st = video_ref.one_euro(xs[i & 3].reshape(1, -1), 0.004, 0.005, state=st)
        host_ms = (time.perf_counter() - t) * 1e3 / 8
        cms = copy_ms(3 * n, steps, warmup)                  # x, state_x, state_dx in; y, state_x, state_dx out: 24 B / element
        res.update(tracks=B, coordinates=shape[0] * shape[1], ms_per_call=round(ms, 4), algorithmic_MB=round(24 * n / 1e6, 2),
                   GBps=round(24 * n / ms / 1e6, 1), copy_ms=round(cms, 4), copy_GBps=round(24 * n / cms / 1e6, 1),
                   copy_ceiling_fraction=round(cms / ms, 4), numpy_step_ms=round(host_ms, 2),
                   speedup_over_numpy_step=round(host_ms / ms, 1))
    else:
        lens, J = pw3d_lengths(), 14
        N = sum(lens)
        order = rng.permutation(N)                           # dataset positions of the videos' frames: not contiguous
        vi, a = [], 0
        for n in lens:
            vi.append(np.sort(order[a:a + n]))
            a += n
        gt = (rng.standard_normal((N, J, 3)) * 250).astype(np.float32)
        pred = (gt + rng.standard_normal((N, J, 3)).astype(np.float32) * 25).astype(np.float32)
        ve = video.VideoEvaluator(vi, J)
        pg, gg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
        for first in range(0, N, 64):
            ve.put(first, pg[first:first + 64], gg[first:first + 64])
        torch.cuda.synchronize()
        for _ in range(warmup):
            out = ve.summary()
        t = time.perf_counter()
        for _ in range(steps):
            out = ve.summary()
        ms = (time.perf_counter() - t) * 1e3 / steps            # wall clock: summary() ends with its sync
        rows, ptr = video_ref.tables(vi)
        t = time.perf_counter()
        sm = video_ref.one_euro_seqs(pred.reshape(N, -1), ptr, 0.004, 0.005, rows=rows).reshape(N, J, 3)
        ref = video_ref.video_eval(sm, gt[rows], ptr)
        host_ms = (time.perf_counter() - t) * 1e3
        for key, want in zip(("accel_error", "mpjpe", "pa_mpjpe"), ref["totals"]):
            assert abs(out[key] - want) <= 1e-9 * abs(want), (key, out[key], want)
        res.update(videos=len(lens), frames=N, J=J, ms_per_summary=round(ms, 4), numpy_loop_ms=round(host_ms, 1),
                   speedup_over_numpy_loop=round(host_ms / ms, 1), accel_error=round(out["accel_error"], 4),
                   mpjpe=round(out["mpjpe"], 4), pa_mpjpe=round(out["pa_mpjpe"], 4))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--leg-timeout", type=int, default=240)
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
            print(f"video_throughput: leg {name} ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps({"video_throughput": res, "steps": args.steps}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
