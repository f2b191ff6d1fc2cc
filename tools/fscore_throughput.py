#!/usr/bin/env python3
"""Test-loop throughput with F-scores, B = 64 (GPU).  Prints one JSON line of meshes/s for
  smpl.infer         GraphedInference alone on the H36M-joint SMPL-size golden graphs (6890 vertices)
  smpl.infer_eval_f  the same plus MeshEvaluator (stage A + E, PA-MPVPE) and FScoreEvaluator (centred + aligned, 5 / 15 mm)
                     per batch, one summary() each at the end
  mano.*             the same two for the MANO-size net (778 vertices)
  *.infer_host_f     GraphedInference plus the host path the F-score kernels replace: .cpu().numpy() per batch, then per
                     sample the float64 transforms (tests/fscore_ref.py) and a scipy.spatial.cKDTree query per direction
and, for the F-score launches alone (cuda events around back-to-back calls), their time per batch, the f32 VALU bound
from the search kernel's own instruction count and the share of that bound achieved:
  pairs = B x nv^2 x 2 directions x 2 variants;  the search loop issues 104 vector instructions per 16 pairs (48 v_sub,
  16 v_mul, 32 v_fmac, 8 v_min3: 6.5 per pair, none packed); a SIMD issues a wave64 instruction over 2 cycles (32 lanes
  per clock), so the chip retires 256 CUs x 4 SIMDs x 32 lanes per clock at <= 2.4 GHz.  The bound leaves out the query
  tiles' tails (7 x 1024 queries for 6890 vertices: + 4 %), the prepare and fold launches and the LDS staging.
Usage: python tools/fscore_throughput.py [--steps 50] [--warmup 5] [--host-steps 2]"""
import argparse
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

INSTR_PER_PAIR = 6.5
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def timed(body, steps, warmup):
    for i in range(warmup):
        body(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        body(i)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def leg(joint_set, nv, R, args):
    import fscore_ref
    import helpers
    from scipy.spatial import cKDTree
    from pose2mesh_release_amd import evaluate, infer, pose2mesh_net, synth
    B = 64
    gL, _, rev = helpers.golden_graphs(joint_set)
    J = int(gL[-1].shape[0])
    net = pose2mesh_net.get_model(J, gL, mano=(joint_set == "mano"))
    net.load_state_dict(helpers.numpy_state(net.state_dict(), 2))
    net = net.cuda().eval()
    if R is None:
        R = synth.synthetic_regressor(J, nv)
    step = infer.GraphedInference(net, np.asarray(rev), nv, R, B, scale=1000.0)
    xs = [synth.pose2d_batch(B, J, seed=s).cuda() for s in range(4)]
    # ground truth: the net's own output of another batch, perturbed (metres, read x 1000): distances of a few mm
    with torch.no_grad():
        base = step(xs[3])[0].clone()
    rng = np.random.default_rng(0)
    gt = (base + torch.from_numpy(rng.standard_normal((B, nv, 3)).astype(np.float32) * 4.0).cuda()) / 1000.0
    ev = evaluate.MeshEvaluator(nv, R, 0, regressor_E=R, root_E=0, pa_mesh=True, gt_mesh_scale=1000.0)
    fs = evaluate.FScoreEvaluator(nv, R, 0, thresholds=(5.0, 15.0), gt_mesh_scale=1000.0)
    res = {}
    res["infer"] = B * args.steps / timed(lambda i: step(xs[i % 4]), args.steps, args.warmup)

    def body(i):
        mesh, _, _ = step(xs[i % 4])
        ev(mesh, gt)
        fs(mesh, gt)
    ev.reset()
    fs.reset()
    dt = timed(body, args.steps, args.warmup)
    t0 = time.perf_counter()
    s, sf = ev.summary(), fs.summary()                           # the syncs of a whole test set
    dt += time.perf_counter() - t0
    assert s["samples"] == sf["samples"] == B * (args.steps + args.warmup) and np.isfinite(sf["pa_f@5"])
    res["infer_eval_f"] = B * args.steps / dt

    gt_h = gt.cpu().numpy()

    def host(i):
        m = step(xs[i % 4])[0].cpu().numpy()
        for al in (False, True):
            P, G = fscore_ref.transformed(m, gt_h, 1000.0, R, 0, aligned=al)
            for p, g in zip(P, G):
                dp, dg = cKDTree(g).query(p)[0], cKDTree(p).query(g)[0]
                [fscore_ref.score(dp, dg, th) for th in (5.0, 15.0)]
    res["infer_host_f"] = B * args.host_steps / timed(host, args.host_steps, 1)

    # the F-score launches alone
    mesh = step(xs[0])[0].clone()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.warmup):
        fs(mesh, gt)
    e0.record()
    for _ in range(args.steps):
        fs(mesh, gt)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    bound_ms = 1e3 * B * nv * nv * 4 * INSTR_PER_PAIR / LANE_OPS_PER_S
    infer_ms = 1e3 * B / res["infer"]
    return {"nv": nv, "meshes_per_s": {k: round(v, 1) for k, v in res.items()},
            "eval_f_cost_pct": round(100.0 * (res["infer"] / res["infer_eval_f"] - 1.0), 2),
            "vs_host": round(res["infer_eval_f"] / res["infer_host_f"], 1),
            "infer_ms": round(infer_ms, 3), "fscore_ms": round(ms, 4), "fscore_share_of_infer_pct": round(100.0 * ms / infer_ms, 2),
            "valu_bound_ms": round(bound_ms, 4), "valu_bound_share": round(bound_ms / ms, 3),
            "f": {k: round(v, 4) for k, v in sf.items() if k.startswith(("f@", "pa_f@"))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fscore_throughput needs the GPU"
    import helpers
    from pose2mesh_release_amd import ops
    line = {"B": 64, "arith": ops.GEMM_ARITH, "steps": args.steps,
            "smpl": leg("human36", 6890, helpers.golden_regressor("demo_h36m.npz"), args),
            "mano": leg("mano", 778, None, args)}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
