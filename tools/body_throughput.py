#!/usr/bin/env python3
"""Throughput of the body-model layer (pose2mesh_release_amd.body) on the GPU, by HIP events: samples/s of
  smpl   B = 256, SMPL-size synthetic model (6890 vertices, 24 joints, 217 coefficients) with a 17-joint extra regressor
  mano   B = 512, MANO-size synthetic model (778 vertices, 16 joints, 145 coefficients, 21 joints out)
  smpl_grad / mano_grad   the same models and batch sizes through the differentiable entry (body.BodyLayer): forward plus
         backward to pose, betas and trans from given gradients of every output, and the same step through stock torch
         autograd on the same GPU (tests/body_grad_ref.py, its fp32 mode on CUDA) - what a user runs without the layer
with the algorithmic bytes of a call - the direction, template and weight tables once per sample tile of the skinning
kernel (and once more, plus the vertex-major direction table, per sample tile of the backward's vertex stage), the
per-sample workspace and the backward's per-block partials written and read once, the outputs written and their gradients
read once - and the fraction of the 6.3 TB/s copy ceiling those bytes per second come to.  Prints one JSON line.  Each leg
runs in a child process of its own under `timeout`; the first leg that fails ends the run.
Usage: python tools/body_throughput.py [--steps 200] [--warmup 20] [--leg-timeout 240]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COPY_CEILING = 6.3e12
LEGS = {"smpl": ("smpl", 256, 17), "mano": ("mano", 512, 0), "smpl_grad": ("smpl", 256, 17), "mano_grad": ("mano", 512, 0)}


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


def grad_leg(name, steps, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import body_grad_ref
    from pose2mesh_release_amd import body, synth
    assert torch.cuda.is_available(), "body_throughput needs the GPU"
    kind, B, nx = LEGS[name]
    m = synth.body_model(kind)
    V, J = m["num_vertex"], len(m["parents"])
    reg = synth.synthetic_regressor(nx, V) if nx else None
    model = body.BodyModel(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["weights"], m["parents"],
                           betas=m["betas"], hands_mean=m.get("hands_mean"), tip_vertices=m.get("tip_vertices"),
                           joint_order=m.get("joint_order"), scale=m.get("scale", 1.0), extra_regressor=reg)
    layer = body.BodyLayer(model)
    rng = np.random.default_rng(0)

    def cuda(a, grad=False):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().requires_grad_(grad)
    ins = [cuda(rng.standard_normal((B, 3 * J)) * 0.6, True), cuda(rng.standard_normal((B, 10)), True),
           cuda(rng.standard_normal((B, 3)), True)]
    ups = [cuda(rng.standard_normal(s)) for s in [(B, V, 3), (B, model.NJ, 3)] + ([(B, nx, 3)] if nx else [])]
    grads = torch.autograd.grad(layer(*ins), ins, ups)
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    ms = event_ms(lambda: torch.autograd.grad(layer(*ins), ins, ups), steps, warmup)
    plain = [x.detach() for x in ins]
    ms_fwd = event_ms(lambda: model(*plain), steps, warmup)
    tables = {k: (torch.from_numpy(np.asarray(v, np.float32)).cuda() if isinstance(v, np.ndarray) else v) for k, v in m.items()}
    treg = None if reg is None else cuda(reg)

    def stock():
        out = body_grad_ref.forward(tables, ins[0], ins[1], ins[2], None, treg, dtype=torch.float32, device="cuda")
        return torch.autograd.grad(out, ins, ups)
    ref = stock()
    worst = max(float((a - b).norm() / b.norm()) for a, b in zip(grads, ref))
    assert worst < 1e-4, f"the layer and stock autograd disagree: {worst}"
    ms_torch = event_ms(stock, max(steps // 10, 5), max(warmup // 10, 2))
    K = 10 + 9 * (J - 1)
    kpad = -(-K // 4) * 4
    tiles, nblk = -(-B // body.SAMPLE_TILE), -(-V // body.VERTEX_TILE)
    ws = K + 12 * J + 4
    part = 24 * (J + 1) + kpad
    fwd = tiles * (K * 3 * V + 3 * V + J * V) + B * (2 * ws + 3 * J + 13) + B * 3 * (V + model.NJ + nx)
    bwd = (tiles * (K * 3 * V + kpad * 3 * V + 3 * V + J * V) + B * ws + 2 * nblk * B * part + B * 3 * (V + model.NJ + nx)
           + B * (6 * J + 26))
    nbytes = 4 * (fwd + bwd)
    return {"B": B, "V": V, "J": J, "coeffs": K, "ms_per_call": round(ms, 4), "ms_forward_only": round(ms_fwd, 4),
            "samples_per_s": round(B / ms * 1e3, 1), "us_per_sample": round(ms * 1e3 / B, 3),
            "algorithmic_MB": round(nbytes / 1e6, 2), "algorithmic_MB_forward": round(4 * fwd / 1e6, 2),
            "copy_ceiling_fraction": round(nbytes / (ms * 1e-3) / COPY_CEILING, 4),
            "torch_autograd_ms_per_call": round(ms_torch, 4), "speedup_over_torch_autograd": round(ms_torch / ms, 2)}


def leg(name, steps, warmup):
    if name.endswith("_grad"):
        return grad_leg(name, steps, warmup)
    import numpy as np
    import torch
    from pose2mesh_release_amd import body, synth
    assert torch.cuda.is_available(), "body_throughput needs the GPU"
    kind, B, nx = LEGS[name]
    m = synth.body_model(kind)
    V, J = m["num_vertex"], len(m["parents"])
    reg = synth.synthetic_regressor(nx, V) if nx else None
    layer = body.BodyModel(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["weights"], m["parents"],
                           betas=m["betas"], hands_mean=m.get("hands_mean"), tip_vertices=m.get("tip_vertices"),
                           joint_order=m.get("joint_order"), scale=m.get("scale", 1.0), extra_regressor=reg)
    rng = np.random.default_rng(0)
    pose = torch.from_numpy((rng.standard_normal((B, 3 * J)) * 0.6).astype(np.float32)).cuda()
    betas = torch.from_numpy(rng.standard_normal((B, 10)).astype(np.float32)).cuda()
    trans = torch.from_numpy(rng.standard_normal((B, 3)).astype(np.float32)).cuda()
    for _ in range(warmup):
        out = layer(pose, betas, trans)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in out)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        layer(pose, betas, trans)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    K = 10 + 9 * (J - 1)
    tiles = -(-B // body.SAMPLE_TILE)
    ws = K + 12 * J + 4
    nbytes = 4 * (tiles * (K * 3 * V + 3 * V + J * V) + B * (2 * ws + 3 * J + 13) + B * 3 * (V + layer.NJ + nx))
    return {"B": B, "V": V, "J": J, "coeffs": K, "ms_per_call": round(ms, 4), "samples_per_s": round(B / ms * 1e3, 1),
            "us_per_sample": round(ms * 1e3 / B, 3), "algorithmic_MB": round(nbytes / 1e6, 2),
            "copy_ceiling_fraction": round(nbytes / (ms * 1e-3) / COPY_CEILING, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--leg", choices=sorted(LEGS))
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(args.leg, args.steps, args.warmup)), flush=True)
        return 0
    res = {}
    for name in ("smpl", "mano", "smpl_grad", "mano_grad"):
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"body_throughput: leg {name} ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps({"body_throughput": res, "copy_ceiling_TBps": COPY_CEILING / 1e12, "steps": args.steps}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
