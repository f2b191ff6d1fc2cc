#!/usr/bin/env python3
"""Render throughput (GPU).  Prints one JSON line:
  smpl / mano       B = 64 hull meshes of SMPL size (6890 vertices, 13776 faces) / MANO size (778, 1552) into 64 images of
                    500 x 500 (batch mode, culling on, a per-mesh background): ms per call and renders/s of MeshRenderer alone
                    (cuda events around back-to-back calls), then meshes/s of GraphedInference alone and of GraphedInference
                    followed by a render that depends on its output (`infer_render`; `infer_render_noise`: the raw output of
                    the random-weight net, vertex noise), and the render's share of the inference step
  scene             one 1920 x 1080 image of 8 SMPL-size bodies, list order: ms per call, renders (images)/s
  yardstick_s_per_mesh   for scale only: tests/render_ref.py on the host, one mesh of each size at 500 x 500
Usage: python tools/render_throughput.py [--steps 50] [--warmup 5] [--no-infer] [--no-host]"""
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


def oriented(points, faces):
    """The hull's faces wound outwards (scipy leaves the winding open; culling needs it)."""
    p, f = np.asarray(points, np.float64), np.asarray(faces, np.int64).copy()
    n = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    flip = (n * p[f].mean(1)).sum(1) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return f


def event_ms(body, steps, warmup):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        body()
    e0.record()
    for _ in range(steps):
        body()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def wall(body, steps, warmup):
    for i in range(warmup):
        body(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        body(i)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def batch_leg(joint_set, nv, args):
    from pose2mesh_release_amd import render, synth
    B, H, W = 64, 500, 500
    pts, faces = synth.hull_mesh(nv)
    faces = oriented(pts, faces)
    rng = np.random.default_rng(0)
    verts = torch.from_numpy((pts[None] * rng.uniform(0.5, 0.9, (B, 1, 1))).astype(np.float32)).cuda()
    cam = torch.from_numpy(np.concatenate([rng.uniform(0.7, 1.0, (B, 2)), rng.uniform(-0.2, 0.2, (B, 2))], 1).astype(np.float32)).cuda()
    bg = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    r = render.MeshRenderer(faces, H, W, num_vertex=nv)
    out = r(verts, cam, background=bg)
    res = {"nv": nv, "nf": int(faces.shape[0]), "covered_share": round(float(out["mask"].float().mean()), 3)}
    ms = event_ms(lambda: r(verts, cam, background=bg), args.steps, args.warmup)
    res["render_ms"], res["renders_per_s"] = round(ms, 4), round(1e3 * B / ms, 1)
    if not args.no_infer:
        import helpers
        from pose2mesh_release_amd import infer, pose2mesh_net
        gL, _, rev = helpers.golden_graphs(joint_set)
        J = int(gL[-1].shape[0])
        net = pose2mesh_net.get_model(J, gL, mano=(joint_set == "mano"))
        net.load_state_dict(helpers.numpy_state(net.state_dict(), 2))
        net = net.cuda().eval()
        step = infer.GraphedInference(net, np.asarray(rev), nv, synth.synthetic_regressor(J, nv), B, scale=1000.0)
        xs = [synth.pose2d_batch(B, J, seed=s).cuda() for s in range(4)]
        with torch.no_grad():
            m = step(xs[0])[0]
            ext = float(m.abs().max())
        # The net carries seeded random weights: its output is vertex noise, every face spans the whole mesh (about 10^8
        # fragments per image) - nothing a trained net produces.  `infer_render` therefore renders the hull displaced by 2 % of
        # the output (one fused torch op on the inference's result: the same data dependency, a mesh-like mesh, in the
        # output's mm); `infer_render_noise` renders the raw output, the worst case of depth complexity.
        cam_mm = torch.tensor([[0.8 / ext, 0.8 / ext, 0.0, 0.0]], device="cuda").repeat(B, 1)
        rm = render.MeshRenderer(faces, H, W, num_vertex=nv, z_range=(-2 * ext, 2 * ext))
        base = (verts * ext).contiguous()
        shown = torch.empty_like(base)
        t_inf = wall(lambda i: step(xs[i % 4]), args.steps, args.warmup)

        def both(i):
            mesh, _, _ = step(xs[i % 4])
            torch.add(base, mesh, alpha=0.02, out=shown)
            rm(shown, cam_mm, background=bg)

        def noise(i):
            mesh, _, _ = step(xs[i % 4])
            rm(mesh, cam_mm, background=bg)
        t_both = wall(both, args.steps, args.warmup)
        t_noise = wall(noise, max(2, args.steps // 10), 1)
        res["meshes_per_s"] = {"infer": round(B * args.steps / t_inf, 1), "infer_render": round(B * args.steps / t_both, 1),
                               "infer_render_noise": round(B * max(2, args.steps // 10) / t_noise, 1)}
        res["infer_ms"] = round(1e3 * t_inf / args.steps, 3)
        res["render_share_of_infer_pct"] = round(100.0 * ms / (1e3 * t_inf / args.steps), 1)
    return res, (pts, faces)


def scene_leg(pts, faces, args):
    from pose2mesh_release_amd import render
    H, W, B = 1080, 1920, 8
    rng = np.random.default_rng(1)
    verts = torch.from_numpy((pts[None] * 0.9 * np.array([0.45, 1.0, 0.3])).astype(np.float32)).repeat(B, 1, 1).cuda()
    cam = np.zeros((B, 4), np.float32)
    cam[:, 0], cam[:, 1] = 0.45 * H / W, 0.45                    # bodies about 430 px tall
    cam[:, 2], cam[:, 3] = np.linspace(-3.0, 3.0, B), rng.uniform(-0.6, 0.6, B)
    cam = torch.from_numpy(cam).cuda()
    bg = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    col = torch.from_numpy(rng.uniform(0.3, 1.0, (B, 3)).astype(np.float32)).cuda()
    r = render.MeshRenderer(faces, H, W, mode="scene", order="list", num_vertex=pts.shape[0])
    out = r(verts, cam, col, bg)
    ms = event_ms(lambda: r(verts, cam, col, bg), args.steps, args.warmup)
    return {"H": H, "W": W, "bodies": B, "covered_share": round(float(out["mask"].float().mean()), 3),
            "render_ms": round(ms, 4), "renders_per_s": round(1e3 / ms, 1)}


def host_leg(pts, faces):
    import render_ref
    c = dict(verts=(0.8 * pts[None]).astype(np.float32), faces=faces, cam=np.array([[0.9, 0.9, 0.0, 0.0]], np.float32), H=500,
             W=500, mode="batch", order="list", cull=True, colours=np.array([[1.0, 1.0, 0.9]], np.float32), background=None,
             z_range=(-1.0, 1.0), lights=np.array([[0.0, 0.0, -1.0, 0.7]], np.float32), ambient=0.3)
    t0 = time.perf_counter()
    render_ref.render_case(c)
    return round(time.perf_counter() - t0, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-infer", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "render_throughput needs the GPU"
    from pose2mesh_release_amd import ops
    smpl, body = batch_leg("human36", 6890, args)
    mano, hand = batch_leg("mano", 778, args)
    line = {"B": 64, "image": [500, 500], "arith": ops.GEMM_ARITH, "steps": args.steps, "smpl": smpl, "mano": mano,
            "scene": scene_leg(*body, args)}
    if not args.no_host:
        line["yardstick_s_per_mesh"] = {"smpl": host_leg(*body), "mano": host_leg(*hand)}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
