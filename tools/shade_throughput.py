#!/usr/bin/env python3
"""Shading throughput (GPU).  Prints one JSON line with, for each of
  smpl / mano       B = 64 hull meshes of SMPL size (6890 vertices, 13776 faces) / MANO size (778, 1552) in 64 images of
                    500 x 500 (batch mode, culling on, a per-mesh background)
  scene             one 1920 x 1080 image of 8 SMPL-size bodies, list order
the time of one call, in the same process and on the same buffers, of
  render            p2m_mesh_render alone (MeshRenderer)
  normals           p2m_vertex_normals
  flat / smooth / full   p2m_mesh_shade through the C ABI on the rasteriser's visibility buffer: flat with mesh colours; with
                    interpolated normals; with normals, vertex colours, C = 3 attributes, barycentrics and a one-pixel wire
  copy_*            a device-to-device copy that moves the kernel's ALGORITHMIC bytes (half read, half written): ids 8 B + background
                    3 B + image 3 B (+ 12 B bary, + 4 C B attributes) per pixel, and every per-vertex array once
  empty             a one-element fill: what a launch costs
Each time is the median over `--repeats` windows of `--steps` back-to-back calls between two device events (ms), with the spread
(max - min) / median over the windows beside it; share_of_copy = copy time / kernel time; vs_render = kernel time / render time.
Usage: python tools/shade_throughput.py [--steps 50] [--warmup 5] [--repeats 5]"""
import argparse
import ctypes as ct
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from render_throughput import oriented  # noqa: E402


def timed(body, args):
    """(median ms per call, spread) over args.repeats windows of args.steps calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.warmup):
        body()
    w = []
    for _ in range(args.repeats):
        e0.record()
        for _ in range(args.steps):
            body()
        e1.record()
        torch.cuda.synchronize()
        w.append(e0.elapsed_time(e1) / args.steps)
    med = float(np.median(w))
    return med, (max(w) - min(w)) / med


def copy_of(nbytes):
    half = max(1, nbytes // 2)
    a, b = torch.zeros(half, dtype=torch.uint8, device="cuda"), torch.zeros(half, dtype=torch.uint8, device="cuda")
    return lambda: b.copy_(a)


def leg(r, verts, cam, col, bg, args):
    from pose2mesh_release_amd import _lib, render
    lib = _lib.hip()
    p = lambda t: None if t is None else ct.c_void_p(t.data_ptr())                    # noqa: E731
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, nv = int(verts.shape[0]), int(verts.shape[1])
    H, W, scene = r.height, r.width, r.mode == "scene"
    n = 1 if scene else B
    out = r(verts, cam, col, bg)
    table = render.vertex_face_table(r.faces_host, nv).on(verts.device)
    normals, nst = render.vertex_normals(verts, table)
    assert not int(nst.any()) and not int(out["status"].any())
    rng = np.random.default_rng(2)
    vcol = torch.from_numpy(rng.uniform(0.1, 1.0, (B, nv, 3)).astype(np.float32)).cuda()
    attrs = torch.from_numpy(rng.uniform(-1.0, 1.0, (B, nv, 3)).astype(np.float32)).cuda()
    image = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    bary = torch.zeros((n, H, W, 3), dtype=torch.float32, device="cuda")
    attr_out = torch.zeros((n, H, W, 3), dtype=torch.float32, device="cuda")
    status = torch.zeros((B,), dtype=torch.int32, device="cuda")
    wire_rgb = (ct.c_uint8 * 3)(20, 20, 20)
    per = 1 if bg.dim() == 4 else 0

    def shade(colours, vc, nrm, att, wire_T, bary_out, att_out):
        def body():
            rc = lib.p2m_mesh_shade(p(out["face_id"]), p(out["mesh_id"]), p(verts), p(r._faces), r.nf, p(cam), p(colours), p(vc), 0,
                                    p(nrm), r._lights, len(r.lights), r.ambient, p(att), 3 if att is not None else 0, wire_T,
                                    wire_rgb, 0, p(bg), per, 0.0, B, nv, H, W, 1 if scene else 0, p(image), p(bary_out),
                                    p(att_out), p(status), stream)
            assert rc == 0, lib.p2m_last_error_string()
        return body

    def normals_body():
        rc = lib.p2m_vertex_normals(p(verts), p(table.faces), p(table.ptr), p(table.idx), int(table.idx.numel()), B, nv, r.nf,
                                    p(normals), p(nst), stream)
        assert rc == 0

    px, vb = n * H * W, B * nv * 12
    bytes_of = {"normals": 2 * vb + r.nf * 12 + (nv + 1) * 4 + int(table.idx.numel()) * 4,
                "flat": px * 14 + vb, "smooth": px * 14 + 2 * vb, "full": px * (14 + 12 + 12) + 4 * vb}
    bodies = {"normals": normals_body, "flat": shade(r._bufs[(B, nv)]["colours"], None, None, None, 0, None, None),
              "smooth": shade(r._bufs[(B, nv)]["colours"], None, normals, None, 0, None, None),
              "full": shade(None, vcol, normals, attrs, 256, bary, attr_out)}
    res = {"B": B, "nv": nv, "nf": r.nf, "H": H, "W": W, "covered_share": round(float(out["mask"].float().mean()), 3)}
    render_ms, spread = timed(lambda: r(verts, cam, col, bg), args)
    res["render"] = {"ms": round(render_ms, 4), "spread": round(spread, 3)}
    for k, body in bodies.items():
        ms, spread = timed(body, args)
        cms, cspread = timed(copy_of(bytes_of[k]), args)
        res[k] = {"ms": round(ms, 4), "spread": round(spread, 3), "bytes": bytes_of[k], "copy_ms": round(cms, 4),
                  "copy_spread": round(cspread, 3), "share_of_copy": round(cms / ms, 3), "vs_render": round(ms / render_ms, 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "shade_throughput needs the GPU"
    from pose2mesh_release_amd import render, synth
    line = {"steps": args.steps, "repeats": args.repeats}
    one = torch.zeros(1, device="cuda")
    ms, spread = timed(lambda: one.fill_(1.0), args)
    line["empty"] = {"ms": round(ms, 4), "spread": round(spread, 3)}
    for name, nv in (("smpl", 6890), ("mano", 778)):
        B, H, W = 64, 500, 500
        pts, faces = synth.hull_mesh(nv)
        faces = oriented(pts, faces)
        rng = np.random.default_rng(0)
        verts = torch.from_numpy((pts[None] * rng.uniform(0.5, 0.9, (B, 1, 1))).astype(np.float32)).cuda()
        cam = torch.from_numpy(np.concatenate([rng.uniform(0.7, 1.0, (B, 2)), rng.uniform(-0.2, 0.2, (B, 2))], 1).astype(np.float32)).cuda()
        bg = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
        col = torch.tensor([1.0, 1.0, 0.9], device="cuda")
        line[name] = leg(render.MeshRenderer(faces, H, W, num_vertex=nv), verts, cam, col, bg, args)
        if name == "smpl":
            body = (pts, faces)
    pts, faces = body
    H, W, B = 1080, 1920, 8
    rng = np.random.default_rng(1)
    verts = torch.from_numpy((pts[None] * 0.9 * np.array([0.45, 1.0, 0.3])).astype(np.float32)).repeat(B, 1, 1).cuda()
    cam = np.zeros((B, 4), np.float32)
    cam[:, 0], cam[:, 1] = 0.45 * H / W, 0.45                    # bodies about 430 px tall
    cam[:, 2], cam[:, 3] = np.linspace(-3.0, 3.0, B), rng.uniform(-0.6, 0.6, B)
    bg = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    col = torch.from_numpy(rng.uniform(0.3, 1.0, (B, 3)).astype(np.float32)).cuda()
    r = render.MeshRenderer(faces, H, W, mode="scene", order="list", num_vertex=pts.shape[0])
    line["scene"] = leg(r, verts, torch.from_numpy(cam).cuda(), col, bg, args)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
