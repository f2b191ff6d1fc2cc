#!/usr/bin/env python3
"""Throughput of the annotation layer (pose2mesh_release_amd.annot) on the GPU, by HIP events, at B = 256, SMPL size (24
joints, 10 betas, 6890 vertices, 17 annotated joints) and N = 1e6 table rows, the Human3.6M flag set:
  gather      src(idx): one p2m_annot_gather launch, idx a slice of a device permutation
  bank_1      GenderedBody of one model: the model's own forward (nothing added)
  bank_3      GenderedBody of three models: three forwards and the p2m_body_select launch
  select      the p2m_body_select launch of bank_3 alone (bank_3 minus three forwards, measured directly)
  chain       idx -> src -> bank of three -> TrainSampleBuilder (table noise, drawn rot / flip) -> the train step's tensors
  host_loop   what `gather` replaces, on this machine's CPU: the same glue per sample in numpy + scipy's Rotation (the
              reference uses transforms3d), one Python loop over the batch; no GPU involved
Each timed window is `steps` calls between two events; the figure is the median of `repeats` windows.  Prints one JSON
line.  Each leg runs in a child process of its own under `timeout`; the first leg that fails ends the run.
Usage: python tools/annot_throughput.py [--steps 100] [--warmup 20] [--repeats 7] [--rows 1000000] [--leg-timeout 240]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, NV, JR = 256, 6890, 17
LEGS = ("gather", "bank_1", "bank_3", "select", "chain", "host_loop")


def make_tables(N, G, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    f4 = np.float32
    v = rng.standard_normal((N, 3))
    v *= rng.uniform(0.05, 3.1, (N, 1)) / np.linalg.norm(v, axis=1, keepdims=True)
    from scipy.spatial.transform import Rotation
    return dict(pose=(rng.standard_normal((N, 72), dtype=f4) * f4(0.6)), betas=rng.standard_normal((N, 10), dtype=f4),
                trans=(rng.standard_normal((N, 3)) * 0.5 + [0, 0, 1]).astype(f4),
                cam_R=Rotation.from_rotvec(v).as_matrix().astype(f4),
                cam_t=(rng.standard_normal((N, 3)) * [400, 400, 600] + [0, 0, 4500]).astype(f4),
                focal=rng.uniform(1000, 1500, (N, 2)).astype(f4), princpt=rng.uniform(400, 600, (N, 2)).astype(f4),
                gender=rng.integers(0, G, N).astype(np.uint8),
                given_cam=(rng.standard_normal((N, JR, 3), dtype=f4) * f4(300)), given_img=rng.uniform(0, 1000, (N, JR, 2)).astype(f4))


def make_bank(G, with_extra=True):
    from pose2mesh_release_amd import annot, body, synth
    reg = synth.synthetic_regressor(JR, NV, seed=5) if with_extra else None
    models = []
    for s in range(G):
        m = synth.body_model("smpl", NV, seed=s)
        models.append(body.BodyModel(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["weights"], m["parents"],
                                     betas=m["betas"], extra_regressor=reg))
    return annot.GenderedBody(models), reg


def timed(call, steps, warmup, repeats):
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            call()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / steps)
    med = statistics.median(ms)
    return {"B": B, "ms_per_call": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "samples_per_s": round(B / med * 1e3, 1)}


def host_glue(t, rows, root_template, root_shapedirs):
    """The Human3.6M glue on the parameters for the rows of one batch, as the dataset code does it per sample."""
    import numpy as np
    from scipy.spatial.transform import Rotation
    out = []
    for r in rows:
        pose, shape = t["pose"][r].astype(np.float64).reshape(-1, 3), t["betas"][r].astype(np.float64)
        R = t["cam_R"][r].astype(np.float64)
        if (np.abs(shape) > 3).any():
            shape = np.zeros_like(shape)
        pose[0] = (Rotation.from_matrix(R) * Rotation.from_rotvec(pose[0])).as_rotvec()
        g = t["gender"][r]
        J0 = root_template[g] + root_shapedirs[g] @ shape
        trans = R @ t["trans"][r] + t["cam_t"][r] / 1000 - J0 + R @ J0
        out.append((pose.reshape(-1).astype(np.float32), shape.astype(np.float32), trans.astype(np.float32), t["focal"][r],
                    t["princpt"][r], g, t["given_cam"][r], t["given_img"][r]))
    return [np.stack([o[k] for o in out]) for k in range(8)]


def leg(name, steps, warmup, repeats, N):
    import numpy as np
    if name == "host_loop":
        t = make_tables(min(N, 100000), 3)
        rng = np.random.default_rng(1)
        rt, rs = rng.standard_normal((3, 3)) * 0.1, rng.standard_normal((3, 3, 10)) * 0.01
        ms = []
        for _ in range(repeats + 1):
            rows = rng.integers(0, len(t["pose"]), B)
            t0 = time.perf_counter()
            host_glue(t, rows, rt, rs)
            ms.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ms[1:])
        return {"B": B, "ms_per_call": round(med, 3), "ms_min": round(min(ms[1:]), 3), "ms_max": round(max(ms[1:]), 3),
                "samples_per_s": round(B / med * 1e3, 1), "threads": 1}
    import torch
    from pose2mesh_release_amd import _lib, annot, sample
    assert torch.cuda.is_available(), "annot_throughput needs the GPU"
    res = {}
    if name in ("gather", "chain"):
        bank, reg = make_bank(3)
        t = make_tables(N, 3)
        src = annot.AnnotationSource(t["pose"], t["betas"], t["trans"], t["cam_R"], t["cam_t"], focal=t["focal"],
                                     princpt=t["princpt"], gender=t["gender"], given_cam=t["given_cam"],
                                     given_img=t["given_img"], models=bank, preset="human36m")
        del t
        perm = torch.randperm(N, device="cuda")
        pos = [0]

        def next_idx():
            if pos[0] + B > N:
                pos[0] = 0
            pos[0] += B
            return perm[pos[0] - B:pos[0]]
        if name == "gather":
            res = timed(lambda: src(next_idx()), steps, warmup, repeats)
            res["rows"] = N
            res["bytes_per_sample"] = 4 * (2 * (72 + 10 + 4 + 5 * JR) + 3 + 9 + 3 + 3 + 2) + 1 + 8
            assert int(src(next_idx()).status.max()) in (0, 4)
            return res
        table = (np.zeros((JR, 2)), np.full((JR, 2), 3.0), np.full(JR, 0.5))
        build = sample.TrainSampleBuilder(reg, None, (), (0, 0), ((1, 4), (2, 5), (3, 6), (14, 11), (15, 12), (16, 13)),
                                          noise="table", table=table, rotate_factor=30, flip=True)

        def chain():
            b = src(next_idx())
            verts, _, _ = bank(b.pose, b.betas, b.trans, b.gender)
            return build(verts, b.focal, b.princpt, given=(b.given_cam, b.given_img))
        res = timed(chain, steps, warmup, repeats)
        s = chain()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(s.mesh).all()) and bool(torch.isfinite(s.pose2d).all())
        res.update(rows=N, nv=NV, models=3)
        return res
    G = 1 if name == "bank_1" else 3
    bank, _ = make_bank(G)
    rng = np.random.default_rng(2)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    pose, betas = cu(rng.standard_normal((B, 72)) * 0.6), cu(rng.standard_normal((B, 10)))
    trans = cu(rng.standard_normal((B, 3)) * 0.7)
    gender = torch.from_numpy(rng.integers(0, G, B).astype(np.int32)).cuda()
    if name != "select":
        res = timed(lambda: bank(pose, betas, trans, gender), steps, warmup, repeats)
        res.update(nv=NV, models=G)
        return res
    import ctypes
    outs = [m(pose, betas, trans) for m in bank.models]
    buf = bank._buffers(B, pose.device)
    ptrs = [(ctypes.c_void_p * G)(*[o[k].data_ptr() for o in outs]) for k in range(3)]
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731

    def select():
        _lib.check(_lib.hip().p2m_body_select(ptrs[0], ptrs[1], ptrs[2], G, p(gender), B, bank.V, bank.NJ, bank.JX, p(buf[0]),
                                              p(buf[1]), p(buf[2]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    res = timed(select, steps, warmup, repeats)
    nbytes = 2 * B * 3 * 4 * (bank.V + bank.NJ + bank.JX)
    res.update(nv=NV, models=G, GB_per_s=round(nbytes / res["ms_per_call"] / 1e6, 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--leg", choices=LEGS)
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(args.leg, args.steps, args.warmup, args.repeats, args.rows)), flush=True)
        return 0
    res = {}
    for name in LEGS:
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--rows", str(args.rows)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"annot_throughput: leg {name} ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"{name}: {res[name]}", file=sys.stderr, flush=True)
    print(json.dumps({"annot_throughput": res, "steps": args.steps, "repeats": args.repeats}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
