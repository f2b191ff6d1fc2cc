"""Fixture maker for the camera tests: records what the REAL reference computes (run on a machine that has the reference
checkout; P2M_REFERENCE_ROOT, default as in oracle/ref_loader.py).  Data only.

  camfit_ref.npz
    prep_<pose>_*   for the poses of prep_poses(): the outputs of the reference's own get_bbox, process_bbox (both calls),
                    j2d_processing (both calls) and the standardisation of demo/run.py:150-159, for FLOAT inputs (float64
                    arrays holding fp32 values, so nothing is truncated as in the int64 demo file).
    fit_<case>_*    for the cases of fit_cases(): inputs, 96 starts (torch.rand((1, 3)) after torch.manual_seed(k)), and for
                    each start the final camera of the real OptimzeCamLayer + nn.L1Loss + optim.Adam loop of run.py:176-189
                    (1500 iterations, the rate lowered after j == 500 and j == 1000) on the CPU, with its float64 loss; the
                    exact optimum and its loss from camfit_ref.l1_optimum.
    sched_*         the same loop stopped after 3 and after 502 iterations, from a start for which the float64 yardstick meets
                    no residual within 1e-3 px of zero: pins the step indices of the rate changes.

    python tests/golden/make_golden_camfit.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import camfit_ref  # noqa: E402
import ref_loader  # noqa: E402

N_STARTS = 96          # the tests launch the first 32; the scatter of conditions (a), (b) is taken over all of them
CROP = 500
BAND = 1e-3


def prep_poses():
    """name -> [J, 2] float32 pixel joints."""
    rng = np.random.default_rng(2024)
    demo = np.load(os.path.join(HERE, "demo_h36m.npz"))["joint_input"].astype(np.float32)
    coco = (np.array([620.0, 340.0]) + rng.normal(0, 1, (19, 2)) * np.array([60.0, 150.0])).astype(np.float32)
    hand = (np.array([150.0, 90.0]) + rng.normal(0, 1, (21, 2)) * np.array([35.0, 30.0])).astype(np.float32)
    wide = (np.array([400.0, 300.0]) + rng.normal(0, 1, (17, 2)) * np.array([220.0, 25.0])).astype(np.float32)
    return {"demo": demo + np.float32(0.25), "coco": coco, "hand": hand, "wide": wide}


def fit_cases():
    """name -> (joints3d [J, 3] fp32 metres, target [J, 2] fp32 crop pixels): a known camera plus 4 px of noise."""
    out = {}
    for name, J, seed, cam in (("j17", 17, 1, (0.9, 0.05, -0.1)), ("j19", 19, 2, (0.7, -0.2, 0.15)),
                               ("j21", 21, 3, (1.6, 0.1, 0.05)), ("outlier", 17, 4, (0.8, 0.0, 0.1))):
        rng = np.random.default_rng(seed)
        p = rng.normal(0, 0.3, (J, 3)).astype(np.float32)
        s, tx, ty = cam
        t = (p[:, :2].astype(np.float64) + np.array([tx, ty])) * s * (CROP / 2) + CROP / 2 + rng.normal(0, 4.0, (J, 2))
        if name == "outlier":
            t[5] += np.array([120.0, -90.0])
        out[name] = (p, t.astype(np.float32))
    p, t = out["outlier"]
    keep = np.arange(17) != 5
    out["outlier_w0"] = (p[keep], t[keep])           # the fourth case without its outlier joint (the weight test)
    return out


def reference_prep(ns, joints):
    """The reference's own functions in the order demo/run.py:150-159 calls them."""
    au, cu = ns.aug_utils, ns.coord_utils
    H, W = ns_cfg.MODEL.input_shape
    px = joints.astype(np.float64)
    tight = cu.get_bbox(px)
    boxes = {"bbox1": cu.process_bbox(tight.copy(), aspect_ratio=1.0, scale=1.25), "bbox2": cu.process_bbox(tight.copy())}
    in_crop = au.j2d_processing(px.copy(), (CROP, CROP), boxes["bbox1"], 0, 0, None)[0][:, :2]
    in_net = au.j2d_processing(px.copy(), (W, H), boxes["bbox2"], 0, 0, None)[0][:, :2] / np.array([[W, H]])
    z = (in_net - in_net.mean(axis=0)) / in_net.std(axis=0)
    return dict(tight=tight, target=in_crop, pose2d=z, **boxes)


RATE_AFTER = {500: 0.05, 1000: 0.001}        # run.py:184-189: the rate that holds AFTER the iteration with this index


def reference_fit(project_net, joints3d, target, start, iterations=1500):
    """The reference's OptimzeCamLayer under torch's L1Loss and Adam (lr 0.1), `iterations` times; `start` replaces the
    module's own torch.rand((1, 3))."""
    import torch
    layer = project_net.get_model(CROP)
    with torch.no_grad():
        layer.cam_param.copy_(torch.from_numpy(start.reshape(1, 3)))
    x, t = torch.from_numpy(joints3d[None]), torch.from_numpy(target[None])
    l1 = torch.nn.L1Loss()
    adam = torch.optim.Adam(layer.parameters(), lr=0.1)
    layer.train()
    for it in range(iterations):
        adam.zero_grad()
        l1(layer(x), t).backward()
        adam.step()
        if it in RATE_AFTER:
            for group in adam.param_groups:
                group["lr"] = RATE_AFTER[it]
    return layer.cam_param[0].detach().numpy().copy()


def _fit_all(args):
    """One case from all starts (a worker process: the reference is loaded there)."""
    import torch
    torch.set_num_threads(1)
    p, t, starts = args
    ref_loader.load()
    from models import project_net
    return np.stack([reference_fit(project_net, p, t, s) for s in starts]).astype(np.float32)


def main():
    global ns_cfg
    import torch
    torch.set_num_threads(1)
    base = ref_loader.load()
    ns_cfg = base.cfg
    aug = ref_loader.load_aug()
    from models import project_net
    out = {}
    for name, joints in prep_poses().items():
        rec = reference_prep(aug, joints)
        out[f"prep_{name}_joints"] = joints
        for k, v in rec.items():
            out[f"prep_{name}_{k}"] = np.asarray(v)
        print("prep", name, "bbox1", rec["bbox1"], "bbox2", rec["bbox2"], flush=True)
    cases = fit_cases()
    starts = []
    for k in range(N_STARTS):
        torch.manual_seed(k)
        starts.append(torch.rand((1, 3))[0].numpy().copy())
    starts = np.stack(starts).astype(np.float32)
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max_workers=len(cases)) as ex:
        all_cams = dict(zip(cases, ex.map(_fit_all, [(p, t, starts) for p, t in cases.values()])))
    for name, (p, t) in cases.items():
        cams = all_cams[name]
        S = len(starts)
        losses = camfit_ref.loss64(cams, np.repeat(p[None], S, 0), np.repeat(t[None], S, 0), None, CROP / 2)
        ocam, oloss = camfit_ref.l1_optimum(p, t, None, CROP / 2)
        out.update({f"fit_{name}_joints3d": p, f"fit_{name}_target": t, f"fit_{name}_starts": starts, f"fit_{name}_cams": cams,
                    f"fit_{name}_losses": losses, f"fit_{name}_opt_cam": ocam, f"fit_{name}_opt_loss": np.float64(oloss)})
        med = np.median(cams, 0)
        print("fit", name, "optimum", ocam, oloss, "max excess loss", (losses - oloss).max(), "max |cam - median|",
              np.abs(cams - med).max(0), flush=True)
    # the schedule pin: a start of case j17 whose float64 run meets no residual within the band in 502 steps
    p, t = cases["j17"]
    rng = np.random.default_rng(7)
    cand = rng.uniform(0, 1, (4096, 3)).astype(np.float32)
    _, _, mar = camfit_ref.fit(np.repeat(p[None], len(cand), 0), np.repeat(t[None], len(cand), 0), None, cand, steps=502,
                               img_res=CROP / 2)
    good = np.flatnonzero(mar > BAND)
    assert len(good), "no start keeps every residual out of the band for 502 steps: record more candidates"
    best = int(np.argmax(mar))                     # the widest margin of the candidates
    s0 = cand[best]
    out["sched_start"] = s0
    out["sched_cam3"] = reference_fit(project_net, p, t, s0, 3).astype(np.float32)
    out["sched_cam502"] = reference_fit(project_net, p, t, s0, 502).astype(np.float32)
    print("sched start", s0, "min |residual|", mar[best], "of", len(good), "candidates", flush=True)
    path = os.path.join(HERE, "camfit_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
