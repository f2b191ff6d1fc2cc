"""Fixture maker for the sample-noise tests: records what the REAL reference computes (run on a machine that has the
reference checkout; P2M_REFERENCE_ROOT, default as in oracle/ref_loader.py).  Data only.

  sample_noise_ref.npz   for each pose of sample_cases.histogram_poses(): the histogram of N_DRAWS draws of the reference's
                         synthesize_pose(joints, area, num_overlap=0) (lib/noise_utils.py:17-285) - per joint, the displacement
                         from the ground truth over 24 radial bins (sample_ref.displacement_histogram) x 8 octants, and the
                         count of zeroed joints.  Counts, not draws.

  sample_chain.npz       for the samples of sample_cases.chain_fixture_cases(): what the reference's own functions give for the
                         deterministic chain of data/AMASS/dataset.py:263-292 - cam2pixel, get_bbox, process_bbox,
                         j2d_processing (with its trans: the area of :315-320), flip_2d_joint, j3d_processing and the
                         standardisation - from the float64 joints this script regresses from the case's point cloud.

    python tests/golden/make_golden_sample.py [chain | noise]
"""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_loader  # noqa: E402
import sample_cases  # noqa: E402
import sample_ref  # noqa: E402

N_DRAWS = 4000


def load_noise_utils():
    """lib/noise_utils.py imports easydict, which is not installed here: a dict with attribute access stands in."""
    if "easydict" not in sys.modules:
        class EasyDict(dict):
            __getattr__ = dict.__getitem__
            __setattr__ = dict.__setitem__
        mod = types.ModuleType("easydict")
        mod.EasyDict = EasyDict
        sys.modules["easydict"] = mod
    lib = os.path.join(ref_loader.REF_ROOT, "lib")
    if lib not in sys.path:
        sys.path.insert(0, lib)
    import noise_utils
    return noise_utils


def one_pose(args):
    name, joints, area, seed = args
    nu = load_noise_utils()
    np.random.seed(seed)
    random.seed(seed)
    draws = np.stack([nu.synthesize_pose(joints.astype(np.float64), float(area), num_overlap=0) for _ in range(N_DRAWS)])
    hist, zeroed = sample_ref.displacement_histogram(draws, joints, float(area), np.asarray(nu.cfg.kps_sigmas))
    return name, hist, zeroed


def chain_fixture():
    ns = ref_loader.load_aug()
    au, cu = ns.aug_utils, ns.coord_utils
    out = {}
    for name, c in sample_cases.chain_fixture_cases().items():
        W, H, pairs = c["W"], c["H"], [list(p) for p in c["flip_pairs"]]
        rec = {k: [] for k in ("joint_cam", "img", "tight", "bbox", "px", "area", "flipped", "lift", "pose2d")}
        for i in range(len(c["verts"])):
            mesh = (c["verts"][i].astype(np.float64) + c["trans"][i].astype(np.float64)) * c["mesh_scale"]
            if c["in_R"] is None:
                cam = c["reg_R"].astype(np.float64) @ mesh
            else:
                cam = c["in_R"].astype(np.float64) @ mesh
                cam = np.concatenate([cam] + [((cam[a] + cam[b]) * 0.5)[None] for a, b in c["midpoints"]])
            img = cu.cam2pixel(cam / 1000, c["focal"][i], c["princpt"][i])
            img[:, 2] = 1
            rel = cam - cam[c["input_root"]][None]
            tight = cu.get_bbox(img)
            bbox = cu.process_bbox(tight.copy(), aspect_ratio=W / H)
            rot, flip = float(c["rot"][i]), int(c["flip"][i])
            px, trans = au.j2d_processing(img.copy(), (W, H), bbox, rot, 0, None)
            x0, y0, x1, y1 = tight[0], tight[1], tight[0] + tight[2], tight[1] + tight[3]
            p1, p2, p3 = (au.affine_transform(np.array(q), trans) for q in ([x0, y0], [x1, y0], [x1, y1]))
            area = np.sqrt(((p2 - p1) ** 2).sum()) * np.sqrt(((p3 - p2) ** 2).sum())
            fl = au.flip_2d_joint(px.copy(), W, pairs) if flip else px.copy()
            lift = au.j3d_processing(rel.copy(), rot, flip, pairs)
            p = fl[:, :2] / np.array([[W, H]])
            p = (p - np.mean(p, axis=0)) / np.std(p, axis=0)
            for k, v in zip(rec, (cam, img[:, :2], tight, bbox, px[:, :2], area, fl[:, :2], lift, p)):
                rec[k].append(np.asarray(v, np.float64))
        for k, v in rec.items():
            out[f"{name}_{k}"] = np.stack(v)
    path = os.path.join(HERE, "sample_chain.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def main():
    if "noise" not in sys.argv[1:]:
        chain_fixture()
    if "chain" in sys.argv[1:]:
        return
    from concurrent.futures import ProcessPoolExecutor
    poses = sample_cases.histogram_poses()
    jobs = [(n, j, a, 1000 + i) for i, (n, (j, a)) in enumerate(poses.items())]
    out = {"n_draws": np.int64(N_DRAWS)}
    with ProcessPoolExecutor(max_workers=len(jobs)) as ex:
        for name, hist, zeroed in ex.map(one_pose, jobs):
            out[name + "_hist"], out[name + "_zeroed"] = hist.astype(np.int32), zeroed.astype(np.int32)
            out[name + "_joints"], out[name + "_area"] = poses[name][0], np.float64(poses[name][1])
            print(name, "draws", N_DRAWS, "zeroed", zeroed.tolist(), flush=True)
    path = os.path.join(HERE, "sample_noise_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
