#!/usr/bin/env python3
"""Generates tests/golden/video_ref.npz by running the REAL reference on the CPU: smooth_pose (lib/smooth_utils.py, imported
by path: it needs only numpy) and compute_error_accel / rigid_align (lib/coord_utils.py, through
oracle/ref_loader.load_aug()).  Run where the reference tree exists (the GPU box has none):
    python tests/golden/make_golden_video.py

Inputs are drawn from numpy PCG64 and stored as float32: joints of 14 x 3 at mm scale, a smooth motion plus jitter, every
joint set with positive variance (no frame is degenerate for the alignment).

  filter   flt_x [237, 14, 3] float32, flt_seq_ptr (sequences of 40, 77 and 120 frames), flt_params [4, 2] = (min_cutoff,
           beta) and flt_y<k> [237, 14, 3] float32: smooth_pose of each sequence on the float32 input (the reference then
           computes in float32)
  loop     a dataset of 130 frames in two videos, given as the boolean masks of data/PW3D/dataset.py:160-163: video 0 owns
           positions 0-49 and 90-129 (two runs, as a two-person video has after the sort by person_id), video 1 owns 50-89.
           ev_pred, ev_gt [130, 14, 3] float32 in dataset order, ev_masks [2, 130] bool.  The reference's loop of
           dataset.py:391-414 (smooth_pose(0.004, 0.005) on the float32 prediction; the metrics on the float64 casts of its
           float32 output and of the ground truth): ev_smoothed [130, 14, 3] float32 in video order, ev_accel_error,
           ev_mpjpe_list, ev_pa_mpjpe (its three totals' ingredients: per-video accel means, per-video MPJPE means, the
           pooled per-frame PA rows [130, 14]) and ev_totals = (accel error, MPJPE, PA-MPJPE)
  accel    compute_error_accel(gt, pred) and compute_error_accel(gt, pred, vis) on video 1 of the loop (raw float32
           prediction, float64 casts): acc_plain [38], acc_vis_mask [40] bool (gaps), acc_vis [k]
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_loader  # noqa: E402

PARAMS = ((0.004, 0.7), (0.004, 0.005), (1.0, 0.0), (0.05, 3.0))


def load_smooth():
    spec = importlib.util.spec_from_file_location("smooth_utils", os.path.join(ref_loader.REF_ROOT, "lib", "smooth_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def motion(rng, T, J=14):
    """A skeleton (joints spread over ~1 m) moving smoothly, mm."""
    base = rng.standard_normal((J, 3)) * rng.uniform(150, 350, 3)
    t = np.arange(T)[:, None, None]
    sway = 80.0 * np.sin(2 * np.pi * t / rng.uniform(20, 60, (1, J, 3)) + rng.uniform(0, 6, (1, J, 3)))
    drift = np.cumsum(rng.standard_normal((T, 1, 3)) * 4.0, axis=0)
    return base[None] + sway + drift


def main():
    rng = np.random.default_rng(20240)
    sm = load_smooth()
    cu = ref_loader.load_aug().coord_utils
    out = {}
    # -- filter
    lens = (40, 77, 120)
    x = np.concatenate([motion(rng, T) + rng.standard_normal((T, 14, 3)) * 12.0 for T in lens]).astype(np.float32)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    out["flt_x"], out["flt_seq_ptr"], out["flt_params"] = x, ptr, np.asarray(PARAMS, np.float64)
    for k, (mc, b) in enumerate(PARAMS):
        y = np.concatenate([sm.smooth_pose(x[ptr[s]:ptr[s + 1]], min_cutoff=mc, beta=b) for s in range(len(lens))])
        assert y.dtype == np.float32
        out[f"flt_y{k}"] = y
    # -- the evaluation loop
    n = 130
    masks = np.zeros((2, n), bool)
    masks[0, :50] = masks[0, 90:] = True
    masks[1, 50:90] = True
    gt = np.empty((n, 14, 3))
    gt[masks[0]] = motion(rng, 90)
    gt[masks[1]] = motion(rng, 40)
    pred = gt + rng.standard_normal(gt.shape) * 25.0 + rng.standard_normal((n, 1, 3)) * 10.0
    gt, pred = gt.astype(np.float32), pred.astype(np.float32)
    assert (gt.var(axis=1).sum(axis=1) > 1.0).all() and (pred.var(axis=1).sum(axis=1) > 1.0).all()
    out["ev_pred"], out["ev_gt"], out["ev_masks"] = pred, gt, masks
    accel_error, mpjpe_list, pa_list, smoothed = [], [], [], []
    for vid_idx in masks:                                            # dataset.py:391-403
        p32, g = pred[vid_idx], gt[vid_idx].astype(np.float64)
        p32 = sm.smooth_pose(p32, min_cutoff=0.004, beta=0.005)
        assert p32.dtype == np.float32
        smoothed.append(p32)
        p = p32.astype(np.float64)
        accel_error.append(np.mean(cu.compute_error_accel(g, p)))
        mpjpe_list.append(np.mean(np.sqrt(np.sum((p - g) ** 2, 2))))
        for idx in range(len(p)):
            pa_pred = cu.rigid_align(p[idx], g[idx])
            pa_list.append(np.sqrt(np.sum((pa_pred - g[idx]) ** 2, 1)))
    out["ev_smoothed"] = np.concatenate(smoothed)
    out["ev_accel_error"], out["ev_mpjpe_list"], out["ev_pa_mpjpe"] = map(np.asarray, (accel_error, mpjpe_list, pa_list))
    out["ev_totals"] = np.array([np.mean(accel_error), np.mean(mpjpe_list), np.mean(pa_list)])
    # -- compute_error_accel alone
    g, p = gt[masks[1]].astype(np.float64), pred[masks[1]].astype(np.float64)
    vis = np.ones(40, bool)
    vis[[0, 7, 8, 20, 33, 39]] = False
    out["acc_plain"] = cu.compute_error_accel(g, p)
    out["acc_vis_mask"] = vis
    out["acc_vis"] = cu.compute_error_accel(g, p, vis)
    path = os.path.join(HERE, "video_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
