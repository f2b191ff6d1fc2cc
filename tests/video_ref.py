"""Numpy restatements of pose2mesh_release_amd.video, written from the formulas (not imported from the reference):

  one_euro, one_euro_seqs      the One-Euro filter of lib/smooth_utils.py as include/p2m.h defines p2m_one_euro: op by op in
                               np.float32, every operation rounded once.  On float32 input the reference's smooth_pose computes
                               exactly this (tests/test_video_cpu.py holds the two equal bitwise), so the GPU kernel is pinned
                               bit for bit against it.
  error_accel, video_eval      float64: compute_error_accel (lib/coord_utils.py:194-222) and the smoothed block of
                               data/PW3D/dataset.py:391-414 with p2m_video_eval's outputs and aggregation
"""
import numpy as np

import eval_ref

F = np.float32


def one_euro(x, min_cutoff, beta, d_cutoff=1.0, dt=1.0, state=None):
    """x [T, C] float32 -> (y [T, C] float32, (xp, dxp)).  state: (xp, dxp) float32 [C] to continue from, or None: the first
    frame initialises the filter."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    mc, b, te = F(min_cutoff), F(beta), F(dt)
    k2, kd = F(2.0 * np.pi), F(2.0 * np.pi * float(d_cutoff))
    one = F(1.0)
    y = np.empty_like(x)
    t0 = 0
    if state is None:
        if x.shape[0] == 0:
            return y, None
        y[0] = x[0]
        xp, dxp = x[0].copy(), np.zeros(x.shape[1], F)
        t0 = 1
    else:
        xp, dxp = np.asarray(state[0], F).copy(), np.asarray(state[1], F).copy()
    with np.errstate(all="ignore"):
        rd = kd * te
        ad = rd / (rd + one)
        for t in range(t0, x.shape[0]):
            dx = (x[t] - xp) / te
            dxh = ad * dx + (one - ad) * dxp
            cut = mc + b * np.abs(dxh)
            r = (k2 * cut) * te
            a = r / (r + one)
            yt = a * x[t] + (one - a) * xp
            assert yt.dtype == np.float32 and dxh.dtype == np.float32
            y[t] = yt
            xp, dxp = yt, dxh
    return y, (xp, dxp)


def one_euro_seqs(x, seq_ptr, min_cutoff, beta, d_cutoff=1.0, dt=1.0, rows=None):
    """The ragged batch: x [Nx, C] float32, seq_ptr [S + 1], rows [N] or None -> y [N, C] in sequence order."""
    x = np.asarray(x)
    src = x if rows is None else x[np.asarray(rows)]
    y = np.empty_like(src)
    for s in range(len(seq_ptr) - 1):
        a, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
        y[a:e] = one_euro(src[a:e], min_cutoff, beta, d_cutoff, dt)[0]
    return y


def tables(video_indices, n=None):
    """rows, seq_ptr of a list of boolean masks / index arrays over the dataset order (the evaluator's host-side step)."""
    rows, ptr = [], [0]
    for v in video_indices:
        v = np.asarray(v)
        idx = np.flatnonzero(v) if v.dtype == np.bool_ else v.astype(np.int64).reshape(-1)
        rows.append(idx)
        ptr.append(ptr[-1] + len(idx))
    return np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32), np.asarray(ptr, np.int32)


def error_accel(gt, pred, vis=None):
    """One sequence, float64: (accel [N], valid [N]); entry i is the triple (i, i + 1, i + 2), 0 / False where undefined."""
    gt, pred = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    N = gt.shape[0]
    accel, valid = np.zeros(N), np.zeros(N, bool)
    for i in range(N - 2):
        if vis is not None and not (vis[i] and vis[i + 1] and vis[i + 2]):
            continue
        ap = pred[i] - 2.0 * pred[i + 1] + pred[i + 2]
        ag = gt[i] - 2.0 * gt[i + 1] + gt[i + 2]
        accel[i] = np.sqrt(((ap - ag) ** 2).sum(axis=1)).mean()
        valid[i] = True
    return accel, valid


def video_eval(pred, gt, seq_ptr, vis=None, want_pa=True):
    """pred, gt [N, J, 3] (float32 values, taken to float64) in sequence order -> dict of float64 arrays with
    p2m_video_eval's layout: accel [N], valid [N], mpjpe [N, J], pa_mpjpe [N, J], seq_stats [S, 8], totals [8]."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    N, J = pred.shape[:2]
    S = len(seq_ptr) - 1
    accel, valid = np.zeros(N), np.zeros(N, bool)
    mpjpe = np.sqrt(((pred - gt) ** 2).sum(axis=2))
    pa = np.zeros((N, J))
    if want_pa:
        with np.errstate(all="ignore"):
            for i in range(N):
                pa[i] = np.sqrt(((eval_ref.rigid_align(pred[i], gt[i]) - gt[i]) ** 2).sum(axis=1))
    seq = np.zeros((S, 8))
    for s in range(S):
        a, e = int(seq_ptr[s]), int(seq_ptr[s + 1])
        accel[a:e], valid[a:e] = error_accel(gt[a:e], pred[a:e], None if vis is None else np.asarray(vis)[a:e])
        nv = valid[a:e].sum()
        seq[s, 0], seq[s, 1] = e - a, nv
        seq[s, 2] = accel[a:e][valid[a:e]].mean() if nv else np.nan
        seq[s, 3] = mpjpe[a:e].mean() if e > a else np.nan
        if want_pa:
            seq[s, 4], seq[s, 5] = pa[a:e].sum(), (e - a) * J
    has_acc, has_frames = seq[:, 1] > 0, seq[:, 0] > 0
    tot = np.array([seq[has_acc, 2].mean() if has_acc.any() else np.nan,
                    seq[has_frames, 3].mean() if has_frames.any() else np.nan,
                    seq[:, 4].sum() / seq[:, 5].sum() if seq[:, 5].sum() > 0 else np.nan,
                    has_acc.sum(), S - has_acc.sum(), has_frames.sum(), S - has_frames.sum(), seq[:, 0].sum()])
    return {"accel": accel, "valid": valid, "mpjpe": mpjpe, "pa_mpjpe": pa, "seq_stats": seq, "totals": tot}
