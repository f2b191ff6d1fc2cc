"""TEST INFRASTRUCTURE ONLY - the yardstick of the camera kernels: include/p2m.h, "The demo's camera", restated in numpy.

  prepare(joints, ...)          p2m_pose_prepare: float64 (or the kernel's fp32 operation sequence)
  start(seed, first_index, S)   the stage-10 start values of the Philox stream
  fit(...)                      p2m_camera_fit: float64, or fp32 with the header's butterfly sums (order=None) or with the
                                joints summed sequentially in an arbitrary order (order = a permutation of range(J));
                                returns (cam, loss, min_abs_residual)
  loss64 / residuals64          the float64 objective and its residuals at a given camera
  l1_optimum                    the exact minimum of the objective: a linear program in a = s r, bx = s tx r, by = s ty r

Why two kinds of check: the objective is piecewise linear, its gradient a sum of signs.  While no
residual comes near zero, every arithmetic computes the same signs and the trajectories agree to rounding; the first residual
that crosses zero a step earlier in one arithmetic than in another separates them for good.  So short runs whose
min_abs_residual stays above a band are compared step-exactly, full runs through the objective value they reach.
"""
import numpy as np

import sample_ref

ST_CAM_START = 10
DEFAULT_SCHEDULE = ((0, 0.1), (501, 0.05), (1001, 0.001))


# ---- preparation ------------------------------------------------------------------------------------------------------------
def prepare(joints, in_W=288.0, in_H=384.0, crop=500.0, dtype=np.float64):
    """joints [S, J, 2] -> dict(pose2d, target [S, J, 2], bbox [S, 4], status [S], bbox2 [S, 4], tight [S, 4])."""
    dt = dtype
    j = np.asarray(joints, np.float32).astype(dt)
    S, J = j.shape[:2]
    in_W, in_H, crop = dt(in_W), dt(in_H), dt(crop)
    with np.errstate(all="ignore"):
        x0, y0 = j[:, :, 0].min(1), j[:, :, 1].min(1)
        tw, th = j[:, :, 0].max(1) - x0, j[:, :, 1].max(1) - y0
        w, h = tw - dt(1), th - dt(1)
        ok = np.isfinite(j).all(axis=(1, 2)) & (tw * th > 0) & (w >= 0) & (h >= 0)
        cx, cy = x0 + w / dt(2), y0 + h / dt(2)
        aspect = in_W / in_H
        w2, h2 = w.copy(), h.copy()
        a, b = w2 > aspect * h2, w2 < aspect * h2
        h2 = np.where(a, w2 / aspect, h2)
        w2 = np.where(b & ~a, h2 * aspect, w2)
        side = np.maximum(w, h)
        w1 = h1 = side * dt(1.25)
        ok &= (w2 > 0) & (w1 > 0)
        s2, s1 = in_W / w2, crop / w1
        dx, dy = j[:, :, 0] - cx[:, None], j[:, :, 1] - cy[:, None]
        target = np.stack([s1[:, None] * dx + crop / dt(2), s1[:, None] * dy + crop / dt(2)], 2)
        p = np.stack([(s2[:, None] * dx + in_W / dt(2)) / in_W, (s2[:, None] * dy + in_H / dt(2)) / in_H], 2)
        p[~ok] = 0
        if dt == np.float32:
            mean = np.stack([_butterfly(p[:, :, c]) for c in range(2)], 1) / dt(J)
            e = p - mean[:, None]
            sd = np.sqrt(np.stack([_butterfly(e[:, :, c] * e[:, :, c]) for c in range(2)], 1) / dt(J))
        else:
            e = p - p.mean(1, keepdims=True)
            sd = np.sqrt((e * e).mean(1))
        ok &= (sd > 0).all(1) & np.isfinite(sd).all(1)
        pose2d = e / sd[:, None]
        bbox = np.stack([cx - w1 / dt(2), cy - h1 / dt(2), w1, h1], 1)
        bbox2 = np.stack([cx - w2 / dt(2), cy - h2 / dt(2), w2, h2], 1)
    for arr in (pose2d, target, bbox):
        arr[~ok] = 0
    return dict(pose2d=pose2d, target=target, bbox=bbox, status=(~ok).astype(np.int32), bbox2=bbox2,
                tight=np.stack([x0, y0, tw, th], 1))


# ---- the start ----------------------------------------------------------------------------------------------------------------
def start(seed, first_index, S):
    """[S, 3] float64: (s, tx, ty) = words 0, 1, 2 of stage 10, joint 0, block 0 at the global indices first_index + b."""
    index = (np.uint64(first_index) + np.arange(S, dtype=np.uint64))
    w = sample_ref._words(seed, index, 0, ST_CAM_START, np.zeros(1, np.uint64))
    return np.stack([sample_ref.uniforms(w[k][:, 0]) for k in range(3)], 1)


# ---- the fit --------------------------------------------------------------------------------------------------------------------
def _butterfly(v):
    """The header's sum over 64 lanes: v [S, J] fp32 -> [S]; lanes >= J hold +0."""
    S, J = v.shape
    a = np.zeros((S, 64), v.dtype)
    a[:, :J] = v
    n = 64
    # v1[l] = v[l] + v[l ^ 1] .. : lane 0's value is the balanced tree over adjacent pairs
    while n > 1:
        a = a[:, 0:n:2] + a[:, 1:n:2]
        n //= 2
    return a[:, 0]


def _sum(v, dtype, order):
    if dtype == np.float64:
        return v.sum(1)
    if order is None:
        return _butterfly(v)
    acc = np.zeros(v.shape[0], v.dtype)
    for j in order:
        acc = acc + v[:, j]
    return acc


def fit(joints3d, target, weight=None, cam0=None, steps=1500, schedule=DEFAULT_SCHEDULE, img_res=250.0, betas=(0.9, 0.999),
        eps=1e-8, dtype=np.float64, order=None, trace=None):
    """p2m_camera_fit for S samples: joints3d [S, J, 3], target [S, J, 2], weight [S, J] or None, cam0 [S, 3].  Returns
    (cam [S, 3], loss [S], min_abs_residual [S]): the last the smallest |pred - t| over the joints of positive weight met in
    any step's gradient evaluation (inf for steps = 0).  dtype float64: everything in float64, the per-step corrections
    unrounded.  dtype float32: the header's operation sequence.  trace: a list that receives (cam, loss, min_abs_residual) of
    the start and after every step - entry n is what a run of n steps returns."""
    dt = dtype
    x = np.asarray(joints3d, np.float32)[:, :, 0].astype(dt)
    y = np.asarray(joints3d, np.float32)[:, :, 1].astype(dt)
    t = np.asarray(target, np.float32).astype(dt)
    S, J = x.shape
    w = np.ones((S, J), dt) if weight is None else np.asarray(weight, np.float32).astype(dt)
    cam = np.asarray(cam0, np.float32).astype(dt).reshape(S, 3).copy()
    r = dt(np.float32(img_res))
    W = _sum(w, dt, order)
    c = (w / (dt(2) * W)[:, None]) * r
    b1, b2 = float(betas[0]), float(betas[1])
    om1, b2f, om2, epsf = dt(1.0 - b1), dt(b2), dt(1.0 - b2), dt(eps)
    m, v = np.zeros((S, 3), dt), np.zeros((S, 3), dt)
    p1 = p2 = 1.0
    k, lr = 0, float(schedule[0][1])
    mar = np.full(S, np.inf)
    live = w > 0

    def objective(cam):
        s, tx, ty = cam[:, 0:1], cam[:, 1:2], cam[:, 2:3]
        ex, ey = (((x + tx) * s) * r + r) - t[:, :, 0], (((y + ty) * s) * r + r) - t[:, :, 1]
        return _sum(w * (np.abs(ex) + np.abs(ey)), dt, order) / (dt(2) * W)

    if trace is not None:
        trace.append((cam.copy(), objective(cam), mar.copy()))
    for i in range(int(steps)):
        if k + 1 < len(schedule) and schedule[k + 1][0] <= i:
            k += 1
            lr = float(schedule[k][1])
        p1 *= b1
        p2 *= b2
        step_size, c2 = dt(lr / (1.0 - p1)), dt(np.sqrt(1.0 - p2))
        s, tx, ty = cam[:, 0:1], cam[:, 1:2], cam[:, 2:3]
        qx, qy = x + tx, y + ty
        ex, ey = ((qx * s) * r + r) - t[:, :, 0], ((qy * s) * r + r) - t[:, :, 1]
        mar = np.minimum(mar, np.where(live, np.minimum(np.abs(ex), np.abs(ey)), np.inf).min(1))
        gx, gy = np.sign(ex) * c, np.sign(ey) * c
        g = np.stack([_sum(gx * qx + gy * qy, dt, order), _sum(gx * s, dt, order), _sum(gy * s, dt, order)], 1)
        m = m + (g - m) * om1
        v = v * b2f + (om2 * g) * g
        cam = cam - (step_size * m) / (np.sqrt(v) / c2 + epsf)
        if trace is not None:
            trace.append((cam.copy(), objective(cam), mar.copy()))
    return cam, objective(cam), mar


def residuals64(cam, joints3d, target, img_res=250.0):
    """pred - target [S, J, 2] in float64 at cam [S, 3]."""
    cam = np.asarray(cam, np.float64).reshape(-1, 3)
    p = np.asarray(joints3d, np.float32).astype(np.float64)[:, :, :2]
    r = float(np.float32(img_res))
    pred = ((p + cam[:, None, 1:3]) * cam[:, None, 0:1]) * r + r
    return pred - np.asarray(target, np.float32).astype(np.float64)


def loss64(cam, joints3d, target, weight=None, img_res=250.0):
    """The objective [S] in float64 at cam [S, 3]."""
    e = np.abs(residuals64(cam, joints3d, target, img_res)).sum(2)
    w = np.ones(e.shape) if weight is None else np.asarray(weight, np.float32).astype(np.float64)
    return (w * e).sum(1) / (2.0 * w.sum(1))


def l1_optimum(joints3d, target, weight=None, img_res=250.0):
    """One sample: joints3d [J, 3], target [J, 2], weight [J] or None -> (cam [3], loss): the exact minimum of the objective.
    pred_x = a x + bx + r with a = s r, bx = s tx r: minimise sum_j w_j (u_jx + u_jy) / (2 W) over (a, bx, by, u) subject to
    u >= +-(a x_j + bx + r - t_jx) (and likewise y): a linear program."""
    from scipy.optimize import linprog
    p = np.asarray(joints3d, np.float32).astype(np.float64)
    t = np.asarray(target, np.float32).astype(np.float64)
    J = p.shape[0]
    w = np.ones(J) if weight is None else np.asarray(weight, np.float32).astype(np.float64)
    r = float(np.float32(img_res))
    n = 3 + 2 * J
    cost = np.zeros(n)
    cost[3:3 + J] = cost[3 + J:] = w / (2.0 * w.sum())
    A, ub = [], []
    for axis in range(2):
        for j in range(J):
            for sg in (1.0, -1.0):
                row = np.zeros(n)
                row[0], row[1 + axis], row[3 + axis * J + j] = sg * p[j, axis], sg, -1.0
                A.append(row)
                ub.append(sg * (t[j, axis] - r))
    res = linprog(cost, A_ub=np.asarray(A), b_ub=np.asarray(ub), bounds=[(None, None)] * 3 + [(0, None)] * (2 * J),
                  method="highs")
    assert res.status == 0, res.message
    a, bx, by = res.x[:3]
    cam = np.array([a / r, bx / a, by / a])
    return cam, float(loss64(cam[None], p[None], t[None], None if weight is None else w[None], img_res)[0])
