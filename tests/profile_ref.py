"""Float64 restatement of the error-profile definition of include/p2m.h (p2m_error_profile), the yardstick of
pose2mesh_release_amd.evaluate.ErrorProfile.  Neither the reference tree nor the FreiHAND server code is here, so this file,
written from the definition, pins it:

  per sample, P prediction and G ground truth [N, 3] (G read times gt_scale), all in float64:
    root    both sets minus their own point `root`
    align   P similarity-aligned onto G over the valid points (eval_ref.rigid_transform_3D, numpy's SVD)
    e_i   = sqrt(dx dx + dy dy + dz dz), d = P_i - G_i, the sum taken left to right
    bin_i = #{k: t[k] < e_i} = the first k with e_i <= t[k], K if there is none (non-strict); NaN goes to bin K
  per sample: the histogram of the bins over the valid points, and the sum of e in THE KERNEL'S ORDER (sample_sum below):
  that order is part of the contract, since the unaligned sums are compared bit for bit;
  running totals per group (row 0: overall) and per point, added to in sample order starting from the value found there;
  the derived figures: mean = sum / count, pck[k] = cumsum(hist)[k] / count,
    auc = sum_k (pck[k] + pck[k + 1]) / 2 * (t[k + 1] - t[k]) / (t[K - 1] - t[0]),
    auc_points = the mean of the per-point auc over the points with count > 0.

The unaligned path has no tolerance: float64 subtraction, products, sums in a fixed order and a correctly rounded square root
are the same on both sides.  The aligned path inherits the project's alignment tolerance (fscore_ref.ALIGN_REL per coordinate
of the largest centroid-centred |coordinate| Mc of the sets that enter the alignment - the device solves Horn's quaternion by
Jacobi, numpy the SVD, both on the centroid-centred sets): delta = sqrt(3) ALIGN_REL Mc on a distance, see align_delta."""
import numpy as np

import eval_ref
import fscore_ref

NT = 256                              # lanes of the per-sample block


# ---- the definition --------------------------------------------------------------------------------------------------------
def errors(pred, gt, valid=None, gt_scale=1.0, root=None, align=False):
    """(e [B, N] float64 with 0 where a point is not valid, on [B, N] bool)."""
    P = np.asarray(pred, np.float32).astype(np.float64)
    G = np.asarray(gt, np.float32).astype(np.float64) * np.float64(np.float32(gt_scale))
    on = np.ones(P.shape[:2], bool) if valid is None else np.asarray(valid) != 0
    e = np.zeros(P.shape[:2])
    for b in range(P.shape[0]):
        p, g, m = P[b], G[b], on[b]
        if root is not None:
            p, g = p - p[root], g - g[root]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if align and m.any():
                try:
                    c, R, t = eval_ref.rigid_transform_3D(p[m], g[m])
                    p = (c * R @ p.T).T + t
                except np.linalg.LinAlgError:                    # non-finite input: no transform, no finite error
                    p = np.full_like(p, np.nan)
            d = p - g
            eb = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        e[b] = np.where(m, eb, 0.0)
    return e, on


def bins(e, on, t, strict=False):
    """bin per point (int64, -1 where not valid).  strict=True plants the fault of an implementation that compares with <:
    the first k with e < t[k]."""
    k = np.searchsorted(np.asarray(t, np.float64), e, side="right" if strict else "left")
    return np.where(on, k, -1).astype(np.int64)


def sample_sum(e_row):
    """The sum of one sample's errors in the kernel's order: lane l of 256 adds its points l, l + 256, ... in ascending
    order, the 64 lanes of a wave by the xor butterfly (32, 16, 8, 4, 2, 1), then the four wave totals in wave order."""
    n = e_row.shape[0]
    rows = np.zeros(((n + NT - 1) // NT) * NT)
    rows[:n] = e_row
    lane = np.zeros(NT)
    for r in rows.reshape(-1, NT):
        lane = lane + r
    w = lane.reshape(NT // 64, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w[:, :o] + w[:, o:2 * o]
    s = w[0, 0]
    for i in range(1, NT // 64):
        s = s + w[i, 0]
    return s


def evaluate(pred, gt, t, valid=None, gt_scale=1.0, root=None, align=False, B_real=None, strict=False):
    """A call's per-sample results: error [B, N], bins [B, N] (-1: not counted), sample_sum, sample_mean [B], sample_count
    [B], sample_pck [B, K + 1].  Rows >= B_real are padding: zeros, never read, bins -1."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    B, N = pred.shape[:2]
    B_real = B if B_real is None else B_real
    K = len(t)
    out = {"error": np.zeros((B, N)), "bins": np.full((B, N), -1, np.int64), "sample_sum": np.zeros(B),
           "sample_mean": np.zeros(B), "sample_count": np.zeros(B, np.int64), "sample_pck": np.zeros((B, K + 1), np.int64)}
    e, on = errors(pred[:B_real], gt[:B_real], None if valid is None else np.asarray(valid)[:B_real], gt_scale, root, align)
    out["error"][:B_real] = e
    out["bins"][:B_real] = bins(e, on, t, strict)
    for b in range(B_real):
        with np.errstate(invalid="ignore", divide="ignore"):
            out["sample_sum"][b] = sample_sum(e[b])
            out["sample_count"][b] = on[b].sum()
            out["sample_mean"][b] = out["sample_sum"][b] / np.float64(out["sample_count"][b])
        out["sample_pck"][b] = np.bincount(out["bins"][b][on[b]], minlength=K + 1)
    return out


# ---- running totals ----------------------------------------------------------------------------------------------------------
def new_state(N, K, n_groups=32, per_point=True):
    s = {"group_sum": np.zeros(n_groups + 1), "group_count": np.zeros(n_groups + 1, np.int64),
         "group_hist": np.zeros((n_groups + 1, K + 1), np.int64)}
    if per_point:
        s.update(point_sum=np.zeros(N), point_count=np.zeros(N, np.int64), point_hist=np.zeros((N, K + 1), np.int64))
    return s


def accumulate(state, res, B_real=None, group=None):
    """Adds a call's results (evaluate) to the totals, in sample order."""
    B = res["error"].shape[0]
    B_real = B if B_real is None else B_real
    n_groups = state["group_sum"].shape[0] - 1
    for r in range(n_groups + 1):
        for b in range(B_real):
            if r > 0 and (group is None or int(group[b]) != r - 1):
                continue
            with np.errstate(invalid="ignore"):
                state["group_sum"][r] = state["group_sum"][r] + res["sample_sum"][b]
            state["group_count"][r] += res["sample_count"][b]
            state["group_hist"][r] += res["sample_pck"][b]
    if "point_sum" in state:
        idx = np.arange(res["error"].shape[1])
        for b in range(B_real):
            m = res["bins"][b] >= 0
            with np.errstate(invalid="ignore"):
                state["point_sum"][m] = state["point_sum"][m] + res["error"][b][m]
            state["point_count"][m] += 1
            np.add.at(state["point_hist"], (idx[m], res["bins"][b][m]), 1)
    return state


def curves(total, count, hist, t):
    """mean, pck [..., K], auc of totals (module docstring)."""
    t = np.asarray(t, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.asarray(count).astype(np.float64)
        mean = np.asarray(total, np.float64) / n
        pck = np.ascontiguousarray(np.cumsum(np.ascontiguousarray(hist), axis=-1)[..., :-1] / n[..., None])
        auc = np.sum((pck[..., :-1] + pck[..., 1:]) / 2 * np.diff(t), axis=-1) / (t[-1] - t[0])
    return mean, pck, auc


def summary(state, t):
    """What ErrorProfile.summary() returns, from a state."""
    t = np.asarray(t, np.float64)
    mean, pck, auc = curves(state["group_sum"], state["group_count"], state["group_hist"], t)

    def row(r):
        return {"count": int(state["group_count"][r]), "mean": float(mean[r]), "pck": pck[r], "auc": float(auc[r])}
    out = dict(row(0), thresholds=t)
    groups = {g: row(g + 1) for g in range(len(mean) - 1) if state["group_count"][g + 1] > 0}
    if groups:
        out["groups"] = groups
    if "point_sum" in state:
        pm, pp, pa = curves(state["point_sum"], state["point_count"], state["point_hist"], t)
        out["points"] = {"count": state["point_count"], "mean": pm, "pck": pp, "auc": pa}
        seen = state["point_count"] > 0
        out["auc_points"] = float(np.mean(pa[seen])) if seen.any() else float("nan")
    return out


def pck_direct(e, on, t):
    """The PCK curve without a histogram: the share of the valid errors with e <= t[k]."""
    v = np.asarray(e)[np.asarray(on)]
    return np.array([np.mean(v <= tk) for tk in np.asarray(t, np.float64)])


# ---- the aligned path's tolerance ------------------------------------------------------------------------------------------------
def align_delta(pred, gt, valid=None, gt_scale=1.0):
    """delta [B] = sqrt(3) ALIGN_REL Mc: Mc is the largest |coordinate| of the two sets of a sample about their own centroids
    over the valid points - the sets the alignment is solved on (subtracting `root` from a set does not change them)."""
    P = np.asarray(pred, np.float32).astype(np.float64)
    G = np.asarray(gt, np.float32).astype(np.float64) * np.float64(np.float32(gt_scale))
    on = np.ones(P.shape[:2], bool) if valid is None else np.asarray(valid) != 0
    out = np.zeros(P.shape[0])
    for b in range(P.shape[0]):
        p, g = P[b][on[b]], G[b][on[b]]
        Mc = max(np.abs(p - p.mean(0)).max(), np.abs(g - g.mean(0)).max())
        out[b] = np.sqrt(3.0) * fscore_ref.ALIGN_REL * Mc
    return out


def count_bounds(e_ref, on, t, delta):
    """(lo, hi) [K] of one sample: every cumulative count of an implementation whose errors are within delta of e_ref lies
    in [#(e_ref < t[k] - delta), #(e_ref <= t[k] + delta)]."""
    v = np.asarray(e_ref)[np.asarray(on)]
    t = np.asarray(t, np.float64)
    return np.array([(v < tk - delta).sum() for tk in t]), np.array([(v <= tk + delta).sum() for tk in t])
