"""Float64 numpy restatement of the reference's evaluation loop bodies, one sample at a time, written from the formulas
(not imported from the reference):

  rigid_transform_3D / rigid_align                lib/coord_utils.py:127-149 (SVD of H, det < 0 fix, c = sum(s) / varP)
  compute_both_err                                data/PW3D/dataset.py:273-286
  evaluate (regress, root-align, MPJPE, MPVPE,    data/PW3D/dataset.py:322-375, data/Human36M/dataset.py:514-572
            H36M joints, PA-MPJPE; PA-MPVPE as in the commented-out PW3D lines 360-361)

This is the CPU yardstick of pose2mesh_release_amd.evaluate (tests/test_eval_cpu.py checks it against the fixtures that
tests/golden/make_golden_eval.py produced with the real reference)."""
import numpy as np

EVAL_KEYS = ("mpjpe_E", "pa_mpjpe_E", "mpjpe_A", "mpvpe", "pa_mpvpe")


def rigid_transform_3D(A, B):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    n = A.shape[0]
    cA, cB = A.mean(axis=0), B.mean(axis=0)
    H = (A - cA).T @ (B - cB) / n
    U, s, V = np.linalg.svd(H)
    R = V.T @ U.T
    if np.linalg.det(R) < 0:
        s[-1] = -s[-1]
        V[2] = -V[2]
        R = V.T @ U.T
    varP = np.var(A, axis=0).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.sum(s) / varP
    t = cB - (c * R) @ cA
    return c, R, t


def rigid_align(A, B):
    c, R, t = rigid_transform_3D(A, B)
    return (c * R @ np.asarray(A, np.float64).T).T + t


def batch_rigid(A, B):
    """[nb, N, 3] pairs -> c [nb], R [nb, 3, 3], t [nb, 3], A2 [nb, N, 3] (float64)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = [rigid_transform_3D(a, b) for a, b in zip(A, B)]
    c = np.array([o[0] for o in out])
    R = np.stack([o[1] for o in out])
    t = np.stack([o[2] for o in out])
    A2 = c[:, None, None] * np.einsum("bij,bnj->bni", R, A) + t[:, None, :]
    return c, R, t, A2


def _l2(x):
    return np.sqrt(np.sum(x ** 2, axis=-1))


def mesh_eval(pred, gt, reg_A, root_A, sub_A=None, reg_E=None, root_E=0, sub_E=None, pa_mesh=False, gt_scale=1.0,
              pred_joints_A=None, gt_joints_A=None, gt_joints_E=None):
    """Per-sample metrics of a batch ([B, nv, 3] meshes) as pose2mesh_release_amd.evaluate.MeshEvaluator defines them:
    dict of float64 arrays mpjpe_A [B, |sub_A|], mpvpe [B], and (with reg_E) mpjpe_E, pa_mpjpe_E [B, |sub_E|], (pa_mesh)
    pa_mpvpe [B]."""
    pred = np.asarray(pred, np.float64)
    gt = np.asarray(gt, np.float64) * float(gt_scale)
    B = pred.shape[0]
    res = {k: [] for k in EVAL_KEYS}
    for n in range(B):
        mo, mg = pred[n], gt[n]
        jo = np.asarray(pred_joints_A[n], np.float64) if pred_joints_A is not None else np.asarray(reg_A, np.float64) @ mo
        jg = np.asarray(gt_joints_A[n], np.float64) if gt_joints_A is not None else np.asarray(reg_A, np.float64) @ mg
        # root joint alignment (PW3D 339-344, H36M 535-538, compute_both_err 275-276)
        mo, mg = mo - jo[root_A], mg - jg[root_A]
        po, pg = jo - jo[root_A], jg - jg[root_A]
        if sub_A is not None:
            po, pg = po[list(sub_A)], pg[list(sub_A)]
        res["mpjpe_A"].append(_l2(po - pg))
        res["mpvpe"].append(_l2(mo - mg).mean())
        if pa_mesh:                                              # PW3D 360-361
            res["pa_mpvpe"].append(_l2(rigid_align(mo, mg) - mg).mean())
        if reg_E is not None:                                   # PW3D 363-372, H36M 558-567
            RE = np.asarray(reg_E, np.float64)
            eo = RE @ mo
            eg = np.asarray(gt_joints_E[n], np.float64) if gt_joints_E is not None else RE @ mg
            eo, eg = eo - eo[root_E], eg - eg[root_E]
            if sub_E is not None:
                eo, eg = eo[list(sub_E)], eg[list(sub_E)]
            res["mpjpe_E"].append(_l2(eo - eg))
            res["pa_mpjpe_E"].append(_l2(rigid_align(eo, eg) - eg))
    return {k: np.array(v) for k, v in res.items() if v}


def summary(per_sample, group=None):
    """Dataset-level means as evaluate() prints them (np.mean over every entry: with equal counts per sample, the mean of
    the per-sample means) and, with group ids, the per-group means (Human36M.evaluate's per-action table)."""
    out = {k: float(np.mean(v)) for k, v in per_sample.items()}
    out["samples"] = len(next(iter(per_sample.values())))
    if group is not None:
        group = np.asarray(group)
        out["groups"] = {}
        for g in sorted(set(group.tolist())):
            m = group == g
            out["groups"][int(g)] = {k: float(np.mean(v[m])) for k, v in per_sample.items()}
            out["groups"][int(g)]["samples"] = int(m.sum())
    return out


def alignment_spectrum(A, B):
    """How well one pair of sets [N, 3] fixes its rotation: dict of s (the singular values s1 >= s2 >= s3 of
    H = (A - cA)^T (B - cB) / N), sign (of det H, +1 for det H = 0), gap = 2 (s2 + sign s3) / s1 (the distance between the
    two largest eigenvalues of Horn's 4x4 matrix over s1; nan for H = 0 and for non-finite data) and varP (population
    variance of A summed over the axes).  gap = 0: a one-parameter family of rotations attains the optimum."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        H = (A - A.mean(axis=0)).T @ (B - B.mean(axis=0)) / A.shape[0]
        varP = float(np.var(A, axis=0).sum())
    if not np.isfinite(H).all():
        return {"s": np.full(3, np.nan), "sign": 1.0, "gap": float("nan"), "varP": varP}
    s = np.linalg.svd(H, compute_uv=False)
    sign = -1.0 if np.linalg.det(H) < 0 else 1.0
    gap = float(2.0 * (s[1] + sign * s[2]) / s[0]) if s[0] > 0 else float("nan")
    return {"s": s, "sign": sign, "gap": gap, "varP": varP}


def optimum(A, B):
    """(c, rms) of one pair: the optimal scale and the root-mean-square residual |c R A + t - B| over the points.  Both are
    unique even where R is not (every maximiser of tr(R H) has the same c and the same residual); the residual is
    evaluated at the SVD's maximiser, not from the closed form varB - lam^2 / varP, which cancels for exact similarities."""
    c, R, t = rigid_transform_3D(A, B)
    A2 = (c * R @ np.asarray(A, np.float64).T).T + t
    return float(c), float(np.sqrt(np.mean(np.sum((A2 - np.asarray(B, np.float64)) ** 2, axis=-1))))
