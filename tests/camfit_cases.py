"""TEST INFRASTRUCTURE ONLY - the cases of the camera tests and what the yardstick (camfit_ref.py) says about them, computed
once per session and shared by tests/test_camfit_cpu.py and tests/test_gpu_camfit.py."""
import functools
import os

import numpy as np

import camfit_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camfit_ref.npz")
CROP, IMG_RES = 500.0, 250.0
BAND = 1e-3                                    # px: a short-run case whose residuals came closer to zero is left out
SHORT_B, SHORT_J, SHORT_STEPS = (1, 5, 67), (1, 2, 17, 19, 21, 64), (0, 1, 2, 8, 32)
N_ORDERS = 8
FIT_CASES = ("j17", "j19", "j21", "outlier")
PREP_POSES = ("demo", "coco", "hand", "wide")
OUTLIER_JOINT = 5
N_LAUNCH = 32                                  # the tests launch the first 32 recorded starts of a fixture case


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def short_batch(B, J):
    """N(0, 0.3) joints, a camera near the demo's, 4 px of noise on the target, uniform starts: [B, J, 3], [B, J, 2], [B, 3].
    Of 2 B + 8 candidates drawn this way the first B are taken whose float64 run of 32 steps keeps every residual 2 BAND away
    from zero: the yardstick alone decides, so that it leaves out none of them afterwards."""
    rng = np.random.default_rng(1000 * B + J)
    n = 2 * B + 8
    p = rng.normal(0, 0.3, (n, J, 3)).astype(np.float32)
    cam = np.stack([rng.uniform(0.6, 1.4, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n)], 1)
    t = (p[:, :, :2].astype(np.float64) + cam[:, None, 1:]) * cam[:, None, :1] * IMG_RES + IMG_RES + rng.normal(0, 4.0, (n, J, 2))
    t, c0 = t.astype(np.float32), rng.uniform(0, 1, (n, 3)).astype(np.float32)
    _, _, mar = camfit_ref.fit(p, t, None, c0, steps=max(SHORT_STEPS), img_res=IMG_RES)
    take = np.flatnonzero(mar >= 2 * BAND)[:B]
    assert len(take) == B, (B, J, len(take))
    return p[take], t[take], c0[take]


def yardstick(p, t, w, c0):
    """steps -> dict(cam, loss: float64 results; keep [S]: min_abs_residual >= BAND; dcam, dloss: the largest |fp32 mode -
    float64 mode| over the kept samples and N_ORDERS shuffled summation orders)."""
    n, J = max(SHORT_STEPS), p.shape[1]
    tr64 = []
    camfit_ref.fit(p, t, w, c0, steps=n, img_res=IMG_RES, trace=tr64)
    rng = np.random.default_rng(5)
    tr32 = []
    for _ in range(N_ORDERS):
        tr = []
        camfit_ref.fit(p, t, w, c0, steps=n, img_res=IMG_RES, dtype=np.float32, order=rng.permutation(J), trace=tr)
        tr32.append(tr)
    out = {}
    for s in SHORT_STEPS:
        cam, loss, mar = tr64[s]
        keep = mar >= BAND
        dcam = max((np.abs(tr[s][0][keep] - cam[keep]).max() if keep.any() else 0.0) for tr in tr32)
        dloss = max((np.abs(tr[s][1][keep] - loss[keep]).max() if keep.any() else 0.0) for tr in tr32)
        out[s] = dict(cam=cam, loss=loss, keep=keep, dcam=float(dcam), dloss=float(dloss))
    return out


@functools.lru_cache(maxsize=None)
def short_yardstick(B, J):
    p, t, c0 = short_batch(B, J)
    return yardstick(p, t, None, c0)


def weight_case():
    """The fourth fixture case with weight 0 on its outlier joint, from the 32 recorded starts: p, t, w [32, J, .], c0."""
    rec = fit_case("outlier")
    S = N_LAUNCH
    w = np.ones(len(rec["joints3d"]), np.float32)
    w[OUTLIER_JOINT] = 0.0
    return np.repeat(rec["joints3d"][None], S, 0), np.repeat(rec["target"][None], S, 0), np.repeat(w[None], S, 0), rec["starts"][:S]


@functools.lru_cache(maxsize=None)
def weight_yardstick():
    return yardstick(*weight_case())


def fit_case(name):
    """The recorded case: joints3d [J, 3], target [J, 2], starts [N, 3], reference cams [N, 3] and float64 losses [N], the
    exact optimum and its loss."""
    g = golden()
    return {k: g[f"fit_{name}_{k}"] for k in ("joints3d", "target", "starts", "cams", "losses", "opt_cam", "opt_loss")}


def full_run_bounds(rec):
    """Conditions (a) and (b): (the bound on L - L*, the median reference camera, the bound on |cam - median| per component)."""
    excess = float((rec["losses"] - rec["opt_loss"]).max())
    med = np.median(rec["cams"].astype(np.float64), axis=0)
    return 2.0 * excess, med, 2.0 * np.abs(rec["cams"].astype(np.float64) - med).max(axis=0)


def check_full_run(cam, rec, joints3d=None, target=None, weight=None):
    """Asserts (a) and (b) for cam [S, 3] against the record; returns (max L - L*, max |cam - median| per component)."""
    S = len(cam)
    p = np.repeat((rec["joints3d"] if joints3d is None else joints3d)[None], S, 0)
    t = np.repeat((rec["target"] if target is None else target)[None], S, 0)
    w = None if weight is None else np.repeat(weight[None], S, 0)
    L = camfit_ref.loss64(cam, p, t, w, IMG_RES)
    bound_a, med, bound_b = full_run_bounds(rec)
    excess, dev = (L - rec["opt_loss"]).max(), np.abs(np.asarray(cam, np.float64) - med).max(axis=0)
    print(f"full run: max L - L* = {excess:.3e} (bound {bound_a:.3e}); max |cam - median| = {dev} (bound {bound_b})")
    assert excess <= bound_a, (excess, bound_a)
    assert (dev <= bound_b).all(), (dev, bound_b)
    return excess, dev
