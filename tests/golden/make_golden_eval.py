#!/usr/bin/env python3
"""Generates tests/golden/eval_*.npz by running the REAL reference's rigid_transform_3D / rigid_align
(lib/coord_utils.py:127-149, imported read-only through oracle/ref_loader.load_aug()) on CPU, in float64.  Run where the
reference tree exists (the GPU box has none):   python tests/golden/make_golden_eval.py

Inputs are drawn from numpy PCG64, cast to fp32 and back: the fixture stores them as float32, so the GPU sees exactly the
numbers the reference saw.  Outputs are float64.

  eval_align.npz       per case <name>_A, <name>_B [nb, N, 3] and the reference's <name>_c [nb], _R [nb, 3, 3], _t [nb, 3],
                       _A2 [nb, N, 3]: random well-conditioned sets (N = 3, 14, 17, 21, 778), a mirrored B (the det < 0
                       branch), a planar A
  eval_mesh_smpl.npz   a stage-A/E/PA case on SMPL-size meshes (6890 vertices, mm): pred, gt [B, nv, 3], the real H36M
                       regressor (CSR triplets of demo_h36m.npz) as both stage A (root 0, the 14 eval joints) and stage E
                       (root 0, the 14 eval joints), and the per-sample metrics of the reference's loop body
                       (data/PW3D/dataset.py:335-372) with its rigid_align
  eval_mesh_mano.npz   the same on MANO-size meshes (778 vertices) with a synthetic 21-joint regressor (root 0, all joints)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import helpers  # noqa: E402
import ref_loader  # noqa: E402
from pose2mesh_release_amd import synth  # noqa: E402

H36M_EVAL_JOINT = (1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15, 16)    # data/Human36M/dataset.py:62


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def align_case(rng, nb, N, kind):
    A = np.empty((nb, N, 3))
    B = np.empty((nb, N, 3))
    for i in range(nb):
        a = rng.standard_normal((N, 3)) * rng.uniform(50, 400, 3) + rng.uniform(-1000, 1000, 3)     # mm-scale
        if kind == "planar":
            n = rng.standard_normal(3)
            n /= np.linalg.norm(n)
            a = a - np.outer((a - a.mean(0)) @ n, n)
        b = rng.uniform(0.7, 1.4) * a @ rotation(rng).T + rng.uniform(-800, 800, 3) + rng.standard_normal((N, 3)) * 20
        if kind == "mirror":
            b[:, 0] = -b[:, 0]
        A[i], B[i] = a, b
    return f32(A), f32(B)


def save(name, d):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    assert size < 1 << 20, (name, size)
    print(f"{name}: {size / 1024:.0f} KB")


def make_align(cu):
    rng = np.random.default_rng(20261016)
    cases = [("rand3", 16, 3, "rand"), ("rand14", 16, 14, "rand"), ("rand17", 16, 17, "rand"), ("rand21", 8, 21, "rand"),
             ("rand778", 3, 778, "rand"), ("mirror14", 8, 14, "mirror"), ("mirror778", 2, 778, "mirror"),
             ("planar17", 8, 17, "planar"), ("planar778", 2, 778, "planar")]
    d = {"cases": np.array([c[0] for c in cases])}
    for name, nb, N, kind in cases:
        A, B = align_case(rng, nb, N, kind)
        out = [cu.rigid_transform_3D(A[i].astype(np.float64), B[i].astype(np.float64)) for i in range(nb)]
        A2 = np.stack([cu.rigid_align(A[i].astype(np.float64), B[i].astype(np.float64)) for i in range(nb)])
        d[f"{name}_A"], d[f"{name}_B"] = A, B
        d[f"{name}_c"] = np.array([o[0] for o in out], np.float64)
        d[f"{name}_R"] = np.stack([o[1] for o in out]).astype(np.float64)
        d[f"{name}_t"] = np.stack([np.asarray(o[2]).reshape(3) for o in out]).astype(np.float64)
        d[f"{name}_A2"] = A2.astype(np.float64)
    save("eval_align.npz", d)


def ref_loop(cu, pred, gt, reg, root, sub, regE, rootE, subE):
    """data/PW3D/dataset.py:335-372 for one sample (both regressions on the meshes; PA-MPVPE of lines 360-361 enabled)."""
    jo, jg = np.dot(reg, pred), np.dot(reg, gt)
    mo, mg = pred - jo[root], gt - jg[root]
    po, pg = (jo - jo[root])[list(sub)], (jg - jg[root])[list(sub)]
    out = {"mpjpe_A": np.sqrt(np.sum((po - pg) ** 2, 1)), "mpvpe": np.sqrt(np.sum((mo - mg) ** 2, 1)).mean()}
    out["pa_mpvpe"] = np.sqrt(np.sum((cu.rigid_align(mo, mg) - mg) ** 2, 1)).mean()
    eo, eg = np.dot(regE, mo), np.dot(regE, mg)
    eo, eg = (eo - eo[rootE])[list(subE)], (eg - eg[rootE])[list(subE)]
    out["mpjpe_E"] = np.sqrt(np.sum((eo - eg) ** 2, 1))
    out["pa_mpjpe_E"] = np.sqrt(np.sum((cu.rigid_align(eo, eg) - eg) ** 2, 1))
    return out


def make_mesh(cu, name, nv, reg, sub, B, seed):
    rng = np.random.default_rng(seed)
    verts, _ = synth.hull_mesh(nv, 0)
    body = verts.astype(np.float64) * np.array([250.0, 800.0, 150.0])            # a body-sized ellipsoid, mm
    gt = np.empty((B, nv, 3))
    pred = np.empty((B, nv, 3))
    for b in range(B):
        g = body @ rotation(rng).T + rng.uniform(-500, 500, 3) + np.array([0, 0, 4000.0])
        gt[b] = g
        m = g.mean(0)                                             # prediction: a perturbed similarity of the truth
        pred[b] = (g - m) @ _small_rot(rng).T * rng.uniform(0.95, 1.05) + m + rng.uniform(-80, 80, 3) \
            + rng.standard_normal((nv, 3)) * 15
    pred, gt_m = f32(pred), f32(gt / 1000.0)                      # ground truth stored in metres (read x 1000)
    gt_mm = gt_m.astype(np.float64) * 1000.0
    reg64 = np.asarray(reg, np.float32).astype(np.float64)
    outs = [ref_loop(cu, pred[b].astype(np.float64), gt_mm[b], reg64, 0, sub, reg64, 0, sub) for b in range(B)]
    d = {"pred": pred, "gt": gt_m, "gt_scale": np.float64(1000.0), "root": np.int64(0), "sub": np.asarray(sub, np.int32)}
    rows, cols = np.nonzero(reg)
    d["reg_rows"], d["reg_cols"] = rows.astype(np.int32), cols.astype(np.int32)
    d["reg_vals"] = np.asarray(reg, np.float32)[rows, cols]
    d["reg_shape"] = np.array(reg.shape, np.int64)
    for k in outs[0]:
        d[k] = np.stack([np.asarray(o[k], np.float64) for o in outs])
    save(name, d)


def _small_rot(rng, deg=15.0):
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    th = np.deg2rad(rng.uniform(-deg, deg))
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def main():
    assert ref_loader.available(), f"reference tree not found at {ref_loader.REF_ROOT}"
    cu = ref_loader.load_aug().coord_utils
    make_align(cu)
    make_mesh(cu, "eval_mesh_smpl.npz", 6890, helpers.golden_regressor("demo_h36m.npz"), H36M_EVAL_JOINT, 2, 7)
    make_mesh(cu, "eval_mesh_mano.npz", 778, synth.synthetic_regressor(21, 778, seed=3), tuple(range(21)), 3, 8)


if __name__ == "__main__":
    main()
