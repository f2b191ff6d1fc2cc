#!/usr/bin/env python3
"""Generates tests/golden/body_smpl.npz and body_mano.npz by running the REAL reference layers' forward on the CPU:
smplpytorch's SMPL_Layer (smpl_layer.py:65-158) and manopth's ManoLayer (manolayer.py:109-273, built as lib/_mano.py:33
builds it: use_pca=False, flat_hand_mean=False).  Run where the reference tree exists (the GPU box has none):

    python tests/golden/make_golden_body.py

The licensed .pkl models are absent, so the layer objects are made with __new__ + Module.__init__ and get the th_* buffers
of a seeded synthetic model (pose2mesh_release_amd.synth.body_model); their forward code is the reference's own.  The
fixture stores the model's kind / seed / vertex count / float64 checksum, not the model (SMPL-size tables are 18 MB).

Per case <n> (names in "cases"): <n>_pose, _betas, _trans (fp32 inputs; absent when the case passes None), _center (-1:
None), _extra_reg (optional regressor, fp32), the float64 outputs _verts, _joints, _extra of the reference run in float64
on the fp32-rounded model and inputs, and _err32: the max per-vertex L2 error of the reference's own fp32 run against that
float64 run.  ManoLayer ignores kintree_parents (its tree is hard-coded), so the MANO-like model carries that tree."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from pose2mesh_release_amd import synth  # noqa: E402

REF_ROOT = os.environ.get("P2M_REFERENCE_ROOT", "/root/reference")


def _import_layers():
    import importlib
    import types
    for p in (os.path.join(REF_ROOT, "smplpytorch"), os.path.join(REF_ROOT, "manopth")):
        if p not in sys.path:
            sys.path.insert(0, p)

    def imp(name):
        for _ in range(8):                                   # stub whatever the .pkl readers want (chumpy, cv2, ...)
            try:
                return importlib.import_module(name)
            except ModuleNotFoundError as e:
                if e.name is None or e.name.split(".")[0] in ("smplpytorch", "manopth", "mano"):
                    raise
                sys.modules[e.name] = types.ModuleType(e.name)
        raise ImportError(name)
    return imp("smplpytorch.pytorch.smpl_layer").SMPL_Layer, imp("manopth.manolayer").ManoLayer


def reference_layer(model, center_idx=None, dtype=torch.float64):
    """The reference layer object for a synth.body_model dict (kind "mano": ManoLayer, else SMPL_Layer)."""
    SMPL_Layer, ManoLayer = _import_layers()
    mano = model["kind"] == "mano"
    cls = ManoLayer if mano else SMPL_Layer
    layer = cls.__new__(cls)
    torch.nn.Module.__init__(layer)

    def t(a):
        return torch.from_numpy(np.asarray(a, np.float32)).to(dtype)
    layer.register_buffer("th_betas", t(model["betas"]).unsqueeze(0))
    layer.register_buffer("th_shapedirs", t(model["shapedirs"]))
    layer.register_buffer("th_posedirs", t(model["posedirs"]))
    layer.register_buffer("th_v_template", t(model["v_template"]).unsqueeze(0))
    layer.register_buffer("th_J_regressor", t(model["J_regressor"]))
    layer.register_buffer("th_weights", t(model["weights"]))
    layer.kintree_parents = [4294967295] + list(model["parents"][1:])      # kintree_table[0] of the .pkl files
    layer.center_idx = center_idx
    if mano:
        layer.side, layer.rot, layer.ncomps, layer.use_pca = "right", 3, 45, False
        layer.joint_rot_mode = layer.root_rot_mode = "axisang"
        layer.flat_hand_mean, layer.robust_rot = False, False
        layer.register_buffer("th_hands_mean", t(model["hands_mean"]).unsqueeze(0))
    else:
        layer.num_joints = len(model["parents"])
        layer.gender = "neutral"
    return layer


def run_reference(model, pose, betas, trans, center_idx, dtype):
    layer = reference_layer(model, center_idx, dtype)

    def t(a):
        return None if a is None else torch.from_numpy(a).to(dtype)
    kw = {}
    if trans is not None:
        kw["th_trans"] = t(trans)
    with torch.no_grad():
        v, j = layer(t(pose), t(betas), **kw)
    return v.double().numpy(), j.double().numpy()


def inputs(rng, B, J, nb):
    pose = rng.standard_normal((B, J, 3)) * 0.6
    if B >= 5:
        pose[1] = 0.0                                        # the all-zero pose
        d = rng.standard_normal((J, 3))
        pose[2] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(3.0, 4.0, (J, 1))    # angles beyond pi
    betas = rng.standard_normal((B, nb))
    betas[B - 1, 0] = 3.5                                    # one |beta| > 3
    trans = rng.standard_normal((B, 3)) * 0.7
    return [np.ascontiguousarray(x, np.float64).astype(np.float32) for x in (pose.reshape(B, -1), betas, trans)]


# (name, kind, B, betas given, trans given, center_idx, extra regressor joints)
SMPL_CASES = [("rand_b1", "smpl", 1, True, False, None, 0), ("rand_b5", "smpl", 5, True, True, 0, 0),
              ("rand_b37", "smpl", 37, True, False, 0, 17), ("rand_b5_nobeta", "smpl", 5, False, True, None, 0),
              ("chain_b1", "chain", 1, True, True, None, 0), ("chain_b5", "chain", 5, True, False, 0, 0),
              ("star_b1", "star", 1, False, False, 0, 0), ("star_b5", "star", 5, True, True, 0, 0)]
MANO_CASES = [("b1", "mano", 1, False, False, None, 0), ("b1_trans", "mano", 1, True, True, None, 0),
              ("b5", "mano", 5, True, True, 0, 21), ("b37", "mano", 37, True, False, 0, 0)]


def make(path, cases, V, seed):
    out = {"cases": np.array([c[0] for c in cases]), "seed": np.int64(seed), "num_vertex": np.int64(V)}
    models = {}
    for i, (name, kind, B, has_b, has_t, center, nx) in enumerate(cases):
        m = models.setdefault(kind, synth.body_model(kind, V, seed))
        out[f"checksum_{kind}"] = np.float64(m["checksum"])
        J = len(m["parents"])
        pose, betas, trans = inputs(np.random.default_rng([seed, 77, i]), B, J, 10)
        betas, trans = (betas if has_b else None), (trans if has_t else None)
        v64, j64 = run_reference(m, pose, betas, trans, center, torch.float64)
        v32, _ = run_reference(m, pose, betas, trans, center, torch.float32)
        out[f"{name}_kind"] = np.array(kind)
        out[f"{name}_pose"] = pose
        if has_b:
            out[f"{name}_betas"] = betas
        if has_t:
            out[f"{name}_trans"] = trans
        out[f"{name}_center"] = np.int64(-1 if center is None else center)
        out[f"{name}_verts"], out[f"{name}_joints"] = v64, j64
        out[f"{name}_err32"] = np.float64(np.sqrt(((v32 - v64) ** 2).sum(-1)).max())
        if nx:
            reg = synth.synthetic_regressor(nx, V, seed=5)
            out[f"{name}_extra_reg"] = reg
            out[f"{name}_extra"] = np.einsum("jv,bvc->bjc", reg.astype(np.float64), v64)
        print(f"{os.path.basename(path)} {name}: B={B} |v|max={np.abs(v64).max():.3f} err32={out[f'{name}_err32']:.3e}")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    make(os.path.join(HERE, "body_smpl.npz"), SMPL_CASES, 257, 0)
    make(os.path.join(HERE, "body_mano.npz"), MANO_CASES, 778, 0)
