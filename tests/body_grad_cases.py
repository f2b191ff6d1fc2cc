"""The committed gradient fixtures (tests/golden/body_grad_*.npz, written by tests/golden/make_golden_body_grad.py with the
real layers' autograd) as test cases, on top of the forward cases of body_cases (same models, same inputs).  The loss
coefficients are regenerated from the stored seed and checked against the stored checksum: a mismatch is FIXTURE DRIFT."""
import functools
import os

import numpy as np

import body_cases
import body_grad_ref

FILES = {"smpl": "body_grad_smpl.npz", "mano": "body_grad_mano.npz"}
NAMES = ("pose", "betas", "trans")


@functools.lru_cache(maxsize=None)
def fixture(flavour):
    z = np.load(os.path.join(body_cases.GOLDEN, FILES[flavour]))
    return {k: z[k] for k in z.files}


def out_shapes(c):
    """Shapes of (verts, joints[, extra]) of a body_cases case."""
    shapes = [c["verts"].shape, c["joints"].shape]
    return shapes + ([c["extra"].shape] if c["extra_reg"] is not None else [])


@functools.lru_cache(maxsize=None)
def case(flavour, name):
    """The body_cases case plus "coeffs" (the loss coefficients, one float64 array per output), "grads" (float64 g_pose,
    g_betas, g_trans; None where the case passes no such input) and "gerr32" (the reference's own fp32 figures, likewise)."""
    c = dict(body_cases.case(flavour, name))
    z = fixture(flavour)
    coeffs, csum = body_grad_ref.loss_coeffs(int(z[f"{name}_cseed"]), out_shapes(c))
    want = float(z[f"{name}_cchecksum"])
    assert abs(csum - want) <= 1e-9 * abs(want), f"fixture drift: the loss coefficients of {FILES[flavour]} {name} do not regenerate"
    c["coeffs"] = coeffs
    c["grads"] = [z.get(f"{name}_g_{n}") for n in NAMES]
    c["gerr32"] = [None if f"{name}_gerr32_{n}" not in z else float(z[f"{name}_gerr32_{n}"]) for n in NAMES]
    return c


@functools.lru_cache(maxsize=None)
def file_gerr32(flavour):
    """Per gradient tensor, the reference's fp32 figure as the maximum over all cases of the file: {name: figure}."""
    out = {}
    for n in body_cases.fixture(flavour)["cases"]:
        for k, e in zip(NAMES, case(flavour, str(n))["gerr32"]):
            if e is not None:
                out[k] = max(out.get(k, 0.0), e)
    return out
