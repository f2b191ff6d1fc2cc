"""The committed body-model fixtures (tests/golden/body_*.npz, written by tests/golden/make_golden_body.py) as test cases,
shared by the CPU and the GPU tests.  The synthetic models are regenerated from the stored seed and checked against the
stored checksum: a mismatch is FIXTURE DRIFT (numpy's generator or synth.body_model changed), not a kernel error."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = {"smpl": "body_smpl.npz", "mano": "body_mano.npz"}


@functools.lru_cache(maxsize=None)
def fixture(flavour):
    z = np.load(os.path.join(GOLDEN, FILES[flavour]))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def model(kind, V, seed=0):
    from pose2mesh_release_amd import synth
    return synth.body_model(kind, V, seed)


def fixture_model(flavour, kind):
    z = fixture(flavour)
    m = model(kind, int(z["num_vertex"]), int(z["seed"]))
    want = float(z[f"checksum_{kind}"])
    assert abs(m["checksum"] - want) <= 1e-9 * abs(want), \
        f"fixture drift: synth.body_model({kind!r}) no longer regenerates the model the {FILES[flavour]} outputs were made with"
    return m


def case_ids():
    return [(f, str(n)) for f in FILES for n in fixture(f)["cases"]]


def case(flavour, name):
    """dict: model, pose, betas / trans (None when the case passes none), center_idx, extra_reg, verts, joints, extra, err32."""
    z = fixture(flavour)
    c = int(z[f"{name}_center"])
    return {"model": fixture_model(flavour, str(z[f"{name}_kind"])), "pose": z[f"{name}_pose"], "betas": z.get(f"{name}_betas"),
            "trans": z.get(f"{name}_trans"), "center_idx": None if c < 0 else c, "extra_reg": z.get(f"{name}_extra_reg"),
            "verts": z[f"{name}_verts"], "joints": z[f"{name}_joints"], "extra": z.get(f"{name}_extra"),
            "err32": float(z[f"{name}_err32"])}
