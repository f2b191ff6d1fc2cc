"""The cases shared by tests/test_profile_cpu.py (the float64 audit of tests/profile_ref.py) and tests/test_gpu_profile.py (the
kernels of csrc/profile.hip).  Point counts sit on the edges of the 256-lane block and its 64-lane waves (1, 63, 64, 65, 255,
256, 257) plus FreiHAND's 778; batches of 1, 3 and 5; tables of 2, 100 and 256 thresholds and one that is not uniform."""
import numpy as np

import helpers

NS = (1, 63, 64, 65, 255, 256, 257, 778)
BS = (1, 3, 5)
TABLES = {"k2": np.linspace(0.0, 50.0, 2), "k100": np.linspace(0.0, 50.0, 100), "k256": np.linspace(0.0, 80.0, 256),
          "steps": np.array([0.5, 1.0, 2.0, 5.0, 10.0, 15.0, 20.0, 30.0, 50.0, 75.0, 150.0])}
HIT_TABLE = np.linspace(0.0, 50.0, 101)           # == 0.5 * arange(101) bit for bit (tests/test_profile_cpu.py)


def cloud(B, N, seed, sigma=15.0):
    """Seeded point sets in camera space, mm: gt = N(0, 80) about (200, -300, 4000), pred = gt + N(0, sigma): errors of about
    1.6 sigma, spread over the 0-50 mm tables with a tail past them (bin K).  fp32 [B, N, 3] each."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((B, N, 3)) * 80.0 + np.array([200.0, -300.0, 4000.0])
    p = g + rng.standard_normal((B, N, 3)) * sigma
    return p.astype(np.float32), g.astype(np.float32)


def exact_hits():
    """Differences (3, 4, 0), (0, 0, 0), (6, 8, 0) and (60, 80, 0) between small-integer coordinates: the errors are exactly
    5, 0, 10 and 100 in every arithmetic.  Against HIT_TABLE (t[k] = k / 2) they sit ON t[10], t[0] and t[20]: bins 10, 0
    and 20 with the non-strict comparison (11, 1 and 21 with a strict one); 100 is past t[100] = 50: bin 101 = K."""
    g = np.tile(np.array([[10.0, 20.0, 30.0]]), (4, 1))
    d = np.array([[3.0, 4.0, 0.0], [0.0, 0.0, 0.0], [6.0, 8.0, 0.0], [60.0, 80.0, 0.0]])
    return (g + d)[None].astype(np.float32), g[None].astype(np.float32), np.array([10, 0, 20, 101])


def mano():
    """The reference-made FreiHAND-size fixture: pred in mm, gt in metres (read x 1000), B = 3, N = 778."""
    z = helpers.golden("eval_mesh_mano.npz")
    return z["pred"], z["gt"], float(z["gt_scale"])


# the aligned cases: name -> (pred, gt, gt_scale, table)
def aligned_case(name):
    if name == "mano778":
        p, g, s = mano()
        return p, g, s, TABLES["k100"]
    z = helpers.golden("eval_align.npz")
    # (a mirrored ground truth cannot be reached by a proper rotation: errors of hundreds of mm)
    table = np.linspace(0.0, 1000.0, 100) if name.startswith("mirror") else np.linspace(0.0, 100.0, 100)
    return z[name + "_A"], z[name + "_B"], 1.0, table


ALIGNED = ("mano778", "rand21", "rand778", "mirror14", "planar17")
