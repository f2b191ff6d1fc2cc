"""The case table shared by tests/test_fscore_cpu.py (the float64 audit: cKDTree agreement, empty bands, the fp32 emulation)
and tests/test_gpu_fscore.py (the kernels).  Sizes sit on the launch edges of csrc/fscore.hip: 1, 2, the query tile of small
sets (512) and the target tile (1024) - 1 / exact / + 1, the switch to 4 queries per lane (2048 / 2049), the query tile of
large sets (1024 per block: 3071 / 3072 / 3073), FreiHAND's 778 (B = 3) and SMPL's 6890 (B = 2) from the reference-made
eval_mesh_* fixtures.  tests/test_fscore_cpu.py asserts that the exported tile sizes are the ones this table was laid out for."""
import numpy as np

import helpers

TARGET_TILE = 1024
QUERY_TILE_SMALL, QUERY_TILE_LARGE, SMALL_MAX = 512, 1024, 2048
SHELL_NV = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073)
SHELL_TH = (3.0, 5.0, 8.0, 15.0)         # sigma = 4 mm: F@15 is 1.0, 3 and 8 mm give non-trivial values


# seeds other than 1000 + nv: the first of 1000 + nv + 10000 k whose bands are empty (the rule of tests/fscore_ref.py: a
# vertex in the band means another seed, never another bound)
SHELL_SEED = {3072: 14072, 3073: 14073}


def shell_cloud(nv, B, seed, shuffle, radius=100.0, sigma=4.0, offset=(200.0, -300.0, 4000.0)):
    """Seeded shell clouds in camera space: gt on a sphere of `radius` mm around `offset` + a per-sample shift (the returned
    centre), pred = gt + N(0, sigma) noise.  shuffle: pred's rows are permuted (the index correspondence carries nothing;
    an alignment over it would be meaningless).  Otherwise pred is moved by a small similarity about the centre (3 degrees,
    x 1.03, 4 mm), which the aligned variant undoes.  Returns fp32 pred, gt [B, nv, 3] and float64 centres [B, 3]."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((B, nv, 3))
    cen = np.asarray(offset) + rng.uniform(-50, 50, (B, 3))
    g = radius * d / np.linalg.norm(d, axis=-1, keepdims=True)
    p = g + sigma * rng.standard_normal((B, nv, 3))
    if shuffle:
        p = np.stack([x[rng.permutation(nv)] for x in p])
    else:
        a = np.deg2rad(3.0)
        Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        p = 1.03 * p @ Rz.T + np.array([4.0, 0.0, 0.0])
    return (p + cen[:, None]).astype(np.float32), (g + cen[:, None]).astype(np.float32), cen


def fixture_regressor(z):
    R = np.zeros(tuple(int(v) for v in z["reg_shape"]), dtype=np.float32)
    R[z["reg_rows"], z["reg_cols"]] = z["reg_vals"]
    return R


def _shell_case(nv):
    """Odd sizes: rows shuffled, centred only, centres given by the caller (the sphere's centre, jittered per mesh).  Even
    sizes: rows in order and a similarity between the meshes, centred and aligned; up to 1024 points they are compared
    where they are (no centre: the alignment's term of the bound then scales with the 4 m to the camera, and above 1024
    points some of the ~25 000 distances would fall into a band that wide), above with given centres."""
    B = 2
    odd = nv % 2 == 1
    pred, gt, cen = shell_cloud(nv, B, seed=SHELL_SEED.get(nv, 1000 + nv), shuffle=odd)
    case = dict(name=f"shell{nv}", pred=pred, gt=gt, gt_scale=1.0, regressor=None, root=0, pred_root=None, gt_root=None,
                thresholds=SHELL_TH, centred=True, aligned=not odd and nv >= 64)   # (2 points do not fix a similarity)
    if odd or nv > 1024:
        rng = np.random.default_rng(5000 + nv)
        case["pred_root"] = (cen + rng.uniform(-1, 1, (B, 3))).astype(np.float32)
        case["gt_root"] = (cen + rng.uniform(-1, 1, (B, 3))).astype(np.float32)
    return case


def _fixture_case(name, fname, thresholds=(5.0, 15.0), centred=True, aligned=True):
    z = helpers.golden(fname)
    return dict(name=name, pred=z["pred"], gt=z["gt"], gt_scale=float(z["gt_scale"]), regressor=fixture_regressor(z),
                root=int(z["root"]), pred_root=None, gt_root=None, thresholds=thresholds, centred=centred, aligned=aligned)


# FreiHAND's 5 and 15 mm on both fixtures.  On the aligned variant of the SMPL-size fixture one vertex lies 1.00 x its bound
# from 15 mm (13 780 distances per threshold: a gap of the bound's size is to be expected somewhere), so that variant is
# audited at 5, 8 and 20 mm, where its band is empty, and the centred one keeps 5 and 15.
_FIXTURES = {"mano778": ("eval_mesh_mano.npz", (5.0, 15.0), True, True),
             "smpl6890": ("eval_mesh_smpl.npz", (5.0, 15.0), True, False),
             "smpl6890_pa": ("eval_mesh_smpl.npz", (5.0, 8.0, 20.0), False, True)}


_cache = {}


def case(name):
    if name not in _cache:
        if name.startswith("shell"):
            _cache[name] = _shell_case(int(name[5:]))
        else:
            _cache[name] = _fixture_case(name, *_FIXTURES[name])
    return _cache[name]


CASE_NAMES = [f"shell{nv}" for nv in SHELL_NV] + list(_FIXTURES)

_ref_cache = {}


def reference(name):
    """fscore_ref.evaluate of a case, computed once per session and shared (callers must not modify it)."""
    import fscore_ref
    if name not in _ref_cache:
        c = case(name)
        _ref_cache[name] = fscore_ref.evaluate(c["pred"], c["gt"], c["thresholds"], c["gt_scale"], c["regressor"], c["root"],
                                               c["pred_root"], c["gt_root"], c["centred"], c["aligned"])
    return _ref_cache[name]


# p2m_point_nn with nA != nB: (nb, nA, nB); both below / above the queries-per-lane switch, a set of one point
NN_SHAPES = ((2, 700, 1300), (3, 1025, 64), (1, 1, 513), (2, 2100, 90))


def nn_pair(nb, nA, nB, seed):
    rng = np.random.default_rng(seed)
    off = np.array([-150.0, 900.0, 3000.0])
    A = (rng.standard_normal((nb, nA, 3)) * 60 + off).astype(np.float32)
    Bm = (rng.standard_normal((nb, nB, 3)) * 60 + off + 20).astype(np.float32)
    return A, Bm


def far_shells(nv=TARGET_TILE + 1, B=2, seed=77):
    """The true nearest target is farther than the staging origin: prediction on a shell of radius 10 mm, ground truth on one
    of radius 100 mm about the same centre, nv one past a target tile.  Every d_pred is about 90 mm; a target tile whose tail
    was left as zeros (the origin, 10 mm away) would report about 10.  A case dict like the table's (no centre, centred only)."""
    rng = np.random.default_rng(seed)
    cen = np.array([200.0, -300.0, 4000.0]) + rng.uniform(-50, 50, (B, 1, 3))
    d = rng.standard_normal((2, B, nv, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return dict(name="far_shells", pred=(10.0 * d[0] + cen).astype(np.float32), gt=(100.0 * d[1] + cen).astype(np.float32),
                gt_scale=1.0, regressor=None, root=0, pred_root=None, gt_root=None, thresholds=(50.0, 95.0), centred=True,
                aligned=False)


def five_hands(seed=9):
    """Five 778-point shell clouds, a small similarity apart, centres given, three thresholds: the padding, batch-independence
    and group-total tests.  (Seed: bands empty, checked in tests/test_fscore_cpu.py.)"""
    pred, gt, cen = shell_cloud(778, 5, seed, shuffle=False)
    return dict(name="five_hands", pred=pred, gt=gt, gt_scale=1.0, regressor=None, root=0, pred_root=cen.astype(np.float32),
                gt_root=cen.astype(np.float32), thresholds=(3.0, 5.0, 8.0), centred=True, aligned=True)
