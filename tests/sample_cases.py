"""Seeded case tables of the sample-noise tests (CPU audit, GPU comparison, fixture maker).  Everything is built from one
standing COCO pose in a 288 x 384 crop; the seeds are part of the cases: the robustness audit (test_sample_cpu.py) holds
for them."""
import numpy as np

from pose2mesh_release_amd.synth import COCO_STANDING_POSE

POSE = np.array(COCO_STANDING_POSE, np.float32)
AREA = 104.0 * 291.0          # the tight box of POSE


def _pose(valid=None, move=None):
    j = np.concatenate([POSE, np.ones((17, 1), np.float32)], axis=1)
    if valid is not None:
        j[:, 2] = 0
        j[list(valid), 2] = 1
    for k, xy in (move or {}).items():
        j[k, :2] = xy
    return j


def histogram_poses():
    """The three poses whose reference histograms tests/golden/sample_noise_ref.npz records: name -> (joints [17, 3], area)."""
    return {
        "all_valid": (_pose(), AREA),
        "valid8": (_pose(valid=(0, 1, 2, 5, 6, 7, 11, 12)), AREA),
        "valid4_close": (_pose(valid=(5, 6, 11, 12), move={6: (169.0, 100.0)}), AREA),     # shoulders 6 px apart
    }


def _jittered(B, seed, **kw):
    """B copies of a pose, each moved by a seeded N(0, 3^2) per joint and scaled about the crop centre by U(0.6, 1.2)."""
    rng = np.random.default_rng(seed)
    j = np.repeat(_pose(**kw)[None], B, axis=0)
    s = rng.uniform(0.6, 1.2, (B, 1, 1)).astype(np.float32)
    j[:, :, :2] = (j[:, :, :2] - np.float32([144, 192])) * s + np.float32([144, 192]) + rng.normal(0, 3, (B, 17, 2)).astype(np.float32)
    return j, (AREA * s[:, 0, 0] ** 2).astype(np.float32)


def noise_cases():
    """name -> dict(joints [B, 17, 3], area [B], seed, first_index, coincident: units held to the weak invariants only).
    B walks {1, 3, 9, 65}."""
    cases = {}

    def add(name, B, seed, first, area=None, fix=None, coincident=(), **kw):
        j, a = _jittered(B, seed, **kw)
        if fix is not None:
            fix(j)
        cases[name] = dict(joints=j, area=a if area is None else np.full(B, area, np.float32), seed=seed, first_index=first,
                           coincident=tuple(coincident))

    add("all_valid", 65, 11, 0)
    add("valid_le10", 9, 12, 1000, valid=(0, 1, 2, 5, 6, 7, 11, 12))
    add("valid_le5", 9, 13, (1 << 32) - 4, valid=(5, 6, 11, 12))                  # the index crosses 2^32
    add("partner_invalid", 3, 14, 7, valid=(0, 1, 3, 5, 7, 9, 11, 13, 15, 16))

    def close(j):
        j[:, 6, :2] = j[:, 5, :2] + np.float32([0.5, 0.0])
    add("pair_half_px", 9, 15, 50, fix=close)
    add("tiny_area", 3, 16, 3, area=1e-6)

    def coincide(j):                         # the hips coincide: margin 0 by construction (unit 6)
        j[:, 12, :2] = j[:, 11, :2]
    add("coincident_pair", 9, 17, 123456789012, fix=coincide, coincident=(6,))
    add("single", 1, 18, 5)
    return cases


def zeroed_lower_case():
    """A lower joint that gets zeroed and feeds (0, 0) to its partner.  Coincidence alone does not zero a joint (a miss
    candidate lies ks_50 .. ks_10 from both sources at once and usually passes); an area of 0 on top of it does: all radii
    are 0, every candidate sits on its source, and against a coincident partner nothing passes (0 > 0 is false, in any
    precision).  The eyes (unit 1) and the hips (unit 6) coincide: joints 1 and 11 are zeroed, and joints 2 and 12 then see
    their partner at (0, 0), where every candidate passes."""
    j = np.repeat(_pose()[None], 3, axis=0)
    j[:, 2, :2] = j[:, 1, :2]
    j[:, 12, :2] = j[:, 11, :2]
    return dict(joints=j, area=np.zeros(3, np.float32), seed=19, first_index=9, coincident=(1, 6))


COCO_FLIP_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
H36M_FLIP_PAIRS = ((1, 4), (2, 5), (3, 6), (14, 11), (15, 12), (16, 13))
COCO_MIDPOINTS = ((11, 12), (5, 6))          # pelvis, neck (add_pelvis_and_neck)
W, H = 288, 384


def regressor(J, nv, seed):
    """Sparse row-stochastic joint regressor, min(6, nv) vertices per joint (synth.synthetic_regressor's shape, any nv)."""
    rng = np.random.default_rng(seed)
    R = np.zeros((J, nv), np.float32)
    k = min(6, nv)
    for j in range(J):
        w = rng.random(k).astype(np.float32)
        R[j, rng.choice(nv, size=k, replace=False)] = w / w.sum()
    return R


def chain_case(B, nv, seed, joint_set="coco", rot=None, flip=None):
    """A seeded batch for the chain: a person-sized point cloud 3 - 6 m in front of a 1000 - 1500 px camera.  joint_set
    'coco': 17 regressed joints + pelvis + neck, root = pelvis (index 17); 'human36': the input set is the reg set.
    nv = 1 makes every joint coincide: the degenerate bbox."""
    rng = np.random.default_rng(seed)
    verts = (rng.normal(0, 1, (B, nv, 3)) * [0.25, 0.5, 0.15]).astype(np.float32)
    trans = np.stack([rng.uniform(-0.4, 0.4, B), rng.uniform(-0.4, 0.4, B), rng.uniform(3, 6, B)], axis=1).astype(np.float32)
    focal = rng.uniform(1000, 1500, (B, 2)).astype(np.float32)
    princpt = rng.uniform(400, 600, (B, 2)).astype(np.float32)
    c = dict(verts=verts, trans=trans, focal=focal, princpt=princpt, reg_R=regressor(17, nv, seed + 1), reg_root=0,
             mesh_scale=1000.0, W=W, H=H, joint_set=joint_set)
    if joint_set == "coco":
        c.update(in_R=regressor(17, nv, seed + 2), midpoints=COCO_MIDPOINTS, input_root=17, flip_pairs=COCO_FLIP_PAIRS)
    else:
        c.update(in_R=None, midpoints=(), input_root=0, flip_pairs=H36M_FLIP_PAIRS)
    c["rot"] = rng.choice([0.0, 17.5, -60.0, 90.0, 33.25], B).astype(np.float32) if rot is None else np.asarray(rot, np.float32)
    c["flip"] = rng.integers(0, 2, B).astype(np.int32) if flip is None else np.asarray(flip, np.int32)
    return c


GIVEN_OFFSET_MM = np.array([0.0, 10.0, 50.0, 200.0])       # mean fit error planted into given_joints, per sample


def given_joints(c, base):
    """'Annotated' reg joints [B, 17, 3] in mm for a chain_case of B = 4: the regressed ones, moved as a whole by (7, -3, 11)
    mm (the mean alignment removes that), and then joints 0 .. 15 by GIVEN_OFFSET_MM[b] * 17 / 16 along +x (even j) or -x
    (odd j); joint 16 stays.  The offsets sum to zero, so the alignment keeps them and the mean distance over the 17 joints
    is GIVEN_OFFSET_MM[b]."""
    reg = base["reg_pose3d"].astype(np.float64)
    sign = np.where(np.arange(17) % 2 == 0, 1.0, -1.0)
    sign[16] = 0.0
    g = reg + np.array([7.0, -3.0, 11.0])
    g[:, :, 0] += GIVEN_OFFSET_MM[:len(g), None] * 17.0 / 16.0 * sign[None]
    return g.astype(np.float32)


def chain_kwargs(c):
    """The keyword arguments of sample_ref.chain for a chain_case."""
    return {k: c[k] for k in ("reg_R", "reg_root", "in_R", "midpoints", "input_root", "trans", "mesh_scale", "flip_pairs", "W", "H")}


def chain_fixture_cases():
    """The samples tests/golden/sample_chain.npz records: rot in {0, 17.5, -60, 90} x flip in {0, 1} in the coco set, and
    the four rotations with alternating flip in the human36 set, on a 40-point cloud."""
    rots = [0.0, 17.5, -60.0, 90.0]
    return {"coco": chain_case(8, 40, 31, "coco", rot=rots * 2, flip=[0] * 4 + [1] * 4),
            "human36": chain_case(4, 40, 32, "human36", rot=rots, flip=[0, 1, 0, 1])}


def table(J, seed):
    """A seeded synthetic error table: mean [J, 2], std [J, 2], weight [J] (one weight 0 and one 1: the mask's two ends)."""
    rng = np.random.default_rng(seed)
    mean = rng.normal(0, 2, (J, 2)).astype(np.float32)
    std = rng.uniform(0.5, 6, (J, 2)).astype(np.float32)
    weight = rng.uniform(0.05, 0.95, J).astype(np.float32)
    weight[0] = 0.0
    weight[J - 1] = 1.0                      # J = 1: the one joint always gets its error, so values are compared
    return mean, std, weight
