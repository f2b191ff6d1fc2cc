"""Synthetic stand-ins for the licensed SMPL/MANO assets (none ship with the reference):
sphere-hull meshes with SMPL's / MANO's exact vertex, edge and face counts, the reference's joint
skeletons, and benchmark inputs normalised like the datasets do."""
import numpy as np

H36M_SKELETON = ((0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12), (12, 13), (8, 14), (14, 15), (15, 16),
                 (0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6))                 # data/Human36M/dataset.py:56-59
H36M_FLIP = ((1, 4), (2, 5), (3, 6), (14, 11), (15, 12), (16, 13))
COCO_SKELETON = ((1, 2), (0, 1), (0, 2), (2, 4), (1, 3), (6, 8), (8, 10), (5, 7), (7, 9), (12, 14), (14, 16),
                 (11, 13), (13, 15), (17, 11), (17, 12), (17, 18), (18, 5), (18, 6), (18, 0))   # demo/run.py:88-91
COCO_FLIP = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
MANO_SKELETON = ((0, 1), (0, 5), (0, 9), (0, 13), (0, 17), (1, 2), (2, 3), (3, 4), (5, 6), (6, 7), (7, 8), (9, 10),
                 (10, 11), (11, 12), (13, 14), (14, 15), (15, 16), (17, 18), (18, 19), (19, 20))   # demo/run.py:110
MANO_HORI = ((1, 5), (5, 9), (9, 13), (13, 17), (2, 6), (6, 10), (10, 14), (14, 18), (3, 7), (7, 11), (11, 15),
             (15, 19), (4, 8), (8, 12), (12, 16), (16, 20))                      # data/FreiHAND/dataset.py:38-40

JOINT_SETS = {
    "human36": (17, H36M_SKELETON, H36M_FLIP, 9),
    "coco": (19, COCO_SKELETON, COCO_FLIP, 9),
    "mano": (21, MANO_SKELETON, MANO_HORI, 6),
}


def hull_mesh(num_vertex, seed=0):
    """Convex hull of `num_vertex` random unit vectors: a closed triangle mesh with V=num_vertex,
    F=2V-4, E=3V-6 (6890 -> 13776 faces / 20664 edges, exactly SMPL's counts)."""
    from scipy.spatial import ConvexHull
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((num_vertex, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    return p.astype(np.float32), ConvexHull(p).simplices.astype(np.int64)


def make_graphs(joint_set="human36", num_vertex=None, seed=0):
    """(faces, graph_L list as build_coarse_graphs returns it, perm_reverse, num_joint)."""
    from . import graph_utils
    J, skel, flip, levels = JOINT_SETS[joint_set]
    if num_vertex is None:
        num_vertex = 778 if joint_set == "mano" else 6890
    _, faces = hull_mesh(num_vertex, seed)
    _, graph_L, _, perm_rev = graph_utils.build_coarse_graphs(faces, J, skel, flip, levels=levels)
    return faces, graph_L, perm_rev, J


def pose2d_batch(B, J, seed=123):
    """N(0,1) joints, then per-sample per-axis standardisation over joints
    (data/Human36M/dataset.py:387-388)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, J, 2, generator=g)
    x = (x - x.mean(dim=1, keepdim=True)) / x.std(dim=1, keepdim=True, unbiased=False)
    return x


def synthetic_regressor(J, nv, seed=5):
    """Sparse row-stochastic joint regressor like data/Human36M/J_regressor_h36m_correct.npy ((17, 6890), 107 nnz):
    6 vertices per joint, weights summing to 1."""
    rng = np.random.default_rng(seed)
    R = np.zeros((J, nv), dtype=np.float32)
    for j in range(J):
        idx = rng.choice(nv, size=6, replace=False)
        w = rng.random(6).astype(np.float32)
        R[j, idx] = w / w.sum()
    return R


MANO_PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)      # the tree manolayer.py:196-230 hard-codes
MANO_TIPS_RIGHT = (745, 317, 444, 556, 673)                               # manolayer.py:253
MANO_JOINT_ORDER = (0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20)   # manolayer.py:259
BODY_KINDS = ("smpl", "chain", "star", "mano")


def body_checksum(model):
    """Float64 checksum of a body-model dict's arrays (position-weighted, so a permutation changes it)."""
    s = 0.0
    for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "parents", "betas", "hands_mean"):
        if model.get(k) is None:
            continue
        a = np.asarray(model[k], dtype=np.float64).reshape(-1)
        s += float(np.abs(a).sum() + (a * ((np.arange(a.size) % 97) + 1.0)).sum() / 97.0)
    return s


def body_model(kind, num_vertex=None, seed=0):
    """Seeded synthetic stand-in for a licensed body model (the .pkl files are absent, like the real faces): a dict of
    the arrays BodyModel takes, fp32, plus "kind", "seed", "num_vertex" and "checksum" (body_checksum, float64).

      kind  "smpl"   24 joints, 10 betas, 207 pose directions, a random parents[j] < j tree, metres
            "chain"  the same with parents[j] = j - 1 (depth J - 1);  "star": all parents 0
            "mano"   16 joints on MANO's own tree (ManoLayer hard-codes it), hands_mean, five tip vertices, the 21-joint
                     order, outputs x 1000
    Template points lie on a squashed sphere, directions are small Gaussians, J_regressor rows are 12-sparse and sum to
    1, skinning weights are 4-sparse and sum to 1.  num_vertex defaults to 6890 / 778."""
    if kind not in BODY_KINDS:
        raise ValueError(f"kind: one of {BODY_KINDS}, got {kind!r}")
    mano = kind == "mano"
    J, nb = (16, 10) if mano else (24, 10)
    V = int(num_vertex) if num_vertex is not None else (778 if mano else 6890)
    if V < 1:
        raise ValueError("num_vertex < 1")
    rng = np.random.default_rng([seed, BODY_KINDS.index(kind), V])
    size = 0.1 if mano else 1.0
    p = rng.standard_normal((V, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    v_template = p * np.array([0.3, 0.9, 0.2]) * size
    shapedirs = rng.standard_normal((V, 3, nb)) * 0.01 * size
    posedirs = rng.standard_normal((V, 3, 9 * (J - 1))) * 0.002 * size
    J_regressor = np.zeros((J, V))
    nr = min(12, V)
    for j in range(J):
        w = rng.random(nr) + 0.05
        J_regressor[j, rng.choice(V, size=nr, replace=False)] = w / w.sum()
    weights = np.zeros((V, J))
    nw = min(4, J)
    for v in range(V):
        w = rng.random(nw) + 0.05
        weights[v, rng.choice(J, size=nw, replace=False)] = w / w.sum()
    if mano:
        parents = list(MANO_PARENTS)
    elif kind == "chain":
        parents = [-1] + list(range(J - 1))
    elif kind == "star":
        parents = [-1] + [0] * (J - 1)
    else:
        parents = [-1] + [int(rng.integers(0, j)) for j in range(1, J)]
    f32 = np.float32
    m = {"kind": kind, "seed": int(seed), "num_vertex": V,
         "v_template": v_template.astype(f32), "shapedirs": shapedirs.astype(f32), "posedirs": posedirs.astype(f32),
         "J_regressor": J_regressor.astype(f32), "weights": weights.astype(f32), "parents": parents,
         "betas": (rng.standard_normal(nb) * 0.1).astype(f32)}
    if mano:
        m["hands_mean"] = (rng.standard_normal(3 * (J - 1)) * 0.3).astype(f32)
        m["tip_vertices"] = list(MANO_TIPS_RIGHT) if V > max(MANO_TIPS_RIGHT) else [min(V - 1, (i + 1) * V // 6) for i in range(5)]
        m["joint_order"] = list(MANO_JOINT_ORDER)
        m["scale"] = 1000.0
    m["checksum"] = body_checksum(m)
    return m


# A standing figure in a 288 x 384 crop: x, y of the 17 COCO joints (nose, eyes, ears, shoulders, elbows, wrists, hips, knees,
# ankles; left first) - the pose of the sample-noise tests and of tools/sample_throughput.py
COCO_STANDING_POSE = ((144, 60), (150, 54), (138, 54), (158, 58), (130, 58), (175, 100), (113, 100), (190, 150), (98, 150),
                      (196, 195), (92, 195), (164, 205), (124, 205), (166, 275), (122, 275), (168, 345), (120, 345))
