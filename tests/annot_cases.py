"""Seeded cases of the annotation tests (tests/test_annot_cpu.py, tests/test_gpu_annot.py): annotation tables, a batch of row
indices and the flag set of a preset.  Tables of N >= 8 rows carry the special rows below at fixed indices; every B = 37
batch draws all of them, the first and the last row, and repeats.

  row 0  an all-zero root pose (the reference's 0 / 0; here the identity)
  row 1  a root angle beyond pi
  row 2  a root chosen so that the angle of R . exp(root) is within 1e-4 of pi
  row 3  root (pi, 0, 0) with R = I: the exactly-pi case (PI_ROW), whose axis sign is undefined
  row 4  a root angle of 1e-7
  row 5  betas with one entry at exactly 3.0: no reset
  row 6  betas with one entry one fp32 step above 3.0: reset
  row 7  a gender equal to G (status bit 1) where the table has genders, else an ordinary row"""
import functools

import numpy as np

import annot_ref
from pose2mesh_release_amd import annot, body, synth

PI_ROW, N_SPECIAL = 3, 8
JR = 17
SHAPES = {"smpl": (24, 10), "mano": (16, 10)}
# (preset, kind, N, B, G): every preset at the full batch on a gender bank, then the small tables and batches
CASES = [(p, "smpl", 1000, 37, 3) for p in annot.PRESETS] + [
    ("human36m", "mano", 1000, 37, 3), ("human36m", "smpl", 1, 1, 1), ("human36m", "smpl", 1000, 5, 1),
    ("amass", "mano", 1000, 5, 1), ("freihand", "mano", 1, 5, 3), ("freihand", "mano", 1000, 37, 1), ("pw3d", "smpl", 1000, 1, 3),
    ("muco", "smpl", 1, 37, 1)]


def case_ids():
    return ["-".join(str(x) for x in c) for c in CASES]


@functools.lru_cache(maxsize=None)
def model_dicts(kind, V, G):
    return tuple(synth.body_model(kind, V, seed=s) for s in range(G))


def body_model(m, extra_reg=None):
    return body.BodyModel(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["weights"], m["parents"],
                          betas=m["betas"], hands_mean=m.get("hands_mean"), tip_vertices=m.get("tip_vertices"),
                          joint_order=m.get("joint_order"), scale=m.get("scale", 1.0), extra_regressor=extra_reg)


@functools.lru_cache(maxsize=None)
def bank(kind, V, G, with_extra=False):
    reg = synth.synthetic_regressor(JR, V, seed=7) if with_extra else None
    return annot.GenderedBody([body_model(m, reg) for m in model_dicts(kind, V, G)])


def random_rotations(rng, n):
    v = rng.standard_normal((n, 3))
    v *= (rng.uniform(0.05, 3.1, (n, 1)) / np.linalg.norm(v, axis=1, keepdims=True))
    return np.stack([annot_ref.exp_root(x) for x in v])


def tables(kind, N, G, seed, with_trans=True, with_R=True, with_given=True):
    """dict of fp32 tables (uint8 gender), None where a table is left out."""
    J, nb = SHAPES[kind]
    rng = np.random.default_rng([seed, N, G, J])
    f4 = np.float32
    pose = (rng.standard_normal((N, J, 3)) * 0.6).reshape(N, -1).astype(f4)
    betas = rng.standard_normal((N, nb)).astype(f4)
    R = random_rotations(rng, N).astype(f4)
    gender = rng.integers(0, G, N).astype(np.uint8)
    if N >= N_SPECIAL:
        pose[0, :3] = 0.0
        d = rng.standard_normal(3)
        pose[1, :3] = (d / np.linalg.norm(d) * 3.7).astype(f4)
        ax = rng.standard_normal(3)
        target = annot_ref.exp_root(ax / np.linalg.norm(ax) * (np.pi - 5e-5))
        pose[2, :3] = annot_ref.log_rot(R[2].astype(np.float64).T @ target).astype(f4)
        pose[PI_ROW, :3] = (np.pi, 0.0, 0.0)
        R[PI_ROW] = np.eye(3, dtype=f4)
        d = rng.standard_normal(3)
        pose[4, :3] = (d / np.linalg.norm(d) * 1e-7).astype(f4)
        betas[5] = (rng.standard_normal(nb) * 0.5).clip(-2, 2)
        betas[5, 3] = 3.0
        betas[6] = (rng.standard_normal(nb) * 0.5).clip(-2, 2)
        betas[6, nb - 1] = -np.nextafter(f4(3.0), f4(4.0))
        gender[7] = G
    t = {"pose": pose, "betas": betas, "cam_R": R.reshape(N, 9) if with_R else None,
         "trans": (rng.standard_normal((N, 3)) * [0.5, 0.5, 0.3] + [0, 0, 1.0]).astype(f4) if with_trans else None,
         "cam_t": (rng.standard_normal((N, 3)) * [400, 400, 600] + [0, 0, 4000]).astype(f4),
         "focal": rng.uniform(1000, 1500, (N, 2)).astype(f4), "princpt": rng.uniform(400, 600, (N, 2)).astype(f4),
         "gender": gender if G > 1 else None,
         "given_cam": (rng.standard_normal((N, JR, 3)) * 300).astype(f4) if with_given else None,
         "given_img": rng.uniform(0, 1000, (N, JR, 2)).astype(f4) if with_given else None}
    if N >= N_SPECIAL and with_R:
        assert abs(np.linalg.norm(annot_ref.log_rot(R[2].astype(np.float64) @ annot_ref.exp_root(pose[2, :3]))) - np.pi) < 1e-4
    return t


def batch_indices(N, B, seed):
    rng = np.random.default_rng([seed, N, B])
    if N < N_SPECIAL:
        return rng.integers(0, N, B).astype(np.int64)
    lead = list(range(N_SPECIAL)) + [N - 1, 0, 5]           # the specials, the last row, repeats of the first and of row 5
    if B >= len(lead):
        return np.concatenate([lead, rng.integers(0, N, B - len(lead))]).astype(np.int64)
    return np.asarray(([0, N - 1, 2, 2, 6] * B)[:B] if B > 1 else [N - 1], np.int64)


@functools.lru_cache(maxsize=None)
def case(i):
    """dict: preset, kind, N, B, G, flags, tables, idx (int64 numpy), root_template, root_shapedirs (fp32; of a V = 31 bank)."""
    preset, kind, N, B, G = CASES[i]
    flags = dict(annot.PRESETS[preset])
    amass_like = preset in ("amass", "freihand")
    t = tables(kind, N, G, seed=100 + i, with_trans=not amass_like, with_R=preset not in ("pw3d", "surreal", "muco", "coco"),
               with_given=kind == "smpl")
    if t["cam_R"] is None:
        t["cam_t"] = None                                  # the camera-frame datasets: trans as annotated
    if amass_like:
        t["cam_t"] = (t["cam_t"] / 1000).astype(np.float32)  # metres
    rt, rs = bank(kind, 31, G).root_tables()
    return dict(preset=preset, kind=kind, N=N, B=B, G=G, flags=flags, tables=t, idx=batch_indices(N, B, seed=i),
                root_template=rt, root_shapedirs=rs)


@functools.lru_cache(maxsize=None)
def chain_case(kind, V):
    """The Human3.6M case of `kind` (N = 1000, B = 37, G = 3) for a run through the body models: the root tables of the V-vertex
    bank, and world / camera translations drawn so that the camera-frame translation has the spread (0.7 per axis) of the
    batch that sets the forward's error bar in tests/test_gpu_body.py - a translation of metres would add its own fp32
    rounding to every vertex, which that bar does not cover."""
    c = dict(case(CASES.index(("human36m", kind, 1000, 37, 3))))
    rng = np.random.default_rng([9, V])
    t = dict(c["tables"])
    t["trans"] = (rng.standard_normal((c["N"], 3)) * 0.3).astype(np.float32)
    t["cam_t"] = (rng.standard_normal((c["N"], 3)) * 600).astype(np.float32)
    c["tables"] = t
    c["root_template"], c["root_shapedirs"] = bank(kind, V, 3, True).root_tables()
    return c


def reference(c, idx=None):
    return annot_ref.gather(c["tables"], c["idx"] if idx is None else idx, c["G"], c["root_template"], c["root_shapedirs"],
                            **c["flags"])
