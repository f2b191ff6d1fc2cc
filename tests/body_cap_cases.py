"""Seeded general body models and the case table of tests/test_gpu_body_caps.py, shared with its CPU audit
(tests/test_body_caps_cpu.py).  synth.body_model makes SMPL- and MANO-shaped models only (J in {16, 24}, nb = 10); the
kernels advertise J <= 64, K = nb + 9 (J - 1) <= 640, 64 tips and 64 extra joints and size LDS and loops from those caps.
model() is synth.body_model's recipe for any (J, nb, V, tree); CASES names one model per loop pass, chunk edge, cap and
jslot / regressor shape that no SMPL- or MANO-shaped model reaches.  The audit asserts that each case reaches the arm it names.
"""
import functools

import numpy as np

B = 9                                                   # one sample tile plus one
TREES = ("tree", "chain", "star")


@functools.lru_cache(maxsize=None)
def model(J, nb, V, tree="tree", seed=0):
    """A dict as body_ref.forward / body_grad_ref.forward take it: template points on a squashed sphere, shape directions
    0.01 N(0,1), pose directions 0.002 N(0,1), min(12, V)-sparse J_regressor rows and min(4, J)-sparse skinning rows that
    sum to 1, stored betas 0.1 N(0,1); tree: random parents[j] < j, "chain" parents[j] = j - 1, "star" all parents 0."""
    if tree not in TREES:
        raise ValueError(f"tree: one of {TREES}, got {tree!r}")
    rng = np.random.default_rng([int(seed), J, nb, V, TREES.index(tree)])
    p = rng.standard_normal((V, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    v_template = p * np.array([0.3, 0.9, 0.2])
    shapedirs = rng.standard_normal((V, 3, nb)) * 0.01
    posedirs = rng.standard_normal((V, 3, 9 * (J - 1))) * 0.002
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
    if tree == "chain":
        parents = [-1] + list(range(J - 1))
    elif tree == "star":
        parents = [-1] + [0] * (J - 1)
    else:
        parents = [-1] + [int(rng.integers(0, j)) for j in range(1, J)]
    f32 = np.float32
    return {"num_vertex": V, "v_template": v_template.astype(f32), "shapedirs": shapedirs.astype(f32),
            "posedirs": posedirs.astype(f32), "J_regressor": J_regressor.astype(f32), "weights": weights.astype(f32),
            "parents": parents, "betas": (rng.standard_normal(nb) * 0.1).astype(f32)}


def inputs(Bn, J, nb, seed):
    """_inputs of tests/test_gpu_body_grad.py for any nb: N(0, 0.6^2) poses, row 1 all zero and row 2 beyond pi (Bn >= 5),
    N(0,1) betas with one 3.5, 0.7 N(0,1) translations; fp32."""
    rng = np.random.default_rng([int(seed), 99])
    pose = rng.standard_normal((Bn, J, 3)) * 0.6
    if Bn >= 5:
        pose[1] = 0.0
        d = rng.standard_normal((J, 3))
        pose[2] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(3.0, 4.0, (J, 1))
    betas = rng.standard_normal((Bn, nb))
    if nb:
        betas[Bn - 1, 0] = 3.5
    trans = rng.standard_normal((Bn, 3)) * 0.7
    return [x.astype(np.float32) for x in (pose.reshape(Bn, -1), betas, trans)]


def sparse_rows(n, V, seed, k=6):
    """[n, V] fp32, min(k, V) random entries per row that sum to 1 (synth.synthetic_regressor's recipe for any V)."""
    rng = np.random.default_rng([int(seed), 7])
    R = np.zeros((n, V), np.float32)
    for j in range(n):
        w = rng.random(min(k, V)).astype(np.float32)
        R[j, rng.choice(V, size=min(k, V), replace=False)] = w / w.sum()
    return R


def _cap_outputs_tables(V):
    rng = np.random.default_rng(640)
    tips = [V - 1, 0, 5, 5] + [int(t) for t in rng.integers(0, V, 60)]     # the last vertex, the first, a repeated one
    order = [int(o) for o in rng.permutation(128)]
    R = sparse_rows(64, V, 641)
    R[:, 77] = 0.125                                                        # one vertex in every row ...
    R[10] = 0.0                                                             # ... but the empty one
    w = rng.random(V).astype(np.float32) + 0.05
    R[20] = w / w.sum()                                                     # a row over all V vertices
    return tips, order, R


def _reg_rows(V):
    R = np.zeros((4, V), np.float32)                                        # row 0 stays empty
    R[1, V - 1] = 1.0                                                       # a single entry, on the last vertex
    w = np.random.default_rng(650).random(V).astype(np.float32) + 0.05
    R[2] = w / w.sum()                                                      # over all V vertices
    R[3, [3, 17, 40]] = (0.8, -0.3, 0.5)                                    # a negative weight
    return R


def _col64(V):
    R = sparse_rows(64, V, 660, k=5)
    R[:, 7] = 0.25                                                          # vertex 7 in all 64 rows: the longest column
    return R


# name -> model arguments, output options and the runs of the case.  A run is (label, betas, trans, center_idx): betas is
# "given" ([B, nb] input), "stored" (betas=None); trans True adds a translation, False centres on center_idx (or does nothing).
def _case(J, nb, V, tree="tree", seed=1, tips=None, order=None, extra=None, runs=(("", "given", True, None),), Bn=B):
    return dict(J=J, nb=nb, V=V, tree=tree, seed=seed, tips=tips, order=order, extra=extra, runs=runs, B=Bn)


def _build():
    t, o, r = _cap_outputs_tables(130)
    rng = np.random.default_rng(22)
    tips22 = [int(x) for x in rng.integers(0, 65, 22)]
    return {
        "cap_both": _case(64, 73, 130, seed=11),
        "cap_chain": _case(64, 73, 130, "chain", seed=12, runs=(("", "given", False, 63),)),
        "cap_shape": _case(2, 631, 65, seed=13),
        "cap_outputs": _case(64, 73, 130, seed=14, tips=t, order=o, extra=r),
        "fold_1024": _case(48, 13, 65, seed=15),
        "fold_1025": _case(48, 14, 65, seed=16),
        "coef_192": _case(2, 183, 65, seed=17),
        "coef_193": _case(2, 184, 65, seed=18),
        "j1": _case(1, 5, 65, seed=19),
        "k1": _case(1, 1, 1, seed=20),
        "j7": _case(7, 3, 65, seed=21),
        "j8": _case(8, 1, 65, seed=22),
        "drop_joints": _case(24, 10, 65, seed=23, tips=[64, 9], order=[5, 24, 0, 23, 25],
                             runs=(("c3", "given", False, 3), ("c0", "given", False, 0))),
        "tips_only": _case(24, 10, 65, seed=24, tips=[64, 0, 31], order=[24, 25, 26]),
        "tail_22": _case(16, 10, 65, seed=25, tips=tips22, extra=sparse_rows(22, 65, 26)),
        "reg_zero": _case(24, 10, 65, seed=27, extra=np.zeros((5, 65), np.float32)),
        "reg_rows": _case(24, 10, 65, seed=28, extra=_reg_rows(65)),
        "col_64": _case(2, 10, 65, seed=29, extra=_col64(65)),
        "nb0": _case(2, 0, 65, seed=30, runs=(("given", "given", True, None), ("stored", "stored", True, None))),
    }


CASES = _build()
NAMES = tuple(CASES)
COMPANION = {"k1": (1, 1, 65)}                          # V = 1: bars from a V = 65 model of the same (J, nb)


def run_ids():
    return [(n, r[0]) for n in NAMES for r in CASES[n]["runs"]]


def case_model(name, companion=False):
    """The model dict of a case, with its tips and joint order (what body_ref / body_grad_ref read)."""
    c = CASES[name]
    J, nb, V = COMPANION[name] if companion else (c["J"], c["nb"], c["V"])
    m = dict(model(J, nb, V, c["tree"], c["seed"]))
    if c["tips"] is not None:
        m["tip_vertices"] = list(c["tips"])
    if c["order"] is not None:
        m["joint_order"] = list(c["order"])
    return m


def n_joints_out(name):
    c = CASES[name]
    return len(c["order"]) if c["order"] is not None else c["J"] + len(c["tips"] or ())


def run(name, label, companion=False):
    """dict of one run: model, pose, betas (None: stored), trans (None: centred / nothing), center_idx, extra_reg."""
    c = CASES[name]
    _, mode, with_trans, center = next(r for r in c["runs"] if r[0] == label)
    m = case_model(name, companion)
    pose, betas, trans = inputs(c["B"], c["J"], c["nb"], c["seed"])
    return {"model": m, "pose": pose, "betas": betas if mode == "given" else None, "trans": trans if with_trans else None,
            "center_idx": center, "extra_reg": None if companion else c["extra"]}


def vanishing_pose_gradient_scale(name, g64):
    """None for every case but the one-vertex, one-joint model.  There the only joint is regressed from the only vertex with
    weight 1, so the vertex IS the joint, verts = R (x - J) + J = J whatever the pose, and the pose gradient is identically
    zero: a row error relative to |g64| = 0 is undefined.  Its error is taken relative to what cancels in it instead - per
    sample, |upstream force| |x|: the moment of the summed output gradient (= g_trans) at the vertex's distance from the
    origin, the size of each of the two terms R x and R J whose difference is the zero lever arm.  g64: the float64
    gradients (pose, betas, trans) of the run."""
    c = CASES[name]
    if (c["J"], c["V"]) != (1, 1):
        return None
    x = np.asarray(case_model(name)["v_template"], np.float64)
    return np.linalg.norm(g64[2], axis=1) * np.linalg.norm(x[0])


def row_sum_bound(reg):
    """Largest absolute row sum of a regressor: what an error of the vertices can grow by in extra = reg @ verts."""
    return float(np.abs(np.asarray(reg, np.float64)).sum(axis=1).max())


# ---- the kernels' arithmetic, restated (csrc/p2m_body.h, body.hip, body_bwd.hip) --------------------------------------------------
VT, NT, TB, JMAX, KMAX = 64, 192, 8, 64, 640            # p2m_body.h: BODY_VT, BODY_NT = 3 BODY_VT, BODY_TB, BODY_JMAX, BODY_KMAX
FOLD_THREADS = 1024                                     # body_bwd.hip: BODY_BWD_PT
SROW = NT + 4                                           # body_bwd.hip: BODY_BWD_SROW


def n_coef(J, nb):
    return nb + 9 * (J - 1)                             # body.hip p2m_body_forward: K = nb + 9 * (J - 1)


def kpad(K):
    return (K + 3) // 4 * 4                             # body.hip k_body_skin: kpad = ((K + 3) / 4) * 4


def skin_lds(J, K):
    # body.hip body_skin_lds: sizeof(float) * (kpad * BODY_TB + BODY_TB * 12 * J + BODY_TB * BODY_NT + BODY_TB * 4)
    return 4 * (kpad(K) * TB + TB * 12 * J + TB * NT + TB * 4)


def jp8(J):
    return (J + 8) // 8 * 8                             # body_bwd.hip body_bwd_jp8: J + 1 rows, padded to 8


def bwd_lds(J, K):
    r1 = max(kpad(K) * TB, VT * (jp8(J) + 4))           # body_bwd.hip body_bwd_r1: coefficient rows, then the weight tile
    r2 = max(TB * 12 * J, NT * TB)                      # body_bwd.hip body_bwd_r2: A matrices, then g_x
    return 4 * (r1 + r2 + 3 * TB * SROW)                # body_bwd.hip body_bwd_lds: + v_posed (float64) and gv


def n_fold(J, K):
    return 12 * (J + 1) + K                             # body_bwd.hip k_body_bwd_pose: nfold = nA + K, nA = 12 * (J + 1)


def passes(n, step):
    """Trips of `for (i = tid; i < n; i += step)` that some thread of the block makes."""
    return -(-n // step)


def n_chunks(J):
    return jp8(J) // 8                                  # body_bwd.hip k_body_bwd_vertex: nch = body_bwd_jp8(J) / 8


def jslot(name):
    """body.py BodyModel.__init__: output slot of chain joint j, -1 where joint_order drops it."""
    c = CASES[name]
    order = c["order"] if c["order"] is not None else range(c["J"] + len(c["tips"] or ()))
    s = np.full(c["J"], -1, np.int64)
    for slot, src in enumerate(order):
        if src < c["J"]:
            s[src] = slot
    return s
