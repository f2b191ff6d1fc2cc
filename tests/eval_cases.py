"""Seeded case tables shared by tests/test_eval_edges_cpu.py (the float64 audit of the tables themselves) and
tests/test_gpu_eval_edges.py (the kernels of csrc/eval.hip and the solve of csrc/p2m_eval.h).

Alignment cases sit on the launch edges of k_rigid_align (one wave per set up to N = 256, four sets per block; one block
per set above) and on the degenerate spectra of the solve.  Each is a batch [nb, N, 3] of fp32 pairs with a class:

  unique     the rotation is fixed well enough that eval_ref.batch_rigid's R, c, t, A2 are the yardstick (gap >= 1e-6, and
             the float64 reference itself moves by at most half a bar when every input moves by one fp32 ulp:
             tests/test_eval_edges_cpu.py)
  free       R or t is not fixed (gap exactly 0), or fixed so weakly that one input ulp moves the reference's R by more than
             its bar (gap <= FREE_GAP_MAX, or data far from the origin): c, the residual and R's orthogonality are
             compared, and A2 where it is unique (collinear A)
  nonfinite  the sets listed in `bad` have varP = 0 or hold a NaN / inf: their c, t, A2 are non-finite; the other sets of the
             batch meet the `unique` bars

Evaluator cases exercise the joint-fill loops, the stage-E wave and the roots of k_mesh_eval; totals cases the fold."""
import numpy as np

ALIGN_N = (3, 63, 64, 65, 255, 256, 257, 600)
UNIQUE_GAP_MIN = 1e-6
FREE_GAP_MAX = 1e-2
BAR_MM = 2e-4
COORD_MAX = 2000.0


def _rot(rng):
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def _similar(A, rng, noise=8.0, scale=None, shift=250.0):
    """B = c Q A + t + noise per set of A [nb, N, 3] (float64)."""
    B = np.empty_like(A)
    for i in range(A.shape[0]):
        c = rng.uniform(0.8, 1.2) if scale is None else scale
        B[i] = c * A[i] @ _rot(rng).T + rng.uniform(-shift, shift, 3) + noise * rng.standard_normal(A[i].shape)
    return B


def _generic(rng, nb, N):
    return rng.uniform(-600, 600, (nb, N, 3)) + rng.uniform(-150, 150, (nb, 1, 3))


def _triangles(rng, nb):
    """Three points fix a rotation only through their triangle: near-equilateral ones of side ~ 1000 about the origin."""
    a = np.deg2rad(np.array([0.0, 120.0, 240.0]))
    T = np.stack([np.cos(a), np.sin(a), np.zeros(3)], axis=1) * 600.0
    return np.stack([T @ _rot(rng).T + rng.uniform(-40, 40, (3, 3)) for _ in range(nb)])


def _case(name, cls, A, B, **kw):
    d = dict(name=name, cls=cls, A=np.ascontiguousarray(A, dtype=np.float32), B=np.ascontiguousarray(B, dtype=np.float32),
             compare_R=True, a2_unique=False, bad=(), big=False)
    d.update(kw)
    return d


def _cube(e):
    return np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * (e / 2)


def _planar(rng, nb, N):
    A = _generic(rng, nb, N)
    A[:, :, 2] = 0.3 * A[:, :, 0] - 0.5 * A[:, :, 1]
    return A


def _line(rng, nb, N):
    """Exactly collinear sets: integer multiples of one integer direction from an integer origin (exact in fp32)."""
    out = np.empty((nb, N, 3))
    for i in range(nb):
        d = np.array([[3.0, -2.0, 6.0], [1.0, 4.0, -8.0], [-7.0, 4.0, 4.0]][i % 3])
        k = rng.permutation(np.arange(-100, 101))[:N] if N <= 201 else rng.integers(-100, 101, N)
        out[i] = rng.integers(-200, 200, 3).astype(np.float64) + k[:, None] * d
    return out


def _build_align():
    rng = np.random.default_rng(20260)
    cases = []
    # -- unique ------------------------------------------------------------------------------------------------------------
    for N in ALIGN_N:                                           # lanes idle / just filled, the dispatch boundary 256 / 257
        A = _generic(rng, 4, N) if N > 3 else _triangles(rng, 4)
        cases.append(_case(f"generic{N}", "unique", A, _similar(A, rng)))
    for nb in (2, 3, 5, 7):                                     # the wave kernel's last block: 2, 3, 1, 3 sets of 4
        A = _generic(rng, nb, 17)
        cases.append(_case(f"tail17_nb{nb}", "unique", A, _similar(A, rng)))
    A = _generic(rng, 3, 257)
    cases.append(_case("tail257_nb3", "unique", A, _similar(A, rng)))
    for N in (17, 257):
        A = _generic(rng, 2, N)
        cases.append(_case(f"identical{N}", "unique", A, A.copy()))
        A = np.round(_generic(rng, 2, N))
        cases.append(_case(f"translation{N}", "unique", A, A + np.array([250.0, -125.0, 500.0])))
        A = _generic(rng, 3, N).astype(np.float32).astype(np.float64)          # exact 180 degree turns about x, y, z
        B = A.copy()
        for ax in range(3):
            B[ax, :, (ax + 1) % 3] *= -1.0
            B[ax, :, (ax + 2) % 3] *= -1.0
        cases.append(_case(f"turn180_{N}", "unique", A, B))
        A = np.round(_generic(rng, 2, N) / 2.0)                                  # integers: B = 2 P A + t exactly
        P = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
        P2 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        B = np.stack([2.0 * A[0] @ P.T + np.array([100.0, -200.0, 300.0]), 2.0 * A[1] @ P2.T - np.array([64.0, 0.0, 1.0])])
        cases.append(_case(f"integer_similarity{N}", "unique", A, B))
    for N in (64, 257):
        A = _generic(rng, 3, N) * np.array([1.0, 0.55, 0.25])                    # (s2 well above s3: the gap is 2 (s2 - s3) / s1)
        B = _similar(A, rng)
        B[:, :, 1] *= -1.0
        cases.append(_case(f"mirrored{N}", "unique", A, B))
        A = _planar(rng, 3, N)
        cases.append(_case(f"planarA{N}", "unique", A, _similar(A, rng)))
        A = _planar(rng, 3, N)
        cases.append(_case(f"planar_both{N}", "unique", A, _similar(A, rng, noise=0.0)))
        A = _planar(rng, 3, N)
        B = _similar(A, rng)
        B[:, :, 0] *= -1.0
        cases.append(_case(f"planar_mirrored{N}", "unique", A, B))
        A = _generic(rng, 3, N) * 1e-9
        cases.append(_case(f"scaled1e-9_{N}", "unique", A, _similar(A, rng, noise=8e-9, shift=250e-9)))
        A = _generic(rng, 3, N)                                                  # H = 0: c = 0, A2 = cB; R is arbitrary
        B = np.broadcast_to(rng.uniform(-900, 900, (3, 1, 3)), A.shape).copy()
        cases.append(_case(f"constantB{N}", "unique", A, B, compare_R=False))
    # -- free --------------------------------------------------------------------------------------------------------------
    for N in (17, 257):
        A = _line(rng, 3, N)
        cases.append(_case(f"collinearA{N}", "free", A, _similar(A, rng, noise=5.0), a2_unique=True))
        A, B = _line(rng, 3, N), _line(rng, 3, N)[::-1]
        cases.append(_case(f"collinear_both{N}", "free", A, B, a2_unique=True))
        cases.append(_case(f"collinearB{N}", "free", _generic(rng, 3, N), _line(rng, 3, N)))
        # nearly collinear A (off-line spread 1e-4 of the length): gap ~ 1e-4, one input ulp turns R about the line by ~ 1e-4
        A = _line(rng, 3, N) + 0.15 * rng.standard_normal((3, N, 3))
        cases.append(_case(f"near_collinearA{N}", "free", A, _similar(A, rng, noise=0.0), a2_unique=True))
        # 1e6 from the origin, spread 300: an input ulp is 1/16 mm, which moves the reference's R by ~ 1e-5
        A = 300.0 * rng.standard_normal((3, N, 3)) + 1e6
        cases.append(_case(f"offset1e6_{N}", "free", A, _similar(A - 1e6, rng, shift=50.0) + 1e6, big=True))
    A = _generic(rng, 7, 2)
    cases.append(_case("two_points", "free", A, _similar(A, rng), a2_unique=True))
    A = np.stack([_cube(1000.0) for _ in range(3)])             # mirrored cube: s1 = s2 = s3, det H < 0
    B = np.stack([1.1 * (A[i] * np.array([-1.0, 1.0, 1.0])) @ _rot(rng).T + rng.uniform(-100, 100, 3) for i in range(3)])
    B[0] = A[0] * np.array([1.0, 1.0, -1.0])                    # (one of them exactly, integers throughout)
    cases.append(_case("mirrored_cube", "free", A, B))
    A = np.stack([_cube(1000.0) + rng.standard_normal((8, 3)) for _ in range(3)])      # vertex noise 1e-3 of the edge
    B = np.stack([0.9 * (A[i] * np.array([1.0, -1.0, 1.0])) @ _rot(rng).T + rng.uniform(-100, 100, 3) for i in range(3)])
    cases.append(_case("near_mirrored_cube", "free", A, B))
    # -- nonfinite -----------------------------------------------------------------------------------------------------------
    A = _generic(rng, 5, 1)
    cases.append(_case("one_point", "nonfinite", A, _similar(A, rng), bad=(0, 1, 2, 3, 4)))
    for nb, N in ((7, 17), (3, 257)):
        for kind in ("coincident", "nan", "inf"):
            A = _generic(rng, nb, N)
            B = _similar(A, rng)
            if kind == "coincident":
                A[1] = A[1, :1]
            elif kind == "nan":
                A[1, N // 2, 1] = np.nan
            else:
                B[1, N - 1, 2] = np.inf
            cases.append(_case(f"{kind}_{nb}x{N}", "nonfinite", A, B, bad=(1,)))
    return cases


_align = None
_align_ref = {}


def align_cases():
    global _align
    if _align is None:
        _align = _build_align()
    return _align


def align_case(name):
    return next(c for c in align_cases() if c["name"] == name)


def align_names(cls=None):
    return [c["name"] for c in align_cases() if cls is None or c["cls"] == cls]


def align_reference(name):
    """eval_ref.batch_rigid and eval_ref.optimum of a case, computed once per session and shared (callers must not modify
    them): dict c, R, t, A2, copt [nb], rms [nb]."""
    import eval_ref
    if name not in _align_ref:
        k = align_case(name)
        nb, N = k["A"].shape[:2]
        r = dict(c=np.full(nb, np.nan), R=np.full((nb, 3, 3), np.nan), t=np.full((nb, 3), np.nan),
                 A2=np.full((nb, N, 3), np.nan), copt=np.full(nb, np.nan), rms=np.full(nb, np.nan))
        for i in range(nb):
            if i in k["bad"]:                                  # (non-finite by definition; numpy's SVD refuses a NaN)
                continue
            c, R, t, A2 = eval_ref.batch_rigid(k["A"][i:i + 1], k["B"][i:i + 1])
            r["c"][i], r["R"][i], r["t"][i], r["A2"][i] = c[0], R[0], t[0], A2[0]
            r["copt"][i], r["rms"][i] = eval_ref.optimum(k["A"][i], k["B"][i])
        _align_ref[name] = r
    return _align_ref[name]


# ---- evaluator cases -----------------------------------------------------------------------------------------------------
EVAL_B = 5


def meshes(B, nv, seed, in_m=False):
    """mm meshes within +-2000: gt a box cloud of a body's extent turned per sample, about 0.9 m out; pred a perturbed similarity
    of it.  fp32 pred, gt (gt in metres if in_m)."""
    rng = np.random.default_rng(seed)
    body = rng.uniform(-1, 1, (nv, 3)) * np.array([200.0, 600.0, 150.0])
    gt = body[None] @ np.stack([_rot(rng) for _ in range(B)]).transpose(0, 2, 1)
    gt += rng.uniform(-300, 300, (B, 1, 3)) + np.array([0.0, 0.0, 900.0])
    pred = gt * rng.uniform(0.95, 1.05, (B, 1, 1)) + rng.uniform(-60, 60, (B, 1, 3)) + rng.standard_normal(gt.shape) * 15
    assert np.abs(pred).max() <= COORD_MAX and np.abs(gt).max() <= COORD_MAX
    return pred.astype(np.float32), (gt / 1000.0 if in_m else gt).astype(np.float32)


def _sub(n, J, seed, without=None):
    """n joint indices in [0, J), seeded; with repeats once n > J; `without` is left out."""
    rng = np.random.default_rng(seed)
    pool = [j for j in range(J) if j != without]
    if n <= len(pool):
        return [int(j) for j in rng.permutation(pool)[:n]]
    return [int(j) for j in rng.permutation(pool)] + [int(j) for j in rng.choice(pool, n - len(pool))]


def _ecase(name, nv, JA, root_A, JE, root_E, sub_A=None, sub_E=None, pa_mesh=True, in_m=False, reg_A=True,
           given="", shift=0.0, seed=0):
    return dict(name=name, nv=nv, JA=JA, root_A=root_A, JE=JE, root_E=root_E, sub_A=sub_A, sub_E=sub_E, pa_mesh=pa_mesh,
                in_m=in_m, reg_A=reg_A, given=given, shift=shift, seed=seed)


EVAL_CASES = [
    # 1: both joint-fill loops at their largest (2 * 64 * 3 = 384 entries: two trips), the stage-E wave full
    _ecase("full64", 600, 64, 63, 64, 37, in_m=True, seed=1),
    # 2: the first size with a second trip (2 * 43 * 3 = 258 > 256) beside the last without (2 * 42 * 3 = 252)
    _ecase("trip43_42", 63, 43, 42, 42, 1, seed=2),
    # 3: subsets longer than the joint count, with repeats
    _ecase("long_subsets", 257, 17, 5, 5, 4, sub_A=_sub(64, 17, 31), sub_E=_sub(64, 5, 33), seed=3),
    # 4: the stage-E wave nearly empty; the subsets leave root_E out
    _ecase("subE1", 256, 17, 2, 21, 20, sub_E=_sub(1, 21, 41, without=20), seed=4),
    _ecase("subE2", 256, 17, 2, 21, 20, sub_E=_sub(2, 21, 42, without=20), seed=4),
    _ecase("subE3", 256, 17, 2, 21, 20, sub_E=_sub(3, 21, 43, without=20), seed=4),
    # 5: no stage-A regressor, both joint sets given
    _ecase("given_A64", 63, 64, 50, 21, 7, reg_A=False, given="PA", seed=5),
    # 6: annotation joints 10 m from the mesh frame
    _ecase("shifted_gt_joints", 600, 24, 11, 17, 6, given="AE", shift=10240.0, seed=6),
    _ecase("unshifted_gt_joints", 600, 24, 11, 17, 6, given="AE", shift=0.0, seed=6),
    # 7: the mesh passes with fewer vertices than threads, a full block, one over
    _ecase("nv6", 6, 3, 2, 4, 1, seed=7),
    _ecase("nv256", 256, 21, 20, 21, 9, seed=8),
    _ecase("nv257", 257, 24, 1, 17, 16, in_m=True, seed=9),
    # 8: the roots as a discriminator: the same data with the roots exchanged
    _ecase("roots_3_9", 63, 17, 3, 17, 9, seed=10),
    _ecase("roots_9_3", 63, 17, 9, 17, 3, seed=10),
]

_eval_inputs = {}
_eval_ref = {}


def eval_case(name):
    return next(c for c in EVAL_CASES if c["name"] == name)


def eval_inputs(name):
    """The arrays of an evaluator case: pred, gt (fp32 [B, nv, 3]), scale, RA / RE (dense fp32 regressors; RA is None without
    reg_A), pja / gja / gje (given fp32 joints or None)."""
    from pose2mesh_release_amd import synth
    if name in _eval_inputs:
        return _eval_inputs[name]
    k = eval_case(name)
    B, nv = EVAL_B, k["nv"]
    pred, gt = meshes(B, nv, 700 + k["seed"], k["in_m"])
    scale = 1000.0 if k["in_m"] else 1.0
    RA = synth.synthetic_regressor(k["JA"], nv, seed=100 + k["seed"])
    RE = synth.synthetic_regressor(k["JE"], nv, seed=200 + k["seed"])
    rng = np.random.default_rng(900 + k["seed"])
    gt_mm = gt.astype(np.float64) * scale

    def joints(R, m, sigma):
        j = np.einsum("jv,bvk->bjk", R.astype(np.float64), m) + rng.standard_normal((B, R.shape[0], 3)) * sigma
        return np.round(j * 1024.0) / 1024.0                   # multiples of 2^-10 mm: + 10240 stays exact in fp32
    pja = joints(RA, pred.astype(np.float64), 2.0).astype(np.float32) if "P" in k["given"] else None
    gja = (joints(RA, gt_mm, 5.0) + k["shift"]).astype(np.float32) if "A" in k["given"] else None
    gje = (joints(RE, gt_mm, 5.0) - k["shift"]).astype(np.float32) if "E" in k["given"] else None
    _eval_inputs[name] = dict(pred=pred, gt=gt, scale=scale, RA=RA if k["reg_A"] else None, RE=RE, pja=pja, gja=gja, gje=gje)
    return _eval_inputs[name]


def eval_reference(name):
    """eval_ref.mesh_eval of an evaluator case, once per session (callers must not modify it)."""
    import eval_ref
    if name not in _eval_ref:
        k, z = eval_case(name), eval_inputs(name)
        with np.errstate(all="ignore"):
            _eval_ref[name] = eval_ref.mesh_eval(z["pred"], z["gt"], z["RA"], k["root_A"], k["sub_A"], z["RE"], k["root_E"],
                                                 k["sub_E"], k["pa_mesh"], z["scale"], pred_joints_A=z["pja"],
                                                 gt_joints_A=z["gja"], gt_joints_E=z["gje"])
    return _eval_ref[name]


def sample_means(per_sample):
    """[B, 5] per-sample means in eval_ref.EVAL_KEYS order (the kernel's sample_means; 0 for a metric not computed)."""
    import eval_ref
    B = len(per_sample["mpvpe"])
    out = np.zeros((B, 5))
    for i, k in enumerate(eval_ref.EVAL_KEYS):
        if k in per_sample:
            v = per_sample[k]
            with np.errstate(all="ignore"):
                out[:, i] = v.mean(axis=1) if v.ndim == 2 else v
    return out


# ---- totals cases ----------------------------------------------------------------------------------------------------------
TOTALS_N_GROUPS = (0, 41, 42, 100)
TOTALS_CALLS = ((5, 5), (3, 3), (5, 0))             # (B, B_real) of three calls into one evaluator; the last is all padding
TOTALS_NV, TOTALS_J, TOTALS_ROOT_A, TOTALS_ROOT_E = 63, 17, 4, 12
INT32_MAX = 2 ** 31 - 1


def totals_groups(n_groups):
    """Group ids of the three calls: out-of-range ids (-1, n_groups, 2^31 - 1) beside valid ones, the highest valid among
    them; the padding call's ids are valid (they must not count)."""
    hi = n_groups - 1
    if n_groups == 0:
        return [[-1, 0, INT32_MAX, 1, -1], [0, INT32_MAX, -7], [0, 0, 0, 0, 0]]
    return [[hi, -1, 0, n_groups, hi], [INT32_MAX, hi, min(1, hi)], [0, hi, 0, hi, 0]]


def totals_inputs():
    """[(pred, gt)] of the three calls (the last: NaN meshes) and the two regressors."""
    from pose2mesh_release_amd import synth
    calls = []
    for i, (B, B_real) in enumerate(TOTALS_CALLS):
        pred, gt = meshes(B, TOTALS_NV, 800 + i)
        if B_real == 0:
            pred[:], gt[:] = np.nan, np.nan
        calls.append((pred, gt))
    return calls, synth.synthetic_regressor(TOTALS_J, TOTALS_NV, seed=61), synth.synthetic_regressor(TOTALS_J, TOTALS_NV, seed=62)
