"""-m gpu: every arm of the BatchNorm / ReLU / residual family (csrc/bn.hip) against the float64 restatement tests/bn_ref.py.

Two input regimes (generators below; tests/test_bn_ref_cpu.py checks their conditions without a GPU):

  exact     small integers and dyadic coefficients: every product and every partial sum, in any order, is an fp32 number, so
            the kernels must EQUAL the float64 reference (tolerance 0).  The test asserts the headroom from the reference
            before it touches the GPU (sum |g m yhat| in units of 1/2 below 2^24 per column).
  rounding  seeded real data, gamma of both signs with one exact zero, coefficients self-consistent but given.  No float64
            pre-activation lies within 1e-3 of 0 except the planted exact zeros, so the reference has no kink inside the
            margin and NO element is left out of any comparison.  Bounds are those of test_bn_relu_residual_fwd_bwd:
              x <= 1e-5;  gy <= 2e-5 max(1, max|ref|);  dgamma, dbeta <= 1e-5 max(1, max|ref|) sqrt(M);  transpose <= 1e-5.
            Resize pairs whose ratio is no power of two use the "f32"-weight reference and gain the weight-error term
            4 * 2^-24 * Fres * |r[i1] - r[i0]| per element (src <= Fres carries at most three fp32 roundings, w = src - i0 is
            exact; the fourth unit covers a contracted multiply-subtract); the transpose gains the same term summed over
            the contributing |g[j]|.  pair_gx is one fp32 addition of exact inputs (2^-24 |ref|), pair_gy two gy errors plus
            that addition.

Cases per family (each arm at the smallest shapes at which it can go wrong):

  family                      arms / widths                                    rows                                  modes
  forward                     k_bn_act_fwd 4 32 128 256 1024                   1, R/4-1, R/4+1, R-1, R, R+1, 2R+R/4+1   relu 0/1, co / None,
                              k_bn_act_fwd_v4 12 36 96 200                     1 7 64 65                              no / same (shift 0,1) /
                              k_bn_act_fwd_generic 3 5 17 33 257               1 86 1000                              resized residual
  resize pairs Fres->F        64->256 256->128 32->64 96->64 128->48 3->32 100->36 32->5   (forward and p2m_lerp_bwd_add, M 1 3 257)
  reduce + finalize           templates 32 64 128 256, generic 3 36 96 512     1 2 63 64 65 127 129 1000              relu 0/1, accumulate 0/1
                              32, 36 (exact)                                   262080 262144 262145 (rows/block 64 -> 128, splits 48 -> 96)
                              32 (exact, int64 reference on the GPU)           2097151 2097152 (rows/block 512)
  finalize alone              3 32 33 200 256                                  nblk 1 47 48 49 4095 4096 16383 16384 20000
  apply                       the same widths                                  1 2 255 256 257 4RP-1 4RP+1            train / eval, relu 0/1
  apply, pairs                templates                                        2 254 256 258 4RP-2 4RP+2              pair_in / pair_out / both
  row maps                    band graph V = 736 (B = 3) and a tiny level V = 32 (B = 50: one pass wraps several samples);
                              forward classes / real rows, reduce classes, reduce fake, apply and pairs apply with and
                              without zero_holes, pair_sum classes, class_reduce, stats_rows_w; widths 4 32 256 and 36
  eval coefficients           N 1 3 256 257, running_var 0 1e-12 1 1e6, gamma of both signs and zero: 2 ulp
  chain                       finalize / eval coefficients -> forward -> backward -> transpose against torch float64 autograd at
                              F = 36, F = 5, relu = 0, mixed-sign gamma, odd M with res_shift = 1
  refusals                    pairs with odd M, pairs with F = 36, amax_out with F % 4 != 0, res_shift = 2, real_rows_only
                              without a handle

Worst observed figure as a fraction of its bound (one run on an MI355X, 78 tests in 4.9 s; nothing was tightened on its
strength; the exact-regime comparisons have no figure: they are equalities):
  forward x 0.164          apply gy 0.006           reduce dbeta 0.005       reduce dgamma 0.010
  pair_gx 1.000 (half an ulp of a sum that is one fp32 addition: the bound is that rounding)    pair_gy 0.003
  resize transpose 0.115   class_reduce 0.273       stats_rows_w 0.193       finalize coef (1 ulp) 0.499
  eval coeffs (2 ulp) 0.798                         chain x 0.263            chain gy 0.005
  chain dgamma 0.001       chain dbeta 0.001        chain transpose 0.251

k_bn_bwd_reduce<8> (F = 32) reaches the fourth row of a pass only with 128 or more rows per block, that is from 262,145 rows
on: the small shapes cannot see that row, the cases at the rows-per-block switch do.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import bn_ref

pytestmark = pytest.mark.gpu

TEMPLATE_F = (32, 64, 128, 256)
GENERIC_F = (3, 36, 96, 512)
MAIN_F = (4, 32, 128, 256, 1024)
V4_F = (12, 36, 96, 200)
SCALAR_F = (3, 5, 17, 33, 257)
RESIZE_PAIRS = ((64, 256), (256, 128), (32, 64), (96, 64), (128, 48), (3, 32), (100, 36), (32, 5))      # (Fres, F)
GAMMAS = (-2.0, -1.0, 0.0, 0.5, 1.0, 4.0)
INVSTDS = (0.5, 1.0, 2.0)
MARGIN = 1e-3
CHAIN_MARGIN = 1e-5
SENTINEL = 12345.0
WORST = {}            # family -> worst observed error / bound (printed at the end of the module's run)


EXTRA_FWD_F = (64, 48)           # widths that only the resize pairs bring (64: k_bn_act_fwd, 48: k_bn_act_fwd_v4)


def main_arm(F):
    return F % 4 == 0 and F // 4 <= 256 and 256 % (F // 4) == 0


def fwd_rows(F):
    if main_arm(F):
        R = 16384 // F
        return sorted({1, max(1, R // 4 - 1), R // 4 + 1, R - 1, R, R + 1, 2 * R + R // 4 + 1})
    return [1, 7, 64, 65] if F % 4 == 0 else [1, 86, 1000]


def apply_rows(F, pairs=False):
    RP = max(1, 1024 // F)
    if pairs:
        return sorted({2, 254, 256, 258, max(2, 4 * RP - 2), 4 * RP + 2})
    return sorted({1, 2, 255, 256, 257, max(1, 4 * RP - 1), 4 * RP + 1})


def dyadic_ratio(Fres, F):
    a, b = Fres, F
    while a % 2 == 0 and b % 2 == 0:
        a, b = a // 2, b // 2
    return (a == 1 or b == 1) and (a & (a - 1)) == 0 and (b & (b - 1)) == 0


# ---- input generators (numpy, CPU) --------------------------------------------------------------------------------
def exact_coeffs(F, seed):
    """dyadic coefficient block: integer mean and beta, invstd in {0.5, 1, 2}, gamma in GAMMAS (each of them present when F
    allows), scale = gamma invstd, shift = beta - mean scale; a third of the columns have beta = 0, so y = mean is a
    pre-activation of exactly 0 there"""
    rng = np.random.default_rng([seed, F, 1])
    mean = rng.integers(-1, 2, F).astype(np.float64)
    invstd = rng.choice(INVSTDS, F)
    gamma = rng.permutation(np.resize(np.array(GAMMAS), F))
    beta = rng.integers(-2, 3, F).astype(np.float64)
    beta[rng.permutation(F)[:(F + 2) // 3]] = 0.0
    scale = gamma * invstd
    co = np.stack([mean, invstd, scale, beta - mean * scale]).astype(np.float32)
    return co, gamma.astype(np.float32), beta.astype(np.float32)


def exact_case(M, F, seed):
    """y, gx integers in [-4, 4]; where beta = 0 about one entry in eight is set to y = mean (pre-activation exactly 0) with a
    non-zero gradient, so `<= 0` and `< 0` in a mask give different sums"""
    co, gamma, beta = exact_coeffs(F, seed)
    rng = np.random.default_rng([seed, M, F, 2])
    y = rng.integers(-4, 5, (M, F)).astype(np.float32)
    gx = rng.integers(-4, 5, (M, F)).astype(np.float32)
    plant = (rng.random((M, F)) < 0.125) & (beta == 0)[None, :]
    y = np.where(plant, co[0][None, :], y).astype(np.float32)
    gx = np.where(plant, np.float32(3.0), gx).astype(np.float32)
    return {"y": y, "gx": gx, "co": co, "gamma": gamma, "beta": beta, "planted": plant}


def rounding_case(M, F, seed):
    """randn * 2 + 0.5; gamma of both signs, column z with gamma = 0 and shift = 0 (the whole column sits at 0), column p with
    shift = 0 and y = 0 planted (exactly 0 too); every other pre-activation is redrawn until |y scale + shift| >= MARGIN"""
    rng = np.random.default_rng([seed, M, F, 3])
    y = (rng.standard_normal((M, F)) * 2 + 0.5).astype(np.float32)
    gx = rng.standard_normal((M, F)).astype(np.float32)
    gamma = (rng.standard_normal(F) * 0.8).astype(np.float32)
    gamma[np.abs(gamma) < 0.05] = np.float32(0.3)
    beta = (rng.standard_normal(F) * 0.2).astype(np.float32)
    mean = (rng.standard_normal(F) * 0.3 + 0.5).astype(np.float32)
    invstd = (1.0 / np.sqrt(rng.random(F) + 0.5)).astype(np.float32)
    z, p = int(rng.integers(F)), None
    if F >= 3:                                         # both signs, whatever the draw
        gamma[(z + 1) % F], gamma[(z + 2) % F] = abs(gamma[(z + 1) % F]), -abs(gamma[(z + 2) % F])
    gamma[z] = 0.0
    beta[z] = 0.0
    scale = (gamma * invstd).astype(np.float32)
    shift = (beta - mean * scale).astype(np.float32)
    planted = np.zeros((M, F), dtype=bool)
    planted[:, z] = True
    if F > 1:
        p = int((z + 1 + rng.integers(F - 1)) % F)
        beta[p] = mean[p] * scale[p]                 # shift = beta - mean scale = 0
        shift[p] = 0.0
        rows = rng.random(M) < 0.25
        y[rows, p] = 0.0
        planted[rows, p] = True
    co = np.stack([mean, invstd, scale, shift]).astype(np.float32)
    for _ in range(64):
        bad = (np.abs(bn_ref.preact(y, co)) < MARGIN) & ~planted
        if not bad.any():
            break
        y[bad] = (rng.standard_normal(int(bad.sum())) * 2 + 0.5).astype(np.float32)
    else:
        raise AssertionError("rounding_case: could not clear the margin")
    return {"y": y, "gx": gx, "co": co, "gamma": gamma, "beta": beta, "planted": planted}


def make_case(regime, M, F, seed):
    return exact_case(M, F, seed) if regime == "exact" else rounding_case(M, F, seed)


def residual_rows(regime, rows, Fres, seed):
    rng = np.random.default_rng([seed, rows, Fres, 4])
    if regime == "exact":
        return rng.integers(-4, 5, (rows, Fres)).astype(np.float32)
    return rng.standard_normal((rows, Fres)).astype(np.float32)


def exact_headroom(gx, y, co, relu, init=0.0):
    """largest sum over the rows of |g m| and of |g m yhat| per column, in units of 1/2 (the finest quantum of yhat): every
    partial sum in any order is an fp32 number while this stays below 2^24"""
    gm = np.abs(bn_ref.f64(gx)) * bn_ref.mask(y, co, relu)
    yhat = np.abs((bn_ref.f64(y) - bn_ref.f64(co)[0]) * bn_ref.f64(co)[1])
    return 2.0 * (max(gm.sum(0).max(), (gm * yhat).sum(0).max()) + abs(init))


def is_dyadic_block(co, gamma, beta):
    co, gamma, beta = bn_ref.f64(co), bn_ref.f64(gamma), bn_ref.f64(beta)
    return bool((co[0] == np.round(co[0])).all() and np.isin(co[1], INVSTDS).all() and np.isin(gamma, GAMMAS).all()
                and (beta == np.round(beta)).all() and (co[2] == gamma * co[1]).all()
                and (co[3] == beta - co[0] * co[2]).all())


# ---- graphs of the row-map tests (CPU part) ------------------------------------------------------------------------------
def band_graph(V, seed, fake_frac=0.4):
    """tests/test_gpu_ops.py::_band_graph: ring + two chords over the real vertices, isolated fake vertices anywhere"""
    nreal = max(8, int(V * (1 - fake_frac)))
    i = np.arange(nreal)
    rows = np.concatenate([i, (i + 1) % nreal, i, (i + 5) % nreal, i, (i + 17) % nreal])
    cols = np.concatenate([(i + 1) % nreal, i, (i + 5) % nreal, i, (i + 17) % nreal, i])
    A = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(V, V)).tocsr()
    A.data[:] = 1.0
    d = np.asarray(A.sum(axis=0)).ravel() + np.spacing(np.float64(0))
    Dm = sp.diags(1 / np.sqrt(d))
    L = (sp.identity(V) - Dm @ A @ Dm) / 3.0 - sp.identity(V)
    perm = np.random.default_rng(seed).permutation(V)
    return L.tocsr()[perm][:, perm].tocsr()


def real_ids_of(L):
    L = L.tocsr()
    deg = np.diff(L.indptr)
    return np.where(~((deg == 1) & (L.indices[L.indptr[:-1].clip(max=L.nnz - 1)] == np.arange(L.shape[0]))))[0]


ROWMAP_GRAPHS = {"band736": (736, 77, 0.55, 3), "tiny32": (32, 5, 0.7, 50)}          # V, seed, fake_frac, B


def rowmap_level(name):
    """(L, tables) of a row-map test level, all of it computed on the CPU: rep_of, w, live ids, live pairs, fake
    representatives and their weights, real ids"""
    from pose2mesh_release_amd.ops import class_representatives
    V, seed, frac, B = ROWMAP_GRAPHS[name]
    L = band_graph(V, seed, frac)
    real = real_ids_of(L)
    fake = np.setdiff1d(np.arange(V), real)
    rep, fmask = class_representatives(V, fake, 3)
    w = bn_ref.class_weights(rep)
    reps = fake[rep[fake] == fake]
    t = {"V": V, "B": B, "rep": rep, "w": w, "real": real, "fake": fake, "live": np.nonzero(w)[0], "reps": reps,
         "rep_w": w[reps], "live_pairs": np.nonzero((w[0::2] != 0) | (w[1::2] != 0))[0]}
    return L, t


# ---- chain cases ------------------------------------------------------------------------------------------------------
CHAIN_CASES = [  # M, F, Fres, res_shift, training, relu, seed
    (1000, 36, 100, 0, True, True, 1),
    (999, 5, 32, 1, True, True, 2),
    (777, 64, 64, 0, False, False, 3),
    (641, 128, 256, 1, True, False, 20),
    (500, 36, 36, 1, False, True, 5),
]


def chain_inputs(M, Fd, Fres, rshift, seed):
    gen = torch.Generator().manual_seed(1000 * seed + M)
    y = torch.randn(M, Fd, generator=gen) * 2 + 0.5
    gamma = torch.randn(Fd, generator=gen) * 0.8                     # both signs
    gamma[gamma.abs() < 0.05] = 0.3
    beta = torch.randn(Fd, generator=gen) * 0.2
    rm, rv = torch.randn(Fd, generator=gen) * 0.1, torch.rand(Fd, generator=gen) + 0.5
    resid = torch.randn((M + 1) >> 1 if rshift else M, Fres, generator=gen)
    gx = torch.randn(M, Fd, generator=gen)
    return y, gamma, beta, rm, rv, resid, gx


def chain_reference(y, gamma, beta, rm, rv, resid, gx, rshift, training, relu):
    """torch float64 autograd of batch_norm + relu + interpolate + repeat_interleave; also the float64 pre-activation"""
    import torch.nn.functional as Fn
    M, Fd = y.shape
    Fres = resid.shape[1]
    yd = y.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rmd, rvd = rm.double().clone(), rv.double().clone()
    rd = resid.double().requires_grad_(True)
    pre = Fn.batch_norm(yd, rmd, rvd, gd, bd, training, 0.1, 1e-5)
    o = Fn.relu(pre) if relu else pre
    rfull = rd.repeat_interleave(1 << rshift, 0)[:M]
    o = o + (Fn.interpolate(rfull.unsqueeze(0), size=Fd, mode="linear").squeeze(0) if Fres != Fd else rfull)
    o.backward(gx.double())
    return {"x": o.detach(), "gy": yd.grad, "dgamma": gd.grad, "dbeta": bd.grad, "dres": rd.grad, "pre": pre.detach(),
            "rm": rmd, "rv": rvd}


# ---- GPU plumbing --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops(hip_libs):
    from pose2mesh_release_amd import ops as o
    yield o
    for fam in sorted(WORST):
        print(f"test_gpu_bn worst error / bound, {fam}: {WORST[fam]:.3f}")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _lib():
    from pose2mesh_release_amd import _lib as L
    return L


def record(family, err, bound):
    """err, bound: float64 arrays (or scalars) of the same shape; every element takes part"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.isfinite(err).all(), family
    frac = float(np.max(err / bound)) if err.size else 0.0
    WORST[family] = max(WORST.get(family, 0.0), frac)
    return frac


def check_close(family, got, ref, bound, what):
    frac = record(family, np.abs(host(got) - ref) if hasattr(got, "cpu") else np.abs(got - ref), bound)
    assert frac <= 1.0, f"{what}: error / bound = {frac}"


def check_equal(got, ref, what):
    got = host(got) if hasattr(got, "cpu") else got
    bad = got != ref
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[bad][0]!r} != {ref[bad][0]!r}"


def act_fwd(y, co, relu, resid, Fres, rs, M, F, x=None, cls=None, real_only=0, amax=None):
    """raw p2m_bn_act_fwd; returns (status, x)"""
    if x is None:
        x = torch.full((M, F), SENTINEL, device="cuda")
    rc = _lib().hip().p2m_bn_act_fwd(_p(y), _p(None if co is None else co[2]), _p(None if co is None else co[3]), int(relu),
                                     _p(resid), int(Fres), int(rs), _p(x), M, F, cls, int(real_only), _p(amax), None)
    return rc, x


def bwd_reduce(gx, y, co, relu, M, F, cls=None):
    lib = _lib().hip()
    nblk = int(lib.p2m_bn_bwd_blocks(M, F) if cls is None else lib.p2m_bn_bwd_blocks_classes(cls, M, F))
    assert nblk > 0
    part = torch.full((nblk, 2, F), float("nan"), device="cuda")
    _lib().check(lib.p2m_bn_bwd_reduce(_p(gx), _p(y), _p(co[2]), _p(co[3]), _p(co[0]), _p(co[1]), int(relu), _p(part), M, F,
                                       cls, None), "p2m_bn_bwd_reduce")
    return part


def bwd_finalize(part, M, F, dgamma=None, dbeta=None, accumulate=0):
    if dgamma is None:
        dgamma, dbeta = torch.full((F,), SENTINEL, device="cuda"), torch.full((F,), SENTINEL, device="cuda")
    coef = torch.full((2, F), SENTINEL, device="cuda")
    _lib().check(_lib().hip().p2m_bn_bwd_finalize(_p(part), part.shape[0], M, _p(dgamma), _p(dbeta), _p(coef), int(accumulate),
                                                  F, None), "p2m_bn_bwd_finalize")
    return dgamma, dbeta, coef


def bwd_apply(gx, y, co, gamma, coef, relu, M, F, pair_in=False, pair_out=False, cls=None, zero_holes=0, gy=None, pgx=None,
              pgy=None):
    """raw p2m_bn_bwd_apply; returns (status, gy, pair_gx, pair_gy); the outputs come pre-filled with SENTINEL"""
    if gy is None:
        gy = torch.full((M, F), SENTINEL, device="cuda")
    if pair_in and pgx is None:
        pgx = torch.full((M // 2, F), SENTINEL, device="cuda")
    if pair_out and pgy is None:
        pgy = torch.full((M // 2, F), SENTINEL, device="cuda")
    rc = _lib().hip().p2m_bn_bwd_apply(_p(gx), _p(y), _p(co[2]), _p(co[3]), _p(co[0]), _p(co[1]), _p(gamma), _p(coef), int(relu),
                                       _p(gy), _p(pgx), _p(pgy), M, F, cls, int(zero_holes), None, None)
    return rc, gy, pgx, pgy


def gy_bound(ref):
    return 2e-5 * max(1.0, float(np.abs(ref).max()))


def sums_bound(ref, M):
    return 1e-5 * max(1.0, float(np.abs(ref).max())) * np.sqrt(M)


# ---- forward, no graph -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", MAIN_F + V4_F + SCALAR_F + EXTRA_FWD_F)
def test_forward(ops, F):
    """x = relu(y scale + shift) + resize(resid[r >> res_shift]) on the arm the width selects: exact regime equal to float64
    (no, same-width or 2:1 residual), rounding regime to 1e-5 (+ the weight term of a non-dyadic resize)."""
    rows = fwd_rows(F)
    Mmax = max(rows)
    pairs = [Fres for Fres, Fd in RESIZE_PAIRS if Fd == F]
    for regime in ("exact", "rounding"):
        c = make_case(regime, Mmax, F, 11)
        yc, coc = dev(c["y"]), dev(c["co"])
        resids = {Fres: residual_rows(regime, Mmax, Fres, 12) for Fres in [F] + pairs}
        resids_c = {k: dev(v) for k, v in resids.items()}
        for M in rows:
            for relu in (0, 1):
                for with_co in (True, False):
                    variants = [(None, 0, 0), (F, F, 0), (F, F, 1)] + [(Fres, Fres, rs) for Fres in pairs for rs in (0, 1)]
                    for key, Fres, rs in variants:
                        what = f"forward {regime} F={F} M={M} relu={relu} co={with_co} Fres={Fres} res_shift={rs}"
                        rr = None if key is None else resids[key][:(M + 1) >> rs if rs else M]
                        rc = None if key is None else resids_c[key][:rr.shape[0]]
                        status, x = act_fwd(yc[:M], coc if with_co else None, relu, rc, Fres, rs, M, F)
                        assert status == 0, what
                        dy = key is None or Fres == F or dyadic_ratio(Fres, F)
                        ref = bn_ref.act_fwd(c["y"][:M], c["co"] if with_co else None, relu, rr, Fres, rs,
                                             "f64" if dy else "f32")
                        if regime == "exact" and (key is None or Fres == F or Fres == 2 * F):
                            check_equal(x, ref, what)
                            continue
                        bound = np.full(ref.shape, 1e-5)
                        if not dy:
                            bound += 4 * 2.0 ** -24 * Fres * bn_ref.resize_weight_term(rr[np.arange(M) >> rs], F)
                        check_close("forward x", x, ref, bound, what)


# ---- reduce + finalize, no graph -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", TEMPLATE_F + GENERIC_F)
def test_reduce_and_finalize(ops, F):
    """dbeta = sum g m, dgamma = sum g m yhat through p2m_bn_bwd_reduce + p2m_bn_bwd_finalize, overwrite and accumulate."""
    rows = (1, 2, 63, 64, 65, 127, 129, 1000)
    for regime in ("exact", "rounding"):
        c = make_case(regime, max(rows), F, 21)
        gc, yc, coc = dev(c["gx"]), dev(c["y"]), dev(c["co"])
        init_g = np.arange(F, dtype=np.float64) % 7 - 3
        init_b = 5 - np.arange(F, dtype=np.float64) % 11
        for M in rows:
            for relu in (0, 1):
                what = f"reduce+finalize {regime} F={F} M={M} relu={relu}"
                db, dg = bn_ref.bwd_sums(c["gx"][:M], c["y"][:M], c["co"], relu)
                if regime == "exact":
                    assert exact_headroom(c["gx"][:M], c["y"][:M], c["co"], relu, 8.0) < 2.0 ** 24, what
                part = bwd_reduce(gc[:M], yc[:M], coc, relu, M, F)
                assert torch.isfinite(part).all(), what
                for acc in (0, 1):
                    dgo, dbo = dev(init_g), dev(init_b)
                    dgo, dbo, coef = bwd_finalize(part, M, F, dgo, dbo, acc)
                    rg, rb = dg + acc * init_g, db + acc * init_b
                    if regime == "exact":
                        check_equal(dbo, rb, what + f" dbeta accumulate={acc}")
                        check_equal(dgo, rg, what + f" dgamma accumulate={acc}")
                        check_close("finalize coef (ulp)", coef, np.stack([db, dg]) / M, bn_ref.ulp32(np.stack([db, dg]) / M),
                                    what + " coef")
                    else:
                        check_close("reduce dbeta", dbo, rb, sums_bound(rb, M), what + f" dbeta accumulate={acc}")
                        check_close("reduce dgamma", dgo, rg, sums_bound(rg, M), what + f" dgamma accumulate={acc}")


def _exact_big(M, F, seed, lim):
    """exact-regime rows built on the GPU: y, gx integers in [-lim, lim]; the reference sums in int64 (units of 1/4 for the
    pre-activation, of 1/2 for yhat)"""
    co, gamma, beta = exact_coeffs(F, seed)
    if lim < 4:                                   # |yhat| <= lim: mean 0, invstd <= 1
        co[0] = 0.0
        co[1] = np.minimum(co[1], 1.0)
        co[2] = gamma * co[1]
        co[3] = beta
    gen = torch.Generator(device="cuda").manual_seed(seed)
    y = torch.randint(-lim, lim + 1, (M, F), generator=gen, device="cuda")
    g = torch.randint(-lim, lim + 1, (M, F), generator=gen, device="cuda")
    return co, y, g


def _int_sums(y, g, co, relu, M):
    """(dbeta, dgamma, headroom) of the first M rows, in int64 on the GPU"""
    c64 = torch.from_numpy(co.astype(np.float64)).cuda()
    sc4, sh4 = (c64[2] * 4).round().long(), (c64[3] * 4).round().long()
    assert torch.equal(sc4.double() / 4, c64[2]) and torch.equal(sh4.double() / 4, c64[3])
    yh2 = (y[:M] - c64[0].long()) * (c64[1] * 2).round().long()                  # 2 yhat
    gm = g[:M] * ((y[:M] * sc4 + sh4) > 0).long() if relu else g[:M]
    head = max(int(gm.abs().sum(0).max()) * 2, int((gm * yh2).abs().sum(0).max()))
    return gm.sum(0).double().cpu().numpy(), (gm * yh2).sum(0).double().cpu().numpy() / 2, head


@pytest.mark.parametrize("F", [32, 36])
def test_reduce_at_the_rows_per_block_switch(ops, F):
    """262,080 / 262,144 rows: 64 rows per block, 4,095 / 4,096 partial rows (48 / 96 finalize splits); 262,145 rows: 128 rows
    per block.  Exact regime: one dropped or doubled row anywhere changes the sums."""
    lib = _lib().hip()
    assert [int(lib.p2m_bn_bwd_blocks(M, F)) for M in (262080, 262144, 262145)] == [4095, 4096, 2049]
    co, y, g = _exact_big(262145, F, 31, 4)
    yf, gf, coc = y.float(), g.float(), dev(co)
    for M in (262080, 262144, 262145):
        for relu in (0, 1):
            db, dg, head = _int_sums(y, g, co, relu, M)
            assert head < 2 ** 24
            dgo, dbo, coef = bwd_finalize(bwd_reduce(gf[:M], yf[:M], coc, relu, M, F), M, F)
            check_equal(dbo, db, f"dbeta F={F} M={M} relu={relu}")
            check_equal(dgo, dg, f"dgamma F={F} M={M} relu={relu}")


def test_reduce_at_512_rows_per_block(ops):
    """2,097,151 rows: 512-row rounding of the small-M rule (4,096 blocks); 2,097,152 rows: the fixed 512 (4,096 blocks of
    whole rows).  |g|, |yhat| <= 2; inputs and int64 reference on the GPU."""
    F = 32
    lib = _lib().hip()
    assert [int(lib.p2m_bn_bwd_blocks(M, F)) for M in (2097151, 2097152)] == [4096, 4096]
    co, y, g = _exact_big(2097152, F, 41, 2)
    yf, gf, coc = y.float(), g.float(), dev(co)
    for M in (2097151, 2097152):
        db, dg, head = _int_sums(y, g, co, 1, M)
        assert head < 2 ** 24
        dgo, dbo, coef = bwd_finalize(bwd_reduce(gf[:M], yf[:M], coc, 1, M, F), M, F)
        check_equal(dbo, db, f"dbeta M={M}")
        check_equal(dgo, dg, f"dgamma M={M}")


@pytest.mark.parametrize("F", [3, 32, 33, 200, 256])
def test_finalize_alone(ops, F):
    """p2m_bn_bwd_finalize over synthetic integer partials: dgamma, dbeta exact for every split count and a partial-row count
    on either side of each switch; coef within 1 ulp of t / M."""
    gen = torch.Generator(device="cuda").manual_seed(F)
    M = 1000003
    for nblk in (1, 47, 48, 49, 4095, 4096, 16383, 16384, 20000):
        part = torch.randint(-8, 9, (nblk, 2, F), generator=gen, device="cuda").float()
        t = part.double().sum(0).cpu().numpy()
        for acc in (0, 1):
            dgo, dbo, coef = bwd_finalize(part, M, F, dev(np.full(F, 3.0)), dev(np.full(F, -2.0)), acc)
            check_equal(dbo, t[0] - 2.0 * acc, f"finalize dbeta F={F} nblk={nblk} accumulate={acc}")
            check_equal(dgo, t[1] + 3.0 * acc, f"finalize dgamma F={F} nblk={nblk} accumulate={acc}")
            check_close("finalize coef (ulp)", coef, t / M, bn_ref.ulp32(t / M), f"finalize coef F={F} nblk={nblk}")
        dgo, dbo, coef = bwd_finalize(part, 1 << 20, F)
        check_equal(coef, t / (1 << 20), f"finalize coef at M = 2^20, F={F} nblk={nblk}")


# ---- apply -------------------------------------------------------------------------------------------------------------
def _coef_for(regime, F, seed):
    rng = np.random.default_rng([seed, F, 5])
    if regime == "exact":
        return (rng.integers(-4, 5, (2, F)) / 4.0).astype(np.float32)
    return (rng.standard_normal((2, F)) * 0.1).astype(np.float32)


@pytest.mark.parametrize("F", TEMPLATE_F + GENERIC_F)
def test_apply(ops, F):
    """gy = gamma invstd (g m - c0 - yhat c1) with coef given (train) or NULL (eval).  Exact regime: dyadic coef, equality."""
    rows = apply_rows(F)
    for regime in ("exact", "rounding"):
        c = make_case(regime, max(rows), F, 51)
        coef = _coef_for(regime, F, 52)
        gc, yc, coc, gac, cfc = dev(c["gx"]), dev(c["y"]), dev(c["co"]), dev(c["gamma"]), dev(coef)
        for M in rows:
            for relu in (0, 1):
                for train in (True, False):
                    what = f"apply {regime} F={F} M={M} relu={relu} train={train}"
                    ref = bn_ref.bwd_apply(c["gx"][:M], c["y"][:M], c["co"], c["gamma"], coef if train else None, relu)
                    status, gy, _, _ = bwd_apply(gc[:M], yc[:M], coc, gac, cfc if train else None, relu, M, F)
                    assert status == 0, what
                    if regime == "exact":
                        assert bn_ref.representable_f32(ref).all()
                        check_equal(gy, ref, what)
                    else:
                        check_close("apply gy", gy, ref, gy_bound(ref), what)


@pytest.mark.parametrize("F", TEMPLATE_F)
def test_apply_pairs(ops, F):
    """The pairs variant: gy bitwise the plain variant's, pair_gx = gx[2q] + gx[2q+1], pair_gy = gy[2q] + gy[2q+1], each
    by-product alone and both together."""
    rows = apply_rows(F, pairs=True)
    for regime in ("exact", "rounding"):
        c = make_case(regime, max(rows), F, 61)
        coef = _coef_for(regime, F, 62)
        gc, yc, coc, gac, cfc = dev(c["gx"]), dev(c["y"]), dev(c["co"]), dev(c["gamma"]), dev(coef)
        for M in rows:
            for relu, train in ((1, True), (0, True), (1, False)):
                ref = bn_ref.bwd_apply(c["gx"][:M], c["y"][:M], c["co"], c["gamma"], coef if train else None, relu)
                rpx, rpy = bn_ref.pair_sum(c["gx"][:M]), bn_ref.pair_sum(ref)
                _, gy0, _, _ = bwd_apply(gc[:M], yc[:M], coc, gac, cfc if train else None, relu, M, F)
                ps = ops.pair_sum(gc[:M], M // 2, F)
                for pin, pout in ((True, False), (False, True), (True, True)):
                    what = f"pairs {regime} F={F} M={M} relu={relu} train={train} pair_in={pin} pair_out={pout}"
                    status, gy, pgx, pgy = bwd_apply(gc[:M], yc[:M], coc, gac, cfc if train else None, relu, M, F, pin, pout)
                    assert status == 0, what
                    assert torch.equal(gy, gy0), what + ": gy differs from the plain variant"
                    if pin:
                        assert torch.equal(pgx, ps), what + ": pair_gx differs from p2m_pair_sum"
                    if regime == "exact":
                        check_equal(gy, ref, what)
                        if pin:
                            check_equal(pgx, rpx, what + " pair_gx")
                        if pout:
                            check_equal(pgy, rpy, what + " pair_gy")
                    else:
                        check_close("apply gy", gy, ref, gy_bound(ref), what)
                        if pin:
                            check_close("pair_gx", pgx, rpx, 2.0 ** -24 * np.abs(rpx) + 1e-30, what + " pair_gx")
                        if pout:
                            check_close("pair_gy", pgy, rpy, 2 * gy_bound(ref) + 2.0 ** -24 * np.abs(rpy), what + " pair_gy")


# ---- row maps ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(ROWMAP_GRAPHS))
def level(request, ops):
    L, t = rowmap_level(request.param)
    g = ops.DeviceGraph(L, "cuda:0")
    assert np.array_equal(np.sort(g.real_ids_host()), t["real"]) and np.array_equal(g.fake_ids_host(), t["fake"])
    g.set_classes(t["rep"])
    assert g.classes and np.array_equal(g.fake_ids_host(), t["reps"]) and g.n_fake_all == t["fake"].size
    return g, t


def _holed(a, live, fill=np.nan):
    a = np.array(a, dtype=np.float32)
    a[~live] = fill
    return a


def _check_rows(regime, family, got, ref, live, bound, what, holes=SENTINEL):
    """live rows against the reference (equal / within bound), holes bitwise `holes`"""
    got = host(got)
    if regime == "exact":
        check_equal(got[live], ref[live], what)
    else:
        check_close(family, got[live], ref[live], bound, what)
    assert (got[~live] == holes).all(), what + f": a hole does not hold {holes}"


@pytest.mark.parametrize("F", [4, 32, 256, 36])
@pytest.mark.parametrize("regime", ["exact", "rounding"])
def test_row_maps(ops, level, regime, F):
    """Every kernel that takes a row map, on a level with classes: holes of the inputs hold NaN, holes of the outputs keep a
    sentinel bit for bit (zeros with zero_holes), live rows against bn_ref's class forms."""
    g, t = level
    V, B, w = t["V"], t["B"], t["w"]
    M = B * V
    c = make_case(regime, M, F, 71)
    coef = _coef_for(regime, F, 72)
    live = np.tile(w != 0, B)
    wr = np.tile(w, B)
    is_real = np.zeros(V, dtype=bool)
    is_real[t["real"]] = True
    real_rows = np.tile(is_real, B)
    yh, gh = _holed(c["y"], live), _holed(c["gx"], live)
    yc, gc, coc, gac, cfc = dev(yh), dev(gh), dev(c["co"]), dev(c["gamma"]), dev(coef)
    lib = _lib().hip()
    tag = f"{regime} V={V} F={F}"
    # forward with classes / on the real rows only (the main kernel's widths)
    if main_arm(F):
        rs_rows = residual_rows(regime, M, F, 73)
        for relu in (0, 1):
            for resid in (None, rs_rows):
                rh = None if resid is None else dev(_holed(resid, live))
                status, x = act_fwd(yc, coc, relu, rh, F if resid is not None else 0, 0, M, F, cls=g.handle)
                assert status == 0
                ref, _ = bn_ref.act_fwd_classes(yh, c["co"], relu, w, resid, F if resid is not None else 0, 0)
                _check_rows(regime, "forward x", x, ref, live, 1e-5, f"forward classes {tag} relu={relu}")
                yr = _holed(c["y"], real_rows)
                rh = None if resid is None else dev(_holed(resid, real_rows))
                status, x = act_fwd(dev(yr), coc, relu, rh, F if resid is not None else 0, 0, M, F, cls=g.handle, real_only=1)
                assert status == 0
                ref = bn_ref.act_fwd(np.where(real_rows[:, None], c["y"], 0), c["co"], relu, resid,
                                     F if resid is not None else 0, 0)
                _check_rows(regime, "forward x", x, ref, real_rows, 1e-5, f"forward real rows {tag} relu={relu}")
    # reduce with classes
    Mlog = B * t["live"].size
    for relu in (0, 1):
        db, dg = bn_ref.bwd_sums_classes(gh, yh, c["co"], relu, w)
        if regime == "exact":
            assert exact_headroom(np.where(live[:, None], c["gx"], 0), np.where(live[:, None], c["y"], 0), c["co"], relu) < 2.0 ** 24
        part = bwd_reduce(gc, yc, coc, relu, M, F, cls=g.handle)
        assert part.shape[0] == int(lib.p2m_bn_bwd_blocks(Mlog, F)) and torch.isfinite(part).all()
        dgo, dbo, _ = bwd_finalize(part, M, F)
        if regime == "exact":
            check_equal(dbo, db, f"reduce classes dbeta {tag} relu={relu}")
            check_equal(dgo, dg, f"reduce classes dgamma {tag} relu={relu}")
        else:
            check_close("reduce dbeta", dbo, db, sums_bound(db, Mlog), f"reduce classes dbeta {tag}")
            check_close("reduce dgamma", dgo, dg, sums_bound(dg, Mlog), f"reduce classes dgamma {tag}")
        # the fake-vertex rows alone (the representatives)
        if F in TEMPLATE_F:
            rep_rows = np.zeros(V, dtype=bool)
            rep_rows[t["reps"]] = True
            rep_rows = np.tile(rep_rows, B)
            nb = int(lib.p2m_bn_bwd_blocks_fake(g.handle, B, F))
            assert nb == int(lib.p2m_bn_bwd_blocks(B * t["reps"].size, F)) and nb > 0
            pf = torch.full((nb, 2, F), float("nan"), device="cuda")
            _lib().check(lib.p2m_bn_bwd_reduce_fake(g.handle, _p(gc), _p(yc), _p(coc[2]), _p(coc[3]), _p(coc[0]), _p(coc[1]),
                                                    relu, _p(pf), B, F, None), "p2m_bn_bwd_reduce_fake")
            fb, fg = bn_ref.bwd_sums(np.where(rep_rows[:, None], c["gx"], 0), np.where(rep_rows[:, None], c["y"], 0), c["co"], relu)
            got = host(pf).sum(0)
            if regime == "exact":
                check_equal(got[0], fb, f"reduce fake dbeta {tag}")
                check_equal(got[1], fg, f"reduce fake dgamma {tag}")
            else:
                check_close("reduce dbeta", got[0], fb, sums_bound(fb, int(rep_rows.sum())), f"reduce fake dbeta {tag}")
                check_close("reduce dgamma", got[1], fg, sums_bound(fg, int(rep_rows.sum())), f"reduce fake dgamma {tag}")
    # apply, with and without zero_holes; the pairs variant
    for relu, train in ((1, True), (0, True), (1, False)):
        ref, _ = bn_ref.bwd_apply_classes(gh, yh, c["co"], c["gamma"], coef if train else None, relu, w)
        exact = regime == "exact"
        if exact:
            assert bn_ref.representable_f32(ref).all()
        for zh in (0, 1):
            what = f"apply classes {tag} relu={relu} train={train} zero_holes={zh}"
            status, gy, _, _ = bwd_apply(gc, yc, coc, gac, cfc if train else None, relu, M, F, cls=g.handle, zero_holes=zh)
            assert status == 0, what
            _check_rows(regime, "apply gy", gy, ref, live, gy_bound(ref), what, holes=0.0 if zh else SENTINEL)
            if F not in TEMPLATE_F:
                continue
            rpx, lp = bn_ref.pair_sum_classes(gh, w)
            rpy, _ = bn_ref.pair_sum_classes(np.where(live[:, None], ref, np.nan), w)
            status, gy2, pgx, pgy = bwd_apply(gc, yc, coc, gac, cfc if train else None, relu, M, F, True, True, cls=g.handle,
                                              zero_holes=zh)
            assert status == 0, what
            assert torch.equal(gy2, gy), what + ": gy of the pairs variant differs"
            _check_rows(regime, "pair_gx", pgx, rpx, lp, 2.0 ** -24 * np.abs(rpx[lp]) + 1e-30, what + " pair_gx",
                        holes=0.0 if zh else SENTINEL)
            _check_rows(regime, "pair_gy", pgy, rpy, lp, 2 * gy_bound(ref) + 2.0 ** -24 * np.abs(rpy[lp]), what + " pair_gy",
                        holes=0.0 if zh else SENTINEL)
    # p2m_pair_sum with classes (every pair is written; holes count as zeros)
    rp, _ = bn_ref.pair_sum_classes(gh, w)
    got = ops.pair_sum(gc, M // 2, F, classes=g)
    if regime == "exact":
        check_equal(got, rp, f"pair_sum classes {tag}")
    else:
        check_close("pair_gx", got, rp, 2.0 ** -24 * np.abs(rp) + 1e-30, f"pair_sum classes {tag}")
    # p2m_class_reduce (a full tensor in, class sums out, zeros at the holes)
    out = ops.class_reduce(g, dev(c["gx"]), B, F)
    rc = bn_ref.class_reduce(c["gx"], w)
    if regime == "exact":
        check_equal(out, rc, f"class_reduce {tag}")
    else:
        check_close("class_reduce", out, rc, 8 * 2.0 ** -24 * bn_ref.class_reduce(np.abs(c["gx"]), w) + 1e-30, f"class_reduce {tag}")
    # p2m_stats_rows_w (fp32 partials of double sums: one rounding; the float4 arm sums in fp32: n roundings)
    tps = -(-t["reps"].size // 128)
    st = torch.full((B * tps, 2, F), float("nan"), device="cuda")
    _lib().check(lib.p2m_stats_rows_w(g.handle, _p(yc), B, F, _p(st), None), "p2m_stats_rows_w")
    rst = bn_ref.stats_rows_w(np.where(live[:, None], c["y"], 0), t["reps"], t["rep_w"], B, V)
    got = host(st)
    if regime == "exact":
        check_equal(got[:, 0], rst[:, 0], f"stats_rows_w sums {tag}")
    n = min(128, t["reps"].size)
    ya = bn_ref.stats_rows_w(np.abs(np.where(live[:, None], c["y"], 0)), t["reps"], t["rep_w"], B, V)[:, 0]
    check_close("stats_rows_w", got[:, 0], rst[:, 0], (n + 2) * 2.0 ** -24 * ya + 1e-30, f"stats_rows_w sums {tag}")
    # M2 = sum w d^2 about the tile mean: the first-order effect of the mean's error delta cancels (sum w d = 0), what is left
    # is delta^2 W with delta <= (n + 4) 2^-24 sum w |y| / W, plus (n + 4) roundings of a sum of non-negative terms
    W = bn_ref.stats_rows_w(np.ones_like(c["y"], dtype=np.float64), t["reps"], t["rep_w"], B, V)[:, 0]
    m2b = (n + 4) * 2.0 ** -23 * rst[:, 1] + ((n + 4) * 2.0 ** -24 * ya) ** 2 / W + 1e-30
    check_close("stats_rows_w", got[:, 1], rst[:, 1], m2b, f"stats_rows_w M2 {tag}")


# ---- the resize transpose -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Fres,F", RESIZE_PAIRS)
def test_lerp_bwd_add(ops, Fres, F):
    """dst += W^T g with dst pre-filled; both kernels (Fres == 2 F: k_lerp_bwd_add_half)."""
    dy = dyadic_ratio(Fres, F)
    for regime in ("exact", "rounding"):
        for M in (1, 3, 257):
            what = f"lerp_bwd_add {regime} {Fres}->{F} M={M}"
            g = residual_rows(regime, M, F, 81)
            d0 = residual_rows(regime, M, Fres, 82)
            dst = dev(d0)
            ops.lerp_bwd_add(dev(g), dst, M, F, Fres)
            ref = d0.astype(np.float64) + bn_ref.lerp_transpose(g, F, Fres, "f64" if dy else "f32")
            if regime == "exact" and Fres == 2 * F:
                check_equal(dst, ref, what)
                continue
            bound = np.full(ref.shape, 1e-5)
            if not dy:
                bound += 4 * 2.0 ** -24 * Fres * bn_ref.lerp_transpose_weight_term(g, F, Fres)
            check_close("resize transpose", dst, ref, bound, what)


# ---- eval coefficients ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 256, 257])
def test_eval_coeffs(ops, N):
    """mean exact; invstd and scale within 2 ulp of float64; shift within 2 ulp (at the size of its terms) of
    beta - mean * scale with the scale that was stored."""
    rng = np.random.default_rng(N)
    for rv0 in (0.0, 1e-12, 1.0, 1e6):
        gamma = (rng.standard_normal(N) * 0.8).astype(np.float32)
        gamma[0] = 0.0
        beta = (rng.standard_normal(N) * 0.2).astype(np.float32)
        rm = (rng.standard_normal(N) * 0.3).astype(np.float32)
        rv = np.full(N, rv0, dtype=np.float32)
        if N > 2:
            rv[1:] *= (1 + rng.random(N - 1)).astype(np.float32)
        co = ops.bn_eval_coeffs(dev(gamma), dev(beta), dev(rm), dev(rv), 1e-5)
        got = host(co)
        ref = bn_ref.eval_coeffs(gamma, beta, rm, rv, 1e-5, scale_used=got[2])
        what = f"eval_coeffs N={N} running_var~{rv0}"
        check_equal(got[0], ref[0], what + " mean")
        check_close("eval coeffs (2 ulp)", got[1], ref[1], 2 * bn_ref.ulp32(ref[1]), what + " invstd")
        check_close("eval coeffs (2 ulp)", got[2], ref[2], 2 * bn_ref.ulp32(ref[2]) + 1e-45, what + " scale")
        size = np.abs(bn_ref.f64(beta)) + np.abs(bn_ref.f64(rm) * got[2])
        check_close("eval coeffs (2 ulp)", got[3], ref[3], 2 * bn_ref.ulp32(size) + 1e-45, what + " shift")


# ---- chain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,Fd,Fres,rshift,training,relu,seed", CHAIN_CASES)
def test_chain_against_autograd(ops, M, Fd, Fres, rshift, training, relu, seed):
    """bn_finalize / bn_eval_coeffs -> forward -> backward -> resize transpose against torch float64 autograd, at the widths
    and modes test_bn_relu_residual_fwd_bwd lacks; bounds are that test's (+ the weight term of a non-dyadic resize)."""
    y, gamma, beta, rm, rv, resid, gx = chain_inputs(M, Fd, Fres, rshift, seed)
    ref = chain_reference(y, gamma, beta, rm, rv, resid, gx, rshift, training, relu)
    assert int((ref["pre"].abs() < CHAIN_MARGIN).sum()) == 0
    yc = y.cuda()
    if training:
        tr = ops.stats_tile_rows()
        nt = (M + tr - 1) // tr
        st = torch.empty(nt, 2, Fd)
        for t in range(nt):
            blk = y[t * tr:(t + 1) * tr].double()
            st[t, 0] = blk.sum(0).float()
            st[t, 1] = ((blk - blk.mean(0)) ** 2).sum(0).float()
        rmc, rvc = rm.cuda(), rv.cuda()
        co = ops.bn_finalize(st.cuda(), M, gamma.cuda(), beta.cuda(), rmc, rvc, 0.1, 1e-5)
        assert (rmc.cpu() - ref["rm"]).abs().max() < 1e-6 and (rvc.cpu() - ref["rv"]).abs().max() < 1e-5
    else:
        co = ops.bn_eval_coeffs(gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), 1e-5)
    dy = Fres == Fd or dyadic_ratio(Fres, Fd)
    x = ops.bn_act_fwd(yc, co, relu, resid.cuda(), Fres, rshift, M, Fd)
    bound = np.full((M, Fd), 1e-5)
    if not dy:
        bound += 4 * 2.0 ** -24 * Fres * bn_ref.resize_weight_term(resid.numpy()[np.arange(M) >> rshift], Fd)
    check_close("chain x", x, ref["x"].numpy(), bound, "chain x")
    gy, dgamma, dbeta = ops.bn_relu_bwd(gx.cuda(), yc, co, gamma.cuda(), relu, training, M, Fd)
    check_close("chain gy", gy, ref["gy"].numpy(), gy_bound(ref["gy"].numpy()), "chain gy")
    check_close("chain dgamma", dgamma, ref["dgamma"].numpy(), sums_bound(ref["dgamma"].numpy(), M), "chain dgamma")
    check_close("chain dbeta", dbeta, ref["dbeta"].numpy(), sums_bound(ref["dbeta"].numpy(), M), "chain dbeta")
    # residual transpose; res_shift = 1 with an odd M: the last parent has one child
    G = gx.cuda()
    if rshift:
        Gs = ops.pair_sum(G, M // 2, Fd) if Fd % 4 == 0 else G[:M // 2 * 2].view(M // 2, 2, Fd).sum(1)
        if M % 2:
            Gs = torch.cat((Gs, G[M - 1:]), 0).contiguous()
    else:
        Gs = G
    Mr = Gs.shape[0]
    assert Mr == resid.shape[0]
    dst = torch.zeros(Mr, Fres, device="cuda")
    if Fres == Fd:
        dst += Gs
    else:
        ops.lerp_bwd_add(Gs, dst, Mr, Fd, Fres)
    bound = np.full((Mr, Fres), 1e-5)
    if not dy:
        bound += 4 * 2.0 ** -24 * Fres * bn_ref.lerp_transpose_weight_term(host(Gs), Fd, Fres)
    check_close("chain transpose", dst, ref["dres"].numpy(), bound, "chain residual gradient")


# ---- refusals (host-side argument checks: nothing is launched) ---------------------------------------------------------------
def test_argument_checks(ops):
    c = exact_case(6, 36, 91)
    gc, yc, coc, gac = dev(c["gx"]), dev(c["y"]), dev(c["co"]), dev(c["gamma"])
    c32 = exact_case(5, 32, 92)
    g32, y32, co32, ga32 = dev(c32["gx"]), dev(c32["y"]), dev(c32["co"]), dev(c32["gamma"])
    status, gy, _, _ = bwd_apply(g32, y32, co32, ga32, None, 1, 5, 32, pair_in=True)           # pairs with an odd M
    assert status != 0 and (gy == SENTINEL).all()
    status, gy, _, _ = bwd_apply(gc, yc, coc, gac, None, 1, 6, 36, pair_out=True)              # pairs with F = 36
    assert status != 0 and (gy == SENTINEL).all()
    c5 = exact_case(4, 5, 93)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    status, x = act_fwd(dev(c5["y"]), dev(c5["co"]), 1, None, 0, 0, 4, 5, amax=word)           # amax_out with F % 4 != 0
    assert status != 0 and (x == SENTINEL).all() and int(word) == 0
    status, x = act_fwd(y32, co32, 1, y32, 32, 2, 5, 32)                                       # res_shift = 2
    assert status != 0 and (x == SENTINEL).all()
    status, x = act_fwd(y32, co32, 1, None, 0, 0, 5, 32, real_only=1)                          # real_rows_only, no handle
    assert status != 0 and (x == SENTINEL).all()
    assert _lib().hip().p2m_last_error_string()
