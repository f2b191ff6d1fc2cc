"""Float64 restatement of the BatchNorm / ReLU / residual family of csrc/bn.hip (include/p2m.h), in plain numpy.

Every function takes the fp32 coefficient block co = [mean, invstd, scale, shift] AS AN INPUT (scale = gamma * invstd and
shift = beta - mean * scale are whatever the caller stored, not re-derived), converts everything to float64 and evaluates
the formula of the header once, with no tiling, no row maps and no order of summation to get wrong:

  act_fwd      x  = relu(y * scale + shift) + resize(resid[r >> res_shift])
  bwd_sums     dbeta = sum g m,  dgamma = sum g m yhat,   m = [y * scale + shift > 0],  yhat = (y - mean) * invstd
  bwd_apply    gy = gamma * invstd * (g m - c0 - yhat * c1)        (coef = None: c0 = c1 = 0, eval mode)

The mask is exact: an fp32 x fp32 product is exact in double and one rounding never changes a sign, so the float64
y * scale + shift has the sign of the kernels' fmaf(y, scale, shift).

Class forms ("classes" in include/p2m.h): a level of V vertices with a weight table w[V] (1 real vertex, class size for a
representative, 0 hole), rows r = b * V + v.  Holes hold no data (the tests fill them with NaN); the functions below never
let a hole's value reach a result.

tests/test_bn_ref_cpu.py pins these functions to torch float64 autograd.
"""
import numpy as np


def f64(a):
    """torch tensor (any device) or array -> float64 numpy array (a copy)."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.array(a, dtype=np.float64)


def representable_f32(a):
    """True where the float64 value is exactly an fp32 number."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return a.astype(np.float32).astype(np.float64) == a


def ulp32(a):
    """Spacing of fp32 at |a| (float64 array)."""
    return np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---- feature-axis resize (F.interpolate(mode='linear', align_corners=False) along an axis of length Fres -> F) ----------
def resize_weights(F, Fres, weights="f64"):
    """(i0, i1, w): out[j] = r[i0[j]] * (1 - w[j]) + r[i1[j]] * w[j].  weights="f32": src = (j + 0.5f) * (Fres / F) - 0.5f,
    the clamp, i0, i1 and w evaluated in np.float32 in the kernels' (and ATen's) order; w is returned as float64."""
    if weights == "f32":
        one = np.float32
        j = np.arange(F, dtype=np.float32)
        ratio = one(Fres) / one(F)
        src = (j + one(0.5)) * ratio - one(0.5)
        src = np.where(src < one(0), one(0), src).astype(np.float32)
        i0 = src.astype(np.int64)
        w = (src - i0.astype(np.float32)).astype(np.float64)
    elif weights == "f64":
        j = np.arange(F, dtype=np.float64)
        src = (j + 0.5) * (float(Fres) / float(F)) - 0.5
        src = np.maximum(src, 0.0)
        i0 = np.floor(src).astype(np.int64)
        w = src - i0
    else:
        raise ValueError(weights)
    i1 = np.minimum(i0 + 1, Fres - 1)
    return i0, i1, w


def resize_matrix(F, Fres, weights="f64"):
    """W [F, Fres] with out = r @ W.T"""
    i0, i1, w = resize_weights(F, Fres, weights)
    W = np.zeros((F, Fres), dtype=np.float64)
    np.add.at(W, (np.arange(F), i0), 1.0 - w)
    np.add.at(W, (np.arange(F), i1), w)
    return W


def resize(r, F, weights="f64"):
    r = f64(r)
    i0, i1, w = resize_weights(F, r.shape[1], weights)
    return r[:, i0] * (1.0 - w) + r[:, i1] * w


def resize_weight_term(r, F):
    """|r[i1] - r[i0]| per output element: what an error of the weight w multiplies."""
    r = f64(r)
    i0, i1, _ = resize_weights(F, r.shape[1], "f32")
    return np.abs(r[:, i1] - r[:, i0])


def lerp_transpose(g, F, Fres, weights="f64"):
    """dst[r, i] = sum_j w(j, i) g[r, j]: the transpose of the resize, g [M, F] -> [M, Fres]."""
    return f64(g) @ resize_matrix(F, Fres, weights)


def lerp_transpose_weight_term(g, F, Fres):
    """sum of |g[r, j]| over the j that contribute to dst[r, i]."""
    P = (resize_matrix(F, Fres, "f32") != 0).astype(np.float64)
    i0, i1, _ = resize_weights(F, Fres, "f32")
    P[np.arange(F), i0] = 1.0
    P[np.arange(F), i1] = 1.0
    return np.abs(f64(g)) @ P


# ---- coefficients --------------------------------------------------------------------------------------------------
def eval_coeffs(gamma, beta, running_mean, running_var, eps, scale_used=None):
    """eval(): [mean, invstd, scale, shift] from the running statistics.  eps is the fp32 number the C ABI receives.
    scale_used (fp32, optional): shift = beta - mean * scale_used, the consistency the forward pass relies on."""
    gamma, beta, rm, rv = f64(gamma), f64(beta), f64(running_mean), f64(running_var)
    invstd = 1.0 / np.sqrt(rv + float(np.float32(eps)))
    scale = gamma * invstd
    sc = scale if scale_used is None else f64(scale_used)
    return np.stack([rm, invstd, scale, beta - rm * sc])


def preact(y, co):
    co = f64(co)
    return f64(y) * co[2] + co[3]


def mask(y, co, relu):
    y = f64(y)
    if not relu:
        return np.ones_like(y)
    with np.errstate(invalid="ignore"):
        return (preact(y, co) > 0).astype(np.float64)


# ---- plain forms -------------------------------------------------------------------------------------------------------
def act_fwd(y, co, relu, resid=None, Fres=0, res_shift=0, weights="f64"):
    y = f64(y)
    M, F = y.shape
    v = y if co is None else preact(y, co)
    if relu:
        v = np.maximum(v, 0.0)
    if resid is not None:
        rr = f64(resid)[np.arange(M) >> res_shift]
        assert rr.shape[1] == Fres
        v = v + (rr if Fres == F else resize(rr, F, weights))
    return v


def bwd_sums(gx, y, co, relu):
    """(dbeta, dgamma) = (sum g m, sum g m yhat)"""
    co = f64(co)
    gm = f64(gx) * mask(y, co, relu)
    yhat = (f64(y) - co[0]) * co[1]
    return gm.sum(0), (gm * yhat).sum(0)


def bwd_apply(gx, y, co, gamma, coef, relu):
    co = f64(co)
    gm = f64(gx) * mask(y, co, relu)
    k = f64(gamma) * co[1]
    if coef is None:
        return k * gm
    coef = f64(coef)
    yhat = (f64(y) - co[0]) * co[1]
    return k * (gm - coef[0] - yhat * coef[1])


def pair_sum(x):
    x = f64(x)
    return x[0::2] + x[1::2]


# ---- class forms ----------------------------------------------------------------------------------------------------
def class_weights(rep_of):
    """w[V] of p2m_graph_set_classes: class size at a representative of a class of > 1, 1 at every other vertex that is its
    own representative, 0 at a hole."""
    rep = np.asarray(rep_of, dtype=np.int64)
    cnt = np.bincount(rep, minlength=rep.size).astype(np.float64)
    return np.where(rep == np.arange(rep.size), cnt, 0.0)


def _rows_w(w, M):
    w = np.asarray(w, dtype=np.float64)
    assert M % w.size == 0
    return np.tile(w, M // w.size)


def _drop_holes(x, wr):
    return np.where(wr[:, None] != 0, f64(x), 0.0)


def act_fwd_classes(y, co, relu, w, resid=None, Fres=0, res_shift=0, weights="f64"):
    """(x, live): x as act_fwd on the live rows (holes: 0 here, UNTOUCHED by the kernel), live [M] bool"""
    M = y.shape[0]
    wr = _rows_w(w, M)
    x = act_fwd(_drop_holes(y, wr), co, relu, resid, Fres, res_shift, weights)
    return np.where(wr[:, None] != 0, x, 0.0), wr != 0


def bwd_sums_classes(gx, y, co, relu, w):
    """gx in class-sum form (a representative carries its class's sum): the sums run over the live rows only"""
    wr = _rows_w(w, y.shape[0])
    return bwd_sums(_drop_holes(gx, wr), _drop_holes(y, wr), co, relu)


def bwd_apply_classes(gx, y, co, gamma, coef, relu, w):
    """gy = k g m - w_r k (c0 + yhat c1): the constant term once per class member; holes 0 (zero_holes) / untouched"""
    co = f64(co)
    wr = _rows_w(w, y.shape[0])
    g, v = _drop_holes(gx, wr), _drop_holes(y, wr)
    k = f64(gamma) * co[1]
    out = k * g * mask(v, co, relu)
    if coef is not None:
        coef = f64(coef)
        out = out - wr[:, None] * k * (coef[0] + (v - co[0]) * co[1] * coef[1])
    return np.where(wr[:, None] != 0, out, 0.0), wr != 0


def pair_sum_classes(x, w):
    """(out, live_pair): holes left out of the sums; live_pair [M/2]: at least one live child"""
    wr = _rows_w(w, x.shape[0])
    return pair_sum(_drop_holes(x, wr)), (wr[0::2] != 0) | (wr[1::2] != 0)


def class_reduce(x, w):
    """out[r] = sum of x over the class of r (w[v] consecutive rows from r), x[r] for real vertices, 0 for holes"""
    x = f64(x)
    wr = _rows_w(w, x.shape[0]).astype(np.int64)
    out = np.zeros_like(x)
    for r in np.nonzero(wr)[0]:
        out[r] = x[r:r + wr[r]].sum(0)
    return out


def stats_rows_w(y, fake_ids, fake_wts, B, V, tile=128):
    """weighted tile partials of the representatives: st[b * tps + t][0] = sum w y, [1] = sum w (y - weighted tile mean)^2"""
    y = f64(y).reshape(B, V, -1)
    ids = np.asarray(fake_ids, dtype=np.int64)
    wts = np.asarray(fake_wts, dtype=np.float64)
    tps = -(-ids.size // tile)
    st = np.zeros((B * tps, 2, y.shape[2]))
    for b in range(B):
        for t in range(tps):
            sel, wv = ids[t * tile:(t + 1) * tile], wts[t * tile:(t + 1) * tile, None]
            blk = y[b, sel]
            s = (wv * blk).sum(0)
            st[b * tps + t, 0] = s
            st[b * tps + t, 1] = (wv * (blk - s / wv.sum()) ** 2).sum(0)
    return st
