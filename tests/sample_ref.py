"""numpy restatement of the sample-noise kernels (csrc/sample.hip, csrc/p2m_philox.h): the same Philox4x32-10 stream, the
same stage numbering and draw order (include/p2m.h, "training-sample noise"), the same sampling scheme.  dtype=np.float64 is
the definition the kernels are held to; dtype=np.float32 runs the same operator sequence in fp32 and gives the error class.

Vectorised over samples: every function takes S samples at once and walks the 17 joints in order, because the higher joint
of a left/right pair sees the already synthesised lower one (lib/noise_utils.py:31-36 updates synth_joints in place).

The robustness band (`band`) - when does an fp32 evaluation decide a candidate like the exact one?
The kernel evaluates, with u = 2^-24 the unit roundoff and every operation rounded once,
    r  = fmaf(hi - lo, ur, lo)                hi, lo = base * C, base = sqrtf(area) * (2 sigma): |hi err| <= 4 u hi
                                              -> |r err| <= 4 u hi + u (hi - lo) + u r <= 6 u R          (R = the stage's hi)
    s, c = sincospif(2 ua)                    2 ua is exact; sincospif is good to 2 ulp -> absolute error <= 4 u
    x  = fmaf(r, c, cx)                       |x err| <= u |x| + |r err| + 4 u r <= u |x| + 10 u R
    dx = ox - x                               |dx err| <= u |dx| + |x err|;  ox itself may be the rounded output of the lower
                                              joint of the pair, carrying the same kind of error with that joint's R <= ks_10
    d2 = fmaf(dx, dx, dy * dy)                |d2 err| <= 2 (|dx| + |dy|) e + 2 u d2,   e = u (2 M + 20 K + d)
    thr = r * r  or  ks_50 * ks_50            |thr err| <= 13 u K^2
with d the exact distance, K = ks_10 of the joint (>= every radius of every stage) and M = the largest |coordinate| of the two
sources plus K (>= every |x|, |y|).  (|dx| + |dy|) <= sqrt(2) d, so
    |(d2 - thr) err| <= 3 d (2 M + 20 K + d) u + 2 u d^2 + 13 u K^2 =: band / 2
and the audit doubles it.  A candidate with |d2 - thr| <= band is `banded`: fp32 may decide it either way.
"""
import numpy as np

U24 = 2.0 ** -24
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

# stages (counter word 2 = joint | stage << 8)
ST_JITTER, ST_MISS_COUNT0, ST_MISS_COUNT1, ST_MISS_PICK0, ST_MISS_PICK1, ST_INV, ST_GOOD, ST_SELECT, ST_TABLE = range(9)
N_JITTER, N_MISS, N_INV, N_GOOD = 500, 2000, 500, 125
KIND_JITTER, KIND_MISS, KIND_INV, KIND_GOOD, KIND_ZERO = 0, 1, 2, 4, -1
# sqrt(-2 ln ks) for ks = 0.10, 0.50, 0.85 as the fp32 constants of the kernel
C10, C50, C85 = (np.float32(np.sqrt(-2.0 * np.log(k))) for k in (0.10, 0.50, 0.85))
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
FAR = np.float32(1.0 + 2.0 ** -10)       # sources further apart than (ks_10 + ks_50) FAR: every miss candidate passes


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10.  Arguments: uint64 arrays (or scalars) holding 32-bit values; returns four uint64 arrays."""
    k0, k1 = np.uint64(k0), np.uint64(k1)          # one key per call
    c0, c1, c2, c3 = (np.array(c, np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3))
    t0, t1 = np.empty_like(c0), np.empty_like(c0)
    for _ in range(10):                            # in place: this loop is the cost of the whole restatement
        np.multiply(c0, M0, out=t0)                # t0 = M0 * c0,  t1 = M1 * c2
        np.multiply(c2, M1, out=t1)
        np.right_shift(t1, S32, out=c0)            # c0' = hi(t1) ^ c1 ^ k0
        c0 ^= c1
        c0 ^= k0
        np.right_shift(t0, S32, out=c2)            # c2' = hi(t0) ^ c3 ^ k1
        c2 ^= c3
        c2 ^= k1
        np.bitwise_and(t1, MASK, out=c1)           # c1' = lo(t1),  c3' = lo(t0)
        np.bitwise_and(t0, MASK, out=c3)
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def _words(seed, index, joint, stage, block):
    """index: [S] uint64 global sample indices; block: [nb] -> four [S, nb] word arrays."""
    seed = np.uint64(seed)
    idx = np.asarray(index, np.uint64)[:, None]
    blk = np.asarray(block, np.uint64)[None, :]
    z = np.zeros((idx.shape[0], blk.shape[1]), np.uint64)
    return philox(z + (idx & MASK), z + (idx >> S32), z + np.uint64(joint | (stage << 8)), z + blk, seed & MASK, seed >> S32)


def uniforms(words):
    return (words >> np.uint64(8)).astype(np.float64) * U24


def _candidates(seed, index, joint, stage, c_lo, c_hi):
    """(angle uniform, radius uniform) of candidates c_lo .. c_hi - 1 (c_lo even): [S, c_hi - c_lo] each.  Candidate c comes
    from draw block c >> 1: words 0, 1 for even c, words 2, 3 for odd c."""
    w = _words(seed, index, joint, stage, np.arange(c_lo >> 1, (c_hi + 1) >> 1))
    ua = np.stack([uniforms(w[0]), uniforms(w[2])], axis=2).reshape(w[0].shape[0], -1)[:, :c_hi - c_lo]
    ur = np.stack([uniforms(w[1]), uniforms(w[3])], axis=2).reshape(w[0].shape[0], -1)[:, :c_hi - c_lo]
    return ua, ur


def _fma(a, b, c, dt):
    """fmaf in fp32 (one rounding, through float64: a 24 x 24 bit product is exact there and the sum rounds twice only in
    vanishing cases), plain arithmetic in fp64."""
    if dt == np.float64:
        return a * b + c
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _eval(ua, ur, lo, hi, ctr, oth, thr2, K, dt):
    """Evaluates candidates.  ua, ur [S, n]; lo, hi, K [S]; ctr, oth [S, 2]; thr2 [S] or None (= r^2).
    Returns x, y, ok (d2 > thr), banded (|d2 - thr| <= band)."""
    ua, ur = ua.astype(dt), ur.astype(dt)
    r = _fma((hi - lo)[:, None], ur, lo[:, None], dt)
    if dt == np.float64:
        ang = np.pi * (2.0 * ua)
    else:
        ang = (np.float32(2.0 * np.pi) * ua).astype(np.float32)
    c, s = np.cos(ang).astype(dt), np.sin(ang).astype(dt)
    x, y = _fma(r, c, ctr[:, 0:1], dt), _fma(r, s, ctr[:, 1:2], dt)
    dx, dy = oth[:, 0:1] - x, oth[:, 1:2] - y
    d2 = _fma(dx, dx, dy * dy, dt)
    thr = r * r if thr2 is None else np.broadcast_to(thr2[:, None], r.shape)
    d = np.sqrt(d2.astype(np.float64))
    Kd = K.astype(np.float64)[:, None]
    M = np.maximum(np.abs(ctr).max(axis=1), np.abs(oth).max(axis=1)).astype(np.float64)[:, None] + Kd
    band = 2.0 * U24 * (3.0 * d * (2.0 * M + 20.0 * Kd + d) + 2.0 * d * d + 13.0 * Kd * Kd)
    diff = d2.astype(np.float64) - thr.astype(np.float64)
    return x, y, diff > 0, np.abs(diff) <= band


def _first_pass(seed, index, joint, stage, N, lo, hi, ctr, oth, has_oth, thr2, K, dt):
    """First passing candidate of a stage: found [S], pt [S, 2], robust [S].  Samples without a second source take candidate 0
    (nothing to compare with).  Not robust: a banded candidate at or before the first pass."""
    S = len(index)
    found, pt, robust = np.zeros(S, bool), np.zeros((S, 2), dt), np.ones(S, bool)
    act = np.arange(S)
    c0 = 0
    while len(act) and c0 < N:
        c1 = min(N, c0 + (128 if has_oth[act].any() else 2))
        ua, ur = _candidates(seed, index[act], joint, stage, c0, c1)
        x, y, ok, banded = _eval(ua, ur, lo[act], hi[act], ctr[act], oth[act], None if thr2 is None else thr2[act], K[act], dt)
        ok = ok | ~has_oth[act][:, None]
        banded = banded & has_oth[act][:, None]
        hit = ok.any(axis=1)
        first = np.where(hit, ok.argmax(axis=1), ok.shape[1] - 1)
        upto = np.arange(ok.shape[1])[None, :] <= first[:, None]
        robust[act] &= ~(banded & upto).any(axis=1)
        rows = np.arange(len(act))
        found[act[hit]] = True
        pt[act[hit], 0], pt[act[hit], 1] = x[rows[hit], first[hit]], y[rows[hit], first[hit]]
        act = act[~hit]
        c0 = c1
    return found, pt, robust


def _count(seed, index, joint, stage, lo, hi, ctr, oth, thr2, K, dt, chunk=512):
    """Passing candidates among N_MISS: n [S], and the range [n_lo, n_hi] the banded ones leave."""
    S = len(index)
    n, nb = np.zeros(S, np.int64), np.zeros(S, np.int64)
    nlo = np.zeros(S, np.int64)
    rows = max(1, 262144 // chunk)
    for s0 in range(0, S, rows):
        sl = slice(s0, min(S, s0 + rows))
        for c0 in range(0, N_MISS, chunk):
            ua, ur = _candidates(seed, index[sl], joint, stage, c0, min(N_MISS, c0 + chunk))
            _, _, ok, banded = _eval(ua, ur, lo[sl], hi[sl], ctr[sl], oth[sl], thr2[sl], K[sl], dt)
            n[sl] += ok.sum(axis=1)
            nlo[sl] += (ok & ~banded).sum(axis=1)
            nb[sl] += banded.sum(axis=1)
    return n, nlo, nlo + nb


def probabilities(j, num_valid):
    """[jitter, miss, inversion] of lib/noise_utils.py:70-83, 105-125, 161-166 (swap is 0, good the remainder)."""
    leg = j == 0 or 13 <= j <= 16
    up = 1 <= j <= 10
    if num_valid <= 10:
        pj = 0.15 if leg else 0.20 if up else 0.25
    else:
        pj = 0.10 if leg else 0.15 if up else 0.20
    face, sa = j <= 4, j in (5, 6, 15, 16)
    if num_valid <= 5:
        pm = 0.15 if face else 0.20 if sa else 0.25
    elif num_valid <= 10:
        pm = 0.10 if face else 0.13 if sa else 0.15
    else:
        pm = 0.02 if face else 0.05 if sa else 0.10
    pi = 0.01 if j <= 4 else 0.03 if j <= 10 else 0.06
    return pj, pm, pi


_PROB = np.array([[probabilities(j, nv) for j in range(17)] for nv in (3, 8, 17)], np.float32)      # [class, joint, 3]


def partner(j):
    return 0 if j == 0 else (j + 1 if j & 1 else j - 1)


def noise_coco(joints, area, sigmas, seed, first_index, dtype=np.float64, fault=None):
    """joints [S, 17, 3] (x, y, valid), area [S], sigmas [17] -> out [S, 17, 3], kind [S, 17] int8, robust [S, 9] (unit 0 the
    nose, unit p the pair (2p - 1, 2p)).  Sample s uses the global index first_index + s.
    fault (tests only): 'swap_radii' exchanges the jitter and good radii, 'no_pair' drops the pair dependence."""
    dt = dtype
    joints = np.asarray(joints, np.float32)
    S = joints.shape[0]
    index = np.uint64(first_index) + np.arange(S, dtype=np.uint64)
    out = joints.astype(dt).copy()
    valid0 = joints[:, :, 2] > 0
    ncls = np.where(valid0.sum(axis=1) <= 5, 0, np.where(valid0.sum(axis=1) <= 10, 1, 2))
    kind = np.zeros((S, 17), np.int8)
    robust = np.ones((S, 9), bool)
    root = np.sqrt(np.maximum(np.asarray(area, np.float32), np.float32(0)).astype(dt)).astype(dt)
    allS = np.arange(S)
    for j in range(17):
        unit = (j + 1) // 2
        base = (root * (np.float32(2) * np.asarray(sigmas, np.float32)[j]).astype(dt)).astype(dt)
        ks10, ks50, ks85 = ((base * C.astype(dt)).astype(dt) for C in (C10, C50, C85))
        own = out[:, j, :2].copy()
        if j == 0 or fault == "no_pair":
            has = np.zeros(S, bool)
            oth = own.copy()
        else:
            has = valid0[:, partner(j)].copy()
            oth = out[:, partner(j), :2].copy()
        zero = np.zeros(S, dt)
        thr50 = (ks50 * ks50).astype(dt)
        jl, jh, gl, gh = (zero, ks85, ks85, ks50) if fault == "swap_radii" else (ks85, ks50, zero, ks85)
        a_j, p_j, r_j = _first_pass(seed, index, j, ST_JITTER, N_JITTER, jl, jh, own, oth, has, None, ks10, dt)
        a_g, p_g, r_g = _first_pass(seed, index, j, ST_GOOD, N_GOOD, gl, gh, own, oth, has, None, ks10, dt)
        a_i, p_i, r_i = np.zeros(S, bool), np.zeros((S, 2), dt), np.ones(S, bool)
        if has.any():
            h = np.flatnonzero(has)
            a, p, r = _first_pass(seed, index[h], j, ST_INV, N_INV, zero[h], ks50[h], oth[h], own[h], has[h], None, ks10[h], dt)
            a_i[h], p_i[h], r_i[h] = a, p, r
        # miss: counts, source, point
        n0 = np.full(S, N_MISS, np.int64)
        n1 = np.zeros(S, np.int64)
        n0lo, n0hi, n1lo, n1hi = n0.copy(), n0.copy(), n1.copy(), n1.copy()
        dsrc = np.sqrt((((own - oth).astype(np.float64)) ** 2).sum(axis=1))
        far = dsrc.astype(dt) > ((ks10 + ks50).astype(dt) * FAR.astype(dt)).astype(dt)
        n1[has & far] = N_MISS
        n1lo[has & far] = n1hi[has & far] = N_MISS
        cnt = np.flatnonzero(has & ~far)
        if len(cnt):
            n0[cnt], n0lo[cnt], n0hi[cnt] = _count(seed, index[cnt], j, ST_MISS_COUNT0, ks50[cnt], ks10[cnt], own[cnt], oth[cnt],
                                                   thr50[cnt], ks10[cnt], dt)
            n1[cnt], n1lo[cnt], n1hi[cnt] = _count(seed, index[cnt], j, ST_MISS_COUNT1, ks50[cnt], ks10[cnt], oth[cnt], own[cnt],
                                                   thr50[cnt], ks10[cnt], dt)
        sel = _words(seed, index, j, ST_SELECT, np.zeros(1, np.uint64))
        k_src, u_cat = (sel[0][:, 0] >> np.uint64(8)).astype(np.int64), uniforms(sel[1][:, 0])

        def source(a, b):                      # 0 / 1, -1: empty pool.  Exact integers, as in the kernel
            pool = a + b // 4
            return np.where(pool == 0, -1, np.where(k_src * pool < (a << 24), 0, 1))
        src = source(n0, n1)
        r_m = (source(n0lo, n1hi) == src) & (source(n0hi, n1lo) == src)
        a_m, p_m = np.zeros(S, bool), np.zeros((S, 2), dt)
        for s_id, st, c_, o_ in ((0, ST_MISS_PICK0, own, oth), (1, ST_MISS_PICK1, oth, own)):
            h = np.flatnonzero(src == s_id)
            if len(h):
                a, p, r = _first_pass(seed, index[h], j, st, N_MISS, ks50[h], ks10[h], c_[h], o_[h], has[h], thr50[h], ks10[h], dt)
                a_m[h], p_m[h] = a, p
                r_m[h] &= r
        # category: one uniform against the cumulative renormalised [jitter, miss, inversion, good]
        pr = _PROB[ncls, j].astype(dt)                                                    # [S, 3]
        pgood = (dt(1) - ((pr[:, 0] + pr[:, 1]).astype(dt) + pr[:, 2]).astype(dt)).astype(dt)
        w = np.stack([pr[:, 0] * a_j, pr[:, 1] * a_m, pr[:, 2] * a_i, pgood * a_g], axis=1).astype(dt)
        norm = ((w[:, 0] + w[:, 1]).astype(dt) + w[:, 2]).astype(dt) + w[:, 3]
        norm = norm.astype(dt)
        t = (u_cat.astype(dt) * norm).astype(dt)
        c1 = w[:, 0]
        c2 = (c1 + w[:, 1]).astype(dt)
        c3 = (c2 + w[:, 2]).astype(dt)
        pick = np.where(t < c1, 0, np.where(t < c2, 1, np.where(t < c3, 2, 3)))
        avail = w > 0
        last = 3 - np.argmax(avail[:, ::-1], axis=1)                                      # the last available type
        pick = np.where(avail[allS, pick], pick, last)
        none = ~avail.any(axis=1)
        near = np.zeros(S, bool)
        for cum in (c1, c2, c3):
            near |= np.abs(t.astype(np.float64) - cum.astype(np.float64)) <= 8 * U24
        pts = np.stack([p_j, p_m, p_i, p_g], axis=1)                                       # [S, 4, 2]
        new = pts[allS, pick]
        out[:, j, 0] = np.where(none, 0, new[:, 0])
        out[:, j, 1] = np.where(none, 0, new[:, 1])
        out[:, j, 2] = np.where(none, 0, 1)
        kind[:, j] = np.where(none, KIND_ZERO, np.array([KIND_JITTER, KIND_MISS, KIND_INV, KIND_GOOD], np.int8)[pick])
        robust[:, unit] &= r_j & r_g & r_i & r_m & ~near
    return out, kind, robust


def box_muller(u0, u1):
    """Two normals from the uniforms (1 - u0, u1): R cos, R sin with R = sqrt(-2 ln(1 - u0))."""
    R = np.sqrt(-2.0 * np.log(1.0 - u0))
    return R * np.cos(2.0 * np.pi * u1), R * np.sin(2.0 * np.pi * u1)


def noise_table(pose, mean, std, weight, W, H, seed, first_index, dtype=np.float64):
    """pose [S, J, 2]; mean, std [J, 2]; weight [J] -> out [S, J, 2], mask [S, J] bool.
    out = pose + [weight > u] * (mean + std * n) / 256 * (W, H); per (sample, joint) one draw block of stage ST_TABLE:
    word 0 the Bernoulli uniform, words 1, 2 the Box-Muller pair (n_x = R cos, n_y = R sin).  The mask compares two fp32
    values (the weight and a 24-bit uniform): exact in either precision."""
    dt = dtype
    pose = np.asarray(pose, np.float32).astype(dt)
    S, J = pose.shape[:2]
    index = np.uint64(first_index) + np.arange(S, dtype=np.uint64)
    out, mask = pose.copy(), np.zeros((S, J), bool)
    mean, std, weight = (np.asarray(a, np.float32).astype(dt) for a in (mean, std, weight))
    sx, sy = dt(W) / dt(256), dt(H) / dt(256)
    for j in range(J):
        w = _words(seed, index, j, ST_TABLE, np.zeros(1, np.uint64))
        u, u0, u1 = (uniforms(w[k][:, 0]).astype(dt) for k in range(3))
        R = np.sqrt(dt(-2) * np.log(dt(1) - u0))
        ang = np.pi * (2.0 * u1) if dt == np.float64 else np.float32(2 * np.pi) * u1
        mask[:, j] = weight[j] > u
        out[:, j, 0] += mask[:, j] * ((mean[j, 0] + std[j, 0] * (R * np.cos(ang))) * sx)
        out[:, j, 1] += mask[:, j] * ((mean[j, 1] + std[j, 1] * (R * np.sin(ang))) * sy)
    return out, mask


ST_AUG = 9
NOISE_NONE, NOISE_COCO, NOISE_TABLE = 0, 1, 2


def draw_aug(seed, first_index, S, rot_factor, flip_enabled, dtype=np.float64):
    """augm_params from the stream (stage 9, joint 0, block 0): rot [S] in degrees, flip [S] bool."""
    dt = dtype
    index = np.uint64(first_index) + np.arange(S, dtype=np.uint64)
    w = _words(seed, index, 0, ST_AUG, np.zeros(1, np.uint64))
    uf, u0, u1, uz = (uniforms(w[k][:, 0]).astype(dt) for k in range(4))
    flip = (uf < 0.5) & bool(flip_enabled)
    R = np.sqrt(dt(-2) * np.log(dt(1) - u0))
    ang = np.pi * (2.0 * u1) if dt == np.float64 else np.float32(2 * np.pi) * u1
    rf = dt(rot_factor)
    rot = np.minimum(dt(2) * rf, np.maximum(-dt(2) * rf, (R * np.cos(ang)).astype(dt) * rf)).astype(dt)
    rot[uz < 0.5] = 0
    return rot, flip


def _swap_index(J, flip_pairs):
    src = np.arange(J)
    for a, b in flip_pairs:
        src[a], src[b] = b, a
    return src


def chain(verts, focal, princpt, reg_R, reg_root=0, in_R=None, midpoints=(), input_root=None, trans=None, mesh_scale=1000.0,
          given_cam=None, given_img=None, fit_thr=0.0, rot=None, flip=None, rot_factor=0.0, flip_enabled=False,
          noise=NOISE_NONE, sigmas=None, table=None, flip_pairs=(), W=288, H=384, seed=0, first_index=0, dtype=np.float64):
    """p2m_train_sample (include/p2m.h, "training samples") for S samples: verts [S, nv, 3]; reg_R [Jr, nv], in_R [Ji, nv] dense
    (None: the input set is the reg set).  Returns a dict of the outputs and of the intermediate values the reference
    fixture pins (img, tight, bbox, px, area).  dtype float32 runs the kernel's operation sequence in fp32 (the regression
    accumulates in fp64 either way)."""
    dt = dtype
    verts = np.asarray(verts, np.float32)
    S, nv = verts.shape[:2]
    t = np.zeros((S, 1, 3), np.float32) if trans is None else np.asarray(trans, np.float32).reshape(S, 1, 3)
    if dt == np.float64:
        mm = (verts.astype(dt) + t.astype(dt)) * dt(np.float32(mesh_scale))
    else:
        mm = ((verts + t).astype(np.float32) * np.float32(mesh_scale)).astype(np.float32)
    regress = lambda R: np.einsum("jv,svc->sjc", np.asarray(R, np.float32).astype(np.float64), mm.astype(np.float64))  # noqa
    jr = regress(reg_R)
    jr = jr.astype(np.float32).astype(dt) if dt == np.float32 else jr
    Jr = jr.shape[1]
    status = np.zeros(S, np.int32)
    fit = np.zeros(S, dt)
    own_set = in_R is not None
    if given_cam is not None:
        g = np.asarray(given_cam, np.float32).astype(dt)
        d = (g - g.mean(axis=1, keepdims=True).astype(dt)) - (jr - jr.mean(axis=1, keepdims=True).astype(dt))
        fit = np.sqrt((d * d).sum(axis=2)).astype(dt).mean(axis=1).astype(dt)
        jr = g
        if fit_thr > 0:
            status[fit > dt(np.float32(fit_thr))] |= 2
    if own_set:
        ji = regress(in_R)
        ji = ji.astype(np.float32).astype(dt) if dt == np.float32 else ji
        mids = [((ji[:, a] + ji[:, b]) * dt(0.5))[:, None] for a, b in midpoints]
        ji = np.concatenate([ji] + mids, axis=1).astype(dt)
    else:
        ji = jr.copy()
    J = ji.shape[1]
    input_root = reg_root if input_root is None else input_root
    f, c = np.asarray(focal, np.float32).astype(dt), np.asarray(princpt, np.float32).astype(dt)
    if not own_set and given_img is not None:
        img = np.asarray(given_img, np.float32).astype(dt)
    else:
        z = ji[:, :, 2] / dt(1000)
        img = np.stack([(ji[:, :, 0] / dt(1000)) / z * f[:, 0:1] + c[:, 0:1], (ji[:, :, 1] / dt(1000)) / z * f[:, 1:2] + c[:, 1:2]],
                       axis=2).astype(dt)
    W_, H_ = dt(W), dt(H)
    with np.errstate(all="ignore"):
        xmin, xmax, ymin, ymax = img[:, :, 0].min(1), img[:, :, 0].max(1), img[:, :, 1].min(1), img[:, :, 1].max(1)
        tw, th = xmax - xmin, ymax - ymin
        w, h = tw - dt(1), th - dt(1)
        ok = np.isfinite(img).all(axis=(1, 2)) & (tw * th > 0) & (w >= 0) & (h >= 0)
        cx, cy, aspect = xmin + w * dt(0.5), ymin + h * dt(0.5), W_ / H_
        wide, tall = w > aspect * h, w < aspect * h
        h2 = np.where(wide, w / aspect, h)
        w2 = np.where(tall & ~wide, h * aspect, w)
        w, h = w2.astype(dt), h2.astype(dt)
        ok &= w > 0
        status[~ok] |= 1
        drot, dflip = draw_aug(seed, first_index, S, rot_factor, flip_enabled, dt)
        rot = drot if rot is None else np.asarray(rot, np.float32).astype(dt)
        flip = dflip if flip is None else np.asarray(flip) != 0
        s = W_ / w
        if dt == np.float64:
            rad = np.pi * (rot / 180.0)
        else:
            rad = (np.float32(np.pi) * (rot / np.float32(180))).astype(np.float32)
        sn, cs = np.sin(rad).astype(dt)[:, None], np.cos(rad).astype(dt)[:, None]
        dx, dy = img[:, :, 0] - cx[:, None], img[:, :, 1] - cy[:, None]
        px = np.stack([s[:, None] * (cs * dx + sn * dy) + W_ * dt(0.5), s[:, None] * (cs * dy - sn * dx) + H_ * dt(0.5)],
                      axis=2).astype(dt)
        area = ((s * tw) * (s * th)).astype(dt)
        bbox = np.stack([cx - w * dt(0.5), cy - h * dt(0.5), w, h], axis=1)
        tight = np.stack([xmin, ymin, tw, th], axis=1)
    dead = (status & 1) != 0
    px[dead] = 0
    pre = px.copy()
    kind = robust = mask = None
    live = np.flatnonzero(~dead)
    if noise == NOISE_COCO and len(live):
        # the noise kernels read pose2d as the fp32 tensor the first launch wrote; dead samples are run and ignored
        j3 = np.concatenate([px[:, :17].astype(np.float32), np.ones((S, 17, 1), np.float32)], axis=2)
        o, kind, robust = noise_coco(j3, area.astype(np.float32), sigmas, seed, first_index, dtype=dt)
        px[live, :17] = o[live, :, :2]
    elif noise == NOISE_TABLE and len(live):
        o, mask = noise_table(px.astype(np.float32), *table, W, H, seed, first_index, dtype=dt)
        px[live] = o[live]
    src = _swap_index(J, flip_pairs)
    p = px.copy()
    fl = np.flatnonzero(flip & ~dead)
    p[fl] = p[fl][:, src]
    p[fl, :, 0] = W_ - p[fl, :, 0] - dt(1)
    flipped = p.copy()
    p = (p / np.array([W_, H_], dt)).astype(dt)
    with np.errstate(all="ignore"):
        mean = p.mean(axis=1, keepdims=True).astype(dt)
        dlt = (p - mean).astype(dt)
        std = np.sqrt((dlt * dlt).mean(axis=1, keepdims=True)).astype(dt)
        bad = ~dead & ~((std > 0) & np.isfinite(std)).all(axis=(1, 2))
        pose2d = (dlt / std).astype(dt)
    status[bad] |= 1
    dead = (status & 1) != 0
    pose2d[dead] = 0
    # targets
    root = jr[:, reg_root:reg_root + 1]
    mesh = ((mm.astype(dt) - root) / dt(1000)).astype(dt)
    reg = (jr - root).astype(dt)
    lift = (ji - ji[:, input_root:input_root + 1]).astype(dt)
    lf = lift.copy()
    lf[fl] = lf[fl][:, src]
    x, y = lf[:, :, 0].copy(), lf[:, :, 1].copy()
    nz = (rot != 0)[:, None]
    lf[:, :, 0] = np.where(nz, cs * x + sn * y, x)
    lf[:, :, 1] = np.where(nz, cs * y - sn * x, y)
    lf[fl, :, 0] = -lf[fl, :, 0]
    lf = lf.astype(dt)
    for a in (mesh, reg, lf):
        a[dead] = 0
    fitbad = (status & 2) != 0
    return dict(pose2d=pose2d, mesh=mesh, lift_pose3d=lf, reg_pose3d=reg,
                mesh_valid=np.repeat((~dead & ~fitbad)[:, None], nv, 1).astype(np.float32),
                lift_valid=np.repeat((~dead & ~(fitbad & own_set))[:, None], J, 1).astype(np.float32),
                reg_valid=np.repeat((~dead)[:, None], Jr, 1).astype(np.float32), status=status, fit_err=fit, rot=rot, flip=flip,
                kind=kind, robust=robust, mask=mask, img=img, tight=tight, bbox=bbox, px=pre, noisy=px, flipped=flipped, area=area,
                joint_cam=ji, lift_raw=lift)


def displacement_histogram(out, joints, area, sigmas, n_radial=24, r_max=None):
    """Per joint: counts of the displacement out - joints over n_radial radial bins x 8 octants, and the zeroed count.
    Radial edges: linspace(0, r_max, n_radial + 1) * ks_50 of the joint, r_max = ks_10 / ks_50 + 1 by default (a miss around
    the partner can lie up to |pair distance| + ks_10 away: the last bin is open-ended).  Returns hist [17, n_radial, 8] and
    zeroed [17] (int64)."""
    out, joints = np.asarray(out, np.float64), np.asarray(joints, np.float64)
    S = out.shape[0]
    if r_max is None:
        r_max = float(C10) / float(C50) + 1.0
    hist, zeroed = np.zeros((17, n_radial, 8), np.int64), np.zeros(17, np.int64)
    for j in range(17):
        ks50 = np.sqrt(area) * 2.0 * sigmas[j] * float(C50)
        z = out[:, j, 2] == 0
        zeroed[j] = z.sum()
        d = (out[:, j, :2] - joints[None, j, :2] if joints.ndim == 2 else out[:, j, :2] - joints[:, j, :2])[~z]
        rad = np.sqrt((d ** 2).sum(axis=1)) / ks50
        rb = np.minimum((rad / r_max * n_radial).astype(np.int64), n_radial - 1)
        ob = np.minimum((np.mod(np.arctan2(d[:, 1], d[:, 0]), 2 * np.pi) / (2 * np.pi) * 8).astype(np.int64), 7)
        np.add.at(hist[j], (rb, ob), 1)
    return hist, zeroed
