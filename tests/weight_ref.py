"""Restatements of the weight kernels of include/p2m.h (p2m_weight_pack, p2m_weight_eff, p2m_weight_grad_unpack,
p2m_weight_grad_unpack2) in numpy, the bounds they are held to and the case tables that tests/test_gpu_weight_kernels.py runs.
No GPU and no library: tests/test_weight_ref_cpu.py audits the tables (which chunk-loop tails, block edges and transpose arms
they reach), checks the restatements against a second spelling and checks that every planted fault moves an expected output.

Free of any summation order.  A permutation has no order.  Every sum here is math.fsum over float64 terms that are EXACT
(an fp32 value; the product of two fp32 values has 48 significant bits), so the result is the correctly rounded value of the true
sum, whichever way the terms are listed.

Exact cases.  Partials, prefilled dW / db and weights are integers |v| <= 8 and the factors are dyadic (S1, S2): every partial
sum of every order is a multiple of 1/8 below 2 * 257 * 8 + 8 < 2^13, so it is an fp32 number - no rounding anywhere, with or
without fused multiply-add, and the kernel must give the restatement's bits.  The integers are drawn as +0, never -0, and at
least one term of every sum is a plain partial, so an exact zero is +0 in every order too.

Real-valued cases.  Normal draws; the factors are those of a real graph (the GPU file takes them from a DeviceGraph; FAKE_A,
FAKE_B below are the same graph family's, for the CPU file).  Bounds, u = 2^-24:
  unpack   |dW - ref| <= (n1 + n2 + 3) u S,  S = sum_c |P_c| + |s_k| sum_c |P2_c| + |dW0|  per element.  n = n1 + n2 terms take
           n - 1 fp32 additions in any order, each within u of its own partial sum, which is at most S (1 + (n - 1) u) (Rump's
           bound for recursive summation in any order: (n - 1) u S exactly, no second-order term); the products s_k P2_c cost
           one more u |s_k| sum |P2_c| whether each is rounded or the sum is scaled once; the conversion to fp32 and the accumulate
           add are one rounding each: n + 2 roundings, and the + 3 leaves the second-order terms a whole u S.  db likewise with
           s = 1, the terms being the Pdb and Pdb2 entries and db0.
  eff      |We - ref| <= 4 u (|w0| + |a w1| + |b w2|) (1 + 2^-22): two products and two additions, each within u of a partial
           result that is at most (|w0| + |a w1| + |b w2|) (1 + u)^3; a fused multiply-add only removes roundings."""
import math

import numpy as np

U = 2.0 ** -24
UNP_CG = 8                          # chunk groups of k_weight_grad_unpack (csrc/weights.hip); P is unrolled 4 ways, P2 2 ways
UNP_BLOCK = 32                      # output elements per block; the first ceil(Fout / 32) blocks also reduce the bias
PACK_BLOCK = 256                    # threads per block of k_weight_pack and k_weight_eff
TILE = 64                           # k_transpose_tiled: 64 x 64 tiles, 16-byte accesses when R and C are multiples of 4
S1, S2 = -0.75, 0.375               # dyadic plane factors / (a, b) of the exact cases
FAKE_A = float(np.float32(1.0 / 3.0 - 1.0))                   # diagonal of an isolated row of L / 3 - I ...
FAKE_B = float(np.float32(2.0 * FAKE_A * FAKE_A - 1.0))       # ... and of 2 L L - I: what p2m_graph_split_info reports for it
INT_MAX = 8


# ---- restatements --------------------------------------------------------------------------------------------------------------

def _fsum0(terms):
    """Correctly rounded sum over axis 0 of a float64 array of exact terms (+ 0.0: an exact zero is +0)."""
    t = np.asarray(terms, np.float64)
    flat = t.reshape(t.shape[0], -1)
    out = np.array([math.fsum(col) for col in flat.T.tolist()], np.float64) + 0.0
    return out.reshape(t.shape[1:])


def _grid(Fout, Fin, K):
    return np.meshgrid(np.arange(Fout), np.arange(Fin), np.arange(K), indexing="ij")


def pack_ref(W, Fout, Fin, K):
    """Wt[k Fin + fin][fout], W2[fout][k Fin + fin], W3[k Fout + fout][fin] from W[fout][fin K + k]: element moves of any dtype
    (the tests hand in uint32 words)."""
    W = np.asarray(W).reshape(Fout, Fin * K)
    fo, fi, k = _grid(Fout, Fin, K)
    Wt, W2, W3 = (np.empty(s, W.dtype) for s in ((K * Fin, Fout), (Fout, K * Fin), (K * Fout, Fin)))
    src = W[fo, fi * K + k]
    Wt[k * Fin + fi, fo] = src
    W2[fo, k * Fin + fi] = src
    W3[k * Fout + fo, fi] = src
    return Wt, W2, W3


def eff_ref(Wt, Ka, N, a, b):
    """(We, S): We[k][n] = Wt[k][n] + a Wt[Ka + k][n] + b Wt[2 Ka + k][n] correctly rounded to float64, a and b as the fp32
    numbers the entry receives; S = |w0| + |a w1| + |b w2|."""
    w = np.asarray(Wt, np.float32).reshape(3, Ka, N).astype(np.float64)
    a, b = float(np.float32(a)), float(np.float32(b))
    terms = np.stack([w[0], a * w[1], b * w[2]])
    return _fsum0(terms), np.abs(terms).sum(0)


def eff_bound(S):
    return 4 * U * S * (1 + 2.0 ** -22)


def unpack_index(layout, Fout, Fin, K):
    """Offset inside one chunk of P of the partial that belongs to dW[fout][fin K + k], as [Fout, Fin, K]."""
    fo, fi, k = _grid(Fout, Fin, K)
    if layout == 0:                 # P[chunk][k Fin + fin][fout]
        return (k * Fin + fi) * Fout + fo
    if layout == 1:                 # P[chunk][fin][k Fout + fout]
        return fi * (K * Fout) + k * Fout + fo
    if layout == 2 and K == 1:      # P[chunk][fout][fin]
        return fo * Fin + fi
    raise ValueError("layout must be 0, 1 or (K = 1) 2")


def unpack_ref(P, Pdb, nchunks, Fout, Fin, K, layout, pdb_stride, dW0=None, db0=None, P2=None, Pdb2=None, nchunks2=0,
               s1=0.0, s2=0.0, want_db=True):
    """p2m_weight_grad_unpack (P2 None) / p2m_weight_grad_unpack2 (P2 given: layout 1, K = 3, pdb_stride = 3 Fout).
    P: nchunks * tot floats; Pdb: nchunks rows of pdb_stride floats of which the first Fout count, or None; P2: nchunks2 chunks
    [fin][fout]; Pdb2: nchunks2 rows of Fout, or None; dW0 / db0: what the outputs held, given exactly when accumulate != 0.
    -> dict(dW [Fout, Fin K] float64, S_dW, n_dW, db [Fout] float64 or None when db or Pdb is NULL, S_db, n_db): the correctly
    rounded sums, the sums of magnitudes and the numbers of terms the bounds need."""
    tot = Fout * Fin * K
    P = np.asarray(P, np.float32).reshape(-1)[:nchunks * tot].reshape(nchunks, tot).astype(np.float64)
    terms = [P[:, unpack_index(layout, Fout, Fin, K)]]                                   # [nchunks, Fout, Fin, K]
    if P2 is not None:
        fo, fi, k = _grid(Fout, Fin, K)
        P2 = np.asarray(P2, np.float32).reshape(-1)[:nchunks2 * Fin * Fout].reshape(nchunks2, Fin * Fout).astype(np.float64)
        factor = np.array([1.0, float(np.float32(s1)), float(np.float32(s2))])[k]        # (1, s1, s2)[k]
        terms.append(P2[:, fi * Fout + fo] * factor)
    if dW0 is not None:
        terms.append(np.asarray(dW0, np.float32).astype(np.float64).reshape(1, Fout, Fin, K))
    terms = np.concatenate(terms)
    out = dict(dW=_fsum0(terms).reshape(Fout, Fin * K), S_dW=np.abs(terms).sum(0).reshape(Fout, Fin * K),
               n_dW=nchunks + (nchunks2 if P2 is not None else 0), db=None, S_db=None, n_db=0)
    if want_db and Pdb is not None:
        Pdb = np.asarray(Pdb, np.float32).reshape(-1).astype(np.float64)
        rows = np.arange(nchunks)[:, None] * pdb_stride + np.arange(Fout)[None, :]
        bt = [Pdb[rows]]
        if Pdb2 is not None:
            bt.append(np.asarray(Pdb2, np.float32).reshape(-1)[:nchunks2 * Fout].reshape(nchunks2, Fout).astype(np.float64))
        if db0 is not None:
            bt.append(np.asarray(db0, np.float32).astype(np.float64).reshape(1, Fout))
        bt = np.concatenate(bt)
        out.update(db=_fsum0(bt), S_db=np.abs(bt).sum(0), n_db=nchunks + (nchunks2 if Pdb2 is not None else 0))
    return out


def unpack_bound(n, S):
    return (n + 3) * U * S


def prescale_p2(P2, nchunks2, Fout, Fin, s1, s2):
    """P2[c][fin][fout] -> [c][fin][k Fout + fout] = (1, s1, s2)[k] P2[c][fin][fout] in fp32: with it unpack2 is unpack (layout
    1) of P followed by an accumulating unpack (layout 1) of this - exact on the exact cases."""
    p = np.asarray(P2, np.float32).reshape(nchunks2, Fin, 1, Fout)
    f = np.array([1.0, s1, s2], np.float32).reshape(1, 1, 3, 1)
    return np.ascontiguousarray((p * f).reshape(nchunks2, Fin * 3 * Fout))


# ---- what a shape reaches (restated from csrc/weights.hip; the CPU audit reads these) -------------------------------------------

def transpose_arms(R, C, w_off=0, wt_off=0, K=1, w2=False, w3=False):
    """Arms of p2m_weight_pack a call takes.  w_off / wt_off: floats by which W / Wt lie behind a 16-byte boundary."""
    if K != 1 or w2 or w3 or w_off % 4 or wt_off % 4:
        return {"general"}
    arms = {"tiled", "vec" if R % 4 == 0 and C % 4 == 0 else "scalar"}
    if R >= TILE and C >= TILE:
        arms.add("full_tile")
    if R % TILE:
        arms.add("partial_rows")
    if C % TILE:
        arms.add("partial_cols")
    if R > TILE or C > TILE:
        arms.add("many_tiles")
    return arms


def chunk_tails(nchunks, unroll):
    """Per chunk group of k_weight_grad_unpack: (trips of the `unroll`-way main loop, trips of the tail loop)."""
    out = []
    for cg in range(UNP_CG):
        c = cg
        main = tail = 0
        while c + (unroll - 1) * UNP_CG < nchunks:
            main, c = main + 1, c + unroll * UNP_CG
        while c < nchunks:
            tail, c = tail + 1, c + UNP_CG
        out.append((main, tail))
    return out


# ---- case tables ---------------------------------------------------------------------------------------------------------------

TRANSPOSE_SHAPES = [(1, 1), (3, 5), (4, 4), (63, 65), (64, 64), (65, 63), (66, 70), (68, 132), (4, 130), (130, 4), (128, 192)]
TRANSPOSE_OFFSETS = [("aligned", 0, 0), ("w_off", 1, 0), ("wt_off", 0, 1)]          # (name, floats W is off, floats Wt is off)

# (Fout, Fin, K, W2 wanted, W3 wanted): Fout Fin K = 255, 256, 257 and larger; K = 1 .. 4; each of W2 / W3 present and NULL
PACK_CASES = [(17, 5, 3, True, True), (16, 8, 2, True, False), (257, 1, 1, False, True), (1, 257, 1, True, False),
              (33, 7, 4, False, False), (45, 19, 3, False, True), (13, 21, 1, True, True), (7, 37, 2, False, True)]

EFF_SHAPES = [(1, 1), (5, 51), (8, 32), (257, 1), (192, 128)]                      # Ka N = 1, 255, 256, 257, 3 * 64 * 128
EFF_MODES = ("exact", "real", "zero")                                              # zero: a = b = 0, non-zero finite weights


def _u(name, Fout, Fin, K, layout, nch, stride, acc, db=True, pdb=True):
    return dict(name=name, entry="unpack", Fout=Fout, Fin=Fin, K=K, layout=layout, nchunks=nch, nchunks2=0,
                pdb_stride={"F": Fout, "3F": 3 * Fout, "F+5": Fout + 5}[stride], accumulate=acc, db=db, pdb=pdb, pdb2=False)


def _v(name, Fout, Fin, nch, nch2, acc, db=True, pdb=True, pdb2=True):
    return dict(name=name, entry="unpack2", Fout=Fout, Fin=Fin, K=3, layout=1, nchunks=nch, nchunks2=nch2,
                pdb_stride=3 * Fout, accumulate=acc, db=db, pdb=pdb, pdb2=pdb2)


UNPACK_CASES = [
    #   name                Fout Fin K layout nch stride acc
    _u("tot1",               1,  1, 1, 0,   1, "F",   0),
    _u("tot31_l0",          31,  1, 1, 0,   2, "F+5", 1),
    _u("tot31_l1",           1, 31, 1, 1,   7, "3F",  0),
    _u("tot32_l2",          32,  1, 1, 2,   8, "F",   0, pdb=False),
    _u("tot32_k2_l0",        8,  2, 2, 0,   9, "F",   1),
    _u("tot32_k2_l1",        2,  8, 2, 1,  55, "F+5", 0),       # 55: seven chunks per group - one unrolled trip and a tail of 3
    _u("tot33_k3_l1",       11,  1, 3, 1,  24, "3F",  0),
    _u("tot33_k3_l0",        1, 11, 3, 0,  25, "F",   0, db=False),
    _u("tot45_l0",           5,  3, 3, 0,  31, "F+5", 1),
    _u("tot45_l1",           3,  5, 3, 1,  32, "3F",  0),
    _u("tot495_l1",         33,  5, 3, 1,  33, "3F",  1),
    _u("tot495_l2",         33, 15, 1, 2,  40, "F",   1, pdb=False),
    _u("tot495_l0",          5, 33, 3, 0,  41, "F",   0),
    _u("tot32_k4_l0",        2,  4, 4, 0,  64, "F+5", 0),
    _u("tot32_k4_l1",        4,  2, 4, 1,  65, "F",   1),
    _u("fout65_l0",         65,  7, 1, 0, 257, "F",   0),
    _u("fout32_bias",       32,  1, 1, 0,  33, "F+5", 1),
    _u("fout65_k3_l1",      65,  2, 3, 1,   9, "3F",  1),
    #   name                Fout Fin nch nch2 acc
    _v("v_tot33_a",          1, 11,   1,   1, 0),
    _v("v_tot33_b",         11,  1,   7,   7, 1),
    _v("v_tot45_a",          5,  3,   8,   8, 0),
    _v("v_tot45_nopdb2",     3,  5,   9,   9, 1, pdb2=False),
    _v("v_tot495_a",        33,  5,  25,  15, 0),
    _v("v_tot495_b",         5, 33,  32,  16, 1),
    _v("v_fout31_nodb",     31,  2,  33,  17, 0, db=False),
    _v("v_fout32_nopdb",    32,  3,  40,  33, 1, pdb=False),
    _v("v_fout65",          65,  2,  65, 257, 1),
    _v("v_tot495_long",     33,  5, 257,   9, 0),
]
UNPACK_MODES = ("exact", "real")


# ---- inputs --------------------------------------------------------------------------------------------------------------------

def _seed_of(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def _ints(rng, *shape):
    return rng.integers(-INT_MAX, INT_MAX + 1, size=shape).astype(np.float32)


def bit_patterns(seed, n):
    """n random 32-bit words with NaNs of several payloads, infinities, -0, +0 and denormals planted at fixed places."""
    w = np.random.default_rng(seed).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0x7F800000,
                        0xFF800000], np.uint32)
    m = min(n, special.size)
    w[np.linspace(0, n - 1, m).astype(np.int64)] = special[:m]
    return w


def eff_inputs(Ka, N, mode, fake=(FAKE_A, FAKE_B)):
    """-> (Wt [3 Ka, N] fp32, a, b)"""
    rng = np.random.default_rng(1000 + Ka * 7 + N)
    if mode == "exact":
        return _ints(rng, 3 * Ka, N), S1, S2
    Wt = rng.standard_normal((3 * Ka, N)).astype(np.float32)
    if mode == "zero":
        Wt[Wt == 0] = 1.0
        return Wt, 0.0, 0.0
    return Wt, fake[0], fake[1]


def unpack_inputs(c, mode, fake=(FAKE_A, FAKE_B)):
    """Arrays of a case of UNPACK_CASES: P [nchunks, tot], Pdb [nchunks, pdb_stride] (always made; pass NULL when not c['pdb']),
    P2 / Pdb2 (unpack2), dW0 / db0 (integers: the prefill when accumulate, else None), s1, s2."""
    rng = np.random.default_rng(_seed_of(c["name"]) + (0 if mode == "exact" else 7919))
    draw = (lambda *s: _ints(rng, *s)) if mode == "exact" else (lambda *s: rng.standard_normal(s).astype(np.float32))
    Fout, Fin, K = c["Fout"], c["Fin"], c["K"]
    d = dict(P=draw(c["nchunks"], Fout * Fin * K), Pdb=draw(c["nchunks"], c["pdb_stride"]), P2=None, Pdb2=None, dW0=None,
             db0=None, s1=0.0, s2=0.0)
    if c["entry"] == "unpack2":
        d.update(P2=draw(c["nchunks2"], Fin * Fout), Pdb2=draw(c["nchunks2"], Fout))
        d["s1"], d["s2"] = (S1, S2) if mode == "exact" else fake
    if c["accumulate"]:
        d.update(dW0=_ints(rng, Fout, Fin * K), db0=_ints(rng, Fout))
    return d


def unpack_expected(c, d, **over):
    """unpack_ref on a case and its inputs as the entry is called (NULL Pdb / Pdb2 / db honoured); over: replaces arguments."""
    kw = dict(P=d["P"], Pdb=d["Pdb"] if c["pdb"] else None, nchunks=c["nchunks"], Fout=c["Fout"], Fin=c["Fin"], K=c["K"],
              layout=c["layout"], pdb_stride=c["pdb_stride"], dW0=d["dW0"], db0=d["db0"], P2=d["P2"],
              Pdb2=d["Pdb2"] if c["pdb2"] else None, nchunks2=c["nchunks2"], s1=d["s1"], s2=d["s2"], want_db=c["db"])
    kw.update(over)
    return unpack_ref(**kw)
