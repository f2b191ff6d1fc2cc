"""-m gpu: the weight kernels of csrc/weights.hip (k_weight_pack, k_transpose_tiled, k_weight_eff, k_weight_grad_unpack) through
the C ABI, against the restatements and on the case tables of tests/weight_ref.py (audited by tests/test_weight_ref_cpu.py).

Every output lies between guard words and is prefilled with a NaN bit pattern (overwrite) or with integers (accumulate); the
guards stay, the inputs are bitwise unchanged after the call, an output that is NULL or whose Pdb is NULL keeps what it held.
  pack / transpose   random 32-bit words (NaN payloads, -0, denormals): the outputs are the restatement's words; the tiled
                     transpose (both bases on 16 bytes) and the general kernel (W, then Wt, 4 bytes off) give the same words
  weight_eff         integer weights and dyadic (a, b): bitwise; a = b = 0: plane 0 bitwise; normal draws with a graph's
                     (fake_a, fake_b): 4 roundings' bound
  unpack, unpack2    integer partials and dyadic factors: bitwise; normal draws with a graph's factors: the derived
                     (n1 + n2 + 3) 2^-24 S; unpack2 == unpack of P followed by an accumulating unpack of a pre-scaled P2
  wrappers           ops.weight_pack / weight_eff / weight_grad_unpack / weight_grad_unpack2 give the C ABI's words
  refusals           P2M_ERR_INVALID, a message, nothing written
Every achieved ratio is printed before it is asserted (pytest -rP).

Achieved on the MI355X (graph factors fake_a = -0.6666667, fake_b = -0.1111111): every exact case, every pack / transpose case
and both second routes: 0 differing words.  Error / bound of the real-valued cases:
  weight_eff   Ka x N = 1 x 1: 0.055, 5 x 51: 0.471, 8 x 32: 0.392, 257 x 1: 0.429, 192 x 128: 0.550
  unpack       dW: worst 0.153 (tot31_l0, 2 chunks), 0.092 at 9 chunks, <= 0.047 from 7 chunks on otherwise, 0.001 at 257;
               db: worst 0.191 (tot31_l0), <= 0.064 elsewhere
  unpack2      dW: worst 0.173 (v_tot33_a, 1 + 1 chunks), <= 0.028 elsewhere, 0.001 at 257 chunks; db: <= 0.021
The kernel sums each chunk group in fp32 and the groups in double, so what is left is mostly the one rounding to fp32 - a share
of the bound that falls as 1 / (n + 3).  The whole file takes 3 s."""
import ctypes as ct

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import weight_ref as wr

pytestmark = pytest.mark.gpu

ERR = -1                                                      # P2M_ERR_INVALID
GUARD = 64                                                    # words on either side: 256 bytes, keeps the array's alignment
NAN_WORD = 0x7FC0BEEF                                         # a quiet NaN with a payload: untouched memory is known bit for bit
INT_WORD = int(np.float32(7.0).view(np.uint32))               # guard fill around an output that is accumulated into
F32 = np.float32


@pytest.fixture(scope="module")
def lib(hip_libs):
    from pose2mesh_release_amd import _lib
    return _lib.hip()


@pytest.fixture(scope="module")
def ops(hip_libs):
    from pose2mesh_release_amd import ops as o
    return o


@pytest.fixture(scope="module")
def fake(ops):
    """(fake_a, fake_b) of a real graph: a ring of 12 vertices and 4 isolated padding vertices, rescaled as L / 3 - I."""
    V, n = 16, 12
    i = np.arange(n)
    A = sp.coo_matrix((np.ones(2 * n), (np.concatenate([i, (i + 1) % n]), np.concatenate([(i + 1) % n, i]))), shape=(V, V)).tocsr()
    d = np.asarray(A.sum(axis=0)).ravel() + np.spacing(np.float64(0))
    Dm = sp.diags(1 / np.sqrt(d))
    g = ops.DeviceGraph(((sp.identity(V) - Dm @ A @ Dm) / 3.0 - sp.identity(V)).tocsr(), "cuda:0")
    assert g.n_fake == V - n and g.fake_a != 0 and g.fake_b != 0
    assert np.frexp(g.fake_a)[0] * 2 ** 12 % 1 != 0                 # not dyadic: the products do round
    print(f"fake_a {g.fake_a!r} fake_b {g.fake_b!r}")
    return g.fake_a, g.fake_b


# ---- plumbing ------------------------------------------------------------------------------------------------------------------

def _words(a):
    """numpy fp32 / uint32 array -> its words as int32 (what torch can hold)"""
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.uint32)
    return a.view(np.int32)


class Guarded:
    """A device fp32 array of `shape` inside a buffer with GUARD sentinel words on both sides, everything prefilled with the
    word `fill`; data: words the array itself starts with; offset: floats by which it is pushed off its 16-byte boundary."""

    def __init__(self, shape, fill, offset=0, data=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD + offset,), fill, dtype=torch.int32, device="cuda")
        self.lo, self.n, self.fill = GUARD + offset, n, fill
        self.words = self.buf[self.lo:self.lo + n]
        self.view = self.words.view(torch.float32).view(*shape)
        if data is not None:
            self.words.copy_(torch.from_numpy(_words(data).reshape(-1)))
        self.before = self.bits()
        assert self.view.data_ptr() % 16 == 4 * (offset % 4)

    def ptr(self):
        return ct.c_void_p(self.view.data_ptr())

    def bits(self):
        return self.words.cpu().numpy().view(np.uint32).reshape(self.view.shape)

    def unchanged(self):
        return np.array_equal(self.bits(), self.before)

    def guards_ok(self):
        return bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.lo + self.n:] == self.fill).all())

    def all_written(self):
        return not bool((self.words == self.fill).any())


def _st():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(x):
    return None if x is None else x.ptr()


def _finish(lib, rc, expect_rc, inputs, outputs):
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, lib.p2m_last_error_string())
    for name, g in {**inputs, **outputs}.items():
        assert g is None or g.guards_ok(), f"guard words of {name} were written"
    for name, g in inputs.items():
        assert g is None or g.unchanged(), f"input {name} was written"
    if expect_rc != 0:
        assert lib.p2m_last_error_string()
        for name, g in outputs.items():
            assert g is None or g.unchanged(), f"a refused call wrote {name}"


def _same(what, got, want):
    """bitwise: prints the number of differing words and where the first ones are"""
    got, want = np.asarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    print(f"    {what}: {len(bad)} differing words of {want.size}" + (f", first at {bad[:8].tolist()}" if len(bad) else ""))
    return len(bad) == 0


def _ratio(what, got_bits, ref64, bound):
    got = np.asarray(got_bits).view(F32).astype(np.float64)
    err = np.abs(got - ref64)
    assert np.isfinite(got).all(), what
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny))
    i = np.unravel_index(np.argmax(r), r.shape)
    print(f"    {what}: err {err[i]:.3e}  bound {bound[i]:.3e}  ratio {r[i]:.3f} at {tuple(int(v) for v in i)}")
    return float(r[i])


def abi_pack(lib, W, Fout, Fin, K, w2=True, w3=True, w_off=0, wt_off=0, expect_rc=0, over=None):
    """p2m_weight_pack on the words W [Fout, Fin K] -> dict(rc, Wt, W2, W3 as uint32 arrays, or None when not asked for)"""
    gW = Guarded((Fout, Fin * K), NAN_WORD, offset=w_off, data=W)
    out = dict(Wt=Guarded((K * Fin, Fout), NAN_WORD, offset=wt_off), W2=Guarded((Fout, K * Fin), NAN_WORD),
               W3=Guarded((K * Fout, Fin), NAN_WORD))
    a = dict(W=gW, Wt=out["Wt"], W2=out["W2"] if w2 else None, W3=out["W3"] if w3 else None, Fout=Fout, Fin=Fin, K=K)
    a.update(over or {})
    rc = lib.p2m_weight_pack(_ptr(a["W"]), _ptr(a["Wt"]), _ptr(a["W2"]), _ptr(a["W3"]), a["Fout"], a["Fin"], a["K"], _st())
    _finish(lib, rc, expect_rc, dict(W=gW), out)
    for name in ("W2", "W3"):
        if a[name] is None:
            assert out[name].unchanged()
    return dict(rc=rc, **{k: (g.bits() if a[k] is not None else None) for k, g in out.items()})


def abi_eff(lib, Wt, Ka, N, a, b, expect_rc=0, over=None):
    gW, gE = Guarded((3 * Ka, N), NAN_WORD, data=Wt), Guarded((Ka, N), NAN_WORD)
    p = dict(Wt=gW, We=gE, Ka=Ka, N=N)
    p.update(over or {})
    rc = lib.p2m_weight_eff(_ptr(p["Wt"]), _ptr(p["We"]), p["Ka"], p["N"], float(a), float(b), _st())
    _finish(lib, rc, expect_rc, dict(Wt=gW), dict(We=gE))
    return gE.bits()


def abi_unpack(lib, c, d, expect_rc=0, over=None):
    """p2m_weight_grad_unpack / p2m_weight_grad_unpack2 on a case of wr.UNPACK_CASES and its inputs -> (dW words, db words)"""
    Fout, Fin, K, acc = c["Fout"], c["Fin"], c["K"], c["accumulate"]
    ins = dict(P=Guarded(d["P"].shape, NAN_WORD, data=d["P"]), Pdb=Guarded(d["Pdb"].shape, NAN_WORD, data=d["Pdb"]), P2=None,
               Pdb2=None)
    if c["entry"] == "unpack2":
        ins.update(P2=Guarded(d["P2"].shape, NAN_WORD, data=d["P2"]), Pdb2=Guarded(d["Pdb2"].shape, NAN_WORD, data=d["Pdb2"]))
    fill = INT_WORD if acc else NAN_WORD
    outs = dict(dW=Guarded((Fout, Fin * K), fill, data=d["dW0"] if acc else None),
                db=Guarded((Fout,), fill, data=d["db0"] if acc else None))
    a = dict(P=ins["P"], Pdb=ins["Pdb"] if c["pdb"] else None, nchunks=c["nchunks"], P2=ins["P2"],
             Pdb2=ins["Pdb2"] if c["pdb2"] else None, nchunks2=c["nchunks2"], dW=outs["dW"], db=outs["db"] if c["db"] else None,
             Fout=Fout, Fin=Fin, K=K, accumulate=acc, layout=c["layout"], pdb_stride=c["pdb_stride"])
    a.update(over or {})
    if c["entry"] == "unpack2":
        rc = lib.p2m_weight_grad_unpack2(_ptr(a["P"]), _ptr(a["Pdb"]), a["nchunks"], _ptr(a["P2"]), _ptr(a["Pdb2"]),
                                         a["nchunks2"], float(d["s1"]), float(d["s2"]), _ptr(a["dW"]), _ptr(a["db"]), a["Fout"],
                                         a["Fin"], a["K"], a["accumulate"], _st())
    else:
        rc = lib.p2m_weight_grad_unpack(_ptr(a["P"]), _ptr(a["Pdb"]), a["nchunks"], _ptr(a["dW"]), _ptr(a["db"]), a["Fout"],
                                        a["Fin"], a["K"], a["accumulate"], a["layout"], a["pdb_stride"], _st())
    _finish(lib, rc, expect_rc, ins, outs)
    if expect_rc == 0:
        assert acc or outs["dW"].all_written()
        if a["db"] is None or a["Pdb"] is None:
            assert outs["db"].unchanged(), "db was written although db or Pdb is NULL"
        else:
            assert acc or outs["db"].all_written()
    return outs["dW"].bits(), outs["db"].bits()


def _ids(cases):
    return [c["name"] for c in cases]


# ---- pack and transpose --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,C", wr.TRANSPOSE_SHAPES)
def test_transpose_every_arm_and_the_misaligned_fallback(lib, R, C):
    W = wr.bit_patterns(R * 1000 + C, R * C).reshape(R, C)
    want = wr.pack_ref(W, R, C, 1)[0]
    got, ok = {}, True
    for name, w_off, wt_off in wr.TRANSPOSE_OFFSETS:
        print(f"  {R} x {C} {name}: {sorted(wr.transpose_arms(R, C, w_off, wt_off))}")
        got[name] = abi_pack(lib, W, R, C, 1, w2=False, w3=False, w_off=w_off, wt_off=wt_off)["Wt"]
        ok &= _same(f"Wt ({name}) against the restatement", got[name], want)
    for name in ("w_off", "wt_off"):
        ok &= _same(f"tiled transpose against the general kernel ({name})", got["aligned"], got[name])
    assert ok


@pytest.mark.parametrize("Fout,Fin,K,w2,w3", wr.PACK_CASES)
def test_pack_general(lib, Fout, Fin, K, w2, w3):
    W = wr.bit_patterns(Fout * 1000 + Fin, Fout * Fin * K).reshape(Fout, Fin * K)
    want = dict(zip(("Wt", "W2", "W3"), wr.pack_ref(W, Fout, Fin, K)))
    got = abi_pack(lib, W, Fout, Fin, K, w2=w2, w3=w3)
    ok = True
    for name, asked in (("Wt", True), ("W2", w2), ("W3", w3)):
        if asked:
            ok &= _same(name, got[name], want[name])
        else:
            assert got[name] is None                                # (abi_pack checked that its buffer kept the fill)
    assert ok


# ---- weight_eff ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Ka,N", wr.EFF_SHAPES)
def test_weight_eff(lib, fake, Ka, N):
    worst = 0.0
    for mode in wr.EFF_MODES:
        Wt, a, b = wr.eff_inputs(Ka, N, mode, fake)
        We, S = wr.eff_ref(Wt, Ka, N, a, b)
        got = abi_eff(lib, Wt, Ka, N, a, b)
        if mode == "exact":
            assert _same(f"eff {Ka} x {N} exact", got, We.astype(F32))
        elif mode == "zero":
            assert _same(f"eff {Ka} x {N} a = b = 0 against plane 0", got, Wt[:Ka])
        else:
            worst = _ratio(f"eff {Ka} x {N} real", got, We, wr.eff_bound(S))
    print(f"  WORST weight_eff {Ka} x {N}: {worst:.3f} of its bound")
    assert worst <= 1.0


# ---- the gradient unpack -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", wr.UNPACK_CASES, ids=_ids(wr.UNPACK_CASES))
def test_unpack_exact(lib, c):
    d = wr.unpack_inputs(c, "exact")
    r = wr.unpack_expected(c, d)
    dW, db = abi_unpack(lib, c, d)
    ok = _same(f"{c['name']} dW", dW, r["dW"].astype(F32))
    if r["db"] is not None:
        ok &= _same(f"{c['name']} db", db, r["db"].astype(F32))
    assert ok


@pytest.mark.parametrize("c", wr.UNPACK_CASES, ids=_ids(wr.UNPACK_CASES))
def test_unpack_real(lib, fake, c):
    d = wr.unpack_inputs(c, "real", fake)
    r = wr.unpack_expected(c, d)
    dW, db = abi_unpack(lib, c, d)
    rw = _ratio(f"{c['name']} dW (n = {r['n_dW']})", dW, r["dW"], wr.unpack_bound(r["n_dW"], r["S_dW"]))
    rb = 0.0
    if r["db"] is not None:
        rb = _ratio(f"{c['name']} db (n = {r['n_db']})", db, r["db"], wr.unpack_bound(r["n_db"], r["S_db"]))
    print(f"  WORST {c['name']}: dW {rw:.3f}, db {rb:.3f} of the bound")
    assert rw <= 1.0 and rb <= 1.0


@pytest.mark.parametrize("c", [c for c in wr.UNPACK_CASES if c["entry"] == "unpack2"],
                         ids=_ids([c for c in wr.UNPACK_CASES if c["entry"] == "unpack2"]))
def test_unpack2_is_unpack_then_an_accumulating_unpack_of_scaled_p2(lib, c):
    """An independent second route to the same words, on integer data: layout 1 of P, then accumulate the P2 partials scaled per
    plane on the host (exact: dyadic factors)."""
    d = wr.unpack_inputs(c, "exact")
    Fout, Fin = c["Fout"], c["Fin"]
    one_w, one_b = abi_unpack(lib, c, d)
    cA = dict(c, entry="unpack", nchunks2=0, pdb2=False)
    mid_w, mid_b = abi_unpack(lib, cA, dict(d, P2=None, Pdb2=None))
    cB = dict(name=c["name"] + "/p2", entry="unpack", Fout=Fout, Fin=Fin, K=3, layout=1, nchunks=c["nchunks2"], nchunks2=0,
              pdb_stride=Fout, accumulate=1, db=c["db"], pdb=c["pdb"] and c["pdb2"], pdb2=False)
    dB = dict(P=wr.prescale_p2(d["P2"], c["nchunks2"], Fout, Fin, d["s1"], d["s2"]), Pdb=d["Pdb2"], P2=None, Pdb2=None,
              dW0=mid_w.view(F32), db0=mid_b.view(F32), s1=0.0, s2=0.0)
    two_w, two_b = abi_unpack(lib, cB, dB)
    assert _same(f"{c['name']} dW by the second route", two_w, one_w) & _same(f"{c['name']} db by the second route", two_b, one_b)


# ---- wrappers ------------------------------------------------------------------------------------------------------------------

def _t(a):
    return torch.from_numpy(_words(a).copy()).cuda().view(torch.float32)


def _b(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _case(name):
    return next(c for c in wr.UNPACK_CASES if c["name"] == name)


def test_ops_weight_pack_and_eff_give_the_abi_words(lib, ops, fake):
    Fout, Fin, K = 17, 5, 3
    W = wr.bit_patterns(3, Fout * Fin * K).reshape(Fout, Fin * K)
    want = abi_pack(lib, W, Fout, Fin, K)
    Wt, W2, W3 = ops.weight_pack(_t(W), Fin, K, need_w2=True, need_w3=True)
    assert _same("Wt", _b(Wt), want["Wt"]) & _same("W2", _b(W2), want["W2"]) & _same("W3", _b(W3), want["W3"])
    Wt, W2, W3 = ops.weight_pack(_t(W), Fin, K, need_w2=False)
    assert W2 is None and W3 is None and _same("Wt alone", _b(Wt), want["Wt"])
    R, C = 68, 132                                                   # the transpose, as posenet.py and meshnet.py call it
    W = wr.bit_patterns(4, R * C).reshape(R, C)
    assert _same("transpose", _b(ops.weight_pack(_t(W), C, 1, need_w2=False)[0]), wr.pack_ref(W, R, C, 1)[0])
    Ka, N = 5, 51
    We_in, a, b = wr.eff_inputs(Ka, N, "real", fake)
    assert _same("weight_eff", _b(ops.weight_eff(_t(We_in), Ka, N, a, b)), abi_eff(lib, We_in, Ka, N, a, b))


def test_ops_weight_grad_unpack_gives_the_abi_words(lib, ops, fake):
    # no dW: overwrite, db returned
    c = _case("tot45_l1")
    d = wr.unpack_inputs(c, "real", fake)
    want_w, want_b = abi_unpack(lib, c, d)
    dW, db = ops.weight_grad_unpack(_t(d["P"]), _t(d["Pdb"]), c["nchunks"], c["Fout"], c["Fin"], c["K"], layout=c["layout"])
    assert dW.shape == (c["Fout"], c["Fin"] * c["K"]) and db.shape == (c["Fout"],)
    assert _same("dW", _b(dW), want_w) & _same("db", _b(db), want_b)
    # dW given => accumulate (Pdb's row stride is its second dimension)
    c = _case("tot45_l0")
    d = wr.unpack_inputs(c, "real", fake)
    assert c["accumulate"] and c["pdb_stride"] == c["Fout"] + 5
    want_w, want_b = abi_unpack(lib, c, d)
    dW, db = _t(d["dW0"]), _t(d["db0"])
    r = ops.weight_grad_unpack(_t(d["P"]), _t(d["Pdb"]), c["nchunks"], c["Fout"], c["Fin"], c["K"], dW=dW, db=db, layout=0)
    assert r[0] is dW and r[1] is db and _same("dW +=", _b(dW), want_w) & _same("db +=", _b(db), want_b)
    # Pdb None => db None: no bias gradient is made, a given one is left as it is
    c = _case("tot495_l2")
    d = wr.unpack_inputs(c, "real", fake)
    assert c["accumulate"] and not c["pdb"]
    want_w, want_b = abi_unpack(lib, c, d)
    dW, db = _t(d["dW0"]), _t(d["db0"])
    ops.weight_grad_unpack(_t(d["P"]), None, c["nchunks"], c["Fout"], c["Fin"], 1, dW=dW, db=db, layout=2)
    assert _same("dW += (layout 2)", _b(dW), want_w) & _same("db left alone", _b(db), _words(d["db0"])) & \
        _same("db as the ABI left it", _b(db), want_b)
    dW2, none = ops.weight_grad_unpack(_t(d["P"]), None, c["nchunks"], c["Fout"], c["Fin"], 1, layout=2)
    over_w, _ = abi_unpack(lib, dict(c, accumulate=0), dict(d, dW0=None, db0=None))
    assert none is None and _same("dW (layout 2)", _b(dW2), over_w)


def test_ops_weight_grad_unpack2_gives_the_abi_words(lib, ops, fake):
    for name in ("v_tot45_a", "v_tot495_b"):
        c = _case(name)
        d = wr.unpack_inputs(c, "real", fake)
        want_w, want_b = abi_unpack(lib, c, d)
        args = (_t(d["P"]), _t(d["Pdb"]), c["nchunks"], _t(d["P2"]), _t(d["Pdb2"]), c["nchunks2"], d["s1"], d["s2"], c["Fout"],
                c["Fin"])
        if c["accumulate"]:
            dW, db = _t(d["dW0"]), _t(d["db0"])
            r = ops.weight_grad_unpack2(*args, dW=dW, db=db)
            assert r[0] is dW and r[1] is db
        else:
            dW, db = ops.weight_grad_unpack2(*args)
        assert _same(f"{name} dW", _b(dW), want_w) & _same(f"{name} db", _b(db), want_b)


# ---- repeatability -------------------------------------------------------------------------------------------------------------

def test_two_runs_are_bitwise_equal(lib, fake):
    for R, C, K in ((68, 132, 1), (66, 70, 1), (45, 19, 3)):
        W = wr.bit_patterns(R + C, R * C * K).reshape(R, C * K)
        a, b = (abi_pack(lib, W, R, C, K, w2=K > 1, w3=K > 1) for _ in range(2))
        assert all(_same(f"pack {R} x {C} x {K} {k}", a[k], b[k]) for k in ("Wt", "W2", "W3") if a[k] is not None)
    Wt, a, b = wr.eff_inputs(192, 128, "real", fake)
    assert _same("weight_eff", abi_eff(lib, Wt, 192, 128, a, b), abi_eff(lib, Wt, 192, 128, a, b))
    for name in ("fout65_l0", "tot495_l1", "v_fout65", "v_tot495_long"):
        c = _case(name)
        d = wr.unpack_inputs(c, "real", fake)
        (w1, b1), (w2, b2) = abi_unpack(lib, c, d), abi_unpack(lib, c, d)
        assert _same(f"{name} dW", w1, w2) & _same(f"{name} db", b1, b2)


# ---- refusals ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("over", [dict(W=None), dict(Wt=None), dict(Fout=0), dict(Fout=-1), dict(Fin=0), dict(Fin=-4), dict(K=0),
                                  dict(K=-1)], ids=str)
def test_pack_refusals(lib, over):
    W = wr.bit_patterns(1, 45).reshape(5, 9)
    assert abi_pack(lib, W, 5, 3, 3, expect_rc=ERR, over=over)["rc"] == ERR


@pytest.mark.parametrize("over", [dict(Wt=None), dict(We=None), dict(Ka=0), dict(Ka=-3), dict(N=0), dict(N=-1)], ids=str)
def test_eff_refusals(lib, over):
    Wt, a, b = wr.eff_inputs(5, 51, "exact")
    abi_eff(lib, Wt, 5, 51, a, b, expect_rc=ERR, over=over)


@pytest.mark.parametrize("over", [dict(P=None), dict(dW=None), dict(Fout=0), dict(Fin=0), dict(Fin=-1), dict(K=0), dict(K=-2),
                                  dict(nchunks=0), dict(nchunks=-1), dict(layout=3), dict(layout=-1), dict(layout=2)], ids=str)
def test_unpack_refusals(lib, over):
    c = _case("tot45_l0")                                           # K = 3: layout 2 is refused
    abi_unpack(lib, c, wr.unpack_inputs(c, "exact"), expect_rc=ERR, over=over)


@pytest.mark.parametrize("over", [dict(P=None), dict(P2=None), dict(dW=None), dict(Fout=0), dict(Fin=0), dict(Fout=-5),
                                  dict(nchunks=0), dict(nchunks=-1), dict(nchunks2=0), dict(nchunks2=-2), dict(K=1), dict(K=2),
                                  dict(K=4)], ids=str)
def test_unpack2_refusals(lib, over):
    c = _case("v_tot45_nopdb2")
    abi_unpack(lib, c, wr.unpack_inputs(c, "exact"), expect_rc=ERR, over=over)
