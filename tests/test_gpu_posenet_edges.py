"""-m gpu: the PoseNet stage kernels (csrc/posenet.hip: k_pn_stage_fwd / k_pn_stage_bwd) at their row-pass edges, and the whole
lifter past one pass of the transposed-store tile.

The cases are the table of tests/posenet_ref.py (tests/test_posenet_ref_cpu.py audits what they reach: the second to fifth trip
of pass 1 with only u = 0 live, 1 .. 3 passes of the 256-row tile with a last pass of 1 or 4 rows, 1 .. 7 live column quads next
to dead ones, odd B), each with 1 and 3 chunks of partials and the five variants of tests/test_gpu_amax.py.  Per case:
  float64     z, a, mean, invstd, the running statistics, gz, dgamma, dbeta, dbias against the float64 restatement with the bars of
              test_pn_stage_fwd / test_pn_stage_bwd (1e-5; 2e-5 max(1, max |gz|); 1e-5 sqrt(B) max(1, max |.|) in both accumulate
              modes); torch's own fp32 evaluation of the same lines errs by 0.2e-6 .. 2.8e-6 on a at these shapes
              (test_posenet_ref_cpu.py prints it), so 1e-5 is about 4 x the reference's own rounding.  aT == a.t() and
              gzT == gz.t() bitwise; padding rows exactly 0 with P, resid, rnd, G and the addend POISONED there and everything
              else bitwise what it is without the poison;
  guards      through the C entry, every output inside a larger sentinel-filled allocation, 4 floats (16 bytes) on either side:
              the guards are untouched, the rows are all written, outputs the variant does not have are not touched at all;
  columns     a column quad run alone as an F = 4 problem gives bitwise what it gives inside the wide case;
  padding     (129, 0, 36) and (132, 129, 36) hold the same 129 samples and agree bitwise;
  arms        the arms of the two C entries that no other test calls (posenet_ref.ARMS), each against float64;
  refusals    every argument check of the two entries: -1, the entry named in p2m_last_error_string, no output touched.
Every achieved figure is printed before it is asserted (pytest -s / -rP)."""
import ctypes

import numpy as np
import pytest
import torch

import posenet_ref as pr
from test_gpu_amax import _bits_equal, _chk, _pn_fwd, _poison
from test_gpu_posenet import _check_train, _model, _ref, _rel, arith  # noqa: F401  (arith: the fixture of that file)

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF              # a quiet NaN with a payload: untouched memory is recognised bit for bit
GUARD = 4                          # guard floats on either side: keeps the 16-byte alignment the kernels rely on
INIT = 1.5                         # what dgamma / dbeta / dbias hold before an accumulating backward


@pytest.fixture(scope="module")
def ops(hip_libs):
    from pose2mesh_release_amd import ops as o
    return o


# ---- plumbing ------------------------------------------------------------------------------------------------------------------

def _hip():
    from pose2mesh_release_amd import _lib
    return _lib.hip()


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(d):
    return {k: v.cuda().contiguous() for k, v in d.items()}


def _pad_rows(B, Br):
    return torch.arange(Br, B, device="cuda")


def _poisoned(d, pad):
    """A copy of the inputs with every row tensor poisoned in the padding rows."""
    q = {k: v.clone() for k, v in d.items()}
    if pad.numel():
        for k in pr.ROW_TENSORS:
            for plane in (q[k] if q[k].dim() == 3 else [q[k]]):
                _poison(plane, pad)
    return q


class _Guarded:
    """An output tensor inside a larger allocation prefilled with the sentinel."""

    def __init__(self, *shape, fill=None):
        self.n = int(np.prod(shape))
        self.flat = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.t = self.flat[GUARD:GUARD + self.n].view(*shape)
        assert self.t.data_ptr() % 16 == 0
        if fill is not None:
            self.t.copy_(torch.as_tensor(fill, dtype=torch.float32, device="cuda"))
        self.before = self.flat.clone()

    def guards_ok(self):
        b = self.flat.view(torch.int32)
        return bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + self.n:] == SENTINEL).all())

    def written(self):
        return not bool((self.t.contiguous().view(torch.int32) == SENTINEL).any())

    def untouched(self):
        return _bits_equal(self.flat, self.before)


def _c_fwd(d, nch, B, F, B_real, bias, resid, bn, p_drop, out):
    """p2m_pn_stage_fwd through the C ABI.  out: the tensors for z, a, aT, mean, invstd, rm, rv."""
    return _hip().p2m_pn_stage_fwd(
        _vp(d["P"]), nch, _vp(d["bias"]) if bias else None, _vp(d["resid"]) if resid else None, _vp(out["z"]),
        int(bn is not None), int(bn == "train"), _vp(d["gamma"]), _vp(d["beta"]), _vp(out["rm"]), _vp(out["rv"]), pr.MOMENTUM,
        pr.EPS, _vp(d["rnd"]) if (bn and p_drop > 0) else None, p_drop, _vp(out["a"]), _vp(out["aT"]), _vp(out["mean"]),
        _vp(out["invstd"]), None, B, F, B_real, _st())


def _c_bwd(d, nch, B, F, B_real, resid, bn, p_drop, z, mean, invstd, out, accumulate):
    """p2m_pn_stage_bwd through the C ABI.  out: the tensors for gz, gzT, dgamma, dbeta, dbias."""
    return _hip().p2m_pn_stage_bwd(
        _vp(d["G"]), nch, _vp(d["addend"]) if resid else None, int(bn is not None), int(bn == "train"), _vp(z), _vp(mean),
        _vp(invstd), _vp(d["gamma"]), _vp(d["beta"]), _vp(d["rnd"]) if (bn and p_drop > 0) else None, p_drop, _vp(out["gz"]),
        _vp(out["gzT"]), _vp(out["dgamma"]), _vp(out["dbeta"]), _vp(out["dbias"]), int(accumulate), None, B, F, B_real, _st())


FWD_OUT = ("z", "a", "aT", "mean", "invstd", "rm", "rv")
BWD_OUT = ("gz", "gzT", "dgamma", "dbeta", "dbias")


def _c_stage(d, nch, B, F, B_real, variant, accumulate=False):
    """Forward and backward of one variant through the C ABI with every output guarded.  Returns ({name: tensor}, {name:
    _Guarded}); the guards, `written` and `untouched` are asserted here."""
    bias, resid, bn, p_drop = variant
    init = INIT if accumulate else None
    gd = {"z": _Guarded(B, F), "a": _Guarded(B, F), "aT": _Guarded(F, B), "mean": _Guarded(F), "invstd": _Guarded(F),
          "rm": _Guarded(F, fill=d["rm"]), "rv": _Guarded(F, fill=d["rv"]), "gz": _Guarded(B, F), "gzT": _Guarded(F, B),
          "dgamma": _Guarded(F, fill=init), "dbeta": _Guarded(F, fill=init), "dbias": _Guarded(F, fill=init)}
    out = {k: v.t for k, v in gd.items()}
    rc = _c_fwd(d, nch, B, F, B_real, bias, resid, bn, p_drop, out)
    torch.cuda.synchronize()
    assert rc == 0, _hip().p2m_last_error_string()
    rc = _c_bwd(d, nch, B, F, B_real, resid, bn, p_drop, out["z"], out["mean"], out["invstd"], out, accumulate)
    torch.cuda.synchronize()
    assert rc == 0, _hip().p2m_last_error_string()
    for k, v in gd.items():
        assert v.guards_ok(), (k, variant, "guard words overwritten")
    for k in ("z", "a", "aT", "gz", "gzT", "dbias"):
        assert gd[k].written(), (k, variant, "not wholly written")
    for k in ("mean", "invstd", "dgamma", "dbeta"):
        assert (gd[k].written() if bn is not None else gd[k].untouched()), (k, variant)
    for k in ("rm", "rv"):
        assert bn == "train" or gd[k].untouched(), (k, variant)
    return out, gd


def _ops_bwd(ops, d, nch, B, F, B_real, resid, bn, p_drop, z, mean, invstd, accumulate, affine=True, want_T=True, sums=True):
    init = INIT if accumulate else float("nan")
    dg, db, dbias = (torch.full((F,), init, device="cuda") for _ in range(3))
    bnt = None if bn is None else (z, mean, invstd, d["gamma"] if affine else None, d["beta"] if affine else None, bn == "train")
    gz, gzT = ops.pn_stage_bwd(d["G"], nch, B, F, addend=d["addend"] if resid else None, bn=bnt,
                               rnd=d["rnd"] if (bn and p_drop > 0) else None, p_drop=p_drop, want_T=want_T,
                               dgamma=dg if (bn and sums) else None, dbeta=db if (bn and sums) else None,
                               dbias=dbias if sums else None, accumulate=accumulate, B_real=B_real)
    torch.cuda.synchronize()
    return gz, gzT, dg, db, dbias


def _check_fwd(r, Br, bn, z, a, mean, invstd, rm, rv, d):
    if z is not None:
        _chk("z", (z[:Br].double() - r["z"]).abs().max(), 1e-5)
    _chk("a", (a[:Br].double() - r["a"]).abs().max(), 1e-5)
    if bn is not None:
        _chk("mean", (mean.double() - r["mean"]).abs().max(), 1e-5)
        _chk("invstd", (invstd.double() - r["invstd"]).abs().max(), 1e-5)
        if bn == "train" and rm is not None:
            _chk("running_mean", (rm.double() - r["rm"]).abs().max(), 1e-5)
            _chk("running_var", (rv.double() - r["rv"]).abs().max(), 1e-5)
        elif rm is not None:
            assert torch.equal(rm, d["rm"]) and torch.equal(rv, d["rv"])


def _check_bwd(r, B, Br, bn, gz, dg, db, dbias, base):
    diff = torch.where(r["near"], torch.zeros_like(r["gz"]), gz[:Br].double() - r["gz"])
    _chk("gz", diff.abs().max(), 2e-5 * max(1.0, float(r["gz"].abs().max())))
    if dbias is not None:
        _chk("dbias", (dbias.double() - base - r["dbias"]).abs().max(), pr.sum_bar(B, r["dbias"]))
    if bn is not None and dg is not None:
        _chk("dgamma", (dg.double() - base - r["dgamma"]).abs().max(), pr.sum_bar(B, r["dgamma"]))
        _chk("dbeta", (db.double() - base - r["dbeta"]).abs().max(), pr.sum_bar(B, r["dbeta"]))


def _what(B, B_real, F, nch, variant):
    return f"B {B} B_real {B_real} F {F} nch {nch} bias {variant[0]} resid/addend {variant[1]} bn {variant[2]} p_drop {variant[3]}"


def _kinks(r):
    n = int(r["near"].sum())
    print(f"    {n} elements within {pr.KINK} of the ReLU kink")
    assert n <= pr.KINK_CAP
    return n


# ---- (a) every case against float64, padding poisoned --------------------------------------------------------------------------

@pytest.mark.parametrize("nch", pr.NCH)
@pytest.mark.parametrize("B,B_real,F", pr.EDGE_CASES)
def test_stage_edges_vs_float64(ops, monkeypatch, B, B_real, F, nch):
    """ops.pn_stage_fwd / pn_stage_bwd at the row-pass edges against the float64 restatement of tests/posenet_ref.py, with the
    bars of test_pn_stage_fwd / test_pn_stage_bwd; the backward runs on the z / mean / invstd the forward kernel saved.  Elements
    whose float64 pre-activation is within 1e-5 of the ReLU kink are left out of the gz comparison: at most 2 per variant (the
    seeds of posenet_ref.EDGE_SEEDS give none at all)."""
    monkeypatch.setattr(ops, "GEMM_ARITH", "f16x2")
    Br = B_real or B
    d = _dev(pr.case_inputs(B, B_real, F, nch))
    pad = _pad_rows(B, Br)
    dp = _poisoned(d, pad)
    for variant in pr.PN_VARIANTS:
        bias, resid, bn, p_drop = variant
        print("  " + _what(B, B_real, F, nch, variant))
        r = pr.stage_ref(d, Br, bias, resid, bn, p_drop)
        _kinks(r)
        z0, a0, aT0, mean0, invstd0, rm0, rv0 = _pn_fwd(ops, d, B, B_real, F, nch, bias, resid, bn, p_drop)
        z, a, aT, mean, invstd, rm, rv = _pn_fwd(ops, d, B, B_real, F, nch, bias, resid, bn, p_drop, pad)
        assert torch.isfinite(a).all() and torch.equal(aT, a.t()) and _bits_equal(aT, a.t())
        assert _bits_equal(a, a0) and _bits_equal(aT, aT0) and _bits_equal(z[:Br], z0[:Br])
        assert (a[Br:] == 0).all() and (aT[:, Br:] == 0).all()
        if bn is not None:
            assert _bits_equal(mean, mean0) and _bits_equal(invstd, invstd0) and _bits_equal(rm, rm0) and _bits_equal(rv, rv0)
        _check_fwd(r, Br, bn, z, a, mean, invstd, rm, rv, d)
        for accumulate in (False, True):
            gz0, gzT0, dg0, db0, dbias0 = _ops_bwd(ops, d, nch, B, F, B_real, resid, bn, p_drop, z, mean, invstd, accumulate)
            gz, gzT, dg, db, dbias = _ops_bwd(ops, dp, nch, B, F, B_real, resid, bn, p_drop, z, mean, invstd, accumulate)
            assert torch.isfinite(gz).all() and _bits_equal(gzT, gz.t()) and _bits_equal(gz, gz0) and _bits_equal(gzT, gzT0)
            assert (gz[Br:] == 0).all() and (gzT[:, Br:] == 0).all()
            assert _bits_equal(dbias, dbias0) and (bn is None or (_bits_equal(dg, dg0) and _bits_equal(db, db0)))
            print(f"    accumulate {accumulate}")
            _check_bwd(r, B, Br, bn, gz, dg, db, dbias, INIT if accumulate else 0.0)


# ---- (b) guard words -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nch", pr.NCH)
@pytest.mark.parametrize("B,B_real,F", pr.EDGE_CASES)
def test_stage_edges_guard_words(ops, monkeypatch, B, B_real, F, nch):
    """Both C entries with every output - z, a, aT, mean, invstd, both running vectors, gz, gzT, dgamma, dbeta, dbias - inside a
    sentinel-filled allocation with 4 guard floats on either side, the padding rows of the inputs poisoned: the guards are
    untouched (the kernels write their rows and no more: the dead quads of F = 4, 28, 36, 68, the last tile pass), the outputs
    are wholly written, outputs the variant does not have keep the sentinel, and everything is bitwise what ops.pn_stage_*
    returns."""
    monkeypatch.setattr(ops, "GEMM_ARITH", "f32")
    Br = B_real or B
    d = _dev(pr.case_inputs(B, B_real, F, nch))
    pad = _pad_rows(B, Br)
    dp = _poisoned(d, pad)
    for variant in pr.PN_VARIANTS:
        bias, resid, bn, p_drop = variant
        z, a, aT, mean, invstd, rm, rv = _pn_fwd(ops, d, B, B_real, F, nch, bias, resid, bn, p_drop, pad)
        for accumulate in (False, True):
            out, _ = _c_stage(dp, nch, B, F, B_real, variant, accumulate)
            gz, gzT, dg, db, dbias = _ops_bwd(ops, dp, nch, B, F, B_real, resid, bn, p_drop, z, mean, invstd, accumulate)
            same = {"z": z, "a": a, "aT": aT, "gz": gz, "gzT": gzT, "dbias": dbias}
            if bn is not None:
                same.update(mean=mean, invstd=invstd, rm=rm, rv=rv, dgamma=dg, dbeta=db)
            for k, t in same.items():
                rows = slice(0, Br) if k == "z" else slice(None)
                assert _bits_equal(out[k][rows], t[rows]), (k, variant, accumulate)
    print(f"  B {B} B_real {B_real} F {F} nch {nch}: 12 guarded outputs x {len(pr.PN_VARIANTS)} variants x 2 accumulate modes")


# ---- (c) column independence ---------------------------------------------------------------------------------------------------

def _quads(F):
    """First columns of the quads run alone: the first, the last quad of a full block (or the last live quad next to a dead
    one), the lone quad of the last block."""
    return sorted({0, min(pr.PN_COLS, F) - 4, F - 4})


@pytest.mark.parametrize("nch", pr.NCH)
@pytest.mark.parametrize("B,B_real,F", [c for c in pr.EDGE_CASES if c[2] > 4])
def test_stage_edges_column_independence(B, B_real, F, nch, hip_libs):
    """Columns [c, c + 4) of a case run alone as an F = 4 problem give bitwise the z, a, mean, invstd, gz, dgamma, dbeta and
    dbias they give inside the wide case: a column's sums are formed by the same threads in the same row order whatever the
    block and whatever the quad, so a difference is a cross-column leak in pn_colsum or in the tile."""
    Br = B_real or B
    d = _poisoned(_dev(pr.case_inputs(B, B_real, F, nch)), _pad_rows(B, Br))
    assert _quads(F) == {28: [0, 24], 32: [0, 28], 36: [0, 28, 32], 68: [0, 28, 64]}[F]
    for variant in pr.PN_VARIANTS:
        wide, _ = _c_stage(d, nch, B, F, B_real, variant)
        for c in _quads(F):
            narrow_in = {k: v[..., c:c + 4].contiguous() for k, v in d.items()}
            narrow, _ = _c_stage(narrow_in, nch, B, 4, B_real, variant)
            names = ["z", "a", "gz", "dbias"] + (["mean", "invstd", "dgamma", "dbeta", "rm", "rv"] if variant[2] else [])
            for k in names:
                rows = slice(0, Br) if k == "z" else slice(None)
                assert _bits_equal(narrow[k][rows], wide[k][..., c:c + 4][rows]), (k, c, variant)
            assert _bits_equal(narrow["aT"], wide["aT"][c:c + 4]) and _bits_equal(narrow["gzT"], wide["gzT"][c:c + 4])
    print(f"  B {B} B_real {B_real} F {F} nch {nch}: quads at columns {_quads(F)} bitwise those of the wide case")


# ---- (d) padding independence --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nch", pr.NCH)
def test_stage_edges_padding_independence(ops, monkeypatch, nch):
    """(129, 0, 36) and (132, 129, 36) are the same 129 samples, straight through the C entry with an odd B and zero-padded to a
    multiple of 4: bitwise the same a[:129], mean, invstd, running statistics, gz[:129], dgamma, dbeta and dbias."""
    monkeypatch.setattr(ops, "GEMM_ARITH", "f32")
    F, Br = 36, 129
    runs = []
    for B, B_real in ((129, 0), (132, 129)):
        d = _dev(pr.case_inputs(B, B_real, F, nch))
        d = _poisoned(d, _pad_rows(B, Br))
        res = []
        for bias, resid, bn, p_drop in pr.PN_VARIANTS:
            z, a, aT, mean, invstd, rm, rv = _pn_fwd(ops, d, B, B_real, F, nch, bias, resid, bn, p_drop)
            gz, gzT, dg, db, dbias = _ops_bwd(ops, d, nch, B, F, B_real, resid, bn, p_drop, z, mean, invstd, False)
            res.append({"z": z[:Br], "a": a[:Br], "aT": aT[:, :Br], "mean": mean, "invstd": invstd, "rm": rm, "rv": rv,
                        "gz": gz[:Br], "gzT": gzT[:, :Br], "dgamma": dg, "dbeta": db, "dbias": dbias, "bn": bn})
        runs.append(res)
    for variant, r0, r1 in zip(pr.PN_VARIANTS, *runs):
        for k in r0:
            if k == "bn" or r0[k] is None or (r0["bn"] is None and k in ("dgamma", "dbeta")):
                continue
            assert _bits_equal(r0[k], r1[k]), (k, variant)
    print(f"  nch {nch}: B = 129 and B = 132 with 3 padding rows agree bitwise in {len(pr.PN_VARIANTS)} variants")


# ---- (e) the arms no other test calls ------------------------------------------------------------------------------------------

def _arm(name, B, B_real, F):
    d, Br = pr.arm_inputs(name, B, B_real, F)
    d = _dev(d)
    r = pr.arm_ref(name, d, Br)
    print(f"  {name}: {Br} of {B} rows hold samples")
    _kinks(r)
    return d, _poisoned(d, _pad_rows(B, Br)), Br, r, pr.ARMS[name]


def _bn_tuple(d, bn, affine=True, running=True):
    rm, rv = (d["rm"].clone(), d["rv"].clone()) if running else (None, None)
    return (d["gamma"] if affine else None, d["beta"] if affine else None, rm, rv, pr.MOMENTUM, pr.EPS, bn == "train")


@pytest.mark.parametrize("B,B_real,F", pr.ARM_SHAPES)
def test_stage_arms_without_z(ops, monkeypatch, B, B_real, F):
    """want_z=False (z == NULL: one chunk, no bias, no residual - P is the tensor itself and is read again in pass 2), in train
    mode with dropout, in eval mode and without BatchNorm, against float64."""
    monkeypatch.setattr(ops, "GEMM_ARITH", "f32")
    for name in ("no_z_train", "no_z_eval", "no_z_plain"):
        d, dp, Br, r, (nch, bias, resid, bn, p_drop, affine, _) = _arm(name, B, B_real, F)
        bnt = None if bn is None else _bn_tuple(d, bn)
        keep = dp["P"].clone()
        z, a, aT, mean, invstd = ops.pn_stage_fwd(dp["P"], 1, B, F, want_z=False, bn=bnt, rnd=dp["rnd"] if p_drop > 0 else None,
                                                  p_drop=p_drop, B_real=B_real)
        torch.cuda.synchronize()
        assert z is None and _bits_equal(dp["P"], keep)                      # P is an input: not written
        assert torch.isfinite(a).all() and _bits_equal(aT, a.t()) and (a[Br:] == 0).all()
        _check_fwd(r, Br, bn, None, a, mean, invstd, None if bn is None else bnt[2], None if bn is None else bnt[3], d)
        if bn is None:
            assert _bits_equal(a[:Br], d["P"][0, :Br])                       # a = z = P, copied


@pytest.mark.parametrize("B,B_real,F", pr.ARM_SHAPES)
def test_stage_arms_null_affine_and_no_running(ops, monkeypatch, B, B_real, F):
    """NULL gamma / beta (the kernels' defaults 1 / 0), forward and backward with dgamma / dbeta still formed; training with
    NULL running statistics; the eval-mode backward with an addend.  Each against float64, padding poisoned."""
    monkeypatch.setattr(ops, "GEMM_ARITH", "f32")
    for name in ("null_affine_train", "null_affine_eval", "no_running", "eval_addend"):
        d, dp, Br, r, (nch, bias, resid, bn, p_drop, affine, _) = _arm(name, B, B_real, F)
        running = name != "no_running"
        bnt = _bn_tuple(d, bn, affine, running)
        z, a, aT, mean, invstd = ops.pn_stage_fwd(dp["P"], nch, B, F, bias=d["bias"] if bias else None,
                                                  resid=dp["resid"] if resid else None, bn=bnt,
                                                  rnd=dp["rnd"] if p_drop > 0 else None, p_drop=p_drop, B_real=B_real)
        torch.cuda.synchronize()
        assert torch.isfinite(a).all() and _bits_equal(aT, a.t()) and (a[Br:] == 0).all()
        _check_fwd(r, Br, bn, z, a, mean, invstd, bnt[2], bnt[3], d)
        for accumulate in (False, True):
            gz, gzT, dg, db, dbias = _ops_bwd(ops, dp, nch, B, F, B_real, resid, bn, p_drop, z, mean, invstd, accumulate, affine)
            assert torch.isfinite(gz).all() and _bits_equal(gzT, gz.t()) and (gz[Br:] == 0).all()
            _check_bwd(r, B, Br, bn, gz, dg, db, dbias, INIT if accumulate else 0.0)


@pytest.mark.parametrize("B,B_real,F", pr.ARM_SHAPES)
def test_stage_arms_single_outputs(ops, monkeypatch, B, B_real, F):
    """a without aT and aT without a; the backward without gzT (want_T=False) and, with BatchNorm, without dgamma / dbeta /
    dbias: each against float64 and bitwise what the full call gives."""
    monkeypatch.setattr(ops, "GEMM_ARITH", "f32")
    d, dp, Br, r, (nch, bias, resid, bn, p_drop, affine, _) = _arm("single_outputs", B, B_real, F)

    def fwd(**kw):
        bnt = _bn_tuple(d, bn)
        out = ops.pn_stage_fwd(dp["P"], nch, B, F, bias=d["bias"], resid=dp["resid"], bn=bnt, rnd=dp["rnd"], p_drop=p_drop,
                               B_real=B_real, **kw)
        torch.cuda.synchronize()
        return out + (bnt[2], bnt[3])

    z, a, aT, mean, invstd, rm, rv = fwd()
    z1, a1, aT1, mean1, invstd1, rm1, rv1 = fwd(want_aT=False)
    z2, a2, aT2, mean2, invstd2, rm2, rv2 = fwd(want_a=False)
    assert aT1 is None and a2 is None
    _check_fwd(r, Br, bn, z1, a1, mean1, invstd1, rm1, rv1, d)
    _check_fwd(r, Br, bn, z2, aT2.t(), mean2, invstd2, rm2, rv2, d)
    assert _bits_equal(a1, a) and _bits_equal(aT2, aT) and _bits_equal(aT2, a.t()) and (aT2[:, Br:] == 0).all()
    for x, y in ((z1, z), (z2, z)):
        assert _bits_equal(x[:Br], y[:Br])
    for x, y in ((mean1, mean), (mean2, mean), (invstd1, invstd), (invstd2, invstd), (rm1, rm), (rm2, rm), (rv1, rv), (rv2, rv)):
        assert _bits_equal(x, y)
    gz, gzT, dg, db, dbias = _ops_bwd(ops, dp, nch, B, F, B_real, resid, bn, p_drop, z, mean, invstd, False)
    gz1, gzT1, _, _, dbias1 = _ops_bwd(ops, dp, nch, B, F, B_real, resid, bn, p_drop, z, mean, invstd, False, want_T=False)
    gz2, gzT2, _, _, _ = _ops_bwd(ops, dp, nch, B, F, B_real, resid, bn, p_drop, z, mean, invstd, False, sums=False)
    assert gzT1 is None and _bits_equal(gz1, gz) and _bits_equal(dbias1, dbias)
    assert _bits_equal(gz2, gz) and _bits_equal(gzT2, gzT) and _bits_equal(gzT2, gz.t())
    _check_bwd(r, B, Br, bn, gz1, None, None, dbias1, 0.0)
    _check_bwd(r, B, Br, bn, gz2, None, None, None, 0.0)


@pytest.mark.parametrize("B,B_real,F", pr.ARM_SHAPES)
def test_stage_arms_one_sample(ops, monkeypatch, B, B_real, F):
    """B_real = 1 (all other rows padding, poisoned).  eval: forward and backward against float64.  train, through the C entry
    (PoseNet itself refuses it as F.batch_norm does): mean = z[0] and variance 0, so invstd = 1 / sqrt(eps) - held to 4 fp32
    roundings of its own size, 4 x 2^-24 x 316.2 = 7.5e-5: eps is rounded to fp32 and sqrtf and the division round once each -,
    xhat = 0 exactly and a[0] = dropout(relu(beta)) bit for bit (p = 0.5: the scale 2 is exact); the running variance moves
    towards 0 with the factor 1 in place of Br / (Br - 1); the backward is finite, and as the gradient through a one-sample
    BatchNorm is exactly 0 (g_u - mean(g_u) = 0 and xhat = 0), gz[0] is the addend."""
    monkeypatch.setattr(ops, "GEMM_ARITH", "f32")
    d, dp, Br, r, (nch, bias, resid, bn, p_drop, affine, _) = _arm("one_sample_eval", B, B_real, F)
    assert Br == 1
    bnt = _bn_tuple(d, bn)
    z, a, aT, mean, invstd = ops.pn_stage_fwd(dp["P"], nch, B, F, bias=d["bias"], resid=dp["resid"], bn=bnt, rnd=dp["rnd"],
                                              p_drop=p_drop, B_real=1)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and _bits_equal(aT, a.t()) and (a[1:] == 0).all()
    _check_fwd(r, 1, bn, z, a, mean, invstd, bnt[2], bnt[3], d)
    gz, gzT, dg, db, dbias = _ops_bwd(ops, dp, nch, B, F, 1, resid, bn, p_drop, z, mean, invstd, False)
    assert torch.isfinite(gz).all() and _bits_equal(gzT, gz.t()) and (gz[1:] == 0).all()
    _check_bwd(r, B, 1, bn, gz, dg, db, dbias, 0.0)
    # train mode
    d, dp, Br, r, (nch, bias, resid, bn, p_drop, affine, _) = _arm("one_sample_train", B, B_real, F)
    out, _ = _c_stage(dp, nch, B, F, 1, (bias, resid, bn, p_drop))
    for k in FWD_OUT + BWD_OUT:
        assert torch.isfinite(out[k][:1] if k == "z" else out[k]).all(), k
    assert (out["a"][1:] == 0).all() and (out["aT"][:, 1:] == 0).all() and (out["gz"][1:] == 0).all() and (out["gzT"][:, 1:] == 0).all()
    _chk("z", (out["z"][:1].double() - r["z"]).abs().max(), 1e-5)
    assert _bits_equal(out["mean"], out["z"][0])
    _chk("invstd", (out["invstd"].double() - pr.EPS ** -0.5).abs().max(), 4 * 2.0 ** -24 * pr.EPS ** -0.5)
    want = torch.where(d["rnd"][0] >= p_drop, torch.relu(d["beta"]) * 2.0, torch.zeros_like(d["beta"]))
    assert p_drop == 0.5 and _bits_equal(out["a"][0], want) and _bits_equal(out["aT"][:, 0], want)
    _chk("a", (out["a"][:1].double() - r["a"]).abs().max(), 1e-5)
    _chk("running_mean", (out["rm"].double() - r["rm"]).abs().max(), 1e-5)
    _chk("running_var", (out["rv"].double() - r["rv"]).abs().max(), 1e-5)
    assert float((r["rv"] - 0.9 * d["rv"].double()).abs().max()) < 1e-12
    assert torch.equal(out["gz"][0], d["addend"][0]) and torch.equal(out["gzT"][:, 0], d["addend"][0])
    _chk("gz", (out["gz"][:1].double() - r["gz"]).abs().max(), 2e-5 * max(1.0, float(r["gz"].abs().max())))


# ---- (f) refusals --------------------------------------------------------------------------------------------------------------

def test_stage_refusals(hip_libs):
    """Every argument check of p2m_pn_stage_fwd / p2m_pn_stage_bwd: the call returns -1, p2m_last_error_string names the entry,
    and the sentinel-filled outputs are untouched."""
    B, F, nch = 36, 8, 2
    d = _dev(pr.pn_inputs(B, F, nch, 1))
    lib = _hip()

    def outputs():
        gd = {k: _Guarded(*s) for k, s in (("z", (B, F)), ("a", (B, F)), ("aT", (F, B)), ("mean", (F,)), ("invstd", (F,)),
                                            ("rm", (F,)), ("rv", (F,)), ("gz", (B, F)), ("gzT", (F, B)), ("dgamma", (F,)),
                                            ("dbeta", (F,)), ("dbias", (F,)))}
        return gd, {k: v.t for k, v in gd.items()}

    def refused(entry, rc, gd, why):
        torch.cuda.synchronize()
        msg = lib.p2m_last_error_string()
        print(f"    {why}: status {rc}, {msg.decode()!r}")
        assert rc == -1 and entry in msg, (why, rc, msg)
        assert all(v.untouched() for v in gd.values()), why

    V = (True, True, "train", 0.5)
    fwd_cases = [
        ("F % 4 != 0", dict(F=6)), ("B_real > B", dict(B_real=B + 1)), ("B_real < 0", dict(B_real=-1)), ("nch < 1", dict(nch=0)),
        ("z == NULL with two chunks", dict(want_z=False, variant=(False, False, "eval", 0.0))),
        ("z == NULL with a bias", dict(want_z=False, nch=1, variant=(True, False, "eval", 0.0))),
        ("z == NULL with a residual", dict(want_z=False, nch=1, variant=(False, True, "eval", 0.0))),
        ("BatchNorm without mean", dict(drop=("mean",))), ("BatchNorm without invstd", dict(drop=("invstd",))),
        ("eval BatchNorm without running statistics", dict(running=False, variant=(True, True, "eval", 0.0))),
        ("p_drop = 1 with rnd", dict(variant=(True, True, "train", 1.0))),
        ("p_drop < 0 with rnd", dict(variant=(True, True, "eval", -0.5))),
    ]
    for why, kw in fwd_cases:
        gd, out = outputs()
        for k in kw.get("drop", ()):
            out[k] = None
        bias, resid, bn, p_drop = kw.get("variant", V)
        rnd_on = bn and p_drop != 0                      # (a refused p_drop still comes with its uniform numbers)
        rc = lib.p2m_pn_stage_fwd(
            _vp(d["P"]), kw.get("nch", nch), _vp(d["bias"]) if bias else None, _vp(d["resid"]) if resid else None,
            _vp(out["z"]) if kw.get("want_z", True) else None, int(bn is not None), int(bn == "train"), _vp(d["gamma"]), _vp(d["beta"]),
            _vp(out["rm"]) if kw.get("running", True) else None, _vp(out["rv"]) if kw.get("running", True) else None, pr.MOMENTUM,
            pr.EPS, _vp(d["rnd"]) if rnd_on else None, p_drop, _vp(out["a"]), _vp(out["aT"]), _vp(out["mean"]), _vp(out["invstd"]),
            None, B, kw.get("F", F), kw.get("B_real", 0), _st())
        refused(b"p2m_pn_stage_fwd", rc, gd, "forward, " + why)
    bwd_cases = [
        ("F % 4 != 0", dict(F=6)), ("B_real > B", dict(B_real=B + 1)), ("nch < 1", dict(nch=0)),
        ("BatchNorm without z", dict(no=("z",))), ("BatchNorm without mean", dict(no=("mean",))),
        ("BatchNorm without invstd", dict(no=("invstd",))), ("no gz", dict(drop=("gz",))),
        ("p_drop = 1 with rnd", dict(p_drop=1.0)),
    ]
    stats = {"z": d["resid"], "mean": d["rm"], "invstd": d["rv"]}
    for why, kw in bwd_cases:
        gd, out = outputs()
        for k in kw.get("drop", ()):
            out[k] = None
        s = {k: (None if k in kw.get("no", ()) else v) for k, v in stats.items()}
        rc = lib.p2m_pn_stage_bwd(
            _vp(d["G"]), kw.get("nch", nch), _vp(d["addend"]), 1, 1, _vp(s["z"]), _vp(s["mean"]), _vp(s["invstd"]), _vp(d["gamma"]),
            _vp(d["beta"]), _vp(d["rnd"]), kw.get("p_drop", 0.5), _vp(out["gz"]), _vp(out["gzT"]), _vp(out["dgamma"]),
            _vp(out["dbeta"]), _vp(out["dbias"]), 0, None, B, kw.get("F", F), kw.get("B_real", 0), _st())
        refused(b"p2m_pn_stage_bwd", rc, gd, "backward, " + why)
    # the same arguments without the fault are accepted
    gd, out = outputs()
    assert _c_fwd(d, nch, B, F, 0, True, True, "train", 0.5, out) == 0
    assert _c_bwd(d, nch, B, F, 0, True, "train", 0.5, out["z"], out["mean"], out["invstd"], out, False) == 0
    torch.cuda.synchronize()
    assert all(v.guards_ok() for v in gd.values())


# ---- the whole lifter past one tile pass ---------------------------------------------------------------------------------------

HID = 128      # the narrowest width the HIP path accepts (LinearModel.forward: linear_size % 128 == 0)


@pytest.mark.parametrize("B", [129, 257, 300])
def test_posenet_train_past_one_tile_pass(arith, B):
    """The whole lifter at hid = 128, J = 17, in train() with B = 129, 257 (zero-padded to 132 and 260) and 300: the stage kernels
    make a second and third trip of pass 1 and a second pass of the tile, and B is a tile dimension of every contraction.
    Forward and every gradient against the float64 restatement run with the ReLU masks the kernels used (_check_train of
    tests/test_gpu_posenet.py, loose = 1); running statistics and num_batches_tracked as
    test_posenet_train_batch_statistics_vs_oracle checks them."""
    import meshnet_oracle as mo
    from pose2mesh_release_amd import ops, synth
    J = 17
    net, sd = _model(J, p_dropout=0.0, hid=HID)
    net = net.cuda().train()
    x = synth.pose2d_batch(B, J, seed=6).reshape(B, -1)
    w = torch.randn(B, 3 * J, generator=torch.Generator().manual_seed(10))
    ops.TIMER = ops.KernelTimer()
    try:
        kinks, errs = _check_train(net, sd, x, w, B, loose=1.0)
        launches = ops.TIMER.summary()["pn_gemm"]["launches"]
    finally:
        ops.TIMER = None
    assert launches == 6 + 11                                         # the HIP path ran: every Linear a pn_gemm contraction
    print(f"  B {B} {arith}: kinks {kinks}; worst gradient error {max(errs.values()):.3e} (bound 5e-5)")
    sd32 = {k: v.clone() for k, v in sd.items()}
    mo.posenet_forward(sd32, x, True)                                 # fp32 oracle: updates its running statistics in place
    now = net.state_dict()
    for k, v in sd32.items():
        if "running" in k:
            assert float((now[k].cpu() - v).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max())), k
        if k.endswith("num_batches_tracked") and k.startswith("linear_stages"):
            assert int(now[k]) == int(sd[k]) + 1, k


@pytest.mark.parametrize("B", [129, 257, 300])
def test_posenet_eval_past_one_tile_pass(arith, B):
    """The same lifter in eval(): forward within 2e-5 max(1, max |ref|) and every gradient within 5e-5 (relative L2) of float64,
    the bars of test_posenet_eval_forward_and_gradients_vs_oracle."""
    from pose2mesh_release_amd import synth
    J = 17
    net, sd = _model(J, hid=HID)
    net = net.cuda().eval()
    x = synth.pose2d_batch(B, J, seed=5).reshape(B, -1)
    w = torch.randn(B, 3 * J, generator=torch.Generator().manual_seed(9))
    xg = x.cuda().requires_grad_(True)
    out = net(xg)
    assert out.shape == (B, 3 * J)
    (out * w.cuda()).sum().backward()
    x64 = x.double().requires_grad_(True)
    ref, sd64, names = _ref(sd, x64, False)
    (ref * w.double()).sum().backward()
    ref = ref.detach()
    scale = float(ref.abs().max())
    err = float((out.detach().cpu().double() - ref).abs().max())
    print(f"  B {B} {arith}: forward err {err:.3e}  bound {2e-5 * max(1.0, scale):.3e}")
    assert err <= 2e-5 * max(1.0, scale)
    got = dict(net.named_parameters())
    errs = {k: _rel(got[k].grad, sd64[k].grad) for k in names}
    errs["x"] = _rel(xg.grad, x64.grad)
    print(f"  worst gradient error {max(errs.values()):.3e} ({max(errs, key=errs.get)})  bound 5e-5")
    assert max(errs.values()) <= 5e-5, errs
