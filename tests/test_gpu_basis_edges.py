"""-m gpu: the kernels of csrc/basis.hip that work without a tile plan (k_basis_fwd / k_basis_bwd with and without ids, the generic
forms, k_combine_small / k_expand_small and their _tile forms) and k_basis_tile at its samples-per-block and slice edges, against
the float64 restatements of tests/basis_ref.py.

The cases are the tables of tests/basis_ref.py (tests/test_basis_ref_cpu.py audits what they reach: every fill of a wave's sample
groups, both branches of the block renumbering, every remainder of the last 4-row block, merged rows of 1 .. 17, 24, 33, 64 and 203
entries, every nc and row layout, B around the 8 samples of a block).  The kernels are called through the C ABI on the test's own
buffers.  Per case:
  values      every output element within the per-element bound of basis_ref (derived, not measured); a miss names the sample,
              the row and the column;
  sentinel    outputs are prefilled with a NaN bit pattern and lie between guard regions: every defined element is overwritten,
              the guards and the rows the call does not define keep the pattern bit for bit;
  inputs      lie inside NaN-filled buffers: a read outside the tensor poisons a result;
  bitwise     where the source promises it: the rows of p2m_cheb_basis_fwd_real are those of the full forward (row kernel with
              ids, k_basis_tile), the _tile forms of the narrow kernels give what the row kernel gives alone.
The worst error-to-bound ratio per kernel is printed before anything is asserted (pytest -rP)."""
import ctypes

import numpy as np
import pytest
import torch

import basis_ref as br

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF              # a quiet NaN with a payload: untouched memory is recognised bit for bit
GUARD = 4096                       # floats before and after every output and input
INVALID = -1                       # P2M_ERR_INVALID


@pytest.fixture(scope="module")
def ops(hip_libs):
    from pose2mesh_release_amd import ops as o
    return o


# ---- plumbing -----------------------------------------------------------------------------------------------------------------

def _hip():
    from pose2mesh_release_amd import _lib
    return _lib.hip()


def _ck(rc, what):
    from pose2mesh_release_amd._lib import check
    check(rc, what)


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Out:
    """An output of n floats prefilled with the sentinel, between two guard regions."""

    def __init__(self, *shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(torch.float32)

    def bits(self):
        torch.cuda.synchronize()
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().reshape(self.shape)

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())


def _framed(a):
    """The fp32 array on the device, inside a NaN-filled buffer."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.size + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    buf[GUARD:GUARD + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
    return buf[GUARD:GUARD + a.size]


def _ints(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


class _Worst:
    """Keeps the worst error-to-bound ratio per kernel and every miss; prints before it asserts."""

    def __init__(self):
        self.worst, self.failed = {}, []

    def values(self, kernel, what, out, ref, bound, defined=None, row_ids=None):
        """out: an _Out of the shape [B, rows, C] of ref and bound.  defined [rows] or [B, rows, C] (default all): where the call
        writes.  Defined elements are overwritten and within the bound, the others keep the sentinel, the guards too."""
        bits = out.bits()
        vals = bits.view(np.float32).astype(np.float64)
        dmask = np.ones(bits.shape, bool)
        if defined is not None:
            dmask = np.broadcast_to(defined[None, :, None] if defined.ndim == 1 else defined, bits.shape)
        problems = []
        stale = dmask & (bits == SENTINEL)
        touched = ~dmask & (bits != SENTINEL)
        with np.errstate(invalid="ignore"):
            err = np.abs(vals - ref)
            miss = dmask & ~stale & ~(err <= bound)
        for name, mask in (("not written", stale), ("written but not defined by the call", touched), ("outside the bound", miss)):
            if mask.any():
                at = np.argwhere(mask)
                first = []
                for b, r, c in at[:4]:
                    row = r if row_ids is None else f"{r} (vertex {row_ids[r]})"
                    first.append(f"sample {b} row {row} column {c}: got {vals[b, r, c]:.9g}, reference {ref[b, r, c]:.9g}, "
                                 f"bound {bound[b, r, c]:.3e}")
                problems.append(f"{len(at)} elements {name} (samples {sorted(set(at[:, 0].tolist()))[:8]}, "
                                f"{len(set(at[:, 1].tolist()))} rows); first: " + "; ".join(first))
        if not out.guards_intact():
            problems.append("a guard region next to the output was written")
        ok = dmask & ~stale & (bound > 0) & np.isfinite(err)
        ratio = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
        if kernel not in self.worst or ratio > self.worst[kernel][0]:
            self.worst[kernel] = (ratio, what)
        if problems:
            print(f"  MISS {kernel} | {what}: " + " | ".join(problems))
            self.failed.append((kernel, what, problems))
        return bits

    def same_bits(self, kernel, what, got, want):
        if not np.array_equal(got, want):
            at = np.argwhere(got != want)
            msg = f"{len(at)} elements differ bitwise; first at (sample, row, column) {at[0].tolist()}"
            print(f"  MISS {kernel} | {what}: {msg}")
            self.failed.append((kernel, what, [msg]))

    def done(self):
        for kernel, (ratio, what) in sorted(self.worst.items()):
            print(f"  WORST {kernel}: error / bound {ratio:.3f} ({what})")
        assert not self.failed, self.failed


_graphs = {}


def _dev_graph(ops, name, V):
    """(restated graph, device graph), once per process; the library's split, order and plans are the restated ones."""
    if (name, V) not in _graphs:
        gc = br.graph(name, V)
        g = ops.DeviceGraph(gc.L, "cuda:0")
        p = gc.plans
        assert (g.V, g.n_real, g.n_fake, g.plan_tiles) == (V, p.n_real, p.n_fake, p.plan_tiles), (name, V, g.plan_tiles)
        assert np.array_equal(g.real_ids_host(), gc.real_order), (name, V)
        assert g.n_pair_real == p.n_pair_real and g.max_row == p.max_row and g.nnz_merged == len(gc.m.col)
        _graphs[(name, V)] = (gc, g)
    return _graphs[(name, V)]


def _fwd(g, X, B, V, F, shift):
    T1, T2 = _Out(B, V, F), _Out(B, V, F)
    _ck(_hip().p2m_cheb_basis_fwd(g.handle, _vp(X), _vp(T1.t), _vp(T2.t), B, F, shift, _st()), "p2m_cheb_basis_fwd")
    return T1, T2


def _fwd_real(g, X, B, F, shift):
    T1, T2 = _Out(B, g.n_real, F), _Out(B, g.n_real, F)
    _ck(_hip().p2m_cheb_basis_fwd_real(g.handle, _vp(X), _vp(T1.t), _vp(T2.t), B, F, shift, None, None, _st()),
        "p2m_cheb_basis_fwd_real")
    return T1, T2


def _grid(F, B, nset):
    return br.row_grid(F, B, nset) if F in br.ROW_WIDTHS else -(-B * nset * F // 256)


def _fwd_name(F):
    return f"k_basis_fwd<{F // 4}>" if F in br.ROW_WIDTHS else "k_basis_fwd_generic"


def _bwd_name(F):
    return f"k_basis_bwd<{F // 4}>" if F in br.ROW_WIDTHS else "k_basis_bwd_generic"


# ---- the row kernels ------------------------------------------------------------------------------------------------------------

def _run_forward(ops, worst, index, case):
    name, V, F, shift, B = case[:5]
    gc, g = _dev_graph(ops, name, V)
    what = f"case {index} {name} V {V} F {F} shift {shift} B {B} (grid {_grid(F, B, V)})"
    X, = br.inputs(1000 + index, (B, V >> shift, F))
    R1, R2, e1, e2 = br.planes(gc.m, X, shift)
    T1, T2 = _fwd(g, _framed(X), B, V, F, shift)
    worst.values(_fwd_name(F) + " L", what, T1, R1, e1)
    worst.values(_fwd_name(F) + " L2", what, T2, R2, e2)


@pytest.mark.parametrize("F", br.ROW_WIDTHS)
def test_row_forward(ops, F):
    """p2m_cheb_basis_fwd (k_basis_fwd<F / 4>, all rows) over FWD_CASES."""
    worst = _Worst()
    for index, case in enumerate(br.FWD_CASES):
        if case[2] == F:
            _run_forward(ops, worst, index, case)
    worst.done()


def _run_backward(ops, worst, index, case):
    name, V, F, shift, B, with_resid = case
    gc, g = _dev_graph(ops, name, V)
    Vout = V >> shift
    what = f"case {index} {name} V {V} F {F} shift {shift} B {B} resid {with_resid} (grid {_grid(F, B, Vout)})"
    d0, d1, d2, res = br.inputs(2000 + index, *[(B, V, F)] * 4)
    res = res if with_resid else None
    ref, bound = br.bwd(gc.m, d0, d1, d2, res, shift)
    dX = _Out(B, Vout, F)
    dev = [_framed(t) for t in (d0, d1, d2, res)]                # held until the results have been read
    _ck(_hip().p2m_cheb_basis_bwd(g.handle, _vp(dev[0]), _vp(dev[1]), _vp(dev[2]), _vp(dev[3]), _vp(dX.t), B, F, shift, _st()),
        "p2m_cheb_basis_bwd")
    worst.values(_bwd_name(F), what, dX, ref, bound)


@pytest.mark.parametrize("F", br.ROW_WIDTHS)
def test_row_backward(ops, F):
    """p2m_cheb_basis_bwd (k_basis_bwd<F / 4>) over BWD_CASES."""
    worst = _Worst()
    for index, case in enumerate(br.BWD_CASES):
        if case[2] == F:
            _run_backward(ops, worst, index, case)
    worst.done()


def test_generic_forward_and_backward(ops):
    """k_basis_fwd_generic / k_basis_bwd_generic (any other width) over GENERIC_CASES, both shifts, a short last block."""
    worst = _Worst()
    for index, case in enumerate(br.GENERIC_CASES):
        _run_forward(ops, worst, 100 + index, case)
        _run_backward(ops, worst, 100 + index, case)
    worst.done()


@pytest.mark.parametrize("F", br.ROW_WIDTHS)
def test_forward_of_the_real_rows_without_a_plan(ops, F):
    """p2m_cheb_basis_fwd_real on the star graphs (no plan: k_basis_fwd<F / 4> with ids, compact planes) over IDS_CASES: values,
    and bit for bit the same rows of the full forward."""
    worst = _Worst()
    for index, (name, V, Fc, shift, B) in enumerate(br.IDS_CASES):
        if Fc != F:
            continue
        gc, g = _dev_graph(ops, name, V)
        assert g.plan_tiles == (0, 0, 0)
        order = gc.real_order
        what = f"case {index} {name} V {V} ({len(order)} real) F {F} shift {shift} B {B} (grid {br.row_grid(F, B, len(order))})"
        X, = br.inputs(3000 + index, (B, V >> shift, F))
        R1, R2, e1, e2 = br.planes(gc.m, X, shift)
        Xd = _framed(X)
        T1, T2 = _fwd_real(g, Xd, B, F, shift)
        b1 = worst.values(_fwd_name(F) + " ids L", what, T1, R1[:, order], e1[:, order], row_ids=order)
        b2 = worst.values(_fwd_name(F) + " ids L2", what, T2, R2[:, order], e2[:, order], row_ids=order)
        full1, full2 = _fwd(g, Xd, B, V, F, shift)
        worst.same_bits(_fwd_name(F) + " ids L", what + ", against the full forward", b1, full1.bits()[:, order])
        worst.same_bits(_fwd_name(F) + " ids L2", what + ", against the full forward", b2, full2.bits()[:, order])
    worst.done()


# ---- the narrow kernels -------------------------------------------------------------------------------------------------------

def _kernels(gc, nc, base, real_only=False):
    return " + ".join(f"{base}_tile<{nc}>" if k == "tile" else f"{base}<{nc}>" for k in br.narrow_kernels(gc, nc, real_only))


def _combine(g, P, ldp, nc, bias, Y, B):
    return _hip().p2m_cheb_combine_small(g.handle, _vp(P), ldp, nc, _vp(bias), _vp(Y), B, _st())


def _combine_real(g, P, ldp, nc, bias, Y, B, index, out_rows, scale):
    return _hip().p2m_cheb_combine_small_real(g.handle, _vp(P), ldp, nc, _vp(bias), _vp(Y), B, _vp(index), out_rows, scale, _st())


def _expand(g, G, nc, E, lde, B):
    return _hip().p2m_cheb_expand_small(g.handle, _vp(G), nc, _vp(E), lde, B, _st())


@pytest.mark.parametrize("graph", ["stars", "band", "hub120", "mixed"])
def test_combine_small(ops, graph):
    """p2m_cheb_combine_small and _small_real over COMBINE_CASES: nc 1 .. 4, tight and 32-wide rows of P, with and without the
    bias; the real-only form leaves the padding rows alone, with out_index also the rows no vertex is sent to."""
    worst = _Worst()
    for index, (name, V, nc, ldp, with_bias, B, mode) in enumerate(br.COMBINE_CASES):
        if not name.startswith(graph):
            continue
        gc, g = _dev_graph(ops, name, V)
        what = f"case {index} {name} V {V} nc {nc} ldp {ldp} bias {with_bias} B {B} {mode}"
        P, bias = br.inputs(4000 + index, (B, V, ldp), (nc,))
        bias = bias if with_bias else None
        Pd, bd = _framed(P), _framed(bias)
        kernel = _kernels(gc, nc, "k_combine_small", mode != "full")
        if mode == "full":
            ref, bound = br.combine(gc.m, P, nc, ldp, bias)
            Y = _Out(B, V, nc)
            _ck(_combine(g, Pd, ldp, nc, bd, Y.t, B), "p2m_cheb_combine_small")
            worst.values(kernel, what, Y, ref, bound)
        elif mode == "real":
            ref, bound = br.combine(gc.m, P, nc, ldp, bias)
            Y = _Out(B, V, nc)
            _ck(_combine_real(g, Pd, ldp, nc, bd, Y.t, B, None, 0, 1.0), "p2m_cheb_combine_small_real")
            worst.values(kernel + " real", what, Y, ref, bound, defined=~gc.plans.fake)
        else:
            ref, bound = br.combine(gc.m, P, nc, ldp, bias, 1000.0)
            inv, out_rows = br.out_index(gc, index)
            kept = np.where(inv >= 0)[0]
            vertex = np.full(out_rows, -1)
            vertex[inv[kept]] = kept
            Yref, Ybound = np.zeros((B, out_rows, nc)), np.zeros((B, out_rows, nc))
            Yref[:, inv[kept]], Ybound[:, inv[kept]] = ref[:, kept], bound[:, kept]
            Y, invd = _Out(B, out_rows, nc), _ints(inv)
            _ck(_combine_real(g, Pd, ldp, nc, bd, Y.t, B, invd, out_rows, 1000.0), "p2m_cheb_combine_small_real")
            worst.values(kernel + " out_index", what, Y, Yref, Ybound, defined=vertex >= 0, row_ids=vertex)
    worst.done()


@pytest.mark.parametrize("graph", ["stars", "band", "hub120", "mixed"])
def test_expand_small(ops, graph):
    """p2m_cheb_expand_small over EXPAND_CASES: nc 1 .. 4, rows of 3 nc, 3 nc + 1 and 32 floats (G is copied exactly, the tail
    is zero)."""
    worst = _Worst()
    for index, (name, V, nc, lde, B) in enumerate(br.EXPAND_CASES):
        if not name.startswith(graph):
            continue
        gc, g = _dev_graph(ops, name, V)
        what = f"case {index} {name} V {V} nc {nc} lde {lde} B {B}"
        G, = br.inputs(5000 + index, (B, V, nc))
        ref, bound = br.expand(gc.m, G, nc, lde)
        E, Gd = _Out(B, V, lde), _framed(G)
        _ck(_expand(g, Gd, nc, E.t, lde, B), "p2m_cheb_expand_small")
        worst.values(_kernels(gc, nc, "k_expand_small"), what, E, ref, bound)
    worst.done()


def test_narrow_tile_forms_are_bitwise_the_row_kernel(ops):
    """nc = 3 on a level with a plan (k_combine_small_tile / k_expand_small_tile for the rows with neighbours, the row kernel for
    the rest) against the row kernel alone: the same graph with a star of UCAP + 2 vertices appended has the same coefficients on
    the first V rows and no plan."""
    worst = _Worst()
    for index, (name, V, B) in enumerate(br.TWIN_CASES):
        gc, g = _dev_graph(ops, name, V)
        twin = ops.DeviceGraph(br.no_plan_twin(gc.L), "cuda:0")
        Vt = twin.V
        assert g.plan_tiles[0] > 0 and twin.plan_tiles[0] == 0 and Vt > V
        what = f"case {index} {name} V {V} B {B}"
        P, bias, G = br.inputs(6000 + index, (B, Vt, 32), (3,), (B, Vt, 3))
        Y, Yt = _Out(B, V, 3), _Out(B, Vt, 3)
        Pd, Pt, bd, Gd, Gt = _framed(P[:, :V]), _framed(P), _framed(bias), _framed(G[:, :V]), _framed(G)
        _ck(_combine(g, Pd, 32, 3, bd, Y.t, B), "p2m_cheb_combine_small")
        _ck(_combine(twin, Pt, 32, 3, bd, Yt.t, B), "p2m_cheb_combine_small")
        worst.same_bits("k_combine_small_tile<3> + k_combine_small<3>", what, Y.bits(), Yt.bits()[:, :V])
        E, Et = _Out(B, V, 32), _Out(B, Vt, 32)
        _ck(_expand(g, Gd, 3, E.t, 32, B), "p2m_cheb_expand_small")
        _ck(_expand(twin, Gt, 3, Et.t, 32, B), "p2m_cheb_expand_small")
        worst.same_bits("k_expand_small_tile<3> + k_expand_small<3>", what, E.bits(), Et.bits()[:, :V])
        assert not (Y.bits() == SENTINEL).any() and not (E.bits() == SENTINEL).any()
    worst.done()


# ---- k_basis_tile -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", br.TILE_WIDTHS)
def test_basis_tile(ops, F):
    """p2m_cheb_basis_fwd_real through k_basis_tile over TILE_CASES (B = 8, 9, 16, 17 around the 8 samples of a block; 384 = three
    128-feature slices): values, and bit for bit the row kernel (384: the row kernel on each 128-feature slice)."""
    worst = _Worst()
    for index, (name, V, Fc, shift, B) in enumerate(br.TILE_CASES):
        if Fc != F:
            continue
        gc, g = _dev_graph(ops, name, V)
        nt = g.plan_tiles[shift]
        assert nt > 0
        order = gc.real_order
        what = f"case {index} {name} V {V} F {F} shift {shift} B {B} ({br.tile_blocks(nt, F, B)} blocks)"
        X, = br.inputs(7000 + index, (B, V >> shift, F))
        R1, R2, e1, e2 = br.planes(gc.m, X, shift)
        Xd = _framed(X)
        T1, T2 = _fwd_real(g, Xd, B, F, shift)
        kernel = f"k_basis_tile<{min(F // 4, 32)}> F {F}"
        b1 = worst.values(kernel + " L", what, T1, R1[:, order], e1[:, order], row_ids=order)
        b2 = worst.values(kernel + " L2", what, T2, R2[:, order], e2[:, order], row_ids=order)
        for lo in range(0, F, 128 if F == 384 else F):
            Fs = 128 if F == 384 else F
            Xs = Xd if Fs == F else _framed(X[..., lo:lo + Fs])
            full1, full2 = _fwd(g, Xs, B, V, Fs, shift)
            tag = f"{what}, against the row kernel, columns {lo} .. {lo + Fs - 1}"
            worst.same_bits(kernel + " L", tag, b1[..., lo:lo + Fs], full1.bits()[:, order])
            worst.same_bits(kernel + " L2", tag, b2[..., lo:lo + Fs], full2.bits()[:, order])
    worst.done()


def test_basis_pair(ops):
    """p2m_cheb_basis_pair (k_basis_tile over the paired plan) over PAIR_CASES against the float64 paired operator."""
    worst = _Worst()
    for index, (name, V, F, B) in enumerate(br.PAIR_CASES):
        gc, g = _dev_graph(ops, name, V)
        order = gc.plans.pair_order
        assert g.plan_tiles[2] > 0 and g.n_pair_real == len(order)
        what = f"case {index} {name} V {V} F {F} B {B} ({br.tile_blocks(g.plan_tiles[2], F, B)} blocks)"
        G, = br.inputs(8000 + index, (B, V, F))
        R1, R2, e1, e2 = br.pair_planes(gc.m, G)
        P1, P2, Gd = _Out(B, len(order), F), _Out(B, len(order), F), _framed(G)
        _ck(_hip().p2m_cheb_basis_pair(g.handle, _vp(Gd), _vp(P1.t), _vp(P2.t), B, F, _st()), "p2m_cheb_basis_pair")
        kernel = f"k_basis_tile<{min(F // 4, 32)}> paired F {F}"
        worst.values(kernel + " L", what, P1, R1[:, order], e1[:, order], row_ids=order)
        worst.values(kernel + " L2", what, P2, R2[:, order], e2[:, order], row_ids=order)
    worst.done()


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(ops):
    """Every shape the ABI cannot serve is refused with P2M_ERR_INVALID and a message, before anything is written."""
    _, odd = _dev_graph(ops, "starsA", 541)
    _, even = _dev_graph(ops, "starsA", 542)
    _, band = _dev_graph(ops, "band", 736)
    _, hub = _dev_graph(ops, "hub120", 1472)
    assert even.plan_tiles == (0, 0, 0) and band.plan_tiles[0] > 0 and hub.plan_tiles[2] == 0 and hub.plan_tiles[0] > 0
    B = 2
    big = torch.zeros(B * 1472 * 96, device="cuda")
    sc = torch.ones(384, device="cuda")
    outs = [_Out(B * 1472 * 96), _Out(B * 1472 * 96)]
    o1, o2 = outs[0].t, outs[1].t
    h, s = _hip(), _st()
    calls = [
        ("nc = 5 (combine)", "nc must be 1..4", lambda: _combine(even, big, 32, 5, None, o1, B)),
        ("nc = 5 (combine, real rows)", "nc must be 1..4", lambda: _combine_real(even, big, 32, 5, None, o1, B, None, 0, 1.0)),
        ("nc = 5 (combine, planned level)", "nc must be 1..4", lambda: _combine(band, big, 32, 5, None, o1, B)),
        ("nc = 5 (expand)", "nc must be 1..4", lambda: _expand(even, big, 5, o1, 32, B)),
        ("ldp < 3 nc (combine)", "ldp < 3*nc", lambda: _combine(even, big, 8, 3, None, o1, B)),
        ("ldp < 3 nc (combine, real rows)", "ldp < 3*nc", lambda: _combine_real(band, big, 11, 4, None, o1, B, None, 0, 1.0)),
        ("lde < 3 nc (expand)", "lde < 3*nc", lambda: _expand(band, big, 3, o1, 8, B)),
        ("shift 1 with an odd V (forward)", "even vertex count",
         lambda: h.p2m_cheb_basis_fwd(odd.handle, _vp(big), _vp(o1), _vp(o2), B, 64, 1, s)),
        ("shift 1 with an odd V (forward, generic width)", "even vertex count",
         lambda: h.p2m_cheb_basis_fwd(odd.handle, _vp(big), _vp(o1), _vp(o2), B, 5, 1, s)),
        ("shift 1 with an odd V (forward, real rows)", "even vertex count",
         lambda: h.p2m_cheb_basis_fwd_real(odd.handle, _vp(big), _vp(o1), _vp(o2), B, 64, 1, None, None, s)),
        ("shift 1 with an odd V (backward)", "even vertex count",
         lambda: h.p2m_cheb_basis_bwd(odd.handle, _vp(big), _vp(big), _vp(big), None, _vp(o1), B, 64, 1, s)),
        ("real rows at F = 96 (no plan)", "feature width 96",
         lambda: h.p2m_cheb_basis_fwd_real(even.handle, _vp(big), _vp(o1), _vp(o2), B, 96, 0, None, None, s)),
        ("real rows at F = 96 (planned level)", "feature width 96",
         lambda: h.p2m_cheb_basis_fwd_real(band.handle, _vp(big), _vp(o1), _vp(o2), B, 96, 1, None, None, s)),
        ("activation on load without a plan", "activation on load",
         lambda: h.p2m_cheb_basis_fwd_real(even.handle, _vp(big), _vp(o1), _vp(o2), B, 64, 0, _vp(sc), _vp(sc), s)),
        ("paired planes without a paired plan (stars)", "no paired operator",
         lambda: h.p2m_cheb_basis_pair(even.handle, _vp(big), _vp(o1), _vp(o2), B, 64, s)),
        ("paired planes without a paired plan (hub120)", "no paired operator",
         lambda: h.p2m_cheb_basis_pair(hub.handle, _vp(big), _vp(o1), _vp(o2), B, 64, s)),
    ]
    failed = []
    for what, needle, call in calls:
        rc = call()
        msg = h.p2m_last_error_string().decode()
        print(f"  {what}: rc {rc}, message {msg!r}")
        if rc != INVALID or needle not in msg:
            failed.append((what, rc, msg))
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.buf == SENTINEL).all()), "a refused call wrote to its output"
    assert not failed, failed
