"""-m gpu: the epilogue shared by k_gemm_planes, k_gemm_planes_ws and k_gemm_rows_k1 (csrc/gemm_planes.hip: bias, activation, addend, the
stores through the row table, the un-pool pair sums, the BatchNorm partials and the amax word) at small shapes, in all three
arithmetics, through the C ABI as in tests/test_gpu_gemm_edges.py.

Shapes: B = 2, V = 300; row sets of 130 ids (one full tile + 2 rows) and of 5 ids; flat M = 130 and 257; pair sums at M = 260;
Ka in {32, 64, 128}; N in {32, 64, 128, 256} (32: the upper half of the 64-wide tile is a wave with no column; 256: two n-tiles);
three output planes of Nc in {32, 64, 128}.  The MFMA entries admit Nc % 32 == 0 only (any other Nc runs the scalar kernels, which
have no part in this epilogue), so there is no case with another Nc.
  values      against tests/gemm_ref.py in float64 at tol_fwd; C is prefilled with a NaN sentinel: rows outside the set keep it,
              everything else is written;
  addend      C with an addend is bitwise fp32(C without + addend), formed with torch on the device;
  planes      a three-plane output is bitwise the column blocks of the one-plane run at N = 3 Nc;
  pair sums   bitwise fp32(row 2 r + row 2 r + 1) of the run without them; the amax word is their largest magnitude;
  statistics  the partials, plain and with row weights (classes of 3, 2, 1 rows), within TOL_STAT_*, and - one A plane, the slice
              arithmetics - bitwise those of the other dispatch (P2M_ROWS_K1 = 0, read once per process: one child process runs
              the same cases under it and every array is compared bit for bit);
  amax        the word is the largest |value stored|, exactly.
Every figure is printed before it is asserted (pytest -rP)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gemm_ref as gr                      # noqa: E402
import tile_plan_ref as tp                 # noqa: E402

pytestmark = pytest.mark.gpu

B, V = 2, 300
NSETS = (130, 5)
# (Ka, N, planes of A): every Ka and N of the docstring with one plane (k_gemm_rows_k1 in the slice arithmetics) and the ring
# kernel's three-plane form at both tile widths
ROW_SHAPES = ((32, 32, 1), (64, 64, 1), (128, 128, 1), (32, 256, 1), (64, 128, 3), (32, 32, 3))
FLAT_SHAPES = ((130, 32, 64, 1), (257, 64, 128, 1), (130, 128, 32, 3), (257, 32, 256, 3))        # (M, Ka, N, planes)
PLANE_NC = (32, 64, 128)
SLICED = ("bf16x3", "f16x2")


def level(nset, classes):
    """(L, ids of row set 2, weight of each) of a graph of V vertices whose row set 2 has `nset` rows: a ring with chords of
    real vertices, then the isolated fake ones (tests/_child_rows_k1.py); `classes`: runs of 3, 2, 1 .. fake rows, the first of
    each is its representative."""
    sizes = np.array([3 - i % 3 for i in range(nset)] if classes else [1] * nset, dtype=np.int64)
    nreal = V - int(sizes.sum())
    assert nreal > 34
    i = np.arange(nreal)
    A = tp._sym(np.concatenate([i, i, i]), np.concatenate([(i + 1) % nreal, (i + 5) % nreal, (i + 17) % nreal]), V)
    first = nreal + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rep = np.arange(V, dtype=np.int32)
    for f, s in zip(first, sizes):
        rep[f:f + s] = f
    return tp.laplacian(A, V), first.astype(np.int64), sizes.astype(np.float64), rep


def row_inputs(nset, Ka, N, planes, seed):
    gen = torch.Generator().manual_seed(seed)
    A = [torch.randn(B * V, Ka, generator=gen)] + [torch.randn(B * nset, Ka, generator=gen) for _ in range(planes - 1)]
    Bm = torch.randn(planes * Ka, N, generator=gen) / (planes * Ka) ** 0.5
    return A, Bm, torch.randn(N, generator=gen), torch.randn(B * V, N, generator=gen)


class Runner:
    """The launches of one process: device graphs per (nset, classes), the C ABI calls."""

    def __init__(self):
        import test_gpu_gemm_edges as ge
        from pose2mesh_release_amd import ops
        self.ge, self.ops, self.hip, self.graphs = ge, ops, ge._hip(), {}

    def graph(self, nset, classes):
        if (nset, classes) not in self.graphs:
            L, ids, wts, rep = level(nset, classes)
            g = self.ops.DeviceGraph(L, "cuda:0")
            assert g.V == V
            if classes:
                g.set_classes(rep)
            assert np.array_equal(g.fake_ids_host(), ids), (nset, classes)
            self.graphs[(nset, classes)] = (g, ids, wts)
        return self.graphs[(nset, classes)]

    def rows(self, arith, nset, classes, A, Bm, bias, addend, stats, amax):
        """p2m_gemm_planes_rows over row set 2 -> (C, statistics, amax word)."""
        ge = self.ge
        g, ids, _ = self.graph(nset, classes)
        Ka, N = A[0].shape[1], Bm.shape[1]
        rows = gr.logical_rows(ids, V, B, "cuda")
        word, Bx = ge._word(arith, A[0][rows], *A[1:]), ge._split(Bm, arith)     # (named: they live until the launch has run)
        C = ge._sentinel(B * V, N)
        tps = -(-nset // gr.TILE)
        st = ge._sentinel(B * tps, 2, N) if stats else None
        am = torch.zeros(1, dtype=torch.int32, device="cuda") if amax else None
        a = [ge._vp(t) for t in A] + [None] * (3 - len(A))
        ge._ck(self.hip.p2m_gemm_planes_rows(g.handle, 2, B, a[0], a[1], a[2], len(A), Ka, 0, 1, ge._vp(Bm),
                                             ge._vp(Bx), ge.CODE[arith], ge._vp(word), 0, ge._vp(bias),
                                             ge._vp(addend), ge._vp(C), N, ge._vp(st), None, None, 0, ge._vp(am), None, None,
                                             ge._st()), "p2m_gemm_planes_rows")
        torch.cuda.synchronize()
        return C, st, am

    def flat(self, arith, A, Bm, bias, addend, M, nplanesC=1, pair=False, stats=False, amax=False):
        """p2m_gemm_planes -> (list of output planes, statistics, amax word)."""
        ge = self.ge
        Ka, N = A[0].shape[1], Bm.shape[1]
        Nc = N // nplanesC
        word, Bx = ge._word(arith, *A), ge._split(Bm, arith)                      # (named: they live until the launch has run)
        Cs = [ge._sentinel((M + 1) // 2 if pair else M, Nc) for _ in range(nplanesC)]
        st = ge._sentinel(-(-M // gr.TILE), 2, N) if stats else None
        am = torch.zeros(1, dtype=torch.int32, device="cuda") if amax else None
        a = [ge._vp(t) for t in A] + [None] * (3 - len(A))
        c = [ge._vp(t) for t in Cs] + [None] * (3 - nplanesC)
        ge._ck(self.hip.p2m_gemm_planes(a[0], a[1], a[2], len(A), Ka, 0, ge._vp(Bm), ge._vp(Bx), ge.CODE[arith],
                                        ge._vp(word), 0, ge._vp(bias), ge._vp(addend), c[0], c[1], c[2], nplanesC,
                                        Nc, int(pair), M, ge._vp(st), None, None, 0, ge._vp(am), ge._st()), "p2m_gemm_planes")
        torch.cuda.synchronize()
        return Cs, st, am


def row_cases():
    """(tag, nset, classes, Ka, N, planes, seed)."""
    out = []
    for nset in NSETS:
        for k, (Ka, N, planes) in enumerate(ROW_SHAPES):
            classes = bool((k + (nset == 5)) % 2)
            out.append((f"n{nset}_k{Ka}_N{N}_p{planes}_c{int(classes)}", nset, classes, Ka, N, planes, 8100 + 10 * k + (nset == 5)))
    return out


def run_row_case(rn, arith, case):
    """Both launches of a row-set case (without and with the addend; statistics and the amax word in both)."""
    _, nset, classes, Ka, N, planes, seed = case
    A, Bm, bias, addend = row_inputs(nset, Ka, N, planes, seed)
    A, Bm, bias, addend = [t.cuda() for t in A], Bm.cuda(), bias.cuda(), addend.cuda()
    plain = rn.rows(arith, nset, classes, A, Bm, bias, None, True, True)
    added = rn.rows(arith, nset, classes, A, Bm, bias, addend, True, True)
    return (A, Bm, bias, addend), plain, added


@pytest.fixture(scope="module")
def runner(hip_libs):
    return Runner()


@pytest.fixture(scope="module")
def ring_arm(hip_libs, tmp_path_factory):
    """npz of this file run as a child under P2M_ROWS_K1 = 0 (every one-plane row case in the slice arithmetics)."""
    out = str(tmp_path_factory.mktemp("epilogue") / "ring.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, P2M_ROWS_K1="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    return np.load(out)


def _chk(kind, what, err, tol):
    print(f"    {what}: {kind} err {float(err):.3e}  bound {float(tol):.3e}")
    assert float(err) <= float(tol), (kind, what, float(err), float(tol))


@pytest.mark.parametrize("arith", gr.ARITHS)
def test_row_sets(runner, arith):
    ge = runner.ge
    for case in row_cases():
        tag, nset, classes, Ka, N, planes, _ = case
        (A, Bm, bias, addend), (C0, st0, am0), (C1, st1, am1) = run_row_case(runner, arith, case)
        _, ids, wts = runner.graph(nset, classes)
        w = torch.as_tensor(np.tile(wts, B)).cuda() if classes else None
        rows = gr.logical_rows(ids, V, B, "cuda")
        outside = ge._complement(rows, B * V)
        for name, C, st, am, add in (("plain", C0, st0, am0, None), ("addend", C1, st1, am1, addend)):
            what = f"{tag} {name}"
            _, Yref, stref = gr.planes_rows_ref(ids, V, B, A, 0, 1, Bm, bias, add, weights=w)
            _chk("value", what, (C[rows].double() - Yref).abs().max(), gr.tol_fwd(Yref))
            assert bool((ge._bits(C[outside]) == ge.SENTINEL).all()), ("a row outside the set was written", what)
            _chk("stat sum", what, (st[:, 0].double() - stref[:, 0]).abs().max(), gr.TOL_STAT_SUM)
            _chk("stat M2", what, (st[:, 1].double() - stref[:, 1]).abs().max(), gr.TOL_STAT_M2)
            assert int(am[0]) == int(C[rows].abs().max().view(torch.int32)), ("amax word", what)
        assert torch.equal(ge._bits(C1[rows]), ge._bits(C0[rows] + addend[rows])), ("C + addend is not fp32(C + addend)", tag)


@pytest.mark.parametrize("arith", SLICED)
def test_statistics_bitwise_in_both_dispatches(runner, ring_arm, arith):
    ge = runner.ge
    n = 0
    for case in row_cases():
        if case[5] != 1:
            continue
        _, (C0, st0, am0), (C1, st1, am1) = run_row_case(runner, arith, case)
        for name, C, st, am in (("plain", C0, st0, am0), ("addend", C1, st1, am1)):
            key = f"{arith}::{case[0]}::{name}"
            assert np.array_equal(ring_arm["st::" + key], ge._bits(st).cpu().numpy()), ("statistics differ", key)
            assert np.array_equal(ring_arm["C::" + key], ge._bits(C).cpu().numpy()), ("C differs", key)
            assert np.array_equal(ring_arm["amax::" + key], am.cpu().numpy()), ("amax word differs", key)
            n += 1
    print(f"  {n} launches compared bit for bit with the P2M_ROWS_K1 = 0 arm")
    assert n == 2 * len(NSETS) * sum(s[2] == 1 for s in ROW_SHAPES)


@pytest.mark.parametrize("arith", gr.ARITHS)
def test_flat_rows_addend_statistics(runner, arith):
    ge = runner.ge
    for k, (M, Ka, N, planes) in enumerate(FLAT_SHAPES):
        gen = torch.Generator().manual_seed(8300 + k)
        A = [torch.randn(M, Ka, generator=gen).cuda() for _ in range(planes)]
        Bm = (torch.randn(planes * Ka, N, generator=gen) / (planes * Ka) ** 0.5).cuda()
        bias, addend = torch.randn(N, generator=gen).cuda(), torch.randn(M, N, generator=gen).cuda()
        (C0,), st0, am0 = runner.flat(arith, A, Bm, bias, None, M, stats=True, amax=True)
        (C1,), st1, am1 = runner.flat(arith, A, Bm, bias, addend, M, stats=True, amax=True)
        for name, C, st, am, add in (("plain", C0, st0, am0, None), ("addend", C1, st1, am1, addend)):
            what = f"M {M}, Ka {Ka} x {planes}, N {N}, {name}"
            Yref, stref = gr.gemm_planes_ref(A, 0, Bm, M, bias, add)
            _chk("value", what, (C.double() - Yref).abs().max(), gr.tol_fwd(Yref))
            _chk("stat sum", what, (st[:, 0].double() - stref[:, 0]).abs().max(), gr.TOL_STAT_SUM)
            _chk("stat M2", what, (st[:, 1].double() - stref[:, 1]).abs().max(), gr.TOL_STAT_M2)
            assert int(am[0]) == int(C.abs().max().view(torch.int32)), ("amax word", what)
        assert torch.equal(ge._bits(C1), ge._bits(C0 + addend)), ("C + addend is not fp32(C + addend)", M, Ka, N)


@pytest.mark.parametrize("arith", gr.ARITHS)
def test_three_output_planes(runner, arith):
    ge = runner.ge
    for k, Nc in enumerate(PLANE_NC):
        M, Ka = (130, 257, 130)[k], (64, 32, 128)[k]
        gen = torch.Generator().manual_seed(8400 + k)
        A = [torch.randn(M, Ka, generator=gen).cuda()]
        Bm = (torch.randn(Ka, 3 * Nc, generator=gen) / Ka ** 0.5).cuda()
        bias = torch.randn(3 * Nc, generator=gen).cuda()
        (C,), _, am1 = runner.flat(arith, A, Bm, bias, None, M, amax=True)
        Cs, _, am3 = runner.flat(arith, A, Bm, bias, None, M, nplanesC=3, amax=True)
        Yref, _ = gr.gemm_planes_ref(A, 0, Bm, M, bias)
        _chk("value", f"M {M}, Ka {Ka}, 3 x {Nc}", (C.double() - Yref).abs().max(), gr.tol_fwd(Yref))
        for q in range(3):
            assert torch.equal(ge._bits(Cs[q]), ge._bits(C[:, q * Nc:(q + 1) * Nc])), ("plane differs from its column block", Nc, q)
        assert int(am3[0]) == int(am1[0]) == int(C.abs().max().view(torch.int32)), ("amax word", Nc)


@pytest.mark.parametrize("arith", gr.ARITHS)
def test_pair_sums(runner, arith):
    ge = runner.ge
    M = 260
    for k, (Ka, N) in enumerate(((32, 64), (64, 128), (128, 32))):
        gen = torch.Generator().manual_seed(8500 + k)
        A = [torch.randn(M, Ka, generator=gen).cuda()]
        Bm = (torch.randn(Ka, N, generator=gen) / Ka ** 0.5).cuda()
        for addend in (None, torch.randn(M, N, generator=gen).cuda()):
            (C,), _, _ = runner.flat(arith, A, Bm, None, addend, M)
            (P,), _, am = runner.flat(arith, A, Bm, None, addend, M, pair=True, amax=True)
            what = f"Ka {Ka}, N {N}, addend {addend is not None}"
            Yref, _ = gr.gemm_planes_ref(A, 0, Bm, M, None, addend)
            _chk("value", what, (P.double() - (Yref[0::2] + Yref[1::2])).abs().max(), gr.tol_fwd(Yref))
            assert torch.equal(ge._bits(P), ge._bits(C[0::2] + C[1::2])), ("pair sums are not fp32(row + row)", what)
            assert int(am[0]) == int(P.abs().max().view(torch.int32)), ("amax word of the pair sums", what)


def _child(out):
    from pose2mesh_release_amd import build
    build.build_all()
    rn = Runner()
    res = {}
    for arith in SLICED:
        for case in row_cases():
            if case[5] != 1:
                continue
            _, (C0, st0, am0), (C1, st1, am1) = run_row_case(rn, arith, case)
            for name, C, st, am in (("plain", C0, st0, am0), ("addend", C1, st1, am1)):
                key = f"{arith}::{case[0]}::{name}"
                res["C::" + key] = rn.ge._bits(C).cpu().numpy()
                res["st::" + key] = rn.ge._bits(st).cpu().numpy()
                res["amax::" + key] = am.cpu().numpy()
    np.savez(out, **res)


if __name__ == "__main__":
    _child(sys.argv[1])
