"""The child process of tests/test_gpu_epilogue_copyout.py: what tests/_child_rows_k1.py's table does not reach.

P2M_EPI_COPYOUT is read once per process by the library, so each arm (0: the 4-byte walk, 1: the staged 16-byte copy-out of
gemm_epilogue, csrc/gemm_planes.hip) is one run of this file:   python tests/_child_epilogue_copyout.py OUT.npz   under the arm's
environment.  Every launch below runs in bf16x3 and in f16x2 and its C (sentinel rows included), statistics partials and amax
word are stored bit for bit:
  rows3    row sets with three A planes (k_gemm_planes_ws): the (64, 128, 3) and (32, 32, 3) shapes of
           tests/test_gpu_gemm_epilogue.py with 130 and 5 rows, without / with an addend x without / with statistics;
  flat     M = 130 and 257, N = 32, 64, 128, 256, without / with an addend x without / with statistics;
  planes   three output planes of Nc = 32, 64, 128 (at 32 the two column tiles of a wave lie in different planes);
  pairs    the un-pool pair sums at M = 260, without and with an addend;
  mis      C and the addend at a storage offset of one float (4-byte but not 16-byte aligned): a row set of 129 rows with one
           and with three A planes, and flat M = 130, N = 64 and 128, with an addend - next to the same launch on aligned
           tensors; `guard` counts the sentinel words around C (one in front, eight behind) that were overwritten;
  log      the kernels an aligned and a misaligned launch started, as the profiler saw them."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gemm_ref as gr                      # noqa: E402

ARITHS = ("bf16x3", "f16x2")
ROWS3 = tuple((nset, Ka, N) for nset in (130, 5) for Ka, N in ((64, 128), (32, 32)))
FLAT_M, FLAT_N, FLAT_KA = (130, 257), (32, 64, 128, 256), 64
PLANE_NC = ((32, 130, 64), (64, 257, 32), (128, 130, 128))          # (Nc, M, Ka)
PAIRS = ((32, 64), (64, 128), (128, 32))                            # (Ka, N) at M = 260
MIS_N = (64, 128)
MIS_NSET, MIS_M, MIS_KA = 129, 130, 64
GUARD = 8                                   # sentinel words kept behind a misaligned C (one stands in front of it)


def expected_keys():
    """{kind: number of arrays of that kind a child stores} - the test counts them."""
    n = len(ARITHS)
    launches = len(ROWS3) * 4 + len(FLAT_M) * len(FLAT_N) * 4 + len(PLANE_NC) + 2 * len(PAIRS)
    stats = len(ROWS3) * 2 + len(FLAT_M) * len(FLAT_N) * 2
    mis = 3 * len(MIS_N)
    return dict(C=n * (launches + 2 * len(PLANE_NC)), st=n * stats, amax=n * launches, mis=n * 2 * mis, guard=n * mis, log=2)


def _main(out):
    import test_gpu_gemm_epilogue as te
    from pose2mesh_release_amd import build
    from torch.profiler import ProfilerActivity, profile
    build.build_all()
    rn = te.Runner()
    ge = rn.ge
    res = {}

    def keep(key, Cs, st, am):
        for q, C in enumerate(Cs):
            res[f"C::{key}" + (f"::plane{q}" if len(Cs) > 1 else "")] = ge._bits(C).cpu().numpy()
        if st is not None:
            res["st::" + key] = ge._bits(st).cpu().numpy()
        res["amax::" + key] = am.cpu().numpy()

    def offset_by_one(rows, N):
        """([rows, N] view one float into a sentinel buffer, the buffer)."""
        buf = ge._sentinel(1 + rows * N + GUARD)
        return buf[1:1 + rows * N].view(rows, N), buf

    def guard_hits(buf, rows, N):
        b = ge._bits(buf)
        return np.array([int((b[:1] != ge.SENTINEL).sum()) + int((b[1 + rows * N:] != ge.SENTINEL).sum())])

    def rows_launch(arith, nset, A, Bm, bias, addend, C):
        g, ids, _ = rn.graph(nset, False)
        rows = gr.logical_rows(ids, te.V, te.B, "cuda")
        word, Bx = ge._word(arith, A[0][rows], *A[1:]), ge._split(Bm, arith)
        a = [ge._vp(t) for t in A] + [None] * (3 - len(A))
        ge._ck(rn.hip.p2m_gemm_planes_rows(g.handle, 2, te.B, a[0], a[1], a[2], len(A), A[0].shape[1], 0, 1, ge._vp(Bm),
                                           ge._vp(Bx), ge.CODE[arith], ge._vp(word), 0, ge._vp(bias), ge._vp(addend),
                                           ge._vp(C), Bm.shape[1], None, None, None, 0, None, None, None, ge._st()),
               "p2m_gemm_planes_rows")
        torch.cuda.synchronize()

    def flat_launch(arith, A, Bm, bias, addend, C, M):
        word, Bx = ge._word(arith, *A), ge._split(Bm, arith)
        ge._ck(rn.hip.p2m_gemm_planes(ge._vp(A[0]), None, None, 1, A[0].shape[1], 0, ge._vp(Bm), ge._vp(Bx), ge.CODE[arith],
                                      ge._vp(word), 0, ge._vp(bias), ge._vp(addend), ge._vp(C), None, None, 1, Bm.shape[1], 0,
                                      M, None, None, None, 0, None, ge._st()), "p2m_gemm_planes")
        torch.cuda.synchronize()

    def kernel_names(fn):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
        names = sorted({e.name for e in prof.events() if "k_gemm_" in e.name})
        return np.array(names if names else ["(no kernel of gemm_planes.hip in the profile)"])

    for arith in ARITHS:
        for k, (nset, Ka, N) in enumerate(ROWS3):
            A, Bm, bias, addend = te.row_inputs(nset, Ka, N, 3, 9100 + k)
            A, Bm, bias, addend = [t.cuda() for t in A], Bm.cuda(), bias.cuda(), addend.cuda()
            for add in (False, True):
                for stats in (False, True):
                    C, st, am = rn.rows(arith, nset, False, A, Bm, bias, addend if add else None, stats, True)
                    keep(f"rows3::{arith}::n{nset}_k{Ka}_N{N}_a{int(add)}_s{int(stats)}", [C], st, am)
        for k, (M, N) in enumerate((M, N) for M in FLAT_M for N in FLAT_N):
            gen = torch.Generator().manual_seed(9200 + k)
            A = [torch.randn(M, FLAT_KA, generator=gen).cuda()]
            Bm = (torch.randn(FLAT_KA, N, generator=gen) / FLAT_KA ** 0.5).cuda()
            bias, addend = torch.randn(N, generator=gen).cuda(), torch.randn(M, N, generator=gen).cuda()
            for add in (False, True):
                for stats in (False, True):
                    Cs, st, am = rn.flat(arith, A, Bm, bias, addend if add else None, M, stats=stats, amax=True)
                    keep(f"flat::{arith}::M{M}_N{N}_a{int(add)}_s{int(stats)}", Cs, st, am)
        for k, (Nc, M, Ka) in enumerate(PLANE_NC):
            gen = torch.Generator().manual_seed(9300 + k)
            A = [torch.randn(M, Ka, generator=gen).cuda()]
            Bm = (torch.randn(Ka, 3 * Nc, generator=gen) / Ka ** 0.5).cuda()
            bias = torch.randn(3 * Nc, generator=gen).cuda()
            Cs, st, am = rn.flat(arith, A, Bm, bias, None, M, nplanesC=3, amax=True)
            keep(f"planes::{arith}::Nc{Nc}", Cs, st, am)
        for k, (Ka, N) in enumerate(PAIRS):
            gen = torch.Generator().manual_seed(9400 + k)
            A = [torch.randn(260, Ka, generator=gen).cuda()]
            Bm = (torch.randn(Ka, N, generator=gen) / Ka ** 0.5).cuda()
            addend = torch.randn(260, N, generator=gen).cuda()
            for add in (False, True):
                Cs, st, am = rn.flat(arith, A, Bm, None, addend if add else None, 260, pair=True, amax=True)
                keep(f"pairs::{arith}::k{Ka}_N{N}_a{int(add)}", Cs, st, am)
        for k, N in enumerate(MIS_N):
            rowsV = te.B * te.V
            for planes in (1, 3):
                A, Bm, bias, addend = te.row_inputs(MIS_NSET, MIS_KA, N, planes, 9500 + 10 * k + planes)
                A, Bm, bias, addend = [t.cuda() for t in A], Bm.cuda(), bias.cuda(), addend.cuda()
                key = f"{arith}::rows_p{planes}_N{N}"
                C = ge._sentinel(rowsV, N)
                rows_launch(arith, MIS_NSET, A, Bm, bias, addend, C)
                res[f"mis::{key}::aligned"] = ge._bits(C).cpu().numpy()
                Co, buf = offset_by_one(rowsV, N)
                Ao, _ = offset_by_one(rowsV, N)
                Ao.copy_(addend)
                assert Co.data_ptr() % 16 == 4 and Ao.data_ptr() % 16 == 4
                rows_launch(arith, MIS_NSET, A, Bm, bias, Ao, Co)
                res[f"mis::{key}::offset"] = ge._bits(Co).cpu().numpy()
                res[f"guard::{key}"] = guard_hits(buf, rowsV, N)
            gen = torch.Generator().manual_seed(9600 + k)
            A = [torch.randn(MIS_M, MIS_KA, generator=gen).cuda()]
            Bm = (torch.randn(MIS_KA, N, generator=gen) / MIS_KA ** 0.5).cuda()
            bias, addend = torch.randn(N, generator=gen).cuda(), torch.randn(MIS_M, N, generator=gen).cuda()
            key = f"{arith}::flat_N{N}"
            C = ge._sentinel(MIS_M, N)
            flat_launch(arith, A, Bm, bias, addend, C, MIS_M)
            res[f"mis::{key}::aligned"] = ge._bits(C).cpu().numpy()
            Co, buf = offset_by_one(MIS_M, N)
            Ao, _ = offset_by_one(MIS_M, N)
            Ao.copy_(addend)
            assert Co.data_ptr() % 16 == 4 and Ao.data_ptr() % 16 == 4
            flat_launch(arith, A, Bm, bias, Ao, Co, MIS_M)
            res[f"mis::{key}::offset"] = ge._bits(Co).cpu().numpy()
            res[f"guard::{key}"] = guard_hits(buf, MIS_M, N)

    gen = torch.Generator().manual_seed(9700)
    A = [torch.randn(MIS_M, MIS_KA, generator=gen).cuda()]
    Bm = (torch.randn(MIS_KA, 128, generator=gen) / MIS_KA ** 0.5).cuda()
    addend = torch.randn(MIS_M, 128, generator=gen).cuda()
    C = ge._sentinel(MIS_M, 128)
    res["log::aligned"] = kernel_names(lambda: flat_launch("bf16x3", A, Bm, None, addend, C, MIS_M))
    Co, _ = offset_by_one(MIS_M, 128)
    res["log::offset"] = kernel_names(lambda: flat_launch("bf16x3", A, Bm, None, addend, Co, MIS_M))
    np.savez(out, **res)


if __name__ == "__main__":
    _main(sys.argv[1])
