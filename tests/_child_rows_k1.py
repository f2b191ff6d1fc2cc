"""The case table of tests/test_gpu_rows_k1.py and the child process that runs it.

P2M_ROWS_K1 is read once per process by the library, so each arm (0: k_gemm_planes_ws, 1: k_gemm_rows_k1) is one run of this
file:   python tests/_child_rows_k1.py OUT.npz   under the arm's environment.  It runs every case of CASES in bf16x3 and f16x2
through p2m_gemm_planes_rows and stores C, the statistics partials and the amax word bit for bit, then the DISPATCH launches
under the profiler and stores the names of the kernels each of them started (the launch log).

Graphs: 48 or 49 real vertices (ring + chords 5 and 17, tile_plan_ref.band without the renumbering) followed by the isolated
fake ones, so that the fake rows are consecutive and any partition of them into runs is a valid set of classes.  Row set 2 then
has exactly `nset` rows: the fake vertices themselves, or - `classes` - the representatives of runs of 3, 2, 1, 3, 2, 1 .. rows
with those sizes as their statistics weights."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gemm_ref as gr                      # noqa: E402
import tile_plan_ref as tp                 # noqa: E402

ARITHS = ("bf16x3", "f16x2")
NSETS = (1, 31, 128, 129)                  # a nearly empty tile, a partial one, a full one, one row into the second tile
KAS = (32, 64, 128, 256)                   # 1 pass of 32, 1 / 2 / 4 passes of 64 columns
NOUT = (32, 64, 128, 256)                  # the 64-wide template half empty and full, one and two 128-wide tiles
FLAGS = ("bias", "addend", "stats", "classes", "amax", "in_act", "a0_shift", "compact")


def _cases():
    rng = np.random.default_rng(20250)
    cases = []
    for i in range(32):                    # two latin squares over (nset, Ka, N); B and the flags drawn
        q, r = (i % 16) // 4, i % 4
        c = dict(nset=NSETS[r], Ka=KAS[q], N=NOUT[(r + q * (1 + i // 16) + i // 16) % 4], B=(1, 3)[int(rng.integers(2))])
        c.update({f: bool(rng.integers(2)) for f in FLAGS})
        cases.append(c)
    on = dict(bias=True, addend=False, stats=True, classes=True, amax=True, in_act=True, a0_shift=False, compact=True)
    off = {f: False for f in FLAGS}
    # the shapes of the train step: the finest representative conv, the two projections of the final conv; Ka = 96 (three
    # passes of 32 columns); everything on / off at the largest shape
    cases.append(dict(on, nset=129, Ka=128, N=128, B=3))
    cases.append(dict(off, nset=129, Ka=64, N=32, B=3, bias=True))
    cases.append(dict(off, nset=128, Ka=32, N=64, B=1, a0_shift=True))
    cases.append(dict(on, nset=31, Ka=96, N=96, B=3, addend=True))
    cases.append(dict({f: True for f in FLAGS}, nset=129, Ka=256, N=256, B=3))
    cases.append(dict(off, nset=129, Ka=256, N=256, B=1))
    # many more tiles than the device holds blocks at once (two per CU): launches of 1100, 600 and 1030 blocks with 1, 3 and 2
    # passes per tile; bf16x3 only, and only the set's rows are kept
    cases.append(dict(off, nset=31, Ka=64, N=32, B=1100, bias=True, stats=True, classes=True, amax=True, big=True))
    cases.append(dict(on, nset=129, Ka=96, N=96, B=300, big=True))
    cases.append(dict(off, nset=31, Ka=128, N=128, B=1030, addend=True, stats=True, in_act=True, big=True))
    for c in cases:
        c["classes"] = c["classes"] and c["stats"]          # class weights exist in the statistics only
        c.setdefault("big", False)
    return cases


CASES = _cases()
# outside the dispatch rule of k_gemm_rows_k1 (Ka > 256; three planes), and one launch inside it
DISPATCH = (dict(name="ka288", nset=129, Ka=288, planes=1, N=64, B=2),
            dict(name="planes3", nset=129, Ka=64, planes=3, N=128, B=2),
            dict(name="inside", nset=129, Ka=64, planes=1, N=128, B=2))


def level(nset, classes):
    """(L, V, ids of row set 2, weight of each of them) of the graph that gives row set 2 `nset` rows."""
    sizes = np.array([3 - i % 3 for i in range(nset)] if classes else [1] * nset, dtype=np.int64)
    F = int(sizes.sum())
    nreal = 48 + (48 + F) % 2              # V even: a0_shift = 1 pairs rows
    V = nreal + F
    i = np.arange(nreal)
    A = tp._sym(np.concatenate([i, i, i]), np.concatenate([(i + 1) % nreal, (i + 5) % nreal, (i + 17) % nreal]), V)
    first = nreal + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rep = np.arange(V, dtype=np.int32)
    for f, s in zip(first, sizes):
        rep[f:f + s] = f
    return tp.laplacian(A, V), V, first.astype(np.int64), sizes.astype(np.float64), rep


def inputs(case, seed, planes=1):
    """Seeded CPU tensors of a case (gemm_ref.planes_rows_inputs' distributions)."""
    _, V, ids, _, _ = level(case["nset"], case.get("classes", False))
    B, Ka, N, n = case["B"], case["Ka"], case["N"], case["nset"]
    gen = torch.Generator().manual_seed(seed)
    A = [torch.randn((B * V) >> int(case.get("a0_shift", False)), Ka, generator=gen)]
    A += [torch.randn(B * n, Ka, generator=gen) for _ in range(planes - 1)]
    Bm = torch.randn(planes * Ka, N, generator=gen) / math.sqrt(planes * Ka)
    bias = torch.randn(N, generator=gen) if case.get("bias", True) else None
    addend = torch.randn(B * V, N, generator=gen) if case.get("addend") else None
    in_act = None
    if case.get("in_act"):
        in_act = (torch.rand(Ka, generator=gen) + 0.5, 0.3 + 0.3 * torch.rand(Ka, generator=gen))
    return dict(A=A, Bm=Bm, bias=bias, addend=addend, in_act=in_act)


def reference(case, inp, planes=1):
    """(rows, Y float64, statistics float64) of a case: gemm_ref.planes_rows_ref with the class sizes as weights."""
    _, V, ids, wts, _ = level(case["nset"], case.get("classes", False))
    w = torch.as_tensor(np.tile(wts, case["B"])) if case.get("classes") else None
    return gr.planes_rows_ref(ids, V, case["B"], inp["A"], int(case.get("a0_shift", False)), 1, inp["Bm"], inp["bias"],
                              inp["addend"], inp["in_act"], None, weights=w)


# ---- the child ------------------------------------------------------------------------------------------------------------------

def _main(out):
    import test_gpu_gemm_edges as ge
    from pose2mesh_release_amd import build, ops
    from torch.profiler import ProfilerActivity, profile
    build.build_all()
    hip = ge._hip()
    graphs = {}

    def graph(nset, classes):
        if (nset, classes) not in graphs:
            L, V, ids, _, rep = level(nset, classes)
            g = ops.DeviceGraph(L, "cuda:0")
            assert g.V == V
            if classes:
                g.set_classes(rep)
            assert np.array_equal(g.fake_ids_host(), ids), (nset, classes)
            graphs[(nset, classes)] = g
        return graphs[(nset, classes)]

    def run(case, arith, inp, planes=1):
        g = graph(case["nset"], case.get("classes", False))
        B, N, n, sh = case["B"], case["N"], case["nset"], int(case.get("a0_shift", False))
        A = [ge._cu(t) for t in inp["A"]]
        Bm, bias, addend = ge._cu(inp["Bm"]), ge._cu(inp["bias"]), ge._cu(inp["addend"])
        in_act = tuple(ge._cu(t) for t in inp["in_act"]) if inp["in_act"] else None
        rows = gr.logical_rows(g.fake_ids_host().astype(np.int64), g.V, B, "cuda")
        word = ge._word(arith, A[0][rows >> sh], *A[1:], act=in_act)
        Bx = ge._split(Bm, arith)
        C = ge._sentinel(B * g.V, N)
        tps = int(hip.p2m_rows_tiles_per_sample(g.handle, 2))
        assert tps == -(-n // gr.TILE)
        st = ge._sentinel(B * tps, 2, N) if case.get("stats") else None
        amax = torch.zeros(1, dtype=torch.int32, device="cuda") if case.get("amax") else None
        a = [ge._vp(t) for t in A] + [None] * (3 - len(A))
        ge._ck(hip.p2m_gemm_planes_rows(g.handle, 2, B, a[0], a[1], a[2], planes, case["Ka"], sh,
                                        int(case.get("compact", True)), ge._vp(Bm), ge._vp(Bx), ge.CODE[arith], ge._vp(word), 0,
                                        ge._vp(bias), ge._vp(addend), ge._vp(C), N, ge._vp(st), None, None, 0, ge._vp(amax),
                                        ge._vp(in_act[0]) if in_act else None, ge._vp(in_act[1]) if in_act else None, ge._st()),
               "p2m_gemm_planes_rows")
        torch.cuda.synchronize()
        return C, st, amax

    res = {}

    def keep(tag, C, st, amax, rows=None):
        if rows is None:
            res["C::" + tag] = ge._bits(C).cpu().numpy()
        else:                              # a big case: the set's rows, and how many other rows lost the sentinel
            res["C::" + tag] = ge._bits(C[rows]).cpu().numpy()
            res["out::" + tag] = np.array([int((ge._bits(C[ge._complement(rows, C.shape[0])]) != ge.SENTINEL).sum())])
        if st is not None:
            res["st::" + tag] = ge._bits(st).cpu().numpy()
        if amax is not None:
            res["amax::" + tag] = amax.cpu().numpy()

    for arith in ARITHS:
        for i, case in enumerate(CASES):
            if case["big"] and arith != "bf16x3":
                continue
            rows = None
            if case["big"]:
                g = graph(case["nset"], case["classes"])
                rows = gr.logical_rows(g.fake_ids_host().astype(np.int64), g.V, case["B"], "cuda")
            keep(f"{arith}::{i}", *run(case, arith, inputs(case, 7000 + i)), rows=rows)
    for d in DISPATCH:
        inp = inputs(d, 7900, d["planes"])
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            C, st, amax = run(d, "bf16x3", inp, d["planes"])
        keep("dispatch::" + d["name"], C, st, amax)
        names = sorted({e.name for e in prof.events() if "k_gemm_" in e.name})
        res["log::" + d["name"]] = np.array(names if names else ["(no kernel of gemm_planes.hip in the profile)"])
    np.savez(out, **res)


if __name__ == "__main__":
    _main(sys.argv[1])
