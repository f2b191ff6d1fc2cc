"""The short-K row-set contractions of the train step (one A plane, Ka <= 256: the class-representative convs of every level,
the two projections of the final conv) on the coco graphs at batch B, stand-alone, in bf16x3:
  * per level: vertices, real rows, fake rows, class representatives, tiles per sample and the fill of the last 128-row tile;
  * per shape: time per launch and the HBM rate of its compulsory traffic (rows x (Ka + N) x 4 bytes);
  * with the probe build of tools/k1_trace.sh: k_gemm_rows_k1's phase stamps per block, in s_memtime ticks (they advance at about
    the shader clock: ticks per block x rounds of blocks = the launch's time at 2.1 GHz).
P2M_ROWS_K1=0 | 1 selects the kernel (read once per process):   P2M_ROWS_K1=0 python tools/probes/rows_k1_probe.py [B]"""
import ctypes
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [R]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pose2mesh_release_amd import _lib, ops, pose2mesh_net, synth  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
ops.GEMM_ARITH = "bf16x3"
WIDTHS = {96: (256, 256), 184: (256, 256), 368: (256, 128), 736: (128, 128), 1472: (128, 64), 2944: (64, 64), 5888: (64, 64),
          11776: (64, 32)}                                    # V -> (Fin, Fout) of the level's convs (tools/probes/gemm_probe.py)
_, graph_L, _, J = synth.make_graphs("coco")
model = pose2mesh_net.get_model(J, graph_L).to("cuda:0").train()
cache = next(m._graph_cache for m in model.modules() if hasattr(m, "_graph_cache"))
graphs = cache.on("cuda:0")
lib = _lib.hip()
trace = hasattr(lib, "p2m_k1_trace_dump")
print(f"B = {B}, P2M_ROWS_K1 = {os.environ.get('P2M_ROWS_K1', '(default)')}, trace build: {trace}")
print("level      V   real  fake rows  representatives  tiles/sample  last tile")
for i, g in enumerate(graphs):
    n = g.n_fake
    print(f"{i:5d} {g.V:6d} {g.n_real:6d} {getattr(g, 'n_fake_all', n):10d} {n:16d} {-(-n // 128):13d} "
          f"{(n - 1) % 128 + 1 if n else 0:10d}   classes {bool(getattr(g, 'classes', False))}")


def timed(fn, n=10):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def shape(g, row_set, Ka, N, stats, what):
    n = g.set_size(row_set)
    if n == 0:
        return
    X = torch.randn(B * g.V, Ka, device="cuda")
    W = torch.randn(Ka, N, device="cuda") / Ka ** 0.5
    bias = torch.randn(N, device="cuda")
    C = torch.empty(B * g.V, N, device="cuda")
    Wx = ops.weight_split(W)

    def run():
        ops.gemm_planes_rows(g, row_set, B, [X], Ka, 0, False, W, bias, None, C, N, stats, Bx=Wx)

    us = timed(run)
    mb = B * n * (Ka + N) * 4 / 1e6
    print(f"V {g.V:6d} set {row_set} rows {n:6d} Ka {Ka:3d} N {N:3d} stats {int(stats)}: {us:8.1f} us  {mb:7.1f} MB  "
          f"{mb / us:5.2f} TB/s   {what}", flush=True)
    if trace:
        run()
        buf = np.zeros((4096, 4), dtype=np.uint64)
        assert lib.p2m_k1_trace_dump(buf.ctypes.data_as(ctypes.c_void_p)) == 0
        t = buf.astype(np.int64)
        nb = min(4096, -(-n // 128) * B * max(1, -(-N // 128) if N % 128 == 0 else -(-N // 64)))
        t = t[:nb][(t[:nb] != 0).all(axis=1)]
        if len(t):
            d = np.diff(t, axis=1)
            whole = (t[:, 3] - t[:, 0]).mean()
            print(f"      {len(t)} blocks stamped, ticks per block: prologue {d[:, 0].mean():6.0f} ({d[:, 0].mean() / whole:4.0%})  "
                  f"k loop {d[:, 1].mean():6.0f} ({d[:, 1].mean() / whole:4.0%})  epilogue {d[:, 2].mean():6.0f} "
                  f"({d[:, 2].mean() / whole:4.0%})  whole {whole:6.0f}")

for g in graphs:
    if g.V in WIDTHS and g.n_fake:
        Fin, Fout = WIDTHS[g.V]
        shape(g, 2, Fin, Fout, True, "representative conv, forward")
        if Fin != Fout:
            shape(g, 2, Fout, Fout, True, "representative conv, forward")
            shape(g, 2, Fout, Fin, False, "representative conv, dX")
g0 = graphs[0]
for rs in (1, 2):
    shape(g0, rs, 64, 32, False, "final conv: projection")
    shape(g0, rs, 32, 64, False, "final conv: dX")
