"""No GPU: the audit of tests/gemm_ref.py.  (1) The case table reaches what tests/test_gpu_gemm_edges.py is there for - the
conditions below are properties of the table, computed from it alone.  (2) The float64 restatements agree with a second, dense
formulation (rows gathered one by one into a compact matrix, then `@`).  (3) Every row-set case can tell a wrong row from a
right answer: with one set row dropped, counted twice or replaced by its neighbour the reference moves by at least 100 times the
bound the GPU test holds the kernel to in that case."""
import math

import numpy as np
import pytest
import torch

import gemm_ref as gr
import tile_plan_ref as tp


def _stages(rows, stage):
    return -(-rows // stage)


# ---- 1. what the table covers --------------------------------------------------------------------------------------------------

def test_graphs_of_the_table():
    counts = set()
    for name, (V, nreal, _) in gr.GRAPHS.items():
        assert V % 2 == 0 and V <= 320 and nreal >= 40
        _, Vg, ids = gr.graph_ids(name)
        assert Vg == V and len(ids[1]) == nreal and len(ids[2]) == V - nreal
        assert np.array_equal(np.sort(np.concatenate([ids[1], ids[2]])), np.arange(V))
        counts |= {nreal, V - nreal}
    assert {1, 15, 16, 17, 33, 81} <= counts
    # default behaviour of tp.band unchanged: nreal = int(0.6 V)
    assert tp.Plans(tp.band(100, 3)).n_real == 60 and tp.Plans(tp.band(100, 3, nreal=60)).n_real == 60
    assert (tp.band(100, 3) != tp.band(100, 3, nreal=60)).nnz == 0


def test_paired_graph_is_the_smallest():
    """Row sets 3 / 4 need a paired tile plan; with the default share of fake vertices V = 428 is the first even V that has one."""
    _, V, ids = gr.graph_ids(gr.PAIR_GRAPH)
    assert V == gr.PAIR_V and len(ids[3]) >= tp.MIN_PAIR and len(ids[4]) > 0
    assert len(ids[3]) + len(ids[4]) == V // 2
    assert tp.Plans(tp.band(gr.PAIR_V - 2, gr.PAIR_SEED)).n_pair_real == 0


def test_tn_rows_table_covers_the_pipeline_of_the_sliced_kernel():
    rows = set()
    for c in gr.TN_ROWS_CASES:
        rows |= {r for r in gr.tn_rows_chunk_rows(c, True) if r > 0}
    assert {1, 15, 16, 17, 33, 81} <= rows
    assert set(range(1, 10)) <= {_stages(r, 16) for r in rows}
    rem = {r % 16 for r in rows}
    assert {0, 1, 15} <= rem
    for k in (1, 2, 3):                                       # 4 q + k, q >= 1: a partial row quad behind whole ones
        assert any(x % 4 == k and x >= 4 for x in rem), k
    # the flat form runs the same list as single chunks
    assert set(gr.TN_ROW_COUNTS) <= {M for M, cr, *_ in gr.FLAT_TN_CASES if cr >= M}
    assert set(range(1, 10)) <= {_stages(r, 16) for r in gr.TN_ROW_COUNTS}
    assert any(M > cr and M % cr for M, cr, *_ in gr.FLAT_TN_CASES)          # full chunks + a short last one


def test_tn_rows_table_covers_the_f32_kernel():
    rows = set()
    for c in gr.TN_ROWS_CASES:
        if not c["sliced_only"]:
            assert c["splits"] >= 1
            rows |= {r for r in gr.tn_rows_chunk_rows(c, False) if r > 0}
    assert {1, 2, 3, 4} <= {_stages(r, 32) for r in rows}
    assert {0, 1, 31} <= {r % 32 for r in rows}


def test_tn_rows_table_parameters():
    T = gr.TN_ROWS_CASES
    assert {c["Ka"] for c in T} == {32, 96, 192}
    assert {c["gplanes"] * c["Gc"] for c in T} == {32, 64, 128, 192}
    assert all(c["gplanes"] == 3 and c["Gc"] == 64 for c in T if c["gplanes"] * c["Gc"] == 192)
    assert {c["a0_shift"] for c in T} == {0, 1}
    assert {c["compact"] for c in T if c["gplanes"] == 3} == {0, 1}
    assert {c["splits"] for c in T} == {1, 2, 4, -2, -3}
    assert {c["row_set"] for c in T} == {1, 2, 3, 4}
    assert all(c["graph"] == gr.PAIR_GRAPH for c in T if c["row_set"] >= 3)
    assert all(c["B"] <= 5 for c in T)
    n = lambda c: len(gr.set_rows(c["graph"], c["row_set"])[0])                     # noqa: E731
    # 17 rows in 4 slices: two trailing slices empty in the slice arithmetics; one more case with empty slices in f32 as well
    assert any(n(c) == 17 and c["splits"] == 4 for c in T)
    assert any(0 in [hi - lo for ch in gr.tn_chunks(n(c), 1, c["splits"], False) for _, lo, hi in ch]
               for c in T if c["splits"] >= 1 and not c["sliced_only"])
    # whole samples per chunk: B = 5, the last chunk short, an even and an odd stage count for both chunk sizes
    for S in (2, 3):
        neg = [c for c in T if c["splits"] == -S]
        assert all(c["B"] == 5 and c["sliced_only"] for c in neg)
        assert {_stages(n(c), 16) % 2 for c in neg} == {0, 1}
    assert any(c["a_act"] and n(c) % 16 for c in T)
    # the XCD-aware block mapping of k_gemm_tn_ws starts at 8 chunks
    assert any(c["B"] * c["splits"] >= 8 for c in T) and any(0 < c["B"] * c["splits"] < 8 for c in T)


def test_planes_rows_table_parameters():
    T = gr.PLANES_ROWS_CASES
    n = lambda c: len(gr.set_rows(c["graph"], c["row_set"])[0])                     # noqa: E731
    assert {(c["Ka"], c["planes"]) for c in T} == set(gr.K_PIPE)
    assert {c["planes"] * c["Ka"] // 16 for c in T} == {2, 4, 6, 8, 12}
    assert {c["N"] for c in T} == {32, 96, 128}
    assert {c["a0_shift"] for c in T} == {0, 1}
    assert {c["compact"] for c in T if c["planes"] == 3} == {0, 1}
    assert {c["addend"] for c in T} == {False, True}                 # both epilogue instantiations
    assert {c["row_set"] for c in T} == {1, 2, 3, 4}
    rem = {n(c) % 128 for c in T}
    assert {0, 1, 127} <= rem and any(1 < r < 127 for r in rem)
    assert {1, 2} <= {-(-n(c) // 128) for c in T}
    assert all(c["B"] <= 5 for c in T)
    for key in ("in_act", "act"):                                    # one case each per tile width, the last tile partial
        sel = [c for c in T if c[key]]
        assert {c["N"] == 128 for c in sel} == {False, True} and all(n(c) % 128 for c in sel)
    assert all(not (c["act"] and c["stats"]) for c in T)
    # the flat form: every pipeline depth at every width, M % 128 in {0, 1, 127, other}
    F = gr.FLAT_PLANES_CASES
    assert {(Ka, pl, N) for _, Ka, pl, N, *_ in F} >= {(Ka, pl, N) for Ka, pl in gr.K_PIPE for N in gr.FWD_N}
    assert {0, 1, 127} <= {M % 128 for M, *_ in F}
    assert {(M, N == 128) for M, Ka, N in gr.TN_ACC_CASES} == {(M, w) for M in (32, 36, 100) for w in (False, True)}


# ---- 2. the restatements against a dense formulation ---------------------------------------------------------------------------

def _dense_planes(case, inp, ids, V):
    B, n, s = case["B"], len(ids), case["a0_shift"]
    A = [a.double().numpy() for a in inp["A"]]
    if inp["in_act"] is not None:
        sc, sh = (t.numpy() for t in inp["in_act"])
        A[0] = np.maximum(np.float32(inp["A"][0].numpy() * sc + sh), np.float32(0)).astype(np.float64)
    Z = np.zeros((B * n, case["planes"] * case["Ka"]))
    for b in range(B):
        for i, v in enumerate(ids):
            r = b * V + int(v)
            parts = [A[0][r >> s]] + [p[b * n + i] if case["compact"] else p[r] for p in A[1:]]
            Z[b * n + i] = np.concatenate(parts)
    Y = Z @ inp["Bm"].double().numpy() + inp["bias"].double().numpy()
    if inp["act"] is not None:
        Y = Y * inp["act"][0].double().numpy() + inp["act"][1].double().numpy()
        if inp["act"][2]:
            Y = np.maximum(Y, 0)
    if inp["addend"] is not None:
        Y += np.stack([inp["addend"][b * V + int(v)].double().numpy() for b in range(B) for v in ids])
    return Y


def _dense_tn(case, inp, ids, V):
    B, n, s = case["B"], len(ids), case["a0_shift"]
    A = inp["A"].double().numpy()
    if inp["a_act"] is not None:
        sc, sh = (t.numpy() for t in inp["a_act"])
        A = np.maximum(np.float32(inp["A"].numpy() * sc + sh), np.float32(0)).astype(np.float64)
    G = [g.double().numpy() for g in inp["G"]]
    Zc = np.stack([A[(b * V + int(v)) >> s] for b in range(B) for v in ids])
    Gc = np.stack([np.concatenate([G[0][b * V + int(v)]] + [p[b * n + i] if case["compact"] else p[b * V + int(v)] for p in G[1:]])
                   for b in range(B) for i, v in enumerate(ids)])
    return Zc.T @ Gc, Gc.sum(0)


@pytest.mark.parametrize("index", [2, 9, 24, 25, 26, 28])
def test_planes_rows_ref_against_dense(index):
    case = gr.PLANES_ROWS_CASES[index]
    ids, V = gr.set_rows(case["graph"], case["row_set"])
    inp = gr.planes_rows_inputs(case, index)
    rows, Y, st = gr.planes_rows_case_ref(case, inp, ids, V)
    D = _dense_planes(case, inp, ids, V)
    assert rows.tolist() == [b * V + int(v) for b in range(case["B"]) for v in ids]
    assert np.abs(Y.numpy() - D).max() < 1e-5 if case["in_act"] else np.abs(Y.numpy() - D).max() < 1e-12
    n, tps = len(ids), -(-len(ids) // 128)
    assert st.shape == (case["B"] * tps, 2, case["N"])
    for b in range(case["B"]):
        for t in range(tps):
            blk = D[b * n + t * 128:b * n + min((t + 1) * 128, n)]
            assert np.abs(st[b * tps + t, 0].numpy() - blk.sum(0)).max() < 1e-4 if case["in_act"] else \
                np.abs(st[b * tps + t, 0].numpy() - blk.sum(0)).max() < 1e-10
            assert np.abs(st[b * tps + t, 1].numpy() - ((blk - blk.mean(0)) ** 2).sum(0)).max() < 1e-3 if case["in_act"] else \
                np.abs(st[b * tps + t, 1].numpy() - ((blk - blk.mean(0)) ** 2).sum(0)).max() < 1e-10


@pytest.mark.parametrize("index", [3, 15, 24, 33, 39, 42])
def test_tn_rows_ref_against_dense(index):
    case = gr.TN_ROWS_CASES[index]
    ids, V = gr.set_rows(case["graph"], case["row_set"])
    inp = gr.tn_rows_inputs(case, index)
    for sliced in (True, False):
        P, Pdb, Pc, Pdbc, nrows = gr.tn_rows_case_ref(case, inp, ids, V, sliced)
        D, Ddb = _dense_tn(case, inp, ids, V)
        tol = 1e-4 if case["a_act"] else 1e-10          # (the activation: fused or unfused multiply-add in fp32)
        assert np.abs(P.numpy() - D).max() < tol and np.abs(Pdb.numpy() - Ddb).max() < tol
        assert sum(nrows) == case["B"] * len(ids)
        assert len(nrows) == (case["B"] * case["splits"] if case["splits"] >= 1 else -(-case["B"] // -case["splits"]))


def test_flat_refs_against_dense():
    gen = torch.Generator().manual_seed(7)
    M, Ka = 77, 8
    A = [torch.randn(39, Ka, generator=gen), torch.randn(M, Ka, generator=gen)]
    G = [torch.randn(M, 4, generator=gen), torch.randn(M, 4, generator=gen)]
    Bm, bias = torch.randn(2 * Ka, 5, generator=gen), torch.randn(5, generator=gen)
    Z = np.stack([np.concatenate([A[0][r >> 1].double().numpy(), A[1][r].double().numpy()]) for r in range(M)])
    Y, st = gr.gemm_planes_ref(A, 1, Bm, M, bias)
    assert np.abs(Y.numpy() - (Z @ Bm.double().numpy() + bias.double().numpy())).max() < 1e-12 and st.shape == (1, 2, 5)
    P, Pdb, nrows = gr.gemm_tn_ref(A, 1, G, M, 32)
    Gd = np.concatenate([g.double().numpy() for g in G], 1)
    assert nrows == [32, 32, 13] and np.abs(P.sum(0).numpy() - Z.T @ Gd).max() < 1e-12
    assert np.abs(P[2].numpy() - Z[64:].T @ Gd[64:]).max() < 1e-12 and np.abs(Pdb[2].numpy() - Gd[64:].sum(0)).max() < 1e-12
    P0 = torch.full((Ka, 4), 0.25)
    assert np.abs(gr.gemm_tn_acc_ref(A[1], G[0], P0).numpy() - 0.25 - A[1].double().numpy().T @ Gd[:, :4]).max() < 1e-12


# ---- 3. mutations --------------------------------------------------------------------------------------------------------------

def _mutations(ids, V, B):
    """(name, weights, rows) for the last logical row of the last sample: dropped, counted twice, its vertex id replaced by the
    neighbouring one."""
    n = len(ids)
    rows = gr.logical_rows(ids, V, B)
    for name, w in (("dropped", 0.0), ("twice", 2.0)):
        wt = torch.ones(B * n, dtype=torch.float64)
        wt[-1] = w
        yield name, wt, rows
    moved = rows.clone()
    moved[-1] = (B - 1) * V + (int(ids[-1]) + 1) % V
    yield "neighbour", torch.ones(B * n, dtype=torch.float64), moved


@pytest.mark.parametrize("index", range(len(gr.PLANES_ROWS_CASES)))
def test_planes_rows_cases_tell_a_wrong_row(index):
    """C over ALL rows (rows the set does not name keep the prefill, here 0) and the statistics: a dropped row is a row of C
    not written, a neighbour a row written elsewhere from other operands; a row stored twice is no error of a forward pass, so
    `twice` has to show in the statistics (cases with them)."""
    case = gr.PLANES_ROWS_CASES[index]
    ids, V = gr.set_rows(case["graph"], case["row_set"])
    inp = gr.planes_rows_inputs(case, index)
    B, N = case["B"], case["N"]

    def full(rows, Y, w):
        C = torch.zeros(B * V, N, dtype=torch.float64)
        C[rows[w > 0]] = Y[w > 0]
        return C

    rows, Y, st = gr.planes_rows_case_ref(case, inp, ids, V)
    C = full(rows, Y, torch.ones(len(rows)))
    tol_c = gr.tol_fwd(Y)
    for name, w, mrows in _mutations(ids, V, B):
        r2, Y2, st2 = gr.planes_rows_case_ref(case, inp, ids, V, weights=w, rows=mrows)
        moved_c = float((full(r2, Y2, w) - C).abs().max())
        moved_s = max(float((st2[:, 0] - st[:, 0]).abs().max()) / gr.TOL_STAT_SUM,
                      float((st2[:, 1] - st[:, 1]).abs().max()) / gr.TOL_STAT_M2) if case["stats"] else 0.0
        print(f"  case {index} {name}: C moves {moved_c:.3e} (bound {tol_c:.3e}), statistics {moved_s:.1f} bounds")
        if name == "twice":
            if case["stats"]:
                assert moved_s >= 100, (index, name, moved_s)
        else:
            assert moved_c >= 100 * tol_c, (index, name, moved_c, tol_c)


@pytest.mark.parametrize("index", range(len(gr.TN_ROWS_CASES)))
def test_tn_rows_cases_tell_a_wrong_row(index):
    case = gr.TN_ROWS_CASES[index]
    ids, V = gr.set_rows(case["graph"], case["row_set"])
    inp = gr.tn_rows_inputs(case, index)
    for sliced in ((True,) if case["sliced_only"] else (True, False)):
        _, _, Pc, Pdbc, nrows = gr.tn_rows_case_ref(case, inp, ids, V, sliced)
        c = max(i for i, r in enumerate(nrows) if r > 0)              # the chunk of the last row of the last sample
        tol_p, tol_b = gr.tol_grad(Pc[c], nrows[c]), gr.tol_pdb(nrows[c])
        for name, w, mrows in _mutations(ids, V, case["B"]):
            _, _, P2, Pdb2, _ = gr.tn_rows_case_ref(case, inp, ids, V, sliced, weights=w, rows=mrows)
            moved = float((P2[c] - Pc[c]).abs().max())
            print(f"  case {index} {'sliced' if sliced else 'f32'} {name}: P moves {moved:.3e}, bound {tol_p:.3e}; "
                  f"Pdb {float((Pdb2[c] - Pdbc[c]).abs().max()):.3e}, bound {tol_b:.3e}")
            assert moved >= 100 * tol_p, (index, name, moved, tol_p)
            assert float((P2 - Pc).abs().max()) == moved              # (no other chunk moves)
