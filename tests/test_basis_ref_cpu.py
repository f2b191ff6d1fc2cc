"""No GPU: tests/basis_ref.py itself.  (1) the case tables of tests/test_gpu_basis_edges.py reach every launch edge they claim
(computed from the tables and tile_plan_ref.Plans alone: an edit that loses an edge fails here); (2) merged() against dense float64
L and 2 L L - I; (3) a sequential, unfused float32 evaluation of every chain stays inside the derived bound; (4) planted faults
of the kinds a rewritten gather makes do not."""
import numpy as np

import basis_ref as br
import tile_plan_ref as tp


# ---- 1. what the tables reach -------------------------------------------------------------------------------------------------

def _by_width(cases, widths):
    return {F: [c for c in cases if c[2] == F] for F in widths}


def _audit_row_table(cases, nset_of, need_mod4):
    for F, rows in _by_width(cases, br.ROW_WIDTHS).items():
        S = br.samples_per_wave(F)
        Bs = {c[4] for c in rows}
        assert Bs == set(br.row_batches(F)) == {b for b in (1, S - 1, S, S + 1, 2 * S + 1) if b >= 1}, (F, Bs)
        # a wave that is exactly full, one that is not (S > 1), a second sample group with idle lanes
        assert any(B % S == 0 for B in Bs) and any(B > S for B in Bs)
        assert S == 1 or (any(B > S and B % S for B in Bs) and any(B < S for B in Bs))
        assert {c[3] for c in rows} == {0, 1}, F
        grids = [br.row_grid(F, c[4], nset_of(c)) for c in rows]
        assert {g % 8 == 0 for g in grids} == {True, False}, (F, grids)                   # both branches of xcd_swizzle
        # the renumbering also runs over more than one sample group
        assert any(g % 8 == 0 and -(-c[4] // S) > 1 for g, c in zip(grids, rows)), (F, "swizzle over several groups")
        mod4 = {nset_of(c) % 4 for c in rows}
        assert need_mod4 <= mod4, (F, mod4)
        for c in rows:
            assert c[3] == 0 or c[1] % 2 == 0, c


def test_row_kernel_tables():
    _audit_row_table(br.FWD_CASES, lambda c: c[1], {1, 2, 3})
    _audit_row_table(br.BWD_CASES, lambda c: c[1] >> c[3], {1, 2, 3})
    for F, rows in _by_width(br.BWD_CASES, br.ROW_WIDTHS).items():
        for shift in (0, 1):
            assert {c[5] for c in rows if c[3] == shift} == {True, False}, (F, shift, "resid given and None")
        assert any(c[3] == 1 and (c[1] // 2) % 4 for c in rows), (F, "clamp of the last block at shift 1")
    for c in br.FWD_CASES + br.BWD_CASES:
        assert c[0] in br.STAR_SIZES


def test_ids_table():
    _audit_row_table(br.IDS_CASES, lambda c: br.graph(c[0], c[1]).plans.n_real, {2, 3})
    for g, V, F, shift, B in br.IDS_CASES:
        gc = br.graph(g, V)
        assert gc.plans.plan_tiles == (0, 0, 0) and br.fwd_real_kernel(gc, F, shift) == "row", (g, V)
    assert {c[0] for c in br.IDS_CASES} == set(br.STAR_SIZES)
    assert any(br.graph(c[0], c[1]).plans.n_real % 2 for c in br.IDS_CASES)


def test_star_graphs():
    want = {1} | set(range(2, 18)) | {24, 33, 64, 203}
    for V in (530, 541, 542, 543, 544):
        gc = br.graph("starsA", V)
        lens = set(gc.m.lens.tolist())
        assert lens == want and gc.plans.n_real == 476 and gc.plans.plan_tiles == (0, 0, 0), (V, lens)
        assert {n % 8 for n in lens} == set(range(8)) and {n % 2 for n in lens} == {0, 1} and max(lens) > 64
        # every remainder of the 8 / 4 / 1 unroll of the forward after each number of full steps it can leave
        assert {(n % 8) // 4 for n in lens} == {0, 1} and {n % 4 for n in lens} == {0, 1, 2, 3}
        # the star of s vertices: s rows of s entries
        for s in want - {1}:
            assert int((gc.m.lens == s).sum()) == s
    assert br.graph("starsB", 541).plans.n_real == 459 and br.graph("starsB", 530).plans.n_real == 459
    assert br.graph("starsC", 544).plans.n_real == 478 and -(-478 // br.ROWS_PER_BLOCK) % 8 == 0
    assert tp.UCAP < 203


def test_generic_table():
    assert {c[2] for c in br.GENERIC_CASES} == set(br.GENERIC_WIDTHS) == {3, 5, 96}
    for F in br.GENERIC_WIDTHS:
        rows = [c for c in br.GENERIC_CASES if c[2] == F]
        assert {c[3] for c in rows} == {0, 1} and {c[5] for c in rows} == {True, False}
        for g, V, _, shift, B, resid in rows:
            assert F not in br.ROW_WIDTHS and (shift == 0 or V % 2 == 0)
            assert (B * V * F) % 256 and (B * (V >> shift) * F) % 256, (g, V, F, shift, B)


def test_narrow_tables():
    planned = {("band", 736), ("hub120", 1472)}
    for nc in (1, 2, 3, 4):
        comb = [c for c in br.COMBINE_CASES if c[2] == nc]
        assert {c[3] for c in comb} == {3 * nc, 32}, nc
        assert {(c[3], c[4]) for c in comb} >= {(3 * nc, True), (3 * nc, False), (32, True), (32, False)} or nc != 3
        assert {c[4] for c in comb} == {True, False}
        assert {c[6] for c in comb} == {"full", "real", "index"}
        exp = [c for c in br.EXPAND_CASES if c[2] == nc]
        assert {c[3] for c in exp} == {3 * nc, 3 * nc + 1, 32}, nc
        # the row kernel alone: on a graph without a plan, and (nc != 3) on a graph with one
        for table in (comb, exp):
            assert any(br.narrow_kernels(br.graph(c[0], c[1]), nc) == ("row",) and c[0] in br.STAR_SIZES for c in table)
            assert any((c[0], c[1]) in planned for c in table)
    for g, V in planned:
        gc = br.graph(g, V)
        assert gc.plans.plan[0] is not None and br.narrow_kernels(gc, 3) == ("tile", "row")
        assert br.narrow_kernels(gc, 3, True) == ("tile",) and br.narrow_kernels(gc, 2, True) == ("row",)
        # padding vertices (single-entry rows the tile launch leaves to the row kernel) exist
        assert gc.plans.n_fake > 0
        for table, mode in ((br.COMBINE_CASES, True), (br.EXPAND_CASES, False)):
            Bs = {c[-2] if mode else c[-1] for c in table if (c[0], c[1]) == (g, V) and c[2] == 3 and (not mode or c[6] == "full")}
            assert Bs >= {1, 7, 8, 9, 17}, (g, Bs)
            assert {1, br.SMALL_SPB - 1, br.SMALL_SPB, br.SMALL_SPB + 1, 2 * br.SMALL_SPB + 1} <= Bs
        real = [c for c in br.COMBINE_CASES if (c[0], c[1]) == (g, V) and c[6] != "full"]
        assert {c[6] for c in real if c[2] == 3} == {"real", "index"} and {c[6] for c in real if c[2] != 3} == {"real", "index"}
        assert {c[5] % br.SMALL_SPB for c in real if c[2] == 3} >= {0, 1}
    assert br.graph("hub120", 1472).plans.max_row == tp.UCAP
    for g, V, B in br.TWIN_CASES:
        assert (g, V) in planned and tp.Plans(br.no_plan_twin(br.graph(g, V).L)).plan[0] is None
    assert {c[2] % br.SMALL_SPB for c in br.TWIN_CASES} >= {0, 1}
    for g, V, nc, ldp, bias, B, mode in br.COMBINE_CASES:
        if mode == "index":
            inv, out_rows = br.out_index(br.graph(g, V), 1)
            real = np.sort(br.graph(g, V).real_order)
            kept = inv[real] >= 0
            assert 0 < (~kept).sum() and kept.sum() < out_rows and len(set(inv[real][kept].tolist())) == kept.sum()
            assert (np.delete(inv, real) == -1).all()


def test_tile_tables():
    assert {c[2] for c in br.TILE_CASES} == set(br.TILE_WIDTHS) == {32, 64, 256, 384}
    assert {c[1] for c in br.TILE_CASES} == {736, 1472} and {c[0] for c in br.TILE_CASES} == {"band"}
    padded = set()
    for F in br.TILE_WIDTHS:
        rows = [c for c in br.TILE_CASES if c[2] == F]
        assert {c[4] for c in rows} >= {8, 9, 16, 17} == {br.BASIS_SPB, br.BASIS_SPB + 1, 2 * br.BASIS_SPB, 2 * br.BASIS_SPB + 1}
        assert {c[3] for c in rows} == {0, 1} and {c[1] for c in rows} == {736, 1472}
        for g, V, _, shift, B in rows:
            gc = br.graph(g, V)
            assert br.fwd_real_kernel(gc, F, shift) == "tile", (g, V, shift)
            padded.add(br.tile_blocks(gc.plans.plan_tiles[shift], F, B) % 8 == 0)
    assert padded == {True, False}                        # grids with and without blocks that return at once
    assert {(c[2], c[3]) for c in br.PAIR_CASES} >= {(F, B) for F in (64, 384) for B in (8, 9, 17)}
    for g, V, F, B in br.PAIR_CASES:
        gc = br.graph(g, V)
        assert gc.plans.plan[2] is not None and gc.plans.n_pair_real >= tp.MIN_PAIR
    assert {c[1] for c in br.PAIR_CASES} == {736, 1472}
    # where the refusals of the GPU tests come from: no plan on the stars, no paired plan on hub120
    assert br.graph("hub120", 1472).plans.plan[2] is None and br.graph("starsA", 542).plans.plan[0] is None


# ---- 2. the restated coefficients ---------------------------------------------------------------------------------------------

def test_merged_against_dense_algebra():
    """a against L and b against 2 L L - I in float64.  a is one rounding of L_ij.  b is one rounding of a sum whose products
    2 L_ik L_kj each carry the two roundings of their fp32 factors: |b - B_ij| <= u |B_ij| + 2.01 u sum_k |2 L_ik L_kj|."""
    u = br.U
    for name, V in (("starsA", 541), ("starsB", 530), ("band", 736), ("hub120", 1472)):
        gc = br.graph(name, V)
        m, Ld = gc.m, tp.dense(gc.L)
        rp, mc = tp.merged_pattern(tp._csr(gc.L))
        assert np.array_equal(m.rp, rp) and np.array_equal(m.col, mc), name
        L2 = 2.0 * Ld @ Ld - np.eye(V)
        mag = 2.0 * np.abs(Ld) @ np.abs(Ld)
        rows = np.repeat(np.arange(V), m.lens)
        assert (np.abs(m.a - Ld[rows, m.col]) <= u * np.abs(Ld[rows, m.col])).all(), name
        assert (np.abs(m.b - L2[rows, m.col]) <= u * np.abs(L2[rows, m.col]) + 2.01 * u * mag[rows, m.col]).all(), name
        assert np.array_equal(m.a, br.f32(m.a)) and np.array_equal(m.b, br.f32(m.b))
        # nothing outside the pattern
        mask = np.zeros((V, V), bool)
        mask[rows, m.col] = True
        assert not Ld[~mask].any() and not L2[~mask].any(), name
        for r in range(V):
            assert (np.diff(m.col[m.rp[r]:m.rp[r + 1]]) > 0).all()


def test_paired_rows_are_the_pair_sums():
    gc = br.graph("band", 736)
    m, pm = gc.m, br.paired(gc.m)
    V = gc.V
    A, Bm = m.csr("a").toarray(), m.csr("b").toarray()
    pa, pb = pm.csr("a").toarray(), pm.csr("b").toarray()
    assert pm.nrows == V // 2 and pm.ncols == V
    assert np.array_equal(pa, br.f32(A[0::2] + A[1::2])) and np.array_equal(pb, br.f32(Bm[0::2] + Bm[1::2]))
    for c in range(V // 2):
        assert np.array_equal(pm.row(c)[0], np.union1d(m.row(2 * c)[0], m.row(2 * c + 1)[0]))
    # the rows the library keeps, and their lengths, are those of the planner's restatement
    assert np.array_equal(pm.lens[gc.plans.pair_order], gc.plans.row_len[2])


# ---- 3. a float32 evaluation stays inside the bound ---------------------------------------------------------------------------

def _chain32(m, rows, acc, pairs, shift=0):
    """The kernels' accumulation, unfused: for entry j of row rows[i] in merged column order and every (coefficients, X) of
    pairs in turn, acc[:, i] = fp32(acc[:, i] + fp32(coef_j * X[:, col_j >> shift])).  acc [B, len(rows), F] float32."""
    rows = np.asarray(rows)
    lens = m.lens[rows]
    for j in range(int(lens.max())):
        sel = np.where(lens > j)[0]
        at = m.rp[rows[sel]] + j
        src = m.col[at] >> shift
        for coef, X in pairs:
            prod = coef[at].astype(np.float32)[None, :, None] * X[:, src, :]
            assert prod.dtype == np.float32
            acc[:, sel] = acc[:, sel] + prod
    return acc


def _ratio(out, ref, bound):
    err = np.abs(out.astype(np.float64) - ref)
    assert ((bound > 0) | (err == 0)).all()
    return float((err[bound > 0] / bound[bound > 0]).max())


def test_float32_chains_stay_inside_the_bound():
    worst = {}
    for name, V, shift in (("starsA", 541, 0), ("starsA", 542, 1)):
        gc = br.graph(name, V)
        m, B, F = gc.m, 3, 8
        allrows = np.arange(V)
        X, d0, d1, d2, res = br.inputs(V, (B, V >> shift, F), (B, V, F), (B, V, F), (B, V, F), (B, V, F))
        T1, T2, e1, e2 = br.planes(m, X, shift)
        zero = np.zeros((B, V, F), np.float32)
        worst[f"L plane shift {shift}"] = _ratio(_chain32(m, allrows, zero.copy(), [(m.a, X)], shift), T1, e1)
        worst[f"L2 plane shift {shift}"] = _ratio(_chain32(m, allrows, zero.copy(), [(m.b, X)], shift), T2, e2)
        for resid in (res, None):
            ref, eb = br.bwd(m, d0, d1, d2, resid, shift)
            Vout = V >> shift
            acc = np.zeros((B, Vout, F), np.float32)
            for ch in range(1 << shift):
                rows = (np.arange(Vout) << shift) + ch
                acc = acc + d0[:, rows]
                if resid is not None:
                    acc = acc + resid[:, rows]
                acc = _chain32(m, rows, acc, [(m.a, d1), (m.b, d2)])
            worst[f"backward shift {shift} resid {resid is not None}"] = _ratio(acc, ref, eb)
        if shift == 0:
            for nc, ldp in ((3, 32), (4, 12)):
                P, bias, G = br.inputs(V + nc, (B, V, ldp), (nc,), (B, V, nc))
                ref, eb = br.combine(m, P, nc, ldp, bias, 1000.0)
                acc = _chain32(m, allrows, P[..., :nc] + bias, [(m.a, P[..., nc:2 * nc]), (m.b, P[..., 2 * nc:3 * nc])])
                worst[f"combine nc {nc}"] = _ratio(acc * np.float32(1000.0), ref, eb)
                ref, eb = br.expand(m, G, nc, 3 * nc + 1)
                E = np.zeros((B, V, 3 * nc + 1), np.float32)
                E[..., :nc] = G
                E[..., nc:2 * nc] = _chain32(m, allrows, np.zeros_like(G), [(m.a, G)])
                E[..., 2 * nc:3 * nc] = _chain32(m, allrows, np.zeros_like(G), [(m.b, G)])
                worst[f"expand nc {nc}"] = _ratio(E, ref, eb)
        else:
            pm = br.paired(m)
            P1, P2, e1, e2 = br.pair_planes(m, d0)
            pr = np.arange(V // 2)
            worst["paired L plane"] = _ratio(_chain32(pm, pr, np.zeros((B, V // 2, F), np.float32), [(pm.a, d0)]), P1, e1)
            worst["paired L2 plane"] = _ratio(_chain32(pm, pr, np.zeros((B, V // 2, F), np.float32), [(pm.b, d0)]), P2, e2)
    for k, v in worst.items():
        print(f"  float32 chain / bound, {k}: {v:.3f}")
    assert max(worst.values()) <= 1.0, worst
    # the bound is no blanket either: the float32 chains use a fair share of it
    assert max(worst.values()) > 0.02, worst


# ---- 4. planted faults leave the bound ----------------------------------------------------------------------------------------

def _outside(got, ref, bound, what, every=True):
    """A faulty result `got` [.., rows, F] leaves the bound around ref: on every affected element, or (every=False, faults that
    touch whole tensors, where the misplaced contribution is by chance smaller than the bound on a few elements) on more than
    99 % of them and on at least one feature of every row."""
    excess = np.abs(got - ref) / bound
    share = float((excess > 1.0).mean())
    print(f"  {what}: error / bound over the affected elements: smallest {excess.min():.3g}, median {np.median(excess):.3g}, "
          f"{100 * share:.2f} % above 1")
    if every:
        assert (excess > 1.0).all(), (what, float(excess.min()))
    else:
        assert share > 0.99 and (excess.max(axis=-1) > 1.0).all(), (what, share)


def test_planted_faults_exceed_the_bound():
    gc = br.graph("starsA", 542)
    m, V, B, F = gc.m, 542, 3, 32
    X, d0, d1, d2, res = br.inputs(5, (B, V, F), (B, V, F), (B, V, F), (B, V, F), (B, V, F))
    T1, T2, e1, e2 = br.planes(m, X, 0)
    # the centre of the 203-star: the longest row, and every entry has both coefficients (a leaf has no a towards other leaves)
    long_row = next(r for r in np.where(m.lens == 203)[0] if m.row(r)[1].all() and m.row(r)[2].all())
    assert m.lens[long_row] == m.lens.max() == 203
    # one entry dropped from the longest row (the last one: what an unroll that stops one short leaves out)
    cut = m.edited(long_row, keep=np.arange(202))
    F1, F2, _, _ = br.planes(cut, X, 0)
    _outside(F1[:, long_row], T1[:, long_row], e1[:, long_row], "last entry of the longest row dropped, L plane")
    _outside(F2[:, long_row], T2[:, long_row], e2[:, long_row], "last entry of the longest row dropped, L2 plane")
    others = np.delete(np.arange(V), long_row)
    assert np.array_equal(F1[:, others], T1[:, others])
    # a and b swapped on one row
    for row in (long_row, int(np.where(m.lens == 5)[0][0])):
        sw = m.edited(row, swap=True)
        F1, F2, _, _ = br.planes(sw, X, 0)
        _outside(F1[:, row], T1[:, row], e1[:, row], f"a and b swapped on a row of {m.lens[row]} entries, L plane")
        _outside(F2[:, row], T2[:, row], e2[:, row], f"a and b swapped on a row of {m.lens[row]} entries, L2 plane")
    # child 2p + 1 left out of a shift-1 backward
    ref, eb = br.bwd(m, d0, d1, d2, res, 1)
    fine, _ = br.bwd(m, d0, d1, d2, res, 0)
    _outside(fine[:, 0::2], ref, eb, "child 2p + 1 left out of the backward", every=False)
    # sample b read as sample b - 1
    _outside(np.roll(T1, 1, axis=0)[1:], T1[1:], e1[1:], "sample b - 1 for sample b, L plane", every=False)
    full, fb = br.bwd(m, d0, d1, d2, None, 0)
    _outside(np.roll(full, 1, axis=0)[1:], full[1:], fb[1:], "sample b - 1 for sample b, backward", every=False)
    # column nc + c read as c in the combine: only rows with a neighbour see P1 through more than the diagonal, all rows see it
    for nc, ldp in ((3, 32), (1, 3)):
        P, bias = br.inputs(9 + nc, (B, V, ldp), (nc,))
        Y, yb = br.combine(m, P, nc, ldp, bias)
        Pf = P.copy()
        Pf[..., nc:2 * nc] = P[..., :nc]
        _outside(br.combine(m, Pf, nc, ldp, bias)[0], Y, yb, f"column c for column nc + c in the combine, nc {nc}",
                 every=False)
