"""No GPU: the restatements, bounds and case tables of tests/weight_ref.py, which tests/test_gpu_weight_kernels.py holds the
weight kernels of csrc/weights.hip to.

  audit       the tables reach what they are named for: every residue class of the two chunk tails of k_weight_grad_unpack with
              and without a trip of the unrolled loop, both sides of every block edge (256 threads of k_weight_pack /
              k_weight_eff, 32 outputs of the unpack, the 32-element blocks that reduce the bias), every arm of the transpose by
              shape and alignment, every layout, K, stride and NULL pointer the issue names;
  spelling    the index-by-index restatements equal a plain transpose / einsum spelling;
  order-free  every exact case gives the same bits when summed in fp32 in a shuffled order, forwards and pairwise;
  teeth       nine planted faults, one per line of the kernels a rewrite could get wrong, each change the expected output of
              at least one case (the test prints how many);
  bounds      the derived bounds hold for fp32 emulations in two orders (chunk by chunk with every product rounded; pairwise
              with the P2 sum scaled once) with room to spare.  Largest error / bound seen: unpack dW 0.173 (1 + 1 chunks), db
              0.191 (2 chunks), weight_eff 0.550 (plain and fused alike, 192 x 128)."""
import numpy as np
import pytest

import weight_ref as wr

F32 = np.float32


def _case_ids(cases):
    return [c["name"] for c in cases]


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


# ---- audit ---------------------------------------------------------------------------------------------------------------------

def test_unpack_table_reaches_every_chunk_tail():
    n1 = {c["nchunks"] for c in wr.UNPACK_CASES}
    n2 = {c["nchunks2"] for c in wr.UNPACK_CASES if c["entry"] == "unpack2"}
    assert n1 >= {1, 2, 7, 8, 9, 24, 25, 31, 32, 33, 40, 41, 64, 65, 257}
    assert n2 >= {1, 7, 8, 9, 15, 16, 17, 33, 257}
    for unroll, counts in ((4, n1), (2, n2)):
        seen = {(main > 0, tail) for n in counts for main, tail in wr.chunk_tails(n, unroll)}
        print(f"unroll {unroll}: (main loop ran, tail trips) reached: {sorted(seen)}")
        assert seen >= {(m, t) for m in (False, True) for t in range(unroll)}
        # groups with no chunk at all, and the last chunk in every group position
        assert any(wr.chunk_tails(n, unroll)[wr.UNP_CG - 1] == (0, 0) for n in counts)
        assert {(n - 1) % wr.UNP_CG for n in counts} >= {0, wr.UNP_CG - 2, wr.UNP_CG - 1}
    # chunk_tails is the loop of the kernel: every chunk is visited once
    for n in sorted(n1 | n2):
        for unroll in (2, 4):
            assert sum(unroll * m + t for m, t in wr.chunk_tails(n, unroll)) == n


def test_unpack_table_reaches_every_named_class():
    cs = wr.UNPACK_CASES
    tot = lambda c: c["Fout"] * c["Fin"] * c["K"]
    assert len({c["name"] for c in cs}) == len(cs)
    assert {tot(c) for c in cs} >= {1, 31, 32, 33, 45, 495}
    assert max(c["nchunks"] * tot(c) for c in cs) <= 257 * 495
    assert {c["Fout"] for c in cs if c["db"] and c["pdb"]} >= {1, 31, 32, 33, 65}        # ... with the bias really reduced
    for lay in (0, 1):
        assert {c["K"] for c in cs if c["layout"] == lay and c["entry"] == "unpack"} >= {1, 2, 3, 4}
    assert all(c["K"] == 1 for c in cs if c["layout"] == 2) and any(c["layout"] == 2 for c in cs)
    for lay in (0, 1, 2):
        assert {c["accumulate"] for c in cs if c["layout"] == lay} == {0, 1}
    for ent in ("unpack", "unpack2"):
        sub = [c for c in cs if c["entry"] == ent]
        assert {c["accumulate"] for c in sub} == {0, 1}
        assert any(not c["db"] for c in sub) and any(not c["pdb"] and c["db"] for c in sub)
    assert any(not c["pdb2"] and c["pdb"] and c["db"] for c in cs if c["entry"] == "unpack2")
    un = [c for c in cs if c["entry"] == "unpack" and c["pdb"] and c["db"]]
    assert {"F", "3F", "F+5"} == {("F" if c["pdb_stride"] == c["Fout"] else "3F" if c["pdb_stride"] == 3 * c["Fout"] else "F+5")
                                  for c in un}
    assert all(c["pdb_stride"] == 3 * c["Fout"] and c["K"] == 3 and c["layout"] == 1 for c in cs if c["entry"] == "unpack2")
    # block edges: tot on both sides of 32 and not a multiple of 32; bias blocks: one partial, exactly one, several with a
    # partial last one
    assert {tot(c) % wr.UNP_BLOCK for c in cs} >= {0, 1, 31} and {tot(c) // wr.UNP_BLOCK for c in cs} >= {0, 1, 15}
    # shapes that tell index mistakes apart (per layout and entry at least one case with all three sizes different)
    for key in {(c["entry"], c["layout"]) for c in cs}:
        assert any(c["Fout"] != c["Fin"] and c["K"] * c["Fin"] != c["Fout"] and c["K"] * c["Fout"] != c["Fin"] and
                   c["Fout"] > 1 and c["Fin"] > 1 for c in cs if (c["entry"], c["layout"]) == key), key


def test_transpose_table_reaches_every_arm():
    shapes = wr.TRANSPOSE_SHAPES
    assert set(shapes) >= {(1, 1), (3, 5), (4, 4), (63, 65), (64, 64), (65, 63), (66, 70), (68, 132), (4, 130), (130, 4),
                           (128, 192)}
    assert [o[1:] for o in wr.TRANSPOSE_OFFSETS] == [(0, 0), (1, 0), (0, 1)]
    aligned = {s: wr.transpose_arms(*s) for s in shapes}
    for s, arms in aligned.items():
        print(s, sorted(arms))
        assert "tiled" in arms
        for _, w_off, wt_off in wr.TRANSPOSE_OFFSETS[1:]:
            assert wr.transpose_arms(*s, w_off=w_off, wt_off=wt_off) == {"general"}
    has = lambda *want: any(set(want) <= a for a in aligned.values())
    assert has("vec", "full_tile", "many_tiles") and aligned[(64, 64)] == {"tiled", "vec", "full_tile"}
    assert has("vec", "partial_rows", "partial_cols", "many_tiles") and has("vec", "partial_rows") and has("vec", "partial_cols")
    assert has("scalar", "partial_rows", "partial_cols", "many_tiles") and has("scalar", "full_tile")
    assert aligned[(66, 70)] >= {"scalar"} and aligned[(68, 132)] >= {"vec", "partial_rows", "partial_cols"}
    # R and C a multiple of 4 only one at a time: still the scalar arm
    assert any(r % 4 == 0 and c % 4 and "scalar" in a for (r, c), a in aligned.items())
    assert any(r % 4 and c % 4 == 0 and "scalar" in a for (r, c), a in aligned.items())
    # all of the table but the squares can tell R from C
    assert sum(r != c for r, c in shapes) >= 8


def test_pack_and_eff_tables_reach_the_block_edges():
    tots = {fo * fi * k for fo, fi, k, _, _ in wr.PACK_CASES}
    assert tots >= {255, 256, 257} and max(tots) > 2 * wr.PACK_BLOCK
    assert {k for _, _, k, _, _ in wr.PACK_CASES} == {1, 2, 3, 4}
    assert {(w2, w3) for _, _, _, w2, w3 in wr.PACK_CASES} == {(True, True), (True, False), (False, True), (False, False)}
    for fo, fi, k, w2, w3 in wr.PACK_CASES:
        assert fo != fi and fo % 32 and fi % 32
        assert wr.transpose_arms(fo, fi, K=k, w2=w2, w3=w3) == {"general"}
    assert sorted(ka * n for ka, n in wr.EFF_SHAPES) == [1, 255, 256, 257, 3 * 64 * 128]
    for ka, n in wr.EFF_SHAPES:
        Wt, a, b = wr.eff_inputs(ka, n, "zero")
        assert a == 0 and b == 0 and np.isfinite(Wt).all() and (Wt != 0).all()


# ---- spelling ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Fout,Fin,K", [(fo, fi, k) for fo, fi, k, _, _ in wr.PACK_CASES] + [(r, c, 1) for r, c in
                                                                                               wr.TRANSPOSE_SHAPES])
def test_pack_ref_is_the_transpose_spelling(Fout, Fin, K):
    W = wr.bit_patterns(Fout * 1000 + Fin, Fout * Fin * K).reshape(Fout, Fin * K)
    Wt, W2, W3 = wr.pack_ref(W, Fout, Fin, K)
    W3d = W.reshape(Fout, Fin, K)
    assert np.array_equal(Wt, W3d.transpose(2, 1, 0).reshape(K * Fin, Fout))
    assert np.array_equal(W2, W3d.transpose(0, 2, 1).reshape(Fout, K * Fin))
    assert np.array_equal(W3, W3d.transpose(2, 0, 1).reshape(K * Fout, Fin))
    if K == 1:
        assert np.array_equal(Wt, W.T) and np.array_equal(W2, W) and np.array_equal(W3, W)
    # the planted words are there: a permutation of them must move bits
    if W.size >= 9:
        f = W.view(F32)
        assert np.isnan(f).sum() >= 3 and (W == 0x80000000).any() and (W == 1).any()


@pytest.mark.parametrize("mode", wr.UNPACK_MODES)
@pytest.mark.parametrize("c", wr.UNPACK_CASES, ids=_case_ids(wr.UNPACK_CASES))
def test_unpack_ref_is_the_einsum_spelling(c, mode):
    d = wr.unpack_inputs(c, mode)
    r = wr.unpack_expected(c, d)
    Fout, Fin, K, n = c["Fout"], c["Fin"], c["K"], c["nchunks"]
    P = d["P"].astype(np.float64)
    if c["layout"] == 0:
        dW = np.einsum("ckif->fik", P.reshape(n, K, Fin, Fout))
    elif c["layout"] == 1:
        dW = np.einsum("cikf->fik", P.reshape(n, Fin, K, Fout))
    else:
        dW = P.reshape(n, Fout, Fin, 1).sum(0)
    if d["P2"] is not None:
        fac = np.array([1.0, F32(d["s1"]), F32(d["s2"])], np.float64)
        dW = dW + np.einsum("cif,k->fik", d["P2"].astype(np.float64).reshape(-1, Fin, Fout), fac)
    dW = dW.reshape(Fout, Fin * K) + (0 if d["dW0"] is None else d["dW0"].astype(np.float64))
    tol = 0.0 if mode == "exact" else 1e-12
    assert (np.abs(dW - r["dW"]) <= tol * r["S_dW"]).all()
    if not (c["db"] and c["pdb"]):
        assert r["db"] is None
        return
    db = d["Pdb"].astype(np.float64)[:, :Fout].sum(0)
    if c["pdb2"]:
        db = db + d["Pdb2"].astype(np.float64).sum(0)
    db = db + (0 if d["db0"] is None else d["db0"].astype(np.float64))
    assert (np.abs(db - r["db"]) <= tol * r["S_db"]).all()
    assert r["n_dW"] == n + c["nchunks2"] and r["n_db"] == n + (c["nchunks2"] if c["pdb2"] else 0)


@pytest.mark.parametrize("Ka,N", wr.EFF_SHAPES)
def test_eff_ref_spelling_and_zero_case(Ka, N):
    for mode in wr.EFF_MODES:
        Wt, a, b = wr.eff_inputs(Ka, N, mode)
        We, S = wr.eff_ref(Wt, Ka, N, a, b)
        w = Wt.astype(np.float64)
        plain = w[:Ka] + float(F32(a)) * w[Ka:2 * Ka] + float(F32(b)) * w[2 * Ka:]
        assert (np.abs(plain - We) <= (0 if mode != "real" else 1e-15) * S).all()
        if mode == "zero":
            assert np.array_equal(_bits(We), _bits(Wt[:Ka]))
        if mode == "exact":
            assert np.array_equal(We.astype(F32).astype(np.float64), We) and (Wt == np.round(Wt)).all()


# ---- fp32 emulations -----------------------------------------------------------------------------------------------------------

def _terms32(c, d, scale_once=False):
    """fp32 terms of dW [n, Fout, Fin, K] (+ dW0 last) and of db, every product s_k P2_c rounded to fp32 - or, scale_once, the P2
    terms left unscaled and returned apart with their factor."""
    Fout, Fin, K = c["Fout"], c["Fin"], c["K"]
    terms = [d["P"][:, wr.unpack_index(c["layout"], Fout, Fin, K)]]
    p2 = fac = None
    if d["P2"] is not None:
        fo, fi, k = np.meshgrid(np.arange(Fout), np.arange(Fin), np.arange(K), indexing="ij")
        fac = np.array([1.0, d["s1"], d["s2"]], F32)[k]
        p2 = d["P2"][:, fi * Fout + fo]
        if not scale_once:
            terms.append((p2 * fac).astype(F32))
    t = np.concatenate(terms).astype(F32)
    bt = None
    if c["db"] and c["pdb"]:
        bt = [d["Pdb"][:, :Fout]] + ([d["Pdb2"]] if c["pdb2"] else [])
        bt = np.concatenate(bt).astype(F32)
    return t, p2, fac, bt


def _seq(t):
    acc = t[0].copy()
    for x in t[1:]:
        acc = (acc + x).astype(F32)
    return acc


def _pairwise(t):
    t = list(t)
    while len(t) > 1:
        t = [(t[i] + t[i + 1]).astype(F32) if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0]


def _emulate(c, d, order, rng=None):
    """dW, db in fp32 arithmetic alone.  forward: chunk by chunk, products rounded, then the accumulate add; pairwise: tree sums,
    the P2 sum scaled once; shuffled: every term, prefill included, in a random order."""
    Fout, Fin, K = c["Fout"], c["Fin"], c["K"]
    t, p2, fac, bt = _terms32(c, d, scale_once=order == "pairwise")
    dW0 = None if d["dW0"] is None else d["dW0"].reshape(Fout, Fin, K)
    if order == "shuffled":
        full = t if dW0 is None else np.concatenate([t, dW0[None]])
        dW = _seq(full[rng.permutation(full.shape[0])])
        if bt is not None:
            fb = bt if d["db0"] is None else np.concatenate([bt, d["db0"][None]])
            bt = _seq(fb[rng.permutation(fb.shape[0])])
        return dW.reshape(Fout, Fin * K), bt
    red = _seq if order == "forward" else _pairwise
    dW = red(t)
    if order == "pairwise" and p2 is not None:
        dW = (dW + (red(p2) * fac).astype(F32)).astype(F32)
    if dW0 is not None:
        dW = (dW0 + dW).astype(F32)
    if bt is not None:
        bt = red(bt)
        if d["db0"] is not None:
            bt = (d["db0"] + bt).astype(F32)
    return dW.reshape(Fout, Fin * K), bt


@pytest.mark.parametrize("c", wr.UNPACK_CASES, ids=_case_ids(wr.UNPACK_CASES))
def test_exact_cases_survive_any_summation_order(c):
    d = wr.unpack_inputs(c, "exact")
    for a in (d["P"], d["Pdb"], d["P2"], d["Pdb2"], d["dW0"], d["db0"]):
        assert a is None or ((a == np.round(a)).all() and np.abs(a).max() <= wr.INT_MAX and
                             not (np.signbit(a) & (a == 0)).any())                    # integers, and no -0 among them
    r = wr.unpack_expected(c, d)
    want_w, want_b = r["dW"].astype(F32), None if r["db"] is None else r["db"].astype(F32)
    assert np.array_equal(want_w.astype(np.float64), r["dW"])                      # the expected values ARE fp32 numbers
    rng = np.random.default_rng(5)
    for order in ("forward", "pairwise", "shuffled", "shuffled"):
        dW, db = _emulate(c, d, order, rng)
        assert np.array_equal(_bits(dW), _bits(want_w)), order
        assert (db is None) == (want_b is None) and (db is None or np.array_equal(_bits(db), _bits(want_b))), order


def test_exact_eff_cases_survive_fma_and_order():
    for Ka, N in wr.EFF_SHAPES:
        Wt, a, b = wr.eff_inputs(Ka, N, "exact")
        want = wr.eff_ref(Wt, Ka, N, a, b)[0].astype(F32)
        w0, w1, w2 = Wt[:Ka], Wt[Ka:2 * Ka], Wt[2 * Ka:]
        rounded = ((w0 + (F32(a) * w1).astype(F32)).astype(F32) + (F32(b) * w2).astype(F32)).astype(F32)
        other = (w0 + ((F32(b) * w2).astype(F32) + (F32(a) * w1).astype(F32)).astype(F32)).astype(F32)
        fused = (w0.astype(np.float64) + a * w1.astype(np.float64) + b * w2.astype(np.float64)).astype(F32)
        for got in (rounded, other, fused):
            assert np.array_equal(_bits(got + F32(0)), _bits(want))


_worst = {}


@pytest.mark.parametrize("c", wr.UNPACK_CASES, ids=_case_ids(wr.UNPACK_CASES))
def test_unpack_bound_holds_for_fp32_in_two_orders(c):
    d = wr.unpack_inputs(c, "real")
    r = wr.unpack_expected(c, d)
    for order in ("forward", "pairwise"):
        dW, db = _emulate(c, d, order)
        ratio = float((np.abs(dW.astype(np.float64) - r["dW"]) / wr.unpack_bound(r["n_dW"], r["S_dW"])).max())
        _worst["dW"] = max(_worst.get("dW", 0.0), ratio)
        print(f"{c['name']} {order}: dW err / bound {ratio:.3f}")
        assert ratio <= 0.5
        if db is not None:
            rb = float((np.abs(db.astype(np.float64) - r["db"]) / wr.unpack_bound(r["n_db"], r["S_db"])).max())
            _worst["db"] = max(_worst.get("db", 0.0), rb)
            print(f"{c['name']} {order}: db err / bound {rb:.3f}")
            assert rb <= 0.5
    print("largest so far:", _worst)


def test_eff_bound_holds_for_fp32_with_and_without_fma():
    worst = 0.0
    for Ka, N in wr.EFF_SHAPES:
        Wt, a, b = wr.eff_inputs(Ka, N, "real")
        We, S = wr.eff_ref(Wt, Ka, N, a, b)
        w0, w1, w2 = Wt[:Ka], Wt[Ka:2 * Ka], Wt[2 * Ka:]
        plain = ((w0 + (F32(a) * w1).astype(F32)).astype(F32) + (F32(b) * w2).astype(F32)).astype(F32)
        w1d, w2d = w1.astype(np.float64), w2.astype(np.float64)
        t = (w0.astype(np.float64) + float(F32(a)) * w1d).astype(F32)                 # fma(a, w1, w0), then fma(b, w2, .)
        fused = (t.astype(np.float64) + float(F32(b)) * w2d).astype(F32)
        for name, got in (("plain", plain), ("fused", fused)):
            ratio = float((np.abs(got.astype(np.float64) - We) / wr.eff_bound(S)).max())
            worst = max(worst, ratio)
            print(f"eff {Ka} x {N} {name}: err / bound {ratio:.3f}")
            assert ratio <= 0.75                # an element where |a w1| dominates can take 2.5 of the 4 roundings' worth
    print(f"largest: {worst:.3f}")


# ---- teeth ---------------------------------------------------------------------------------------------------------------------

def _differs(a, b):
    if (a["db"] is None) != (b["db"] is None):
        return True
    return bool((a["dW"] != b["dW"]).any() or (a["db"] is not None and (a["db"] != b["db"]).any()))


def _fault_drop_last_chunk(c, d):
    if c["nchunks"] < 2:
        return None
    return wr.unpack_expected(c, d, nchunks=c["nchunks"] - 1)


def _fault_drop_last_chunk2(c, d):
    if c["entry"] != "unpack2" or c["nchunks2"] < 2:
        return None
    return wr.unpack_expected(c, d, nchunks2=c["nchunks2"] - 1, Pdb2=d["Pdb2"][:-1] if c["pdb2"] else None)


def _fault_plane_factor_shifted(c, d):
    """(1, s1, s2)[k - 1]: plane 0 takes s2, plane 1 takes 1, plane 2 takes s1 - through the second route, P2 pre-scaled."""
    if c["entry"] != "unpack2":
        return None
    Fout, Fin = c["Fout"], c["Fin"]
    f = np.array([d["s2"], 1.0, d["s1"]], F32).reshape(1, 1, 3, 1)
    P2s = (d["P2"].reshape(-1, Fin, 1, Fout) * f).reshape(c["nchunks2"], Fin * 3 * Fout)
    first = wr.unpack_expected(c, d, P2=None, nchunks2=0)                      # Pdb2 is still summed by ...
    out = wr.unpack_ref(P2s, None, c["nchunks2"], Fout, Fin, 3, 1, 3 * Fout, dW0=first["dW"].astype(F32))
    out["db"] = wr.unpack_expected(c, d)["db"]                                # ... the right route: only dW is at fault
    return out


def _fault_ignore_accumulate(c, d):
    if not c["accumulate"]:
        return None
    return wr.unpack_expected(c, d, dW0=None, db0=None)


def _fault_swap_layouts(c, d):
    if c["layout"] == 2:
        return None
    return wr.unpack_expected(c, d, layout=1 - c["layout"])


def _fault_pdb_stride(c, d):
    if c["pdb_stride"] != 3 * c["Fout"] or not (c["pdb"] and c["db"]):
        return None
    return wr.unpack_expected(c, d, pdb_stride=c["Fout"])


def _fault_no_pdb2(c, d):
    if c["entry"] != "unpack2" or not (c["pdb"] and c["db"] and c["pdb2"]):
        return None
    return wr.unpack_expected(c, d, Pdb2=None)


UNPACK_FAULTS = {"drop the last chunk": _fault_drop_last_chunk, "drop the last chunk of P2": _fault_drop_last_chunk2,
                 "plane factor of k - 1": _fault_plane_factor_shifted, "ignore accumulate": _fault_ignore_accumulate,
                 "swap the index maps of layouts 0 and 1": _fault_swap_layouts,
                 "read Pdb at stride Fout where it is 3 Fout": _fault_pdb_stride, "leave Pdb2 out": _fault_no_pdb2}


@pytest.mark.parametrize("mode", wr.UNPACK_MODES)
@pytest.mark.parametrize("fault", list(UNPACK_FAULTS))
def test_planted_unpack_fault_changes_an_expected_output(fault, mode):
    applies = caught = 0
    for c in wr.UNPACK_CASES:
        d = wr.unpack_inputs(c, mode)
        bad = UNPACK_FAULTS[fault](c, d)
        if bad is None:
            continue
        applies += 1
        good = wr.unpack_expected(c, d)
        if mode == "exact":
            hit = _differs(good, bad)
        else:                                                  # real-valued: the fault must clear the bound, not merely differ
            hit = bool((np.abs(good["dW"] - bad["dW"]) > 2 * wr.unpack_bound(good["n_dW"], good["S_dW"])).any())
            if good["db"] is not None and bad["db"] is not None:
                hit |= bool((np.abs(good["db"] - bad["db"]) > 2 * wr.unpack_bound(good["n_db"], good["S_db"])).any())
        caught += hit
        if not hit:
            print(f"  not seen by {c['name']}")
    print(f"{fault} ({mode}): changes {caught} of the {applies} cases it applies to")
    assert applies >= 2 and caught >= 1


def test_the_second_route_is_the_first_on_exact_data():
    """unpack2 == unpack (layout 1) of P, then an accumulating unpack of the pre-scaled P2: the GPU file's independent route."""
    for c in (c for c in wr.UNPACK_CASES if c["entry"] == "unpack2"):
        d = wr.unpack_inputs(c, "exact")
        Fout, Fin = c["Fout"], c["Fin"]
        one = wr.unpack_expected(c, d)
        first = wr.unpack_expected(c, d, P2=None, Pdb2=None, nchunks2=0)
        P2s = wr.prescale_p2(d["P2"], c["nchunks2"], Fout, Fin, d["s1"], d["s2"])
        second = wr.unpack_ref(P2s, d["Pdb2"] if c["pdb2"] else None, c["nchunks2"], Fout, Fin, 3, 1, Fout,
                               dW0=first["dW"].astype(F32), db0=None if first["db"] is None else first["db"].astype(F32),
                               want_db=first["db"] is not None)
        assert np.array_equal(one["dW"], second["dW"])
        if one["db"] is not None:
            assert np.array_equal(one["db"], second["db"] if c["pdb2"] else first["db"])


def test_planted_pack_faults_change_an_expected_output():
    swapped = w3_as_w2 = 0
    shapes = [(fo, fi, k) for fo, fi, k, _, _ in wr.PACK_CASES] + [(r, c, 1) for r, c in wr.TRANSPOSE_SHAPES]
    for Fout, Fin, K in shapes:
        W = wr.bit_patterns(Fout * 1000 + Fin, Fout * Fin * K)
        Wt, W2, W3 = wr.pack_ref(W, Fout, Fin, K)
        if K == 1:                                             # transpose with R and C swapped
            swapped += not np.array_equal(wr.pack_ref(W, Fin, Fout, 1)[0].reshape(-1), Wt.reshape(-1))
        w3_as_w2 += not np.array_equal(W3.reshape(-1), W2.reshape(-1))
    print(f"R and C swapped: changes {swapped} shapes; W3 in W2's layout: changes {w3_as_w2} shapes")
    assert swapped == len([s for s in shapes if s[2] == 1 and s[0] != s[1] and min(s[:2]) > 1]) >= 9
    assert w3_as_w2 == len([s for s in shapes if s[2] > 1 and s[0] > 1]) >= 5
