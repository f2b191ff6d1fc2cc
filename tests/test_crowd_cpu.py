"""No GPU: the yardstick of the crowd kernels (tests/crowd_ref.py) and its cases (tests/crowd_cases.py) on their own.

Every hand-made case gives what the rules give by hand, and is decided by the rule it names: with that one rule turned around
in the yardstick the outcome changes.  The random crowds keep clear of both thresholds, so that the device's fixed-order float64
sums (sequential) and numpy's (pairwise) cannot decide a pair or a score differently.  The colour formula of include/p2m.h is
restated here operation by operation and held to the standard library's colorsys at the sector edges and the rounding ties."""
import colorsys

import numpy as np
import pytest

import crowd_cases as cc
import crowd_ref
import sample_ref

CASES = cc.cases()


def run(case, flip=None, pairs=None):
    return crowd_ref.select(case["dets"], case["num"], flip=flip, pairs=pairs, **case["kw"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_gives_what_the_rules_give_and_is_decided_by_its_rule(name):
    case = CASES[name]
    out = run(case)
    P = case["dets"].shape[1]
    for k, want in case["expect"].items():
        got = out[k][0]
        assert np.array_equal(got, np.asarray(want, got.dtype).reshape(np.shape(got))), (name, k, got, want)
    # invariants of every case
    for b in range(len(out["count"])):
        n = int(out["count"][b])
        kept = np.flatnonzero(out["keep"][b])
        assert n == len(kept) and out["index"][b, :n].tolist() == kept.tolist() and (out["index"][b, n:] == -1).all()
        assert np.isnan(out["joints"][b, n:]).all() and np.isfinite(out["joints"][b, :n]).all()
        assert (out["dup_of"][b][out["reason"][b] != 2] == -1).all()
        for i in np.flatnonzero(out["reason"][b] == 2):
            assert out["dup_of"][b, i] < i and out["keep"][b, out["dup_of"][b, i]]
        J = case["dets"].shape[2]
        assert out["joints"][b, :n, :J].tobytes() == case["dets"][b, kept].tobytes()
    if case["rule"] is not None:
        flipped = run(case, flip=case["rule"])
        assert any(not np.array_equal(flipped[k], out[k]) for k in ("reason", "dup_of")), (name, case["rule"])
    assert P == out["reason"].shape[1]


def test_case_list_covers_every_flip():
    flips = {"greedy", "low", "lowest", "zeros", "empty", "strict_mean", "strict_score", "thr32", "conf_mean", "nonfinite"}
    assert flips <= {c["rule"] for c in CASES.values()}


def test_midpoints_are_the_reference_arithmetic():
    """(a + b) * 0.5 in float64 is not always a float32: the output rounds it once."""
    p = cc.person()
    p[5, 0], p[6, 0] = np.float32(1e5 + 0.0078125), np.float32(3.0000002)
    out = crowd_ref.select(p[None, None])
    neck = (np.float64(p[5, 0]) + np.float64(p[6, 0])) * 0.5
    assert np.float64(np.float32(neck)) != neck and out["joints"][0, 0, 18, 0] == np.float32(neck)
    assert out["joints"][0, 0, 18, 2] == np.float32(np.float64(p[5, 2]) * np.float64(p[6, 2]))
    assert out["joints"][0, 0, 17, 2] == np.float32(np.float64(p[11, 2]) * np.float64(p[12, 2]))


def test_random_crowds_keep_clear_of_the_thresholds():
    case = CASES["random_crowds"]
    pairs = []
    out = run(case, pairs=pairs)
    bad_pairs, bad_scores = cc.band_violations(pairs, out["score"])
    assert not bad_pairs and not len(bad_scores), "regenerate the seed of crowd_cases.random_crowds"
    reason = out["reason"]
    frac = (reason == 2).mean()
    print(f"random crowds: {len(pairs)} comparisons, duplicates {frac:.2f}, low {(reason == 1).mean():.2f}, "
          f"accepted {(reason == 0).mean():.2f}")
    assert 0.4 <= frac <= 0.6 and (reason == 1).any() and (out["count"] >= 4).all()
    # the comparisons are not all far from min_diff: some pairs sit within a factor 2 of it on either side
    means = np.array([p[4] for p in pairs if p[3]])
    assert ((means > 10) & (means < 20)).any() and ((means >= 20) & (means < 40)).any()
    # and the order of a float64 sum moves no decision: sequential sums (the device's order) decide every pair alike
    dets = case["dets"].astype(np.float64)
    for b, i, d, size, mean in pairs:
        if not size:
            continue
        ji, jd = (np.concatenate([dets[b, k]] + [((dets[b, k, a0] + dets[b, k, a1]) * 0.5)[None] for a0, a1 in
                                                 crowd_ref.COCO_MIDPOINTS]) for k in (i, d))
        ci, cd = ([*dets[b, k, :, 2], *(dets[b, k, a0, 2] * dets[b, k, a1, 2] for a0, a1 in crowd_ref.COCO_MIDPOINTS)] for k in (i, d))
        S, n = 0.0, 0
        for j in range(19):
            if ci[j] > 0.1 and cd[j] > 0.1:
                for a in (0, 1):
                    t = abs(ji[j, a] - jd[j, a])
                    if t != 0:
                        S, n = S + t, n + 1
        assert n == size and (S / n < 20.0) == (mean < 20.0) and abs(S / n - mean) <= 1e-12 * mean


# ---- colours ----------------------------------------------------------------------------------------------------------------
def header_formula(h, s, v):
    """p2m_person_colours as include/p2m.h words it, one float64 operation at a time."""
    if s == 0.0:
        return v, v, v
    h6 = h * 6.0
    i = int(h6)
    f = h6 - float(i)
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    return [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)][i % 6]


def test_stage_11_is_a_stage_of_its_own():
    h = crowd_ref.hues(123, 0, 64)
    assert ((h >= 0) & (h < 1)).all() and len(np.unique(h)) == 64
    assert np.array_equal(h * 2.0 ** 24, np.floor(h * 2.0 ** 24))
    cam = sample_ref.uniforms(sample_ref._words(123, np.arange(64, dtype=np.uint64), 0, 10, [0])[0][:, 0])
    assert not np.isin(h, cam).any()                       # stage 10's word 0 at the same indices is something else
    assert np.array_equal(crowd_ref.hues(123, 5, 10), h[5:15])
    assert np.array_equal(crowd_ref.hues(123, 2 ** 32 - 3, 6)[:3], crowd_ref.hues(123, 2 ** 32 - 3, 3))


@pytest.mark.parametrize("n, seed, first", cc.COLOUR_RUNS)
def test_colours_of_the_stream(n, seed, first):
    h = crowd_ref.hues(seed, first, n)
    rgb, u8, rgb64 = crowd_ref.colours_of(h)
    assert rgb.shape == (n, 3) and u8.shape == (n, 3) and rgb.dtype == np.float32 and u8.dtype == np.uint8
    assert np.array_equal(rgb64, np.array([header_formula(x, 0.5, 1.0) for x in h]).reshape(n, 3))
    assert (rgb64.max(1) == 1.0).all() and (rgb64.min(1) == 0.5).all()
    if n == 256:
        assert set((h * 6.0).astype(int) % 6) == set(range(6))           # every sector is hit


def test_sector_edges_and_ties():
    h = cc.edge_hues()
    assert set((h * 6.0).astype(int)) == set(range(6))
    for s, v in cc.TIE_SV:
        rgb, u8, rgb64 = crowd_ref.colours_of(h, s, v)
        mine = np.array([header_formula(x, s, v) for x in h])
        assert np.array_equal(rgb64, mine), (s, v)
        ties = np.abs(255.0 * rgb64 - np.floor(255.0 * rgb64) - 0.5) == 0
        assert ties.any(), (s, v)
        assert (u8[ties] % 2 == 0).all()                                  # half to even, not half up
    assert np.rint(255.0 * 0.5) == 128 and colorsys.hsv_to_rgb(0.25, 0.0, 0.5) == (0.5, 0.5, 0.5)
