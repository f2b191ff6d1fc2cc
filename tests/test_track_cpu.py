"""No GPU: the yardstick of the tracker (tests/track_ref.py) and its cases (tests/track_cases.py) on their own.

Every hand-made case gives what its rule gives by hand, and is decided by that rule: with the rule's parameter or input
flipped the outcome changes.  The walkers are a condition on the inputs: on them the yardstick alone switches no identity and
issues as many ids as there are people.  Feeding the frames in chunks or one by one gives the yardstick the same results."""
import os
import re

import numpy as np
import pytest

import track_cases as tc
import track_ref

CASES = tc.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    """Equal integers; equal bits for floats, with NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


@pytest.fixture(scope="module")
def yard():
    return {n: tc.run_ref(c) for n, c in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_gives_what_its_rule_gives_and_is_decided_by_it(yard, name):
    c = CASES[name]
    out, st = yard[name]
    for f, k, want in c["expect"]:
        got = out[k][f, 0]
        assert same(got, np.asarray(want, got.dtype).reshape(got.shape)), (name, f, k, got, want)
    # invariants of every case
    F, S, P = c["people"].shape[:3]
    T = c["slots"]
    fl = out["flags"]
    for f in range(F):
        for s in range(S):
            present = np.isfinite(c["people"][f, s]).all((1, 2))
            so, po = out["slot_of"][f, s], out["person_of"][f, s]
            assert ((so == -1) == ~present).all() and out["dropped"][f, s] == (so == -2).sum()
            for p in np.flatnonzero(so >= 0):
                assert po[so[p]] == p and out["joints"][f, s, so[p]].tobytes() == c["people"][f, s, p].tobytes()
            assert (po >= 0).sum() == (so >= 0).sum()
            assert np.isnan(out["joints"][f, s][po < 0]).all()
            assert (((fl[f, s] & tc.A) != 0) == (out["uid"][f, s] >= 0)).all() and (((fl[f, s] & tc.Pn) != 0) == (po >= 0)).all()
            assert (np.isnan(out["cost"][f, s]) | ((fl[f, s] & (tc.Pn | tc.B)) == tc.Pn)).all()
    assert (out["uid"].max((0, 2)) < st["next_uid"]).all()             # every id handed out lies below the counter
    assert same(st["uid"], out["uid"][-1]) and st["pose"].shape == (S, T) + c["people"].shape[3:]
    if c["flip"] is not None:
        other, _ = tc.run_ref(tc.flipped(c))
        assert any(not same(other[k], out[k]) for k in track_ref.OUTPUTS), (name, c["rule"])


def test_case_list_covers_every_flag_and_both_negative_slots(yard):
    flags = np.concatenate([o["flags"].ravel() for o, _ in yard.values()])
    for bit in (tc.A, tc.Pn, tc.B, tc.Fr, tc.R):
        assert (flags & bit).any(), bit
    assert ((flags & tc.Fr != 0) & (flags & tc.B == 0)).any()          # fresh by re-acquisition, not by birth
    slots = np.concatenate([o["slot_of"].ravel() for o, _ in yard.values()])
    assert (slots == -1).any() and (slots == -2).any() and (slots >= 0).any()
    assert {c["rule"] for c in tc.hand_cases().values()} >= {"tie between two tracks", "tie between two persons",
                                                              "cost == gate is no match", "greedy, globally ascending"}
    assert all(c["flip"] is not None for c in tc.hand_cases().values())


def test_greedy_triple_differs_from_nearest_and_from_optimal():
    c = CASES["greedy_triple"]
    pairs = []
    out, _ = tc.run_ref(c, pairs=pairs)
    cost = np.full((3, 3), np.nan)
    for p, t, v, n in pairs:
        cost[p, t] = v
    assert not np.isnan(cost).any() and (cost[:2, :2] < c["kw"]["gate"]).all()      # the gate decides nothing among p0, p1
    greedy = out["slot_of"][1, 0].tolist()
    nearest, taken = [], set()
    for p in range(3):                                     # every person in list order takes its nearest free track
        t = min((t for t in range(3) if t not in taken), key=lambda t: cost[p, t])
        nearest.append(t)
        taken.add(t)
    import itertools
    best = min(itertools.permutations(range(3)), key=lambda a: sum(cost[p, a[p]] for p in range(3)))
    assert greedy != nearest and greedy != list(best), (greedy, nearest, best)
    assert sum(cost[p, greedy[p]] for p in range(3)) > sum(cost[p, best[p]] for p in range(3))


def test_walkers_switch_no_identity():
    people, truth = tc.walkers()
    assert same(people, CASES["walkers"]["people"])
    out, st = tc.run_ref(CASES["walkers"])
    ids = {}
    for f, s, p in zip(*np.nonzero(truth >= 0)):
        slot = out["slot_of"][f, s, p]
        assert slot >= 0
        ids.setdefault(int(truth[f, s, p]), set()).add(int(out["uid"][f, s, slot]))
    print(f"walkers: uids per person {ids}, missed detections {(truth[:, 0] >= 0).sum(1).tolist().count(5)} full frames of "
          f"{len(truth)}")
    assert len(ids) == 5 and all(len(v) == 1 for v in ids.values()), "regenerate the seed of track_cases.walkers"
    assert int(st["next_uid"][0]) == 5 and not out["dropped"].any()
    assert (truth[:, 0] >= 0).sum(1).min() < 5                         # detections are missed
    assert any((truth[f, 0] != truth[f + 1, 0]).any() for f in range(len(truth) - 1))      # the list order changes
    assert (out["flags"] & tc.Fr != 0).sum() > 5                       # and tracks are re-acquired


@pytest.mark.parametrize("name", ["walkers", "streams", "retired_slot_waits_a_frame", "ids_not_reused_after_reset"])
def test_chunked_and_frame_by_frame_agree(yard, name):
    out, st = yard[name]
    for chunk in (1, 5):
        o, s = tc.run_ref(CASES[name], chunk=chunk)
        assert all(same(o[k], out[k]) for k in track_ref.OUTPUTS), (name, chunk)
        assert all(same(s[k], st[k]) for k in track_ref.STATE), (name, chunk)


def test_streams_are_independent_in_the_yardstick(yard):
    c = CASES["streams"]
    out, st = yard["streams"]
    for s in (0, 3):
        alone = dict(c, people=c["people"][:, s:s + 1])
        o, z = tc.run_ref(alone)
        assert all(same(o[k][:, 0], out[k][:, s]) for k in track_ref.OUTPUTS) and same(z["pose"][0], st["pose"][s])


def test_header_and_symbol_table_list_the_tracker():
    header = open(os.path.join(ROOT, "include", "p2m.h")).read()
    assert re.search(r"\bint p2m_pose_track\(const float\* people,", header)
    from pose2mesh_release_amd import _lib, build, track
    assert "p2m_pose_track" in _lib.HIP_SYMBOLS and len(_lib.HIP_SYMBOLS["p2m_pose_track"][1]) == 22
    assert "track.hip" in build.HIP_SOURCES and build.HIP_SOURCE_FLAGS["track.hip"] == ["-ffp-contract=off"]
    assert (track.FLAG_ALIVE, track.FLAG_PRESENT, track.FLAG_BORN, track.FLAG_FRESH, track.FLAG_RETIRED) == \
        (tc.A, tc.Pn, tc.B, tc.Fr, tc.R)
    d = track.PoseTracker()
    assert dict(pose_thr=d.pose_thr, gate=d.gate, min_common=d.min_common, max_missed=d.max_missed) == track_ref.DEFAULTS


def test_cpu_tensors_are_refused():
    import torch
    from pose2mesh_release_amd import track, video
    from pose2mesh_release_amd._lib import P2MError
    with pytest.raises(P2MError):
        track.PoseTracker()(torch.zeros(1, 2, 4, 3))
    with pytest.raises(P2MError):
        video.OneEuroFilter().reset(mask=torch.zeros(2, dtype=torch.bool))
    table = torch.arange(12.0).reshape(4, 3)
    assert track.identity_colours(torch.tensor([[-1, 0, 5]]), table).tolist() == [[table[0].tolist(), table[0].tolist(), table[1].tolist()]]
