"""Cases of the tracker tests (tests/test_track_cpu.py, tests/test_gpu_track.py).  The hand-made sequences have integer or
dyadic coordinates and dyadic gates, so that ties and thresholds are exactly representable; each is decided by the rule it
names, and `flip` - another parameter, another input or no reset - changes its outcome.

The hand skeleton is the 4 corners of an 8 x 16 box: a track of it has size 16, and a person shifted by d in x against it has
cost (4 d / 8) / 16 = d / 32.

A case:  people fp32 [F, S, P, Jo, 3];  slots;  kw: the tracker's parameters;  resets: {frame: None | bool [S]} = a reset
BEFORE that frame;  expect: [(frame, output, value of stream 0)];  flip: None or a dict of replacements for people / slots /
kw / resets;  rule: what decides the case."""
import numpy as np

import track_ref

BOX = np.array([[0, 0], [8, 0], [0, 16], [8, 16]], np.float32)
NOBODY = np.full((4, 3), np.nan, np.float32)
A, Pn, B, Fr, R = track_ref.ALIVE, track_ref.PRESENT, track_ref.BORN, track_ref.FRESH, track_ref.RETIRED


def box(dx=0.0, dy=0.0, conf=1.0, scale=1.0):
    p = np.empty((4, 3), np.float32)
    p[:, :2] = BOX * np.float32(scale) + np.array([dx, dy], np.float32)
    p[:, 2] = conf
    return p


def frames(*fr):
    """fr: per frame a list of poses [Jo, 3]; shorter lists are padded with nobody.  -> [F, 1, P, Jo, 3]"""
    P = max(max(len(f) for f in fr), 1)
    Jo = next(p.shape[0] for f in fr for p in f)
    out = np.full((len(fr), 1, P, Jo, 3), np.nan, np.float32)
    for k, f in enumerate(fr):
        for i, p in enumerate(f):
            out[k, 0, i] = p
    return out


def case(people, slots, expect, rule, flip, resets=None, **kw):
    return {"people": people, "slots": slots, "kw": dict(track_ref.DEFAULTS, **kw), "resets": resets or {}, "expect": expect,
            "flip": flip, "rule": rule}


def flipped(c):
    """The case with its flip applied."""
    f = dict(c)
    for k, v in c["flip"].items():
        f[k] = dict(c["kw"], **v) if k == "kw" else v
    f["flip"] = None
    return f


def hand_cases():
    c = {}
    # two tracks at 0 and 16, one person at 8: cost 1/4 to both -> the lower slot.  Flip: at 9, nearer to track 1
    c["tie_tracks_lower_slot"] = case(
        frames([box(0), box(16)], [box(8)]), 2, [(1, "slot_of", [0, -1]), (1, "person_of", [0, -1]), (1, "cost", [0.25, np.nan])],
        "tie between two tracks", {"people": frames([box(0), box(16)], [box(9)])}, gate=0.5)
    # one track at 8, persons at 0 and 16: the lower person gets it, the other is born.  Flip: person 0 at -1 is farther
    c["tie_persons_lower_person"] = case(
        frames([box(8)], [box(0), box(16)]), 2, [(1, "slot_of", [0, 1]), (1, "flags", [A | Pn, A | Pn | B | Fr])],
        "tie between two persons", {"people": frames([box(8)], [box(-1), box(16)])}, gate=0.5)
    c["cost_equals_gate"] = case(
        frames([box(0)], [box(8)]), 2, [(1, "slot_of", [1]), (1, "uid", [0, 1]), (1, "flags", [A, A | Pn | B | Fr])],
        "cost == gate is no match", {"kw": {"gate": 0.2500001}}, gate=0.25)
    weak = box(0)
    weak[:2, 2] = 0.0625                                   # two of the four joints below pose_thr: 2 in common
    c["min_common_minus_one"] = case(
        frames([box(0)], [weak]), 2, [(1, "slot_of", [1]), (1, "dropped", 0)], "fewer than min_common joints in common",
        {"kw": {"min_common": 2}}, gate=0.25, min_common=3)
    # tracks at 0, 3, 20; persons at -2, 1, 20 (costs in 1/32: p0 2 | 5 | 22, p1 1 | 2 | 19, p2 20 | 17 | 0).  Ascending greedy:
    # (p2, t2) 0, (p1, t0) 1, (p0, t1) 5 = 6 in all.  Each person's nearest: p0 -> t0, p1 -> t0.  Optimal: p0 t0, p1 t1 = 4.
    c["greedy_triple"] = case(
        frames([box(0), box(3), box(20)], [box(-2), box(1), box(20)]), 3,
        [(1, "slot_of", [1, 0, 2]), (1, "cost", [1 / 32, 5 / 32, 0.0])], "greedy, globally ascending",
        {"people": frames([box(0), box(3), box(20)], [box(-2), box(2.5), box(20)])}, gate=0.5)
    # slot 0 is retired in frame 1 (max_missed = 0) and free in frame 2, where persons 0 and 2 are new
    c["births_in_person_order"] = case(
        frames([NOBODY, box(0), box(100)], [box(100)], [box(300), box(100), box(200)]), 4,
        [(0, "slot_of", [-1, 0, 1]), (2, "slot_of", [0, 1, 2]), (2, "uid", [2, 1, 3, -1]),
         (2, "flags", [A | Pn | B | Fr, A | Pn, A | Pn | B | Fr, 0])], "births in person order into the lowest free slot",
        {"people": frames([NOBODY, box(0), box(100)], [box(100)], [box(200), box(100), box(300)])}, gate=0.25, max_missed=0)
    c["retired_slot_waits_a_frame"] = case(
        frames([box(0), box(100)], [box(100), box(200)], [box(100), box(200)]), 2,
        [(1, "slot_of", [1, -2]), (1, "flags", [R, A | Pn]), (1, "dropped", 1), (1, "uid", [-1, 1]), (2, "slot_of", [1, 0]),
         (2, "uid", [2, 1])], "a slot retired this frame is free from the next", {"kw": {"max_missed": 1}},
        gate=0.25, max_missed=0)
    c["overflow"] = case(
        frames([box(0), box(100), box(200)], [box(0), box(100), box(200)]), 2,
        [(0, "slot_of", [0, 1, -2]), (0, "dropped", 1), (1, "slot_of", [0, 1, -2]), (1, "dropped", 1), (1, "uid", [0, 1]),
         (1, "flags", [A | Pn, A | Pn]), (1, "cost", [0.0, 0.0])], "no free slot: dropped", {"slots": 3}, gate=0.25)
    c["survives_max_missed"] = case(
        frames([box(0)], [], [], []), 1, [(2, "flags", [A]), (2, "uid", [0]), (3, "flags", [R]), (3, "uid", [-1])],
        "retired at max_missed + 1", {"kw": {"max_missed": 3}}, max_missed=2)
    c["max_missed_zero"] = case(
        frames([box(0)], []), 1, [(1, "flags", [R]), (1, "uid", [-1])], "max_missed = 0", {"kw": {"max_missed": 1}}, max_missed=0)
    c["rematch_after_gap"] = case(
        frames([box(0)], [], [], [box(1)]), 2,
        [(3, "slot_of", [0]), (3, "uid", [0, -1]), (3, "flags", [A | Pn | Fr, 0]), (3, "cost", [1 / 32, np.nan])],
        "re-match after a gap keeps the uid and is fresh", {"people": frames([box(0)], [box(0)], [box(0)], [box(1)])},
        gate=0.25, max_missed=5)
    c["nan_hole"] = case(
        frames([box(0), NOBODY, box(100)]), 3, [(0, "slot_of", [0, -1, 1]), (0, "person_of", [0, 2, -1])],
        "a NaN hole in the middle of the list", {"people": frames([box(0), box(200), box(100)])})
    hot = box(100)
    hot[3] = (np.inf, 0.0, 0.0)                            # in a joint that no cost would look at
    c["infinity_is_absent"] = case(
        frames([box(0), hot]), 3, [(0, "slot_of", [0, -1]), (0, "uid", [0, -1, -1])], "an infinity makes a slot absent",
        {"people": frames([box(0), box(100)])})
    far, near = box(0), box(4)
    far[3] = (1024.0, 1024.0, 0.0625)                      # the track's low joint: neither in the cost nor in the size
    near[3] = (-512.0, 0.0, 1.0)
    c["low_confidence_left_out"] = case(
        frames([far], [near]), 2, [(1, "slot_of", [0]), (1, "cost", [0.125, np.nan])], "low-confidence joints are left out",
        {"kw": {"pose_thr": 0.03125}}, gate=0.25)
    # a track 1/4 x 1/2 px large: size 1, cost (4 / 8 / 8) / 1 = 1/16 (with its own size 1/2 it would be 1/8 > gate)
    c["small_track_size_one"] = case(
        frames([box(scale=1 / 32)], [box(0.125, scale=1 / 32)]), 2, [(1, "slot_of", [0]), (1, "cost", [0.0625, np.nan])],
        "a track smaller than 1 px has size 1", {"kw": {"gate": 0.0625}}, gate=0.09375)
    moved = box(0)
    moved[0, 0] = 16.0                                     # 7 of the 8 terms are 0: they count, mean 2, cost 1/8
    c["coinciding_coordinates_count"] = case(
        frames([box(0)], [moved]), 2, [(1, "slot_of", [0]), (1, "cost", [0.125, np.nan])], "a term equal to 0 counts",
        {"kw": {"gate": 0.125}}, gate=0.25)
    c["empty_frame"] = case(
        frames([box(0), box(100)], []), 3, [(1, "slot_of", [-1, -1]), (1, "flags", [A, A, 0]), (1, "person_of", [-1, -1, -1])],
        "an empty frame", {"people": frames([box(0), box(100)], [box(0)])})
    c["ids_not_reused_after_reset"] = case(
        frames([box(0), box(100)], [box(0), box(100)]), 2, [(1, "uid", [2, 3]), (1, "flags", [A | Pn | B | Fr] * 2)],
        "ids are never reused after reset", {"resets": {}}, resets={1: None})
    one = np.array([[[[[5.0, 7.0, 1.0]]]], [[[[5.5, 7.0, 1.0]]]], [[[[9.0, 7.0, 1.0]]]]], np.float32)      # P = T = Jo = 1
    c["caps_one"] = case(one, 1, [(1, "slot_of", [0]), (1, "cost", [0.25]), (2, "slot_of", [-2]), (2, "flags", [A])],
                         "the smallest shapes", {"kw": {"gate": 0.25}}, gate=0.5, min_common=1)
    return c


def walkers(seed=7, n=5, J=19, F=120, P=8, miss=0.1, jitter=2.0, S=1):
    """n people walking side by side, each a fixed 40 x 100 px shape: (people [F, S, P, J, 3], truth int [F, S, P] = who is in
    list slot p, -1 nobody).  The list order is shuffled every frame, a detection is missed with probability `miss`."""
    rng = np.random.default_rng(seed)
    people = np.full((F, S, P, J, 3), np.nan, np.float32)
    truth = np.full((F, S, P), -1, np.int64)
    for s in range(S):
        shape = rng.uniform(0, 1, (n, J, 2)) * np.array([40.0, 100.0])
        x0 = 200.0 * rng.permutation(n) + rng.uniform(-20, 20, n)
        vx, phase = rng.uniform(0.5, 1.5, n), rng.uniform(0, 6.28, n)
        for f in range(F):
            order = rng.permutation(P)
            for i in range(n):
                if rng.uniform() < miss and f > 0:
                    continue
                centre = np.array([x0[i] + vx[i] * f, 50.0 + 10.0 * np.sin(0.1 * f + phase[i])])
                pose = np.empty((J, 3))
                pose[:, :2] = centre + shape[i] + rng.normal(0, jitter, (J, 2))
                pose[:, 2] = np.where(rng.uniform(0, 1, J) < 0.05, 0.05, rng.uniform(0.3, 1.0, J))
                people[f, s, order[i]] = pose.astype(np.float32)
                truth[f, s, order[i]] = i
    return people, truth


def caps(seed=11):
    """P = T = Jo = 64: frame 0 fills every slot; in frame 1 the people come back in another order with 3 px of jitter, five
    of them missing and five strangers in their list slots, for whom no slot is free."""
    rng = np.random.default_rng(seed)
    shape = rng.uniform(0, 1, (64, 64, 2)) * np.array([40.0, 100.0])
    grid = np.stack([160.0 * (np.arange(64) % 8), 240.0 * (np.arange(64) // 8)], 1)
    conf = np.where(rng.uniform(0, 1, (2, 64, 64)) < 0.1, 0.05, rng.uniform(0.2, 1.0, (2, 64, 64)))
    people = np.empty((2, 1, 64, 64, 3), np.float32)
    people[0, 0, :, :, :2] = grid[:, None] + shape
    order = rng.permutation(64)
    people[1, 0, :, :, :2] = (grid[:, None] + shape + rng.normal(0, 3.0, (64, 64, 2)))[order]
    people[:, 0, :, :, 2] = conf
    strangers = rng.choice(64, 5, replace=False)
    people[1, 0, strangers, :, :2] += 5000.0
    return people, order, strangers


def cases():
    c = hand_cases()
    people, _ = walkers()
    c["walkers"] = case(people, 8, [], None, None)
    people, _ = walkers(seed=21, F=12, S=5, P=6)
    c["streams"] = case(people, 6, [], None, None, max_missed=1)
    people, _, _ = caps()
    c["caps"] = case(people, 64, [(1, "dropped", 5)], None, None)
    return c


def drive(c, call, reset, chunk=None):
    """Feeds the case's frames to call(people [f, S, P, Jo, 3]) -> {output: array [f, S, ...]} in pieces that end at every
    reset and after at most `chunk` frames (None: as many as possible), with reset(mask) before the frames that ask for it.
    Returns the outputs of all frames, concatenated."""
    F = c["people"].shape[0]
    cuts = sorted(set([0, F] + [f for f in c["resets"] if 0 < f < F] + (list(range(0, F, chunk)) if chunk else [])))
    parts = []
    for f0, f1 in zip(cuts[:-1], cuts[1:]):
        if f0 in c["resets"]:
            reset(c["resets"][f0])
        parts.append(call(c["people"][f0:f1]))
    return {k: np.concatenate([p[k] for p in parts]) for k in track_ref.OUTPUTS}


def run_ref(c, chunk=None, pairs=None):
    """The yardstick on a case: (outputs [F, S, ...], the state after the last frame)."""
    S, Jo = c["people"].shape[1], c["people"].shape[3]
    st = track_ref.new_state(S, c["slots"], Jo)
    out = drive(c, lambda x: track_ref.track(x, st, pairs=pairs, **c["kw"]), lambda m: track_ref.reset(st, m), chunk)
    return out, st
