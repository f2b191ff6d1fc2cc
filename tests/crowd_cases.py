"""Cases of the crowd filter (p2m_crowd_select) and the person colours, shared by tests/test_crowd_cpu.py (the yardstick's own
tests, no GPU) and tests/test_gpu_crowd.py (the kernels against the yardstick).

A case is a dict: dets float32 [B, P, J, 3], num (int32 [B] or None), kw (CrowdFilter's arguments), expect ({output: values of
image 0}, what the rules of the issue give by hand) and rule: the flip of crowd_ref that must change the outcome, i.e. the
rule that decides the case (None for the companion of an edge, whose expectation alone pins it).

Coordinates of the hand-made cases are integers (or dyadic fractions), so every sum of the duplicate test is exact in any
order; their people are `person()`: joint j at (x0 + 10 j, y0 + 7 j).  A shift in x alone leaves every y term exactly 0, and
those leave the mean: the mean of a pure x shift s over any co-valid set is |s|.
"""
import functools

import numpy as np

F = np.float32
NEXT_BELOW = lambda v: np.nextafter(F(v), F(0))                                        # noqa: E731


def person(J=17, x0=100.0, y0=100.0, conf=0.875, dx=0.0, dy=0.0):
    p = np.zeros((J, 3), F)
    p[:, 0] = x0 + 10.0 * np.arange(J) + dx
    p[:, 1] = y0 + 7.0 * np.arange(J) + dy
    p[:, 2] = conf
    return p


def image(*people):
    return np.stack(people)[None].astype(F)


def case(dets, rule, expect=None, num=None, **kw):
    return dict(dets=np.ascontiguousarray(dets, F), num=None if num is None else np.asarray(num, np.int32), kw=kw, rule=rule,
                expect=expect or {})


def _spaced(n, step, J=17):
    return [person(J, dx=step * k) for k in range(n)]


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    A = person()
    # ---- greedy order
    c["greedy_chain"] = case(image(A, person(dx=15), person(dx=30)), "greedy",
                             dict(reason=[0, 2, 0], dup_of=[-1, 0, -1], count=2, index=[0, 2, -1]))
    low = person(dx=15, conf=0.0)
    low[:4, 2] = 0.3                                      # four valid joints, score 1.2: valid enough to match, too low to stay
    c["greedy_low_score"] = case(image(A, low, person(dx=30)), "low", dict(reason=[0, 1, 0], dup_of=[-1, -1, -1], count=2))
    c["dup_of_lowest"] = case(image(A, person(dx=30), person(dx=15)), "lowest", dict(reason=[0, 0, 2], dup_of=[-1, -1, 0]))
    # ---- the mean
    # x shifted by 30, y equal: over all co-valid terms the mean is 15, over the non-zero ones 30
    c["zeros_leave_the_mean"] = case(image(A, person(dx=30)), "zeros", dict(reason=[0, 0]))
    top, bottom = person(), person(dx=500, dy=300)
    top[9:, 2], bottom[:9, 2] = 0.0625, 0.0625            # valid: joints 0-8 + neck / joints 9-16 + pelvis: nothing in common
    c["no_covalid_joint"] = case(image(top, bottom), "empty", dict(reason=[0, 2], dup_of=[-1, 0]))
    c["identical"] = case(image(A, A.copy()), "empty", dict(reason=[0, 2], dup_of=[-1, 0]))
    # ---- exact edges
    c["mean_equals_min_diff"] = case(image(A, person(dx=20)), "strict_mean", dict(reason=[0, 0]))
    near = person(dx=20)
    near[3, 0] -= 1.0                                     # 19 terms: 18 x 20 + 19 = 379, mean 19.947..
    c["mean_one_unit_below"] = case(image(A, near), None, dict(reason=[0, 2], dup_of=[-1, 0]))
    s = person(conf=0.0)
    s[:3, 2] = 0.5                                        # 0.5 + 0.5 + 0.5 = 1.5 exactly; hips and shoulders 0: midpoints 0
    c["score_equals_thr"] = case(image(s), "strict_score", dict(reason=[0], score=[1.5]))
    s2 = s.copy()
    s2[2, 2] = NEXT_BELOW(0.5)
    c["score_next_below"] = case(image(s2), None, dict(reason=[1]))
    # validity at the threshold: joint 0 sits 500 px off, joint 1 15 px; with joint 0 valid the mean is 257.5, without it 15
    v = person(dx=15, conf=0.09375)                       # 3/32 < 0.1: invalid, but 15 x 3/32 + 0.875 + 0.1 >= 1.5
    v[0, 0] += 485.0
    v[1, 2] = 0.875
    v[0, 2] = F(0.1)                                      # float32(0.1) = 0.100000001490116.. > the double 0.1: valid
    c["valid_float32_tenth"] = case(image(A, v), "thr32", dict(reason=[0, 0]))
    v2 = v.copy()
    v2[0, 2] = NEXT_BELOW(0.1)
    c["valid_next_below"] = case(image(A, v2), None, dict(reason=[0, 2], dup_of=[-1, 0]))
    # the neck's confidence is the product: 0.3 x 0.3 = 0.09 is invalid although both shoulders are valid.  Left shoulder 24 px
    # off, right shoulder equal: without the neck the mean is 24, with it (24 + 12) / 2 = 18
    m = person(conf=0.09375)
    m[5, 2] = m[6, 2] = 0.3
    m[5, 0] += 24.0
    c["midpoint_conf_is_the_product"] = case(image(A, m), "conf_mean", dict(reason=[0, 0]))
    # ---- shapes
    c["one_slot"] = case(image(A), None, dict(reason=[0], count=1, index=[0]))
    c["p64_all_accepted"] = case(image(*_spaced(64, 30)), None, dict(reason=[0] * 64, count=64, index=list(range(64))))
    last = _spaced(64, 30)
    last[63] = person(dx=30 * 62 + 15)                    # matches slot 62 alone: bit 62 of its mask, bit 63 of the accepted set
    c["p64_last_duplicates_62"] = case(image(*last), None,
                                       dict(reason=[0] * 63 + [2], dup_of=[-1] * 63 + [62], count=63))
    c["p64_all_duplicates_of_0"] = case(image(*[person(dx=0.25 * k) for k in range(64)]), None,
                                        dict(reason=[0] + [2] * 63, dup_of=[-1] + [0] * 63, count=1))
    two = np.concatenate([image(A, person(dx=15), person(dx=30)), image(A, person(dx=15), person(dx=30))])
    c["num_zero"] = case(two, None, dict(reason=[-1, -1, -1], count=0, index=[-1, -1, -1]), num=[0, 3])
    g = np.concatenate([image(A, person(dx=15), person(dx=30), person(dx=15)), image(A, person(dx=40), person(dx=80), A)])
    g[0, 2:] = np.nan                                     # garbage in the unread slots: NaN, infinity, huge
    g[1, 3, :, 0], g[1, 3, :, 1], g[1, 3, :, 2] = np.inf, -3e38, 7.0
    c["num_below_p_with_garbage"] = case(g, None, dict(reason=[0, 2, -1, -1], count=1), num=[2, 3])
    c["j21_no_midpoints"] = case(image(person(21), person(21, dx=15), person(21, dx=30)), "greedy",
                                 dict(reason=[0, 2, 0]), midpoints=())
    c["j62_two_midpoints"] = case(image(person(62), person(62, dx=15), person(62, dx=30)), "greedy",
                                  dict(reason=[0, 2, 0]), midpoints=((60, 61), (0, 1)))
    far = [person(x0=-700.0, y0=-300.0), person(x0=-700.0, y0=-300.0, dx=15), person(x0=1e5, y0=-1e5),
           person(x0=1e5, y0=-1e5, dx=20), person(x0=1e5, y0=-1e5, dx=39)]
    c["negative_and_1e5_coordinates"] = case(image(*far), "strict_mean", dict(reason=[0, 2, 0, 0, 2], dup_of=[-1, 0, -1, -1, 3]))
    nan_p, inf_p = person(dx=5), person(dx=10)
    nan_p[7, 1], inf_p[16, 2] = np.nan, np.inf
    c["non_finite_between_duplicates"] = case(image(A, nan_p, inf_p, person(dx=15)), "nonfinite",
                                              dict(reason=[0, 3, 3, 2], dup_of=[-1, -1, -1, 0], count=1))
    c["random_crowds"] = case(random_crowds(2024), "greedy")
    return c


def random_crowds(seed, B=8, P=32, J=17, n_proto=10):
    """People drawn as jittered copies of a few prototypes, so that roughly half are duplicates of an earlier one (a prototype per 3.2 slots); a few with
    low confidences, and joints below the validity threshold throughout."""
    rng = np.random.default_rng(seed)
    dets = np.zeros((B, P, J, 3), F)
    for b in range(B):
        centre = rng.uniform([100, 100], [1800, 900], (n_proto, 1, 2))
        proto = centre + rng.normal(0, 60, (n_proto, J, 2))
        who = rng.integers(0, n_proto, P)
        sigma = rng.choice([3.0, 8.0, 16.0, 24.0], (P, 1, 1))          # from certain duplicates to pairs around min_diff
        dets[b, :, :, :2] = proto[who] + rng.normal(0, 1, (P, J, 2)) * sigma
        conf = rng.uniform(0, 1, (P, J))
        conf[rng.uniform(size=(P, J)) < 0.15] *= 0.1
        conf[rng.uniform(size=P) < 0.1] *= 0.08
        dets[b, :, :, 2] = conf
    return dets


def band_violations(pairs, scores, score_thr=1.5, min_diff=20.0):
    """The comparisons and scores that a different summation order of a float64 sum could decide otherwise."""
    bad = [p for p in pairs if p[3] and abs(p[4] - min_diff) <= 1e-9 * max(1.0, p[4])]
    s = np.asarray(scores, np.float64).reshape(-1)
    s = s[np.isfinite(s)]
    return bad, s[np.abs(s - score_thr) <= 1e-12]


# ---- colours
COLOUR_RUNS = [(n, seed, first) for n in (1, 7, 256) for seed, first in ((123, 0), (0x9E3779B97F4A7C15, 1_000_003))]
# s, v with a channel c for which 255 c is a tie: the defaults (p = 0.5: 127.5 -> 128), (0.5, 0.5) (v: 127.5; p: 63.75 -> 64),
# (0, 0.5) (grey: 127.5 three times), (0.9, 0.5) (p = 0.05 rounded: 12.75 -> 13, no tie; v: 127.5)
TIE_SV = ((0.5, 1.0), (0.5, 0.5), (0.0, 0.5), (0.9, 0.5))


def edge_hues():
    """Hues on the 2^-24 grid at and next to the six sector edges k / 6, and the ends of [0, 1)."""
    u = 2.0 ** -24
    h = [0.0, 1.0 - u]
    for k in range(1, 6):
        g = np.floor(k / 6.0 / u)
        h += [(g - 1) * u, g * u, (g + 1) * u, (g + 2) * u]
    return np.array(h)
