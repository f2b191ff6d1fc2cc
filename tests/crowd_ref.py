"""numpy restatement, float64, of the head of the reference's crowd demo (demo/run.py): add_pelvis / add_neck (:127-146), the
score filter and the greedy suppression of duplicate detections (:281-306), the colour per person (:314) - the yardstick of
csrc/crowd.hip (include/p2m.h, "The crowd demo's front end").  Where an operation decides an outcome it is the reference's own
numpy / Python operation: the float32 validity masks multiplied in, boolean indexing with != 0, .mean(), Python's sum.  What
the reference does not have is marked `ours`: the non-finite rule, dup_of, the compaction, num.

`flip` names ONE rule to turn around (None: the definition).  tests/test_crowd_cpu.py uses it to show that a case is decided by
the rule it is named after:
  "greedy"     compare with every EARLIER slot that passed the score filter, accepted or not (the naive parallel form)
  "low"        a low-score person still enters the list of people compared against
  "lowest"     dup_of is the highest matching accepted slot
  "zeros"      zero terms stay in the mean's denominator
  "empty"      an empty term set is not a duplicate
  "strict_mean", "strict_score", "strict_valid"    <= / <= / >= in place of < / < / >
  "thr32"      the validity threshold is rounded to float32 first (what an fp32 comparison would do)
  "conf_mean"  a midpoint's confidence is the mean of the two, not the product
  "nonfinite"  a non-finite person is treated like any other (the reference's behaviour)
"""
import colorsys

import numpy as np

import sample_ref

ST_PERSON_COLOUR = 11
REASON_ACCEPTED, REASON_LOW_SCORE, REASON_DUPLICATE, REASON_NON_FINITE, REASON_UNUSED = 0, 1, 2, 3, -1
COCO_MIDPOINTS = ((11, 12), (5, 6))


def add_midpoint(joint_coord, a, b, flip=None):
    """add_pelvis / add_neck (run.py:127-146) for the joint pair (a, b)."""
    mid = (joint_coord[a, :] + joint_coord[b, :]) * 0.5
    mid[2] = joint_coord[a, 2] * joint_coord[b, 2] if flip != "conf_mean" else (joint_coord[a, 2] + joint_coord[b, 2]) * 0.5
    return np.concatenate((joint_coord, mid.reshape(1, 3)))


def valid_mask(conf, pose_thr, flip=None):
    """run.py:287 / :297: (conf.reshape(-1, 1) > pose_thr).astype(np.float32)."""
    conf = conf.copy().reshape(-1, 1)
    if flip == "strict_valid":
        return (conf >= pose_thr).astype(np.float32)
    if flip == "thr32":
        return (conf > np.float32(pose_thr)).astype(np.float32)
    return (conf > pose_thr).astype(np.float32)


def pair_mean(a, b, va, vb, flip=None):
    """run.py:297-299: (number of terms, their mean or None) of a candidate against a drawn person."""
    diff = np.abs(a[:, :2] - b[:, :2]) * va * vb
    if flip != "zeros":
        diff = diff[diff != 0]
    else:                                             # every term of a co-valid joint counts, coinciding coordinates included
        diff = diff[np.broadcast_to(va * vb != 0, diff.shape)]
    return diff.size, (diff.mean() if diff.size else None)


def select_image(dets, midpoints=COCO_MIDPOINTS, pose_thr=0.1, score_thr=1.5, min_diff=20.0, flip=None, pairs=None):
    """One image: dets [n, J, 3] float32, the filled slots only.  Returns reason [n], dup_of [n], score [n] and the list of
    accepted people (float64 [Jo, 3] each).  pairs: a list that receives (i, d, count, mean) of every comparison made."""
    n = len(dets)
    reason, dup_of, score = np.full(n, REASON_UNUSED, np.int8), np.full(n, -1, np.int32), np.full(n, np.nan)
    drawn, drawn_idx, accepted = [], [], []
    with np.errstate(all="ignore"):
        for idx in range(n):
            raw = np.asarray(dets[idx], np.float32)
            if flip != "nonfinite" and not np.isfinite(raw).all():                      # ours
                reason[idx] = REASON_NON_FINITE
                continue
            joint_img = raw.astype(np.float64)                                          # (the json's numbers are doubles)
            for a, b in midpoints:
                joint_img = add_midpoint(joint_img, a, b, flip)
            valid = valid_mask(joint_img[:, 2], pose_thr, flip)
            det_score = sum(joint_img[:, 2])
            score[idx] = det_score
            low = det_score <= score_thr if flip == "strict_score" else det_score < score_thr
            if low:
                reason[idx] = REASON_LOW_SCORE
                if flip == "low":
                    drawn.append(joint_img), drawn_idx.append(idx)
                continue
            hits = []
            for ddx in range(len(drawn)):
                other = drawn[ddx]
                other_val = valid_mask(other[:, 2], pose_thr, flip)
                size, mean = pair_mean(joint_img, other, valid, other_val, flip)
                if pairs is not None:
                    pairs.append((idx, drawn_idx[ddx], size, mean))
                if size == 0:
                    if flip != "empty":
                        hits.append(drawn_idx[ddx])
                elif (mean <= min_diff if flip == "strict_mean" else mean < min_diff):
                    hits.append(drawn_idx[ddx])
            if hits:
                reason[idx] = REASON_DUPLICATE
                dup_of[idx] = max(hits) if flip == "lowest" else min(hits)              # ours
                if flip == "greedy":
                    drawn.append(joint_img), drawn_idx.append(idx)
                continue
            reason[idx] = REASON_ACCEPTED
            drawn.append(joint_img), drawn_idx.append(idx)
            accepted.append((idx, joint_img))
    return reason, dup_of, score, accepted


def select(dets, num=None, midpoints=COCO_MIDPOINTS, pose_thr=0.1, score_thr=1.5, min_diff=20.0, flip=None, pairs=None):
    """The batch: dets float32 [B, P, J, 3], num [B] or None.  Returns the dict of p2m_crowd_select's outputs (ours: the
    compaction, NaN in the slots that hold nobody, -1 for the unused)."""
    dets = np.asarray(dets, np.float32)
    B, P, J, _ = dets.shape
    Jo = J + len(midpoints)
    out = dict(joints=np.full((B, P, Jo, 3), np.nan, np.float32), count=np.zeros(B, np.int32), index=np.full((B, P), -1, np.int32),
               reason=np.full((B, P), REASON_UNUSED, np.int8), dup_of=np.full((B, P), -1, np.int32), score=np.full((B, P), np.nan),
               keep=np.zeros((B, P), bool))
    for b in range(B):
        n = P if num is None else int(np.clip(num[b], 0, P))
        img_pairs = None if pairs is None else []
        r, d, s, acc = select_image(dets[b, :n], midpoints, pose_thr, score_thr, min_diff, flip, img_pairs)
        if pairs is not None:
            pairs.extend((b,) + p for p in img_pairs)
        out["reason"][b, :n], out["dup_of"][b, :n], out["score"][b, :n] = r, d, s
        out["count"][b] = len(acc)
        for k, (idx, joint_img) in enumerate(acc):
            out["index"][b, k] = idx
            out["joints"][b, k] = joint_img.astype(np.float32)                          # rounded once
    out["keep"] = out["reason"] == REASON_ACCEPTED
    return out


def hues(seed, first_index, n):
    """Stage 11 of the Philox stream: joint 0, block 0, word 0 of the global indices first_index .. first_index + n - 1."""
    idx = (np.uint64(first_index) + np.arange(n, dtype=np.uint64))
    w = sample_ref._words(seed, idx, 0, ST_PERSON_COLOUR, [0])
    return sample_ref.uniforms(w[0][:, 0])


def colours_of(h, s=0.5, v=1.0):
    """rgb float32 [n, 3] and u8 [n, 3] from hues: the standard library's colorsys, then one rounding each."""
    rgb64 = np.array([colorsys.hsv_to_rgb(float(x), float(s), float(v)) for x in h], np.float64).reshape(-1, 3)
    return rgb64.astype(np.float32), np.rint(255.0 * rgb64).astype(np.uint8), rgb64


def colours(seed, first_index, n, s=0.5, v=1.0):
    rgb, u8, _ = colours_of(hues(seed, first_index, n), s, v)
    return rgb, u8
