"""The yardstick of p2m_pose_track: include/p2m.h "Tracking people across frames" restated in numpy, float64, one operation at
a time in the order the header gives.  The cost sum is an explicit sequential loop (np.sum adds pairwise, in another order).
Every operation is a correctly rounded IEEE operation in a fixed order, so the device is compared with this EXACTLY: integers
equal, floats bit for bit, NaN equal to NaN."""
import numpy as np

DEFAULTS = dict(pose_thr=0.1, gate=0.3, min_common=3, max_missed=10)
OUTPUTS = ("joints", "slot_of", "person_of", "uid", "flags", "cost", "dropped")
STATE = ("pose", "uid", "missed", "next_uid")
ALIVE, PRESENT, BORN, FRESH, RETIRED = 1, 2, 4, 8, 16


def new_state(S, T, Jo):
    return {"pose": np.zeros((S, T, Jo, 3), np.float32), "uid": np.full((S, T), -1, np.int32),
            "missed": np.zeros((S, T), np.int32), "next_uid": np.zeros((S,), np.int32)}


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def reset(st, mask=None):
    """PoseTracker.reset: frees the slots (of the streams where mask is set); next_uid goes on counting."""
    sel = slice(None) if mask is None else np.asarray(mask, bool)
    st["uid"][sel] = -1
    st["missed"][sel] = 0


def pair_cost(person, track, pose_thr, min_common):
    """(cost, n) of one present person [Jo, 3] against one alive track's stored pose [Jo, 3]; cost None: no candidate."""
    thr = np.float64(pose_thr)
    p, t = person.astype(np.float64), track.astype(np.float64)            # exact
    vp, vt = p[:, 2] > thr, t[:, 2] > thr
    S, n = np.float64(0.0), 0
    for j in range(p.shape[0]):
        if vp[j] and vt[j]:
            S = S + abs(p[j, 0] - t[j, 0])
            S = S + abs(p[j, 1] - t[j, 1])
            n += 2
    if n < 2 * min_common:
        return None, n
    size = np.float64(1.0)
    if vt.any():
        w, h = t[vt, 0].max() - t[vt, 0].min(), t[vt, 1].max() - t[vt, 1].min()
        size = w if w > h else h
        if not size >= 1.0:
            size = np.float64(1.0)
    return (S / np.float64(n)) / size, n


def step(frame, pose, uid, missed, next_uid, T, pose_thr, gate, min_common, max_missed, pairs=None):
    """One frame [P, Jo, 3] of one stream; the state arrays of that stream are updated in place.  Returns the frame's outputs
    and the new next_uid."""
    P, Jo = frame.shape[0], frame.shape[1]
    present = [bool(np.isfinite(frame[p]).all()) for p in range(P)]
    alive = [int(uid[t]) >= 0 for t in range(T)]
    cand = []
    for t in range(T):
        for p in range(P):
            if present[p] and alive[t]:
                c, n = pair_cost(frame[p], pose[t], pose_thr, min_common)
                if pairs is not None:
                    pairs.append((p, t, c, n))
                if c is not None and c < np.float64(gate):
                    cand.append((c, t, p))
    slot_of = np.full(P, -1, np.int32)
    person_of = np.full(T, -1, np.int32)
    cost = np.full(T, np.nan, np.float64)
    cand.sort()                                            # (cost, t, p) ascending: the ties as the header breaks them
    for c, t, p in cand:
        if slot_of[p] < 0 and person_of[t] < 0:
            slot_of[p], person_of[t], cost[t] = t, p, c
    free = [t for t in range(T) if not alive[t]]
    born = np.zeros(T, bool)
    dropped = 0
    for p in range(P):
        if present[p] and slot_of[p] < 0:
            if free:
                t = free.pop(0)
                slot_of[p], person_of[t], born[t] = t, p, True
                uid[t] = next_uid
                next_uid += 1
            else:
                slot_of[p] = -2
                dropped += 1
    joints = np.full((T, Jo, 3), np.nan, np.float32)
    flags = np.zeros(T, np.uint8)
    for t in range(T):
        if person_of[t] >= 0:
            joints[t] = frame[person_of[t]]
            pose[t] = frame[person_of[t]]
            flags[t] = ALIVE | PRESENT | (BORN if born[t] else 0) | (FRESH if born[t] or missed[t] > 0 else 0)
            missed[t] = 0
        elif alive[t]:
            missed[t] += 1
            if missed[t] > max_missed:
                uid[t] = -1
                flags[t] = RETIRED
            else:
                flags[t] = ALIVE
    out = {"joints": joints, "slot_of": slot_of, "person_of": person_of, "uid": uid.copy(), "flags": flags, "cost": cost,
           "dropped": np.int32(dropped)}
    return out, next_uid


def track(people, state, pose_thr=0.1, gate=0.3, min_common=3, max_missed=10, pairs=None):
    """people fp32 [F, S, P, Jo, 3]; state: new_state()'s dict, updated in place.  Returns the outputs [F, S, ...]."""
    people = np.asarray(people, np.float32)
    F, S, P, Jo = people.shape[:4]
    T = state["uid"].shape[1]
    out = {"joints": np.empty((F, S, T, Jo, 3), np.float32), "slot_of": np.empty((F, S, P), np.int32),
           "person_of": np.empty((F, S, T), np.int32), "uid": np.empty((F, S, T), np.int32),
           "flags": np.empty((F, S, T), np.uint8), "cost": np.empty((F, S, T), np.float64), "dropped": np.empty((F, S), np.int32)}
    for s in range(S):
        nu = int(state["next_uid"][s])
        for f in range(F):
            o, nu = step(people[f, s], state["pose"][s], state["uid"][s], state["missed"][s], nu, T, pose_thr, gate,
                         min_common, max_missed, pairs)
            for k in OUTPUTS:
                out[k][f, s] = o[k]
        state["next_uid"][s] = nu
    return out
