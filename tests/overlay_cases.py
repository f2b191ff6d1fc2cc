"""The case table of the 2D pose overlay, seeded: the smallest shapes at which csrc/overlay.hip can still go wrong (32 x 32-pixel
tiles, 4 pixels per lane, 256-record scan chunks).  case(name) -> the dict tests/overlay_ref.py takes; reference(name) -> its
yardstick result, computed once and shared; plan(c) -> what the kernels' plan makes of a case (slots, chunks, the fullest
compaction, tiles met), restated here so that test_overlay_cpu.py can assert that every case reaches what it is named for.
Each case also carries `expect`, the named property as data."""
import functools

import numpy as np

import overlay_ref as orf

TILE, CHUNK = 32, 256
NAN, INF = float("nan"), float("inf")


def _src(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def _case(poses, bones, H, W, seed, colours=None, colour_mode=0, boxes=None, thr=0.4, line_h2=2, mark_h2=6, mark_r16=-1,
          box_h2=1, alpha256=256, box_rgb=(255, 255, 0), expect=None):
    poses = np.ascontiguousarray(poses, np.float32)
    assert poses.ndim == 4
    B, P = poses.shape[:2]
    bones = np.ascontiguousarray(np.asarray(bones, np.int32).reshape(-1, 2))
    L = bones.shape[0]
    rng = np.random.default_rng(seed + 1000)
    if colours is None:
        colours = rng.integers(0, 256, (L, 3) if colour_mode == 0 else (B, P, 3), dtype=np.uint8)
    return dict(poses=poses, bones=bones, colours=np.ascontiguousarray(colours, np.uint8), colour_mode=colour_mode,
                boxes=None if boxes is None else np.ascontiguousarray(boxes, np.float32), box_rgb=tuple(box_rgb),
                src=_src(B, H, W, seed), H=H, W=W, thr=thr, line_h2=line_h2, mark_h2=mark_h2, mark_r16=mark_r16, box_h2=box_h2,
                alpha256=alpha256, expect=expect or {})


def _conf(xy, conf=1.0):
    xy = np.asarray(xy, np.float32)
    return np.concatenate([xy, np.full(xy.shape[:-1] + (1,), conf, np.float32)], -1)


def _random_people(B, P, J, H, W, seed, C=3, margin=8.0):
    rng = np.random.default_rng(seed)
    xy = rng.uniform([-margin, -margin], [W + margin, H + margin], (B, P, J, 2))
    return _conf(xy, 1.0) if C == 3 else xy.astype(np.float32)


def _boxes_around(poses, pad=3.0):
    xy = poses[..., :2]
    lo, hi = xy.min(2) - pad, xy.max(2) + pad
    return np.stack([np.stack([lo[..., 0], lo[..., 1]], -1), np.stack([hi[..., 0], lo[..., 1]], -1),
                     np.stack([hi[..., 0], hi[..., 1]], -1), np.stack([lo[..., 0], hi[..., 1]], -1)], 2).astype(np.float32)


CHAIN = lambda n: [[i, i + 1] for i in range(n - 1)]                               # noqa: E731
COCO19 = [[1, 2], [0, 1], [0, 2], [2, 4], [1, 3], [6, 8], [8, 10], [5, 7], [7, 9], [12, 14], [14, 16], [11, 13], [13, 15],
          [5, 6], [11, 12], [5, 11], [6, 12], [3, 5], [4, 6]]                      # 17 joints, 19 bones


def _geometry(H, W, seed):
    """Lines through tile borders and the tile corner (32, 32): 45 degrees, horizontal, vertical, and a zero-length bone."""
    pts = [(2.7, 3.2), (60.9, 61.1), (1.0, 31.0), (W - 1.0, 31.0), (32.0, 0.0), (32.0, H - 1.0), (10.5, 50.5), (31.0, 33.0),
           (33.9, 30.2)]
    bones = [[0, 1], [2, 3], [4, 5], [6, 6], [7, 8]]
    return _case(_conf(pts)[None, None], bones, H, W, seed, expect=dict(status=[[0]], zero_length=3, all_drawn=True))


def _build(name):
    if name == "one_pixel":
        return _case(np.array([[[[0.9, 0.2], [0.0, 0.99]]]]), [[0, 1]], 1, 1, 1, expect=dict(status=[[0]], all_drawn=True))
    if name == "geometry_63x65":
        return _geometry(63, 65, 2)
    if name == "geometry_65x63":
        return _geometry(65, 63, 3)
    if name == "far_ends_130x70":
        # both endpoints off the image on opposite sides, endpoints at +-16383, two people crossing (the later one wins at
        # the crossing pixel (35, 65)), rings with a hole (vis_coco_skeleton's numbers), one colour per person
        p0 = [(-50.0, 20.0), (120.0, 110.0), (-16383.0, -16313.0), (16383.0, 16453.0 - 70.0), (5.0, 65.0), (65.0, 65.0)]
        p1 = [(16383.9, -16383.9), (-16383.2, 16383.5), (35.0, 40.0), (35.0, 100.0), (20.0, 10.0), (50.0, 12.0)]
        col = np.array([[[250, 10, 20], [5, 240, 200]]], np.uint8)
        return _case(np.array([[p0, p1]]), [[0, 1], [2, 3], [4, 5]], 130, 70, 4, colours=col, colour_mode=1, mark_h2=3,
                     mark_r16=32, expect=dict(status=[[0, 0]], all_drawn=True, wins=(0, 65, 35, (5, 240, 200))))
    if name == "unusable":
        # 16384, NaN and +-inf are unusable (status bit 0, invisible); -16383.99 and 16383.5 are usable
        bad = [(16384.0, 10.0), (10.0, NAN), (INF, 5.0), (7.0, -INF), (-16384.0, 3.0), (-16383.99, 20.0), (16383.5, 25.0),
               (20.0, 20.0)]
        good = [(3.0 + 4 * i, 30.0 - 3 * i) for i in range(8)]
        return _case(_conf([bad, good])[None], [[0, 7], [1, 7], [2, 7], [3, 7], [4, 7], [5, 7], [6, 7]], 40, 45, 5,
                     expect=dict(status=[[1, 0]], hidden_joints=(0, 0, [0, 1, 2, 3, 4])))
    if name == "revisit":
        pts = [(20.0, 20.0), (5.0, 5.0), (38.0, 8.0), (22.0, 37.0)]
        return _case(_conf(pts)[None, None], [[0, 1], [0, 2], [0, 3], [1, 0], [2, 2]], 41, 43, 6,
                     expect=dict(status=[[0]], all_drawn=True))
    if name == "two_chunks":
        # 5 x (3 x 19 + 4) = 305 slots in one image: the scan's second pass runs
        poses = _random_people(1, 5, 17, 70, 131, 7)
        return _case(poses, COCO19, 70, 131, 7, boxes=_boxes_around(poses), expect=dict(min_chunks=2, status=[[0] * 5]))
    if name == "full_chunk":
        # one tile, every slot of the first chunk meets it: the compaction is full
        poses = _random_people(1, 5, 17, 32, 32, 8, margin=-2.0)
        return _case(poses, COCO19, 32, 32, 8, boxes=_boxes_around(poses, 0.5), line_h2=0, mark_h2=2,
                     expect=dict(min_chunks=2, full_chunk=True, status=[[0] * 5]))
    if name == "invisible":
        # image 0: person 1 has every joint under the threshold; image 1: nothing visible at all
        poses = _random_people(2, 3, 6, 37, 67, 9)
        poses[0, 1, :, 2] = 0.1
        poses[1, :, :, 2] = 0.3
        return _case(poses, CHAIN(6), 37, 67, 9, expect=dict(status=[[0] * 3] * 2, empty_people=[(0, 1)], empty_images=[1]))
    if name == "threshold":
        # conf == thr is hidden (strict), a NaN confidence is hidden; bone 0 loses exactly one joint: its line and one mark go
        poses = _conf([(8.0, 8.0), (30.0, 12.0), (20.0, 30.0), (40.0, 30.0)])[None, None]
        poses[0, 0, :, 2] = [0.9, np.float32(0.4), NAN, 0.4000001]
        return _case(poses, [[0, 1], [1, 2], [2, 3], [3, 0]], 36, 47, 10, thr=float(np.float32(0.4)),
                     expect=dict(status=[[0]], drawn_slots=[1, 8, 9, 10, 11]))
    if name == "no_confidence":
        return _case(_random_people(1, 2, 5, 33, 35, 11, C=2), CHAIN(5), 33, 35, 11, thr=2.0,
                     expect=dict(status=[[0, 0]], all_drawn=True))
    if name == "hairline":
        return _case(_random_people(1, 1, 5, 40, 41, 12), CHAIN(5), 40, 41, 12, line_h2=0, mark_h2=0,
                     expect=dict(all_drawn=True))
    if name == "thick_64":
        return _case(_random_people(1, 1, 3, 130, 135, 13, margin=20.0), CHAIN(3), 130, 135, 13, line_h2=64, mark_h2=64,
                     expect=dict(all_drawn=True))
    if name == "round_caps":
        # a thick line with hairline marks: the round caps past both ends (t <= 0, t >= L2) are not painted over
        return _case(_conf([(14.0, 15.0), (38.0, 31.0)])[None, None], [[0, 1]], 48, 53, 21, line_h2=12, mark_h2=0,
                     expect=dict(all_drawn=True, caps=True))
    if name == "ring_160":
        return _case(_conf([(30.0, 30.0), (45.0, 41.0)])[None, None], [[0, 1]], 70, 75, 14, mark_h2=2, mark_r16=160,
                     expect=dict(all_drawn=True, hole=(0, 30, 30)))
    if name == "ring_0":
        return _case(_conf([(10.0, 10.0), (25.0, 21.0)])[None, None], [[0, 1]], 33, 39, 15, mark_h2=5, mark_r16=0,
                     expect=dict(all_drawn=True))
    if name == "boxes_only":
        # L = 0; person 1's box has a NaN corner: skipped as a whole, status bit 1
        poses = _random_people(1, 3, 4, 50, 49, 16)
        boxes = _boxes_around(poses)
        boxes[0, 1, 2, 0] = NAN
        return _case(poses, np.zeros((0, 2), np.int32), 50, 49, 16, boxes=boxes, box_h2=2,
                     expect=dict(status=[[0, 2, 0]], empty_people=[(0, 1)]))
    if name == "bad_box_and_joint":
        poses = _random_people(1, 2, 4, 34, 45, 17)
        poses[0, 0, 3, 0] = 1e9
        boxes = _boxes_around(np.clip(poses, -100, 100))
        boxes[0, 0, 0, 1] = -INF
        return _case(poses, CHAIN(4), 34, 45, 17, boxes=boxes, expect=dict(status=[[3, 0]]))
    if name in ("alpha_128", "alpha_0"):
        c = dict(_build("geometry_63x65"))
        c["alpha256"] = 128 if name == "alpha_128" else 0
        c["expect"] = dict(status=[[0]], unchanged=name == "alpha_0")
        return c
    if name == "one_joint":
        return _case(_conf([(6.0, 4.0)])[None, None], [[0, 0]], 9, 13, 18, expect=dict(status=[[0]], all_drawn=True))
    if name == "people_64":
        return _case(_random_people(1, 64, 3, 40, 50, 19), CHAIN(3), 40, 50, 19, colour_mode=1, mark_h2=3, mark_r16=32,
                     expect=dict(status=[[0] * 64], min_chunks=2))
    if name == "batch_3":
        poses = _random_people(3, 2, 6, 45, 38, 20)
        poses[1, 0, 2, 1] = NAN
        return _case(poses, CHAIN(6), 45, 38, 20, boxes=_boxes_around(np.nan_to_num(poses)), colour_mode=1,
                     expect=dict(status=[[0, 0], [1, 0], [0, 0]]))
    raise KeyError(name)


CASE_NAMES = ["one_pixel", "geometry_63x65", "geometry_65x63", "far_ends_130x70", "unusable", "revisit", "two_chunks",
              "full_chunk", "invisible", "threshold", "no_confidence", "hairline", "thick_64", "round_caps", "ring_160", "ring_0", "boxes_only",
              "bad_box_and_joint", "alpha_128", "alpha_0", "one_joint", "people_64", "batch_3"]


@functools.lru_cache(maxsize=None)
def _cached_case(name):
    return _build(name)


def case(name):
    """A fresh shallow copy: callers may replace entries, the arrays are shared and must be left unchanged."""
    return dict(_cached_case(name))


@functools.lru_cache(maxsize=None)
def reference(name):
    return orf.overlay_case(_cached_case(name))


def plan(c, prims):
    """The kernels' plan for one image, from the primitives in paint order: slots, scan chunks, the most records one (tile, chunk)
    keeps, tiles met / tiles.  The kernel's bbox: inflated by (T - 1) >> 4 with T = 8 h2 + 8 + max(r16, 0), clipped to the image."""
    H, W = c["H"], c["W"]
    tx, ty = -(-W // TILE), -(-H // TILE)
    n = len(prims)
    kept = np.zeros((-(-max(n, 1) // CHUNK), ty, tx), np.int64)
    for s, q in enumerate(prims):
        if not q["drawn"]:
            continue
        r = (8 * q["h2"] + 8 + max(q["r16"], 0) - 1) >> 4
        x0, x1 = max(int(min(q["a"][0], q["b"][0])) - r, 0), min(int(max(q["a"][0], q["b"][0])) + r, W - 1)
        y0, y1 = max(int(min(q["a"][1], q["b"][1])) - r, 0), min(int(max(q["a"][1], q["b"][1])) + r, H - 1)
        if x0 <= x1 and y0 <= y1:
            kept[s // CHUNK, y0 // TILE:y1 // TILE + 1, x0 // TILE:x1 // TILE + 1] += 1
    return dict(slots=n, chunks=-(-n // CHUNK), max_kept=int(kept.max()), tiles=tx * ty, tiles_met=int((kept.sum(0) > 0).sum()))
