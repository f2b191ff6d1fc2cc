"""The yardstick of the 2D pose overlay (csrc/overlay.hip, include/p2m.h: p2m_pose_overlay): the contract in numpy int64.
Snapping, visibility, paint order, the exact integer coverage on the 1/16 grid and the integer blending are restated here from
the header's comment, vectorised per primitive over a generously inflated bbox (one pixel more than the coverage can reach: the
kernel's own, tighter bbox is its business and is checked by the comparison).  isqrt is floor(sqrt(float64)) plus the exact
fix-up, used below 2^53 only; farther pixels are rejected as the contract allows.

A case is a dict: poses fp32 [B, P, J, C], bones int32 [L, 2], colours uint8 ([L, 3] with colour_mode 0, [B, P, 3] with 1), boxes
fp32 [B, P, 4, 2] or None, box_rgb (c0, c1, c2), src uint8 [B, H, W, 3], H, W, thr, line_h2, mark_h2, mark_r16, box_h2, alpha256.
"""
import numpy as np

COORD = 16384
FAR_C = 1 << 26
FAR_X = 1 << 40                      # floor(256 num / den) from which D >= 2^20: no coverage


def snap(v):
    """fp32 coordinates -> ((int)v truncated towards zero as int64, usable)."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        usable = np.isfinite(v) & (np.abs(v) < np.float32(COORD))
    return np.where(usable, np.trunc(np.where(usable, v, 0)), 0).astype(np.int64), usable


def isqrt(x):
    """floor(sqrt(x)) for int64 x in [0, 2^53)."""
    x = np.asarray(x, np.int64)
    assert (x >= 0).all() and (x < (1 << 53)).all()
    d = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    d = d - (d * d > x)
    d = d + ((d + 1) * (d + 1) <= x)
    assert ((d * d <= x) & ((d + 1) * (d + 1) > x)).all()
    return d


def distance16(qx, qy, a, b):
    """D = floor(16 dist(q, segment a - b)) for int64 pixel arrays qx, qy; far pixels get a D of at least 2^20."""
    ax, ay, bx, by = int(a[0]), int(a[1]), int(b[0]), int(b[1])
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    wx, wy = qx - ax, qy - ay
    t = wx * dx + wy * dy
    first = (t <= 0) if L2 else np.ones(t.shape, bool)
    last = ~first & (t >= L2)
    mid = ~first & ~last
    c = wx * dy - wy * dx
    far = mid & (np.abs(c) >= FAR_C)
    c = np.where(far, 0, c)
    num = np.where(first, wx * wx + wy * wy, np.where(last, (qx - bx) ** 2 + (qy - by) ** 2, c * c))
    den = np.where(mid, L2, 1)
    x = (256 * num) // den                                     # exact: 256 num < 2^60
    x = np.where(far, FAR_X, np.minimum(x, FAR_X))
    return isqrt(x)


def coverage(qx, qy, a, b, h2, r16):
    """cov in sixteenths, 0 .. 16."""
    D = distance16(qx, qy, a, b)
    if r16 >= 0:
        D = np.abs(D - r16)
    return np.clip(8 * h2 + 8 - D, 0, 16)


def primitives(c, b):
    """(list of primitives of image b in paint order, status [P]).  A primitive: dict(a, b, h2, r16, colour, kind, p, l, drawn)."""
    poses = np.asarray(c["poses"], np.float32)[b]
    P, J, C = poses.shape
    bones = np.asarray(c["bones"], np.int64).reshape(-1, 2)
    status = np.zeros(P, np.int32)
    out = []
    for p in range(P):
        xy, ok = snap(poses[p, :, :2])
        usable = ok.all(1)
        vis = usable.copy()
        if C == 3:
            with np.errstate(invalid="ignore"):
                vis &= poses[p, :, 2] > np.float32(c["thr"])
        if not usable.all():
            status[p] |= 1
        if c["boxes"] is not None:
            cxy, cok = snap(np.asarray(c["boxes"], np.float32)[b, p])
            good = bool(cok.all())
            if not good:
                status[p] |= 2
            for k in range(4):
                out.append(dict(a=cxy[k], b=cxy[(k + 1) % 4], h2=c["box_h2"], r16=-1, colour=np.asarray(c["box_rgb"], np.int64),
                                kind="box", p=p, l=k, drawn=good))
        for l, (i1, i2) in enumerate(bones):
            assert 0 <= i1 < J and 0 <= i2 < J
            col = np.asarray(c["colours"][l] if c["colour_mode"] == 0 else c["colours"][b, p], np.int64)
            out.append(dict(a=xy[i1], b=xy[i2], h2=c["line_h2"], r16=-1, colour=col, kind="line", p=p, l=l,
                            drawn=bool(vis[i1] and vis[i2])))
            for i in (i1, i2):
                out.append(dict(a=xy[i], b=xy[i], h2=c["mark_h2"], r16=c["mark_r16"], colour=col, kind="mark", p=p, l=l,
                                drawn=bool(vis[i])))
    return out, status


def reach(h2, r16):
    """Pixels beyond which a primitive has no coverage, plus one."""
    return (8 * h2 + 8 + max(r16, 0) + 15) // 16 + 1


def paint(m, prim, H, W):
    """Blend one primitive into the int64 image m [H, W, 3] in place; returns the number of pixels with cov > 0."""
    if not prim["drawn"]:
        return 0
    a, b, r = prim["a"], prim["b"], reach(prim["h2"], prim["r16"])
    x0, x1 = max(int(min(a[0], b[0])) - r, 0), min(int(max(a[0], b[0])) + r, W - 1)
    y0, y1 = max(int(min(a[1], b[1])) - r, 0), min(int(max(a[1], b[1])) + r, H - 1)
    if x0 > x1 or y0 > y1:
        return 0
    qy, qx = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
    cov = coverage(qx, qy, a, b, prim["h2"], prim["r16"])
    sub = m[y0:y1 + 1, x0:x1 + 1]
    sub += ((prim["colour"][None, None, :] - sub) * cov[:, :, None] + 8) >> 4      # (cov = 0: + (8 >> 4) = 0)
    return int((cov > 0).sum())


def overlay_image(c, b):
    H, W = c["H"], c["W"]
    src = np.asarray(c["src"])[b].astype(np.int64)
    prims, status = primitives(c, b)
    m = src.copy()
    touched = [paint(m, q, H, W) for q in prims]
    a = int(c["alpha256"])
    dst = (src * (256 - a) + m * a + 128) >> 8
    assert dst.min() >= 0 and dst.max() <= 255
    return dst.astype(np.uint8), status, prims, touched


def overlay_case(c):
    """-> dict(dst uint8 [B, H, W, 3], status int32 [B, P], prims, touched: per image, the primitives in paint order and the
    number of pixels each one covers)."""
    B = np.asarray(c["poses"]).shape[0]
    res = [overlay_image(c, b) for b in range(B)]
    return dict(dst=np.stack([r[0] for r in res]), status=np.stack([r[1] for r in res]), prims=[r[2] for r in res],
                touched=[r[3] for r in res])
