"""The yardstick of the renderer (csrc/render.hip, include/p2m.h: p2m_mesh_render): float64 projection and snap, exact int64
edge functions with the top-left rule, float64 depth and shading, in numpy.  The reference's own renderer (demo/renderer.py:
trimesh + pyrender + OpenGL) cannot run without an OpenGL context, so the header comment is the contract and this file its
restatement; tests/test_render_cpu.py checks the restatement against properties no rasteriser may miss (watertightness, union
of single faces, mirror symmetry) and tests/test_gpu_render.py holds the kernels to it.

Two bounds are derived here.

DEPTH.  The device evaluates, in fp32 with u = 2^-24 and Z = max(|z0|, |z1|, |z2|) of the face,
    l1 = fl(fl(E2) / fl(A)),  l2 = fl(fl(E0) / fl(A)),  depth = fma(l2, fl(z2 - z0), fma(l1, fl(z1 - z0), z0))
with E0, E2, A = |area2| exact integers, 0 <= E <= A.  Two conversions and one division give l = l_exact (1 + d)^3, an error
of at most 3 u l (+ O(u^2)); z_k - z0 is rounded once, |z_k - z0| <= 2 Z, so each product l (z_k - z0) is off by at most
4 u l 2 Z = 8 u l Z; each fma rounds a value of magnitude at most Z (a convex combination of the z's, up to the errors
above) once: u Z each.  With l1 + l2 <= 1 the sum is 8 u Z + 2 u Z = 10 u Z; DEPTH_ULPS = 12 covers the second-order terms.
The float64 evaluation below errs by about 2^-29 of that.  Per fragment: bound = 12 x 2^-24 x max|z| of its face.

COLOUR.  The device computes v = 255 min(1, colour I) + 0.5 in fp64 per face and stores floor(v); this file computes the
same expression in float64 and returns v itself, so that a test can allow one LSB exactly where v lies within 1e-4 of an
integer (the two fp64 evaluations differ by contraction and the order of a three-term sum only: about 1e-13).
"""
import numpy as np

FIX = 256
CLAMP = 1 << 23
DEPTH_ULPS = 12.0
U32 = 2.0 ** -24
SNAP_MARGIN = 1e-9                       # sub-pixel units: a float64 value this close to a rounding boundary is not compared


def coefficients(cam, H, W):
    """cam (sx, sy, tx, ty) as float32 -> (ax, bx, ay, by) in float64, each operation rounded once (the device's formula)."""
    sx, sy, tx, ty = (np.float64(np.float32(v)) for v in cam)
    hw, hh = np.float64(0.5 * W), np.float64(0.5 * H)
    return hw * sx, hw * (1.0 + sx * tx), hh * sy, hh * (1.0 + sy * ty)


def snap(p):
    """float64 pixel coordinates -> (int64 1/256-pixel coordinates clamped to +-2^23, clamped mask, distance of 256 p from the
    nearest rounding boundary in sub-pixel units)."""
    t = FIX * np.asarray(p, np.float64)
    r = np.rint(t)                                             # ties to even
    with np.errstate(invalid="ignore"):
        hi, lo = ~(r <= CLAMP), r < -CLAMP                     # (NaN counts as +2^23)
    margin = np.abs(np.abs(t - np.floor(t)) - 0.5)
    r = np.where(hi, CLAMP, np.where(lo, -CLAMP, r))
    return r.astype(np.int64), hi | lo, np.where(hi | lo, np.inf, margin)


def project(verts, cam, H, W):
    """verts [nv, 3] float32 -> dict(xy int64 [nv, 2], clamped [nv], margin [nv], px, py float64).  The device fuses
    a v + b into one fma; numpy rounds twice, a difference of one ulp of a pixel coordinate (1e-13 px), far below
    SNAP_MARGIN - which is why vertices inside the margin are left out of the exact comparison."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    ax, bx, ay, by = coefficients(cam, H, W)
    with np.errstate(invalid="ignore", over="ignore"):
        px, py = ax * v[:, 0] + bx, ay * v[:, 1] + by
    X, cx, mx = snap(px)
    Y, cy, my = snap(py)
    return dict(xy=np.stack([X, Y], 1), clamped=cx | cy, margin=np.minimum(mx, my), px=px, py=py,
                mirror=bool((ax < 0) != (ay < 0)))


def face_values(verts, faces, colour, lights, ambient):
    """Per face: v [nf, 3] float64 = 255 min(1, colour_c I) + 0.5, the value whose floor is the stored byte.  I = ambient +
    sum k max(0, n . l), n the float64 unit normal turned towards the viewer (n_z <= 0), l the float64-normalised float32
    direction towards the light."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces)
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    n = np.cross(e1, e2)
    ln = np.sqrt((n * n).sum(1))
    I = np.full(len(f), np.float64(np.float32(ambient)))
    li = np.asarray(lights, np.float32).astype(np.float64).reshape(-1, 4)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(n[:, 2] > 0, -1.0, 1.0) / ln
        for l in li:
            d = l[:3] / np.sqrt((l[:3] * l[:3]).sum())
            I = I + np.where(ln > 0, l[3] * np.maximum(s * (n @ d), 0.0), 0.0)
    c = np.asarray(colour, np.float32).astype(np.float64)
    return 255.0 * np.minimum(1.0, c[None, :] * I[:, None]) + 0.5


def bytes_of(v):
    with np.errstate(invalid="ignore"):
        r = np.floor(v)
    return np.where(r > 0, r, 0).astype(np.uint8)              # (negative and NaN -> 0; v <= 255.5)


def rasterise(meshes, faces, H, W, cull=True, z_range=(-1.0, 1.0), order="depth", single_faces=None):
    """meshes: list (in rank order) of dicts(xy int64 [nv, 2], z float32 [nv], mirror bool).  Returns per pixel, as [H, W]
    arrays: face_id, mesh_id (-1: background), depth (float64 plane value of the winner, +inf: background), bound (its depth
    bound), count (fragments kept), left_out (the winner is not safely decided: another fragment of the same class - all
    fragments in depth order, the winner's mesh in list order - lies within the sum of the two bounds, or a fragment within its
    bound of zmin / zmax could have won), on_edge (a pixel centre exactly on an edge of a kept or dropped fragment).
    single_faces: only these face ids are drawn."""
    zmin, zmax = (np.float64(np.float32(v)) for v in z_range)
    face_id = np.full((H, W), -1, np.int32)
    mesh_id = np.full((H, W), -1, np.int32)
    depth = np.full((H, W), np.inf)
    bound = np.zeros((H, W))
    second_lo = np.full((H, W), np.inf)                       # min (depth - bound) over the other fragments of the class
    unc_lo = np.full((H, W), np.inf)                          # the same over fragments within their bound of a clip plane
    unc_rank = np.full((H, W), -1, np.int32)
    count = np.zeros((H, W), np.int32)
    on_edge = np.zeros((H, W), bool)
    faces = np.asarray(faces, np.int64)
    todo = range(len(faces)) if single_faces is None else single_faces
    for rank, mesh in enumerate(meshes):
        xy, z = np.asarray(mesh["xy"], np.int64), np.asarray(mesh["z"], np.float32).astype(np.float64)
        for f in todo:
            i = faces[f]
            X, Y = xy[i, 0], xy[i, 1]
            area2 = int((X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0]))
            if area2 == 0:
                continue
            front = (area2 > 0) if mesh.get("mirror", False) else (area2 < 0)
            if cull and not front:
                continue
            s = 1 if area2 > 0 else -1
            jx0, jx1 = max((int(X.min()) - FIX // 2 + FIX - 1) // FIX, 0), min((int(X.max()) - FIX // 2) // FIX, W - 1)
            jy0, jy1 = max((int(Y.min()) - FIX // 2 + FIX - 1) // FIX, 0), min((int(Y.max()) - FIX // 2) // FIX, H - 1)
            if jx0 > jx1 or jy0 > jy1:
                continue
            Px = (np.arange(jx0, jx1 + 1, dtype=np.int64) * FIX + FIX // 2)[None, :]
            Py = (np.arange(jy0, jy1 + 1, dtype=np.int64) * FIX + FIX // 2)[:, None]
            inside = np.ones((jy1 - jy0 + 1, jx1 - jx0 + 1), bool)
            closed = inside.copy()
            E = []
            for k in range(3):
                a, b = k, (k + 1) % 3
                A, Bc = -s * (Y[b] - Y[a]), s * (X[b] - X[a])
                Ek = A * (Px - X[a]) + Bc * (Py - Y[a])
                top_left = A > 0 or (A == 0 and Bc > 0)
                inside &= (Ek > 0) | ((Ek == 0) & top_left)
                closed &= Ek >= 0
                E.append(Ek)
            win = (slice(jy0, jy1 + 1), slice(jx0, jx1 + 1))
            on_edge[win] |= closed & ((E[0] == 0) | (E[1] == 0) | (E[2] == 0))
            if not inside.any():
                continue
            area = float(s * area2)
            d = z[i[0]] + (E[2] / area) * (z[i[1]] - z[i[0]]) + (E[0] / area) * (z[i[2]] - z[i[0]])
            bf = DEPTH_ULPS * U32 * float(np.abs(z[i]).max())
            with np.errstate(invalid="ignore"):
                keep = inside & (d >= zmin) & (d <= zmax)
                unc = inside & ((np.abs(d - zmin) <= bf) | (np.abs(d - zmax) <= bf) | ~np.isfinite(d))
            if unc.any():
                r0, u0 = unc_rank[win], unc_lo[win]
                newer = unc & (rank > r0) if order == "list" else np.zeros_like(unc)
                u0 = np.where(newer, np.inf, u0)
                unc_lo[win] = np.where(unc, np.minimum(u0, np.where(np.isfinite(d), d - bf, -np.inf)), u0)
                unc_rank[win] = np.where(unc, rank, r0)
            if not keep.any():
                continue
            bd, br, bfid = depth[win], mesh_id[win], face_id[win]
            if order == "list":
                newer = br < rank                                 # (meshes are drawn in rank order: br <= rank)
                beats = keep & (newer | (d < bd) | ((d == bd) & (f < bfid)))
                same = ~newer
            else:
                beats = keep & ((d < bd) | ((d == bd) & ((rank < br) | ((rank == br) & (f < bfid)))))
                same = np.ones_like(keep)
            sl = second_lo[win]
            old_lo = np.where(same & (bfid >= 0), bd - bound[win], np.inf)
            sl = np.where(beats, np.minimum(np.where(same, sl, np.inf), old_lo), np.where(keep, np.minimum(sl, d - bf), sl))
            second_lo[win] = sl
            depth[win] = np.where(beats, d, bd)
            bound[win] = np.where(beats, bf, bound[win])
            mesh_id[win] = np.where(beats, rank, br)
            face_id[win] = np.where(beats, f, bfid)
            count[win] += keep
    covered = face_id >= 0
    with np.errstate(invalid="ignore"):
        left_out = covered & (second_lo < depth + bound)
        if order == "list":
            left_out |= (unc_rank > mesh_id) | ((unc_rank == mesh_id) & (unc_lo <= depth + bound) & (unc_rank >= 0))
        else:
            left_out |= (unc_rank >= 0) & (unc_lo <= depth + bound)
    return dict(face_id=face_id, mesh_id=mesh_id, depth=depth, bound=bound, count=count, left_out=left_out, on_edge=on_edge)


def shade(ras, values, background, H, W):
    """values: per mesh [nf, 3] (face_values).  -> (image uint8 [H, W, 3], v float64 [H, W, 3], NaN on the background)."""
    img = np.zeros((H, W, 3), np.uint8) if background is None else np.array(background, np.uint8)
    v = np.full((H, W, 3), np.nan)
    for m, val in enumerate(values):
        sel = ras["mesh_id"] == m
        v[sel] = val[ras["face_id"][sel]]
    cov = ras["face_id"] >= 0
    img[cov] = bytes_of(v[cov])
    return img, v


def render_case(c, xy_fix=None):
    """A case of tests/render_cases.py -> list over images of dicts (rasterise's arrays + image, v, and the per-mesh
    projections `proj`).  xy_fix [B, nv, 2]: the device's snapped coordinates to use instead of this file's own."""
    B, H, W = c["verts"].shape[0], c["H"], c["W"]
    proj = [project(c["verts"][b], c["cam"][b], H, W) for b in range(B)]
    meshes = [dict(xy=proj[b]["xy"] if xy_fix is None else np.asarray(xy_fix[b], np.int64), z=c["verts"][b][:, 2],
                   mirror=proj[b]["mirror"]) for b in range(B)]
    vals = [face_values(c["verts"][b], c["faces"], c["colours"][b], c["lights"], c["ambient"]) for b in range(B)]
    groups = [list(range(B))] if c["mode"] == "scene" else [[b] for b in range(B)]
    out = []
    for g in groups:
        ras = rasterise([meshes[b] for b in g], c["faces"], H, W, c["cull"], c["z_range"],
                        c["order"] if c["mode"] == "scene" else "depth")
        bg = c["background"]
        if bg is not None and bg.ndim == 4:
            bg = bg[g[0]]
        ras["image"], ras["v"] = shade(ras, [vals[b] for b in g], bg, H, W)
        if c["mode"] != "scene":                              # mesh_id is the mesh's index in the call
            ras["mesh_id"] = np.where(ras["mesh_id"] >= 0, g[0], -1).astype(np.int32)
        ras["proj"] = [proj[b] for b in g]
        out.append(ras)
    return out


# ---- the device-exact yardstick ---------------------------------------------------------------------------------------------
# rasterise() above decides a pixel only where float64 can: it leaves out exact depth ties and fragments within their bound of a
# clip plane - the pixels where the rules include/p2m.h states bit for bit apply.  rasterise_exact() evaluates the header's own
# fp32 formula (correctly rounded conversions and divisions, z_k - z0 rounded once, two exactly evaluated fmafs), keeps a fragment
# when zmin <= depth <= zmax in fp32 and takes the minimum of the header's 64-bit key: every pixel is decided and depth is
# comparable bitwise.  The two yardsticks check each other in tests/test_render_edges_cpu.py.
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
_TWO128 = 2.0 ** 128


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, rounded once (Python 3.10 has no math.fma).  The float64 product of two fp32 factors is
    exact (48 bits, no over- or underflow); a TwoSum gives product + addend exactly as s + e with s the float64 rounding; the
    fp32 rounding of s is the fp32 rounding of s + e unless s lies exactly half-way between two neighbouring fp32 values and
    e != 0 (no float64 lies strictly between s + e and s, so they are on the same side of every other boundary): there e
    decides.  NaN and +-inf come out of the float64 sum as fmaf gives them; an exact zero has the sign of the float64 sum, which
    is fmaf's."""
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c8 = c.astype(np.float64)
        s = p + c8
        t = s - p
        e = (p - (s - t)) + (c8 - t)
        r = np.asarray(s.astype(np.float32))
        lo = np.where(r.astype(np.float64) <= s, r, np.nextafter(r, np.float32(-np.inf))).astype(np.float32)
        hi = np.nextafter(lo, np.float32(np.inf))
        lo8 = np.where(np.isneginf(lo), -_TWO128, lo.astype(np.float64))      # (the overflow threshold rounds like a value)
        hi8 = np.where(np.isposinf(hi), _TWO128, hi.astype(np.float64))
        half = np.isfinite(s) & (lo8 != s) & ((s - lo8) == (hi8 - s)) & (e != 0)
        r = np.where(half, np.where(e > 0, hi, lo), r)
    return r.astype(np.float32)


def depth_bits(d):
    """Order-preserving bits of an fp32 depth: smaller float <=> smaller unsigned (-0.0 sorts below +0.0)."""
    u = np.ascontiguousarray(d, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def bits_depth(b):
    b = np.ascontiguousarray(b, np.uint32)
    return np.where(b & np.uint32(0x80000000), b & np.uint32(0x7FFFFFFF), ~b).astype(np.uint32).view(np.float32)


def pixel_bbox(X, Y, H, W):
    """Inclusive pixel bbox (jx0, jy0, jx1, jy1) of the centres inside the snapped coordinates' bbox, clipped to the image."""
    jx0, jx1 = max((int(X.min()) - FIX // 2 + FIX - 1) // FIX, 0), min((int(X.max()) - FIX // 2) // FIX, W - 1)
    jy0, jy1 = max((int(Y.min()) - FIX // 2 + FIX - 1) // FIX, 0), min((int(Y.max()) - FIX // 2) // FIX, H - 1)
    return jx0, jy0, jx1, jy1


def rasterise_exact(meshes, faces, H, W, cull=True, z_range=(-1.0, 1.0), order="depth", single_faces=None):
    """rasterise() with depth and the winner as include/p2m.h defines them, in fp32.  Same arguments; per pixel face_id, mesh_id
    (-1: background), depth (float32, +inf: background), count (fragments kept), on_edge, and for rasterise()'s readers bound
    (zeros) and left_out (all False: every pixel is decided).  Besides: ties [H, W], the number of kept fragments at the
    pixel's smallest depth bits (>= 2: an exact depth tie for the front), and kept / dropped, dicts (rank, face) -> covered
    pixels that passed / failed zmin <= depth <= zmax.  A face with an index outside [0, nv) covers nothing."""
    zmin, zmax = np.float32(z_range[0]), np.float32(z_range[1])
    keys = np.full((H, W), NO_KEY, np.uint64)
    min_db = np.full((H, W), 1 << 32, np.uint64)
    ties = np.zeros((H, W), np.int32)
    count = np.zeros((H, W), np.int32)
    on_edge = np.zeros((H, W), bool)
    kept, dropped = {}, {}
    faces = np.asarray(faces, np.int64)
    ids = np.arange(len(faces)) if single_faces is None else np.asarray(single_faces, np.int64)
    f4 = np.float32
    for rank, mesh in enumerate(meshes):
        xy, z = np.asarray(mesh["xy"], np.int64), np.asarray(mesh["z"], np.float32)
        sel = ids[((faces[ids] >= 0) & (faces[ids] < len(xy))).all(1)]
        Xa, Ya = xy[faces[sel], 0], xy[faces[sel], 1]
        a2 = (Xa[:, 1] - Xa[:, 0]) * (Ya[:, 2] - Ya[:, 0]) - (Xa[:, 2] - Xa[:, 0]) * (Ya[:, 1] - Ya[:, 0])
        live = a2 != 0
        if cull:
            live &= (a2 > 0) if mesh.get("mirror", False) else (a2 < 0)
        for f in sel[live]:
            f = int(f)
            i = faces[f]
            X, Y = xy[i, 0], xy[i, 1]
            area2 = int((X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0]))
            s = 1 if area2 > 0 else -1
            jx0, jy0, jx1, jy1 = pixel_bbox(X, Y, H, W)
            if jx0 > jx1 or jy0 > jy1:
                continue
            Px = (np.arange(jx0, jx1 + 1, dtype=np.int64) * FIX + FIX // 2)[None, :]
            Py = (np.arange(jy0, jy1 + 1, dtype=np.int64) * FIX + FIX // 2)[:, None]
            inside = np.ones((jy1 - jy0 + 1, jx1 - jx0 + 1), bool)
            closed = inside.copy()
            E = []
            for k in range(3):
                a, b = k, (k + 1) % 3
                A, Bc = -s * (Y[b] - Y[a]), s * (X[b] - X[a])
                Ek = A * (Px - X[a]) + Bc * (Py - Y[a])
                inside &= (Ek > 0) | ((Ek == 0) & bool(A > 0 or (A == 0 and Bc > 0)))
                closed &= Ek >= 0
                E.append(Ek)
            win = (slice(jy0, jy1 + 1), slice(jx0, jx1 + 1))
            on_edge[win] |= closed & ((E[0] == 0) | (E[1] == 0) | (E[2] == 0))
            if not inside.any():
                continue
            with np.errstate(all="ignore"):
                area = np.int64(s * area2).astype(f4)
                l1, l2 = E[2].astype(f4) / area, E[0].astype(f4) / area
                z0, d1, d2 = z[i[0]], f4(z[i[1]] - z[i[0]]), f4(z[i[2]] - z[i[0]])
                d = fma32(l2, d2, fma32(l1, d1, z0))
                keep = inside & (d >= zmin) & (d <= zmax)
            kept[(rank, f)], dropped[(rank, f)] = int(keep.sum()), int((inside & ~keep).sum())
            if not keep.any():
                continue
            db = depth_bits(d).astype(np.uint64)
            if order == "list":
                key = (np.uint64(255 - rank) << np.uint64(56)) | (db << np.uint64(24)) | np.uint64(f)
            else:
                key = (db << np.uint64(32)) | (np.uint64(rank) << np.uint64(24)) | np.uint64(f)
            keys[win] = np.minimum(keys[win], np.where(keep, key, NO_KEY))
            mb, t = min_db[win], ties[win]
            lt, eq = keep & (db < mb), keep & (db == mb)
            ties[win] = np.where(lt, 1, np.where(eq, t + 1, t))
            min_db[win] = np.where(lt, db, mb)
            count[win] += keep
    covered = keys != NO_KEY
    if order == "list":
        rk, db = np.uint64(255) - (keys >> np.uint64(56)), (keys >> np.uint64(24)) & np.uint64(0xFFFFFFFF)
    else:
        rk, db = (keys >> np.uint64(24)) & np.uint64(0xFF), keys >> np.uint64(32)
    face_id = np.where(covered, (keys & np.uint64(0xFFFFFF)).astype(np.int64), -1).astype(np.int32)
    mesh_id = np.where(covered, rk.astype(np.int64), -1).astype(np.int32)
    depth = np.where(covered, bits_depth(db.astype(np.uint32)), f4(np.inf)).astype(f4)
    return dict(face_id=face_id, mesh_id=mesh_id, depth=depth, bound=np.zeros((H, W)), count=count,
                left_out=np.zeros((H, W), bool), on_edge=on_edge, ties=ties, kept=kept, dropped=dropped)


def render_case_exact(c, xy_fix=None):
    """render_case() on rasterise_exact(): a case of tests/render_cases.py or tests/render_edge_cases.py -> list over images.
    A case may name `single_faces` (the only faces that can cover anything: keeps the host loop short at a large nf); faces
    with an index outside [0, nv) cover nothing and are shaded as face (0, 0, 0), which is never seen."""
    B, H, W = c["verts"].shape[0], c["H"], c["W"]
    nv = c["verts"].shape[1]
    proj = [project(c["verts"][b], c["cam"][b], H, W) for b in range(B)]
    meshes = [dict(xy=proj[b]["xy"] if xy_fix is None else np.asarray(xy_fix[b], np.int64), z=c["verts"][b][:, 2],
                   mirror=proj[b]["mirror"]) for b in range(B)]
    valid = ((c["faces"] >= 0) & (c["faces"] < nv)).all(1)
    safe = np.where(valid[:, None], c["faces"], 0)
    with np.errstate(all="ignore"):
        vals = [face_values(c["verts"][b], safe, c["colours"][b], c["lights"], c["ambient"]) for b in range(B)]
    groups = [list(range(B))] if c["mode"] == "scene" else [[b] for b in range(B)]
    out = []
    for g in groups:
        ras = rasterise_exact([meshes[b] for b in g], c["faces"], H, W, c["cull"], c["z_range"],
                              c["order"] if c["mode"] == "scene" else "depth", c.get("single_faces"))
        bg = c["background"]
        if bg is not None and bg.ndim == 4:
            bg = bg[g[0]]
        ras["image"], ras["v"] = shade(ras, [vals[b] for b in g], bg, H, W)
        if c["mode"] != "scene":
            ras["mesh_id"] = np.where(ras["mesh_id"] >= 0, g[0], -1).astype(np.int32)
        ras["proj"] = [proj[b] for b in g]
        out.append(ras)
    return out
