"""The renderer's edge-case table: the inputs on which the rules include/p2m.h states bit for bit decide the picture - exact
depth ties, the fields of the 64-bit key at their widths, fragments exactly on zmin / zmax, the hand-over list of the whole-block
path at its capacity, shared edges through pixel centres on tile borders, images at the largest extent and the narrowest width,
the per-mesh bbox skip of scene mode, cameras, shading and the status bits.  Same dict format and builders as
tests/render_cases.py; tests/test_render_edges_cpu.py shows that every case reaches the arm it is named for and
tests/test_gpu_render_edges.py holds the kernels to render_ref.rasterise_exact on every pixel of every case.

Two keys more than in render_cases.py: `single_faces` (the only faces that can cover anything; the yardstick loops over them
alone) and `arm`, what the case has to reach, checked on the CPU: a tuple (kind, parameters...).  `cls`: False where MeshRenderer
cannot express the case (it refuses an out-of-range face index before the launch).

A face at a constant z has both products of the depth formula exactly zero, so its device depth is exactly that z: constant-z
faces give exact ties and exact clip-plane hits.  Every case uses the pixel camera unless it is about the camera."""
import numpy as np

import render_cases as rc
from render_cases import _case, background, pixel_cam

F32 = np.float32


def tris(*t):
    """Triangles ((x, y, z), (x, y, z), (x, y, z)) -> (verts [3 n, 3] fp32, faces [n, 3]): no shared vertices."""
    return np.array([p for tri in t for p in tri], F32), np.arange(3 * len(t)).reshape(-1, 3)


def flat(x0, y0, x1, y1, x2, y2, z):
    return ((x0, y0, z), (x1, y1, z), (x2, y2, z))


def right(x, y, w, h, z):
    """The front-facing right triangle with its right angle at (x, y) and legs w (along x) and h (along y)."""
    return flat(x, y, x, y + h, x + w, y, z)


def sparse_faces(nf, rows):
    """nf faces, all the index triple (0, 0, 0) (area 0) except `rows`: {face id: triangle number}, triangle t using the
    vertices 3 t .. 3 t + 2."""
    f = np.zeros((nf, 3), np.int64)
    for fid, t in rows.items():
        f[fid] = (3 * t, 3 * t + 1, 3 * t + 2)
    return f


def grid_mesh(n):
    """n x n quads over [0, 1]^2 cut into front-facing triangles: (verts [(n + 1)^2, 2] float64, faces [2 n^2, 3])."""
    g = np.linspace(0.0, 1.0, n + 1)
    v = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    f = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, i * (n + 1) + j + 1, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1
            f += [(a, c, b), (b, c, d)]
    return v, np.array(f, np.int64)


def _scene_tie():
    """Two meshes, three faces, every fragment at z = 0.5.  Region P (left): mesh 0 face 0, mesh 1 faces 1 and 2; region R
    (right): mesh 0 faces 1 and 2, mesh 1 face 0.  Depth order: the lower rank beats the lower face id (R shows mesh 0 face
    1); list order: the last mesh, and within it the lower face id (P shows mesh 1 face 1)."""
    P, P2, R, R2 = right(2, 2, 20, 24, .5), right(4, 3, 20, 24, .5), right(30, 2, 20, 24, .5), right(32, 3, 20, 24, .5)
    v0, f = tris(P, R, R2)
    v1, _ = tris(R, P, P2)
    return np.stack([v0, v1]), f


def _key_fields(nf, ids):
    """The faces `ids` (ascending) are right triangles of 14 x 14 pixels, each shifted by 5 pixels against the one before and
    nearer than it; every other face is (0, 0, 0)."""
    t = [right(3 + 5 * k, 3 + 5 * k, 14, 14, 0.8 - 0.1 * k) for k in range(len(ids))]
    v, _ = tris(*t)
    return v, sparse_faces(nf, {fid: k for k, fid in enumerate(ids)})


def _big512():
    """One 64 x 64 tile.  Faces 0 .. 511: right triangles with 40-pixel legs, their corners on an 8 x 8 lattice of offsets
    (every clipped bbox 1600 pixels: the whole-block path), at 510 distinct depths and one tied pair (100 and 300, the nearest of
    all).  Faces 512 .. 515: small ones in front, and one more large one.  The first two scan steps fill the 512-entry queue with
    whole-block faces: one flush hands over 512."""
    t = []
    for k in range(512):
        z = 0.05 if k in (100, 300) else 0.1 + 0.0015 * ((k * 197) % 512)
        t.append(right(1.3 + (k % 8) * 2.5, 1.3 + ((k // 8) % 8) * 2.5 + (k // 64) * 0.25, 40, 40, z))
    t += [right(5, 5, 6, 6, 0.01), right(50, 50, 9, 9, 0.02), right(20, 45, 10, 4, 0.03), right(0.7, 0.7, 62, 62, 0.99)]
    return tris(*t)


def _seam():
    """A 5 x 5 quad mesh whose vertices lie on pixel centres at x, y in {0.5, 63.5, 64.5, 127.5, 128.5, 129.5} of a 130 x 130
    image: every vertical and horizontal shared edge runs through the centres of a column / row next to a tile border, on both
    sides of it.  One slanted plane: every pixel has one fragment."""
    g = np.array([0.5, 63.5, 64.5, 127.5, 128.5, 129.5])
    xy = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    _, f = grid_mesh(5)
    z = 0.001 * xy[:, 0] + 0.002 * xy[:, 1] - 0.2
    return np.concatenate([xy, z[:, None]], 1).astype(F32), f


def _long(H, W):
    """One thin triangle along the whole long side (its ends beyond the image) and small ones at both ends."""
    if H >= W:
        L, t = H, lambda a, b, z: (b, a, z)                               # (a along the long side, b across)
    else:
        L, t = W, lambda a, b, z: (a, b, z)
    T = [(t(-2, 0.2, 0.3), t(L // 2, W * 0.99 if H >= W else H * 0.99, 0.1), t(L + 2, 0.3, -0.2)),
         (t(0, 0, 0.5), t(0, 3, 0.5), t(2.2, 0, 0.6)), (t(L, 0, 0.5), t(L - 2.2, 0, 0.6), t(L, 3, 0.5)),
         (t(1, 0, -0.5), t(1.9, 1.2, -0.5), t(3, 0, -0.4)), (t(L - 1, 0, -0.5), t(L - 3, 0, -0.4), t(L - 1.9, 1.2, -0.5))]
    return tris(*T)


def _scene_skip():
    """Five meshes over one 4 x 4 quad grid (32 front-facing faces), 130 x 129 image: 0 and 4 in every tile (4 leaves a margin
    where 0 shows), 1 entirely off the image, 2 mirrored in x (every face back-facing: culled, the mesh's bbox stays the
    sentinel), 3 inside tile (1, 1)."""
    g, f = grid_mesh(4)
    place = [(-5.3, -4.7, 141.0, 139.0, 0.6), (400.2, 10.1, 100.0, 100.0, 0.1), (120.4, 8.8, -110.0, 110.0, 0.2),
             (80.3, 75.6, 21.0, 19.0, 0.3), (30.4, 30.9, 104.0, 107.0, 0.4)]
    vs = []
    for ox, oy, sx, sy, z in place:
        x, y = ox + sx * g[:, 0], oy + sy * g[:, 1]
        vs.append(np.stack([x, y, z + 0.001 * g[:, 0] - 0.0007 * g[:, 1]], 1))
    return np.stack(vs).astype(F32), f


_cache, _ref_cache = {}, {}
HULL_LIGHT = np.array([[0.3, -0.2, -1.0, 0.6]], F32)
FOUR_LIGHTS = np.array([[0.0, 0.0, -1.0, 0.3], [1.0, -1.0, -1.0, 0.25], [-1.0, 0.5, -0.5, 0.2], [0.2, 1.0, -0.1, 0.15]], F32)


def case(name):
    if name not in _cache:
        c = _build(name)
        c["name"] = name
        c.setdefault("arm", ("covered",))
        c.setdefault("cls", True)
        _cache[name] = c
    return _cache[name]


def _flat_case(name, v, f, H, W, **kw):
    kw.setdefault("cull", False)
    return _case(name, v, f, pixel_cam(W, H), H, W, **kw)


def _build(name):
    # ---- ties, batch mode ----
    if name == "tie_two":
        v, f = tris(right(2, 2, 28, 28, .5), right(5, 5, 30, 23, .5))
        return dict(_flat_case(name, v, f, 32, 40, bg=background(32, 40, 21)), arm=("tie", {0}))
    if name == "tie_three":
        v, f = tris(right(2, 2, 28, 28, .25), right(5, 5, 30, 23, .25), right(1, 8, 36, 20, .25), right(0, 0, 40, 32, .7))
        return dict(_flat_case(name, v, f, 32, 40), arm=("tie", {0, 1}))
    if name == "tie_duplicate":
        v, _ = tris(right(3, 2, 30, 25, -.5))
        return dict(_flat_case(name, v, [(0, 1, 2), (0, 1, 2)], 32, 40), arm=("tie", {0}))
    if name in ("tie_steps_low_wins", "tie_steps_high_nearer"):
        # ids 3 and 700 overlap; 300 small faces between them fill the queue, so the two are rasterised in different flushes
        near = name.endswith("nearer")
        t = [right(2, 2, 12, 12, .5), right(5, 5, 12, 12, .25 if near else .5)]
        t += [right(20 + 2 * (k % 20), 2 + 2 * (k // 20), 1.9, 1.9, .1 + k * 1e-3) for k in range(300)]
        v, _ = tris(*t)
        rows = {3: 0, 700: 1}
        rows.update({10 + k: 2 + k for k in range(300)})
        f = sparse_faces(701, rows)
        return dict(_flat_case(name, v, f, 40, 64), arm=("tie", {3}) if not near else ("ids", [3, 700]))
    if name in ("tie_big_small", "tie_small_big"):
        big, small = right(2, 2, 40, 40, .5), right(6, 6, 14, 14, .5)    # clipped bboxes of 1600 and 196 pixels
        v, f = tris(*((big, small) if name == "tie_big_small" else (small, big)))
        return dict(_flat_case(name, v, f, 48, 48), arm=("tie_paths", {0}))
    # ---- ties, scene mode ----
    if name.startswith("scene_identical"):
        v, f = tris(right(2, 2, 28, 28, .5), right(5, 5, 30, 23, .5), ((1, 30, .1), (20, 31, .9), (38, 3, .6)))
        order = name.rsplit("_", 1)[1]
        col = np.array([(1, .3, .3), (.3, 1, .3), (.3, .3, 1)], F32)
        return dict(_flat_case(name, np.stack([v] * 3), f, 32, 40, mode="scene", order=order, colours=col,
                               bg=background(32, 40, 22)), arm=("scene_tie", 0 if order == "depth" else 2))
    if name.startswith("scene_255"):
        v, f = tris(right(1.5, 1.5, 9, 7, .5))
        order = name.rsplit("_", 1)[1]
        col = np.linspace(0.2, 1.0, 255 * 3).reshape(255, 3)
        return dict(_flat_case(name, np.stack([v] * 255), f, 10, 12, mode="scene", order=order, colours=col),
                    arm=("scene_tie", 0 if order == "depth" else 254))
    if name.startswith("scene_rank_vs_face"):
        v, f = _scene_tie()
        order = name.rsplit("_", 1)[1]
        return dict(_flat_case(name, v, f, 32, 56, mode="scene", order=order, colours=[(1, .5, .5), (.5, .5, 1)]),
                    arm=("scene_rank_vs_face", order))
    # ---- key fields ----
    if name == "key_65836":
        ids = [0, 255, 256, 65535, 65536, 65537, 65536 + 300 - 1]
        v, f = _key_fields(65536 + 300, ids)
        return dict(_flat_case(name, v, f, 64, 64), single_faces=ids, arm=("ids", ids))
    if name == "key_2p20":
        ids = [(1 << 20) - 1, 1 << 20]
        v, f = _key_fields((1 << 20) + 1, ids)
        return dict(_flat_case(name, v, f, 64, 64), single_faces=ids, arm=("ids", ids))
    # ---- depth range ----
    if name == "clip_planes":
        zmin, zmax = F32(0.1), F32(0.7)
        z = [zmax, np.nextafter(zmax, F32(np.inf)), zmin, np.nextafter(zmin, F32(-np.inf))]
        t = [right(2 + 12 * k, 2, 10, 20, z[k]) for k in range(4)] + [flat(0, 12, 0, 30, 50, 12, .5)]
        v, f = tris(*t)
        return dict(_flat_case(name, v, f, 32, 52, z_range=(zmin, zmax), bg=background(32, 52, 23)),
                    arm=("clip", [0, 2, 4], [1, 3]))
    if name == "clip_infinite":
        t = [right(2, 2, 20, 20, 3.0e38), right(6, 6, 20, 20, -3.0e38), ((1, 25, -1e30), (30, 28, 1e30), (20, 2, 5.0)),
             right(12, 1, 25, 25, 1e-40)]
        v, f = tris(*t)
        return dict(_flat_case(name, v, f, 32, 40, z_range=(-np.inf, np.inf)), arm=("clip", [0, 1, 2, 3], []))
    if name == "clip_empty":
        v, f = tris(right(2, 2, 28, 28, .5), right(5, 5, 30, 23, .25))
        return dict(_flat_case(name, v, f, 32, 40, z_range=(0.75, 0.25), bg=background(32, 40, 24)), arm=("nothing", [0, 1]))
    if name == "clip_crossing":
        t = [((2, 2, .5), (4, 44, .9), (60, 6, 1.5)), ((60, 44, -1.5), (58, 3, -.6), (3, 40, -.8)), right(1, 1, 50, 40, 1.0)]
        v, f = tris(*t)
        return dict(_flat_case(name, v, f, 48, 64, bg=background(48, 64, 25)), arm=("crossing", [0, 1]))
    if name == "clip_nan_inf_z":
        t = [((2, 2, .5), (2, 30, np.nan), (30, 2, .5)), ((20, 4, .2), (20, 30, .2), (50, 4, np.inf)), right(1, 1, 60, 36, .9)]
        v, f = tris(*t)
        return dict(_flat_case(name, v, f, 40, 64, bg=background(40, 64, 26)), arm=("clip", [2], [0, 1]))
    if name == "neg_zero":
        v, f = tris(right(2, 2, 28, 28, -0.0), right(5, 5, 30, 23, -0.0))
        return dict(_flat_case(name, v, f, 32, 40), arm=("tie", {0}))
    # ---- the hand-over list ----
    if name == "big512":
        v, f = _big512()
        return dict(_flat_case(name, v, f, 64, 64), arm=("big512",))
    if name == "big_straddle":                   # 24 x 30 = 720 pixels of tile (0, 0), 7 x 30 = 210 of tile (0, 1)
        v, f = tris(((40.2, 10.3, .2), (40.4, 39.8, .5), (70.9, 10.1, .3)), ((35, 5, .6), (38, 60, .6), (100, 8, .7)))
        return dict(_flat_case(name, v, f, 66, 129, bg=background(66, 129, 27)), arm=("straddle", 0))
    # ---- seams and extents ----
    if name == "seam_fan":
        v, f = _seam()
        return dict(_flat_case(name, v, f, 130, 130, cull=True, bg=background(130, 130, 28)), arm=("seam",))
    if name.startswith("long_"):
        H, W = (int(t) for t in name[5:].split("x"))
        v, f = _long(H, W)
        return dict(_flat_case(name, v, f, H, W, bg=background(H, W, 29)), arm=("extent",))
    if name == "one_1x1":
        v, f = tris(flat(-3, -2, 0.2, 5, 4, -1, .25), flat(0.6, 0.6, 0.6, 3, 3, 0.6, .1))
        return dict(_flat_case(name, v, f, 1, 1, bg=background(1, 1, 30)), arm=("ids", [0]))
    if name.startswith("narrow_w"):
        W = int(name[8:])
        v, f = tris(((-1, -1, .3), (0.4, 3.4, .5), (W + 0.2, 0.7, .2)), right(W - 1.6, 0.2, 3, 2.4, .1), right(0.3, 1.4, 2, 5, .4))
        return dict(_flat_case(name, v, f, 3, W, bg=background(3, W, 31)), arm=("covered",))
    # ---- the per-mesh bbox skip of scene mode ----
    if name.startswith("scene_skip"):
        v, f = _scene_skip()
        col = np.array([(1, .3, .3), (.3, 1, .3), (.3, .3, 1), (1, 1, .3), (.3, 1, 1)], F32)
        return dict(_flat_case(name, v, f, 130, 129, mode="scene", order=name.rsplit("_", 1)[1], cull=True, colours=col,
                               bg=background(130, 129, 32)), arm=("scene_skip",))
    # ---- cameras and shading ----
    if name.startswith("cam_"):
        v, f = rc.hull(64)
        cam = {"cam_sy_neg": (0.9, -0.9, 0.03, 0.02), "cam_both_neg": (-0.9, -0.85, 0.03, 0.02),
               "cam_sx_zero": (0.0, 0.9, 0.1, 0.0)}
        return dict(_case(name, v, f, cam[name], 64, 64, single=True, bg=background(64, 64, 33), lights=HULL_LIGHT),
                    arm=("nothing", []) if name == "cam_sx_zero" else ("mirror", name == "cam_sy_neg"))
    if name.startswith("shade_"):
        v, f = rc.hull(64)
        kw = {"shade_no_light": dict(lights=np.zeros((0, 4), F32)),
              "shade_four_lights": dict(lights=FOUR_LIGHTS, ambient=0.2),
              "shade_saturated": dict(colours=(3.0, 2.0, 1.5), ambient=0.6),
              "shade_negative": dict(colours=(-0.5, 1.0, 0.5)),
              "shade_behind": dict(lights=np.array([[0.0, 0.0, 1.0, 0.9]], F32), ambient=0.0)}[name]
        bg = 1 + background(33, 47, 34) % 255                           # (no zero byte: a black pixel is a covered one)
        return dict(_case(name, v, f, (0.93, 0.97, 0.021, -0.013), 33, 47, single=True, bg=bg, **kw), arm=("shade", name[6:]))
    # ---- status ----
    if name == "status_b3_mesh1":
        v = np.array([(30, 20, .1), (90, 40, .2), (70, 60, .4), (10, 10, 0), (60, 15, 0), (20, 50, 0)], F32)
        vs = np.stack([v, v, v])
        vs[1, 1, 0] = 1.0e6
        return dict(_case(name, vs, [(0, 1, 2), (3, 4, 5)], pixel_cam(128, 64), 64, 128, cull=False), arm=("status", [0, 1, 0]))
    if name == "status_unreferenced":
        v = np.array([(30, 20, .1), (90, 40, .2), (70, 60, .4), (-3.0e6, 10, 0)], F32)
        return dict(_case(name, v, [(0, 1, 2)], pixel_cam(128, 64), 64, 128, cull=False), arm=("status", [0]))
    if name == "status_both_bits":
        v = np.array([(30, 20, .1), (90, 40, .2), (70, 60, .4), (10, -1.0e7, 0), (60, 15, 0), (20, 50, 0)], F32)
        return dict(_case(name, v, [(0, 1, 2), (3, 4, 5), (0, 1, 6), (2, -1, 1)], pixel_cam(128, 64), 64, 128, cull=False),
                    arm=("status", [3]), cls=False)
    raise KeyError(name)


CASE_NAMES = (["tie_two", "tie_three", "tie_duplicate", "tie_steps_low_wins", "tie_steps_high_nearer", "tie_big_small",
               "tie_small_big"]
              + [f"{s}_{o}" for s in ("scene_identical", "scene_255", "scene_rank_vs_face") for o in ("depth", "list")]
              + ["key_65836", "key_2p20", "clip_planes", "clip_infinite", "clip_empty", "clip_crossing", "clip_nan_inf_z",
                 "neg_zero", "big512", "big_straddle", "seam_fan", "long_8192x3", "long_2x8192", "one_1x1", "narrow_w4",
                 "narrow_w5", "narrow_w7", "narrow_w8", "scene_skip_list", "scene_skip_depth", "cam_sy_neg", "cam_both_neg",
                 "cam_sx_zero", "shade_no_light", "shade_four_lights", "shade_saturated", "shade_negative", "shade_behind",
                 "status_b3_mesh1", "status_unreferenced", "status_both_bits"])


def any_case(name):
    """A case of this table or of tests/render_cases.py."""
    return case(name) if name in CASE_NAMES else rc.case(name)


def reference(name):
    """render_ref.render_case_exact of a case of either table with the yardstick's own snapped coordinates, computed once per
    session and shared (callers must not modify it)."""
    import render_ref
    if name not in _ref_cache:
        _ref_cache[name] = render_ref.render_case_exact(any_case(name))
    return _ref_cache[name]
