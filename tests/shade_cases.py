"""The case table shared by tests/test_shade_cpu.py (the yardstick's own audit) and tests/test_gpu_shade.py (the kernels of
csrc/shade.hip).  The smallest shapes at which each arm can go wrong; the builders and the posed MANO mesh are render_cases'.

A shading case is a dict: name, c (a render case: verts, faces, cam, H, W, mode, order, cull, colours, background, lights,
ambient), smooth (interpolated vertex normals), vertex_colours (None | [B, nv, 3] | [nv, 3]), attrs (None | [B, nv, C]), wire
(None | (T, rgb, only)), attr_fill.  A normals case is a dict: name, verts [B, nv, 3], faces, ptr, idx (the vertex-to-face table,
possibly broken on purpose), status (what every mesh must report) and zero (vertices whose normal must be (0, 0, 0)).

What is where:
  tri16                  one triangle, attributes = the 3 x 3 identity: attr_out must equal bary
  hull_*                 a 48-vertex convex hull at 64 x 64, B = 3, three different cameras, the second mirrored (sx < 0); culled
                         and not (back faces: the normal flips), flat and smooth, mesh colours and vertex colours (per mesh, shared)
  mano_smooth            render_cases' posed MANO mesh, smooth
  scene_two              scene mode, two overlapping hulls in list order with their own cameras; attributes = the mesh's own
                         vertex positions, so a pixel that took the other mesh's vertices or camera shows
  edge_1x1, _17x33, _65x64   launch edges: one pixel; a 99-byte row (byte stores, a lane with one pixel); a row of 16 lanes + the
                         next image row in the same wave; C = 1, 3, 16
  wire_*                 an axis-aligned right triangle on whole pixels in a 32 x 32 image: the centres of column 3 lie at distance
                         exactly 1.5 pixel = 384 / 256 from the edge x = 2 (and those of row 3 from the edge y = 2): on the wire at
                         T = 384, off at T = 383; T = 0; wire_only"""
import numpy as np

import render_cases as rc
from render_cases import _case, background, pixel_cam

F32 = np.float32
HULL_NV = 48
TIE_T = 384
WIRE_RGB = (250, 20, 30)


def _hull_b3(cull):
    v, f = rc.hull(HULL_NV)
    rng = np.random.default_rng(HULL_NV)
    vs = np.stack([v, v * 0.7 + F32(0.05), v[:, [1, 2, 0]] * 0.85])
    cam = np.array([(0.9, 0.9, 0.03, -0.02), (-1.1, 0.8, -0.2, 0.1), (0.7, 1.2, 0.15, 0.3)], F32)
    # without culling a closed hull still hides its back faces behind the front ones: zmin cuts the near cap off, so that the
    # inside of the far half shows (back faces) within a ring of front faces
    return _case("hull_b3", vs, f, cam, 64, 64, cull=cull, colours=rng.uniform(0.2, 1.0, (3, 3)), bg=background(64, 64, 7, 3),
                 lights=rc.TWO_LIGHTS, z_range=(-1.0, 1.0) if cull else (-0.3, 1.0))


def _hull_one(H, W, seed):
    v, f = rc.hull(HULL_NV)
    return _case("hull_one", v, f, (0.93, 0.97, 0.021, -0.013), H, W, bg=background(H, W, seed), lights=rc.TWO_LIGHTS)


def _wire_tri():
    v = np.array([(2, 2, 0.1), (26, 2, 0.25), (2, 26, -0.15)], F32)      # (tilted: a head-on face has I = 1 exactly)
    return _case("wire_tri", v, [(0, 1, 2)], pixel_cam(32, 32), 32, 32, cull=False, bg=background(32, 32, 9),
                 colours=(0.8, 0.55, 0.37))


def _shade(name, c, smooth=False, vertex_colours=None, attrs=None, wire=None, attr_fill=0.0):
    return dict(name=name, c=c, smooth=smooth, vertex_colours=vertex_colours, attrs=attrs, wire=wire, attr_fill=attr_fill)


def _attrs(c, C, seed):
    B, nv = c["verts"].shape[:2]
    return np.random.default_rng(seed).uniform(-2.0, 2.0, (B, nv, C)).astype(F32)


_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]


def _build(name):
    if name == "tri16":
        v = np.array([(1.3, 2.1, 0.1), (14.2, 4.4, -0.2), (5.6, 13.7, 0.3)], F32)
        c = _case(name, v, [(0, 1, 2)], pixel_cam(16, 16), 16, 16, cull=False, bg=background(16, 16, 8))
        return _shade(name, c, attrs=np.eye(3, dtype=F32)[None], attr_fill=-1.0)
    if name.startswith("hull_"):                 # hull_<cull|nocull>_<flat|smooth>_<col|vcol|vcolshared>
        _, cull, shading, colour = name.split("_")
        c = _hull_b3(cull == "cull")
        rng = np.random.default_rng(len(name))
        vc = None if colour == "col" else rng.uniform(0.1, 1.0, (3, HULL_NV, 3) if colour == "vcol" else (HULL_NV, 3)).astype(F32)
        return _shade(name, c, smooth=shading == "smooth", vertex_colours=vc,
                      attrs=_attrs(c, 3, 5) if name == "hull_nocull_smooth_vcol" else None)
    if name == "mano_smooth":
        # (ambient 0.31: at render_cases' 0.3 a pixel that no light reaches has 255 x 0.3f + 0.5 = 77 + 3e-7, on a boundary)
        return _shade(name, dict(rc.case("mano_posed"), ambient=0.31), smooth=True)
    if name == "scene_two":
        v, f = rc.hull(HULL_NV)
        vs = np.stack([v * 0.5 + np.array(o, F32) for o in ((-0.15, 0.0, 0.3), (0.1, 0.1, -0.3))])
        cam = np.array([(0.9, 0.9, 0.0, 0.0), (0.8, 1.0, 0.1, -0.05)], F32)
        c = _case(name, vs, f, cam, 64, 80, mode="scene", order="list", colours=[(1, 0.3, 0.3), (0.3, 1, 0.3)],
                  bg=background(64, 80, 4), lights=rc.TWO_LIGHTS)
        vc = np.random.default_rng(3).uniform(0.1, 1.0, (2, HULL_NV, 3)).astype(F32)
        return _shade(name, c, smooth=True, vertex_colours=vc, attrs=vs.copy(), attr_fill=7.0)
    if name == "edge_1x1":
        c = _hull_one(1, 1, 21)
        return _shade(name, c, smooth=True, attrs=_attrs(c, 1, 1))
    if name == "edge_17x33":
        c = _hull_one(17, 33, 22)
        return _shade(name, c, smooth=True, attrs=_attrs(c, 3, 2), wire=(96, WIRE_RGB, False))
    if name == "edge_65x64":
        c = _hull_one(65, 64, 23)
        return _shade(name, c, smooth=True, attrs=_attrs(c, 16, 3))
    if name.startswith("wire_"):
        wire = {"wire_tie": (TIE_T, WIRE_RGB, False), "wire_tie_minus": (TIE_T - 1, WIRE_RGB, False),
                "wire_off": (0, WIRE_RGB, False), "wire_only": (TIE_T, WIRE_RGB, True)}[name]
        return _shade(name, _wire_tri(), wire=wire)
    raise KeyError(name)


HULL_NAMES = ["hull_cull_flat_col", "hull_cull_smooth_col", "hull_cull_flat_vcol", "hull_cull_smooth_vcolshared",
              "hull_nocull_flat_col", "hull_nocull_smooth_col", "hull_nocull_smooth_vcol", "hull_nocull_flat_vcolshared"]
WIRE_NAMES = ["wire_tie", "wire_tie_minus", "wire_off", "wire_only"]
EDGE_NAMES = ["edge_1x1", "edge_17x33", "edge_65x64"]
CASE_NAMES = ["tri16"] + HULL_NAMES + ["mano_smooth", "scene_two"] + EDGE_NAMES + WIRE_NAMES
# flat, mesh colours, no wire: the image must be the rasteriser's own
PLAIN_RENDER_CASES = ["tri_small", "top_left", "odd_faces", "hull64_65x31_b3", "hull64_33x47_b3_nocull", "scene_list", "mirror_cam"]


def hand_made(c):
    """Visibility buffers no rasteriser wrote, for the render case c -> {name: (face_id, mesh_id)}: nothing covered; ids that
    name no face or no mesh next to a few that do (a pixel outside its face has a negative weight: still defined)."""
    B, nf, H, W = c["verts"].shape[0], len(c["faces"]), c["H"], c["W"]
    n = 1 if c["mode"] == "scene" else B
    none = np.full((n, H, W), -1, np.int32)
    f, m = none.copy(), none.copy()
    f[0, 0, 0], m[0, 0, 0] = nf, 0
    f[0, 0, 1], m[0, 0, 1] = 0, B
    f[0, 0, 2], m[0, 0, 2] = 0, -1
    f[0, 1, 1], m[0, 1, 1] = 0, 0
    f[0, H // 2, W // 2], m[0, H // 2, W // 2] = nf - 1, 0
    f[n - 1, H - 1, W - 1], m[n - 1, H - 1, W - 1] = 1 << 30, 0
    return {"all_background": (none, none.copy()), "bad_ids": (f, m)}


# ---- vertex normals --------------------------------------------------------------------------------------------------------
def _normals_case(name, verts, faces, status, zero=(), ptr=None, idx=None):
    import shade_ref
    verts = np.asarray(verts, F32)
    verts = verts[None] if verts.ndim == 2 else verts
    faces = np.ascontiguousarray(faces, np.int64)
    if ptr is None:
        ok = ((faces >= 0) & (faces < verts.shape[1])).all(1)
        ptr, idx = shade_ref.vertex_face_table(np.where(ok[:, None], faces, 0), verts.shape[1])
    return dict(name=name, verts=verts, faces=faces, ptr=np.asarray(ptr, np.int32), idx=np.asarray(idx, np.int32), status=status,
                zero=list(zero))


def normals_case(name):
    if ("n", name) not in _cache:
        _cache[("n", name)] = _build_normals(name)
    return _cache[("n", name)]


def _build_normals(name):
    import shade_ref
    v, f = rc.hull(HULL_NV)
    if name == "hull_b3":                        # the batch of the hull cases; holds the vertex with the most faces
        return _normals_case(name, _hull_b3(True)["verts"], f, 0)
    if name == "isolated":
        return _normals_case(name, np.concatenate([v, [[0.1, 0.2, 0.3]]]), f, 1, zero=[HULL_NV])
    if name == "cancel":
        return _normals_case(name, v[:3], [(0, 1, 2), (0, 2, 1)], 1, zero=[0, 1, 2])
    if name == "zero_area":                      # a face that names a vertex twice: its cross product is exactly zero
        return _normals_case(name, v, np.concatenate([f, [[f[0, 0], f[0, 0], f[0, 1]]]]), 0)
    if name == "nan":
        vn = v.copy()
        vn[5] = np.nan
        ring = np.unique(f[(f == 5).any(1)])
        return _normals_case(name, vn, f, 1, zero=ring.tolist())
    if name == "bad_table":                      # entries that name no face: skipped, status bit 1
        ptr, idx = shade_ref.vertex_face_table(f, HULL_NV)
        idx = idx.copy()
        idx[ptr[3]], idx[ptr[7] + 1] = len(f), -1
        return _normals_case(name, v, f, 2, ptr=ptr, idx=idx)
    if name == "bad_range":                      # a vertex whose table range leaves the table: nothing read, zero normal
        ptr, idx = shade_ref.vertex_face_table(f, HULL_NV)
        ptr = ptr.copy()
        ptr[HULL_NV] = len(idx) + 5
        return _normals_case(name, v, f, 3, zero=[HULL_NV - 1], ptr=ptr, idx=idx)
    if name == "bad_face":                       # a face with an index outside [0, nv): contributes nothing, status bit 1
        fb = f.copy()
        fb[2, 1] = HULL_NV
        ptr, idx = shade_ref.vertex_face_table(f, HULL_NV)
        return _normals_case(name, v, fb, 2, ptr=ptr, idx=idx)
    raise KeyError(name)


NORMALS_NAMES = ["hull_b3", "isolated", "cancel", "zero_area", "nan", "bad_table", "bad_range", "bad_face"]

# ---- shared references (computed once per session; callers must not modify them) --------------------------------------------
_ref_cache = {}


def visibility(c):
    """(face_id, mesh_id) int32 [n, H, W] of a render case by render_ref's device-exact rasteriser."""
    import render_ref
    key = ("vis", id(c))
    if key not in _ref_cache:
        ims = render_ref.render_case_exact(c)
        _ref_cache[key] = (np.stack([im["face_id"] for im in ims]), np.stack([im["mesh_id"] for im in ims]), c)
    return _ref_cache[key][:2]


def normals_of(c):
    """The yardstick's vertex normals of a render case's meshes [B, nv, 3]."""
    import shade_ref
    key = ("nrm", id(c))
    if key not in _ref_cache:
        ptr, idx = shade_ref.vertex_face_table(c["faces"], c["verts"].shape[1])
        _ref_cache[key] = (np.stack([shade_ref.vertex_normals(v, c["faces"], ptr, idx)[0] for v in c["verts"]]), c)
    return _ref_cache[key][0]


def reference(name):
    """shade_ref.shade of a shading case on the yardstick's own visibility buffer and normals."""
    import shade_ref
    if name not in _ref_cache:
        s = case(name)
        fid, mid = visibility(s["c"])
        _ref_cache[name] = shade_ref.shade(s["c"], fid, mid, vertex_colours=s["vertex_colours"],
                                           normals=normals_of(s["c"]) if s["smooth"] else None, attrs=s["attrs"], wire=s["wire"],
                                           attr_fill=s["attr_fill"])
    return _ref_cache[name]
