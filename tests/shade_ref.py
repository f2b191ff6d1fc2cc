"""The yardstick of the shading pass (csrc/shade.hip, include/p2m.h: p2m_vertex_normals, p2m_mesh_shade), in numpy: the header
comment restated.  The float64 parts are float64 with the header's operation order, the fp32 parts np.float32 operations with
render_ref.fma32 for the fused steps, the wire test Python integers.  Projection, snap, the edge convention and the flat face
values are render_ref's (imported, not copied); the visibility buffer is an INPUT, so every pixel is decided.

What is bit for bit and what is not.  normals, bary, attr_out, the wire mask, covered / background and the status bits are exact
restatements: a test compares them bitwise.  The image's shaded bytes are floor(v) of v = 255 min(1, c I) + 0.5 in float64; the
device forms the same v, but where it shares the rasteriser's code (the flat intensity, the final 255 x + 0.5) that code may
contract a product and a sum into one fma, which numpy does not: the two values of v differ by a few 1e-14 at most (v <= 255.5,
relative error of a handful of roundings at 2^-53).  So `v` is returned and a test allows one LSB exactly where v lies within
1e-4 of an integer - render_ref's rule and constant.

The flat intensity alone (needed with vertex colours, and as the fall-back of a vanishing interpolated normal) is recovered from
render_ref.face_values with the colour 2^-8 per channel: v = 255 (2^-8 I) + 0.5 is never clipped for I < 256, and
I = (v - 0.5) / 255 * 2^8 undoes it with three roundings (the scaling by 2^-8 is exact): relative error below 4 x 2^-53, inside
the 1e-14 above."""
import numpy as np

import render_ref as rr

STATUS_DEGENERATE, STATUS_BAD_INDEX = 1, 2
NEAR = 1e-4                                              # test_gpu_render.py's constant
MAX_WIRE = 1 << 16


def vertex_face_table(faces, nv):
    """(ptr int32 [nv + 1], idx int32): per vertex the ids of its incident faces, ascending."""
    lists = [[] for _ in range(nv)]
    for f, tri in enumerate(np.asarray(faces)):
        for i in sorted(set(int(t) for t in tri)):
            lists[i].append(f)
    ptr = np.zeros(nv + 1, np.int32)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    return ptr, np.array([f for l in lists for f in l], np.int32)


def vertex_normals(verts, faces, ptr, idx):
    """verts [nv, 3] float32 of one mesh -> (normals float32 [nv, 3], status).  float64, table order, one rounding per operation."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    faces = np.asarray(faces, np.int64)
    nv, nf = len(v), len(faces)
    out = np.zeros((nv, 3), np.float32)
    status = 0
    with np.errstate(all="ignore"):
        for i in range(nv):
            e0, e1 = int(ptr[i]), int(ptr[i + 1])
            if e0 < 0 or e1 > len(idx) or e0 > e1:
                status |= STATUS_BAD_INDEX
                e0 = e1 = 0
            n = np.zeros(3)
            for f in idx[e0:e1]:
                if not 0 <= f < nf or (faces[f] < 0).any() or (faces[f] >= nv).any():
                    status |= STATUS_BAD_INDEX
                    continue
                p0, p1, p2 = v[faces[f]]
                a, b = p1 - p0, p2 - p0
                n = n + np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
            q = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            if q > 0 and np.isfinite(q):
                out[i] = (n / np.sqrt(q)).astype(np.float32)
            else:
                status |= STATUS_DEGENERATE
    return out, status


def face_intensity(verts, faces, lights, ambient):
    """The rasteriser's I per face, recovered from render_ref.face_values (module docstring)."""
    c = np.float32(2.0 ** -8)
    return (rr.face_values(verts, faces, (c, c, c), lights, ambient)[:, 0] - 0.5) / 255.0 * 256.0


def edges_at(xy, tri, px, py):
    """xy int64 [P, 3, 2] of the three vertices, pixel centres px, py int64 [P] -> (area2, s, A, Bc, E), A / Bc / E [P, 3] for the
    edges k = 0: v0 -> v1, 1: v1 -> v2, 2: v2 -> v0, in render_ref.rasterise's convention."""
    X, Y = xy[..., 0], xy[..., 1]
    area2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
    s = np.where(area2 > 0, 1, -1).astype(np.int64)
    A, Bc, E = (np.zeros((len(X), 3), np.int64) for _ in range(3))
    for k in range(3):
        a, b = k, (k + 1) % 3
        A[:, k], Bc[:, k] = -s * (Y[:, b] - Y[:, a]), s * (X[:, b] - X[:, a])
        E[:, k] = A[:, k] * (px - X[:, a]) + Bc[:, k] * (py - Y[:, a])
    return area2, s, A, Bc, E


def wire_mask(E, A, Bc, T):
    """E_k^2 <= T^2 (A_k^2 + B_k^2) for some k, in Python integers."""
    Eo, Ao, Bo = (np.asarray(t, np.int64).astype(object) for t in (E, A, Bc))
    hit = (Eo * Eo) <= int(T) * int(T) * (Ao * Ao + Bo * Bo)
    return np.asarray(hit, bool).any(1)


def shade(c, face_id, mesh_id, colours=True, vertex_colours=None, normals=None, attrs=None, wire=None, attr_fill=0.0,
          xy_fix=None):
    """c: a case of tests/render_cases.py (verts, faces, cam, H, W, mode, colours, background, lights, ambient).  face_id, mesh_id
    int32 [n, H, W].  vertex_colours [B, nv, 3] or [nv, 3] (then c's colours are not used), normals [B, nv, 3] or None (flat),
    attrs [B, nv, C], wire (T, rgb, only) or None, xy_fix [B, nv, 2]: snapped coordinates to use instead of render_ref.project's.
    -> dict(image uint8 [n, H, W, 3], v float64 (NaN where nothing was shaded), bary float32, attr float32 or None, wire bool,
    covered bool, status int32 [B])."""
    verts = np.asarray(c["verts"], np.float32)
    faces = np.asarray(c["faces"], np.int64)
    B, nv, nf, H, W = verts.shape[0], verts.shape[1], len(faces), c["H"], c["W"]
    n = face_id.shape[0]
    f32, f64 = np.float32, np.float64
    proj = [rr.project(verts[b], c["cam"][b], H, W) for b in range(B)]
    xy = np.stack([p["xy"] for p in proj]) if xy_fix is None else np.asarray(xy_fix, np.int64)
    mirror = np.array([p["mirror"] for p in proj])
    li = np.asarray(c["lights"], np.float32).astype(f64).reshape(-1, 4)
    amb = f64(f32(c["ambient"]))
    face_ok = ((faces >= 0) & (faces < nv)).all(1)
    safe = np.where(face_ok[:, None], faces, 0)
    with np.errstate(all="ignore"):
        I_face = np.stack([face_intensity(verts[b], safe, li.astype(f32), c["ambient"]) for b in range(B)])
        v_face = None
        if vertex_colours is None:
            v_face = np.stack([rr.face_values(verts[b], safe, c["colours"][b], li.astype(f32), c["ambient"]) for b in range(B)])
    vcol = None
    if vertex_colours is not None:
        vcol = np.asarray(vertex_colours, f32).astype(f64)
        vcol = np.broadcast_to(vcol, (B, nv, 3))
    C = 0 if attrs is None else attrs.shape[2]
    bg = c["background"]
    image = np.zeros((n, H, W, 3), np.uint8)
    vout = np.full((n, H, W, 3), np.nan)
    bary = np.zeros((n, H, W, 3), f32)
    attr = None if attrs is None else np.full((n, H, W, C), f32(attr_fill), f32)
    wire_out = np.zeros((n, H, W), bool)
    cov_out = np.zeros((n, H, W), bool)
    status = np.zeros(B, np.int32)
    for k in range(n):
        if bg is not None:
            image[k] = bg if bg.ndim == 3 else bg[k]
        fid, mid = np.asarray(face_id[k], np.int64), np.asarray(mesh_id[k], np.int64)
        named = fid >= 0
        ok = named & (fid < nf) & (mid >= 0) & (mid < B)
        ii, jj = np.nonzero(ok)
        f, m = fid[ii, jj], mid[ii, jj]
        good = face_ok[f]
        tri = safe[f]
        P = xy[m[:, None], tri]                                              # [P, 3, 2]
        px, py = jj.astype(np.int64) * rr.FIX + rr.FIX // 2, ii.astype(np.int64) * rr.FIX + rr.FIX // 2
        area2, s, A, Bc, E = edges_at(P, tri, px, py)
        good &= area2 != 0
        if (named & ~ok).any() or (~good).any():
            status[0] |= STATUS_BAD_INDEX
        ii, jj, f, m, tri, area2, s, A, Bc, E = (t[good] for t in (ii, jj, f, m, tri, area2, s, A, Bc, E))
        cov_out[k, ii, jj] = True
        area = np.abs(area2).astype(f32)
        with np.errstate(all="ignore"):
            l0, l1, l2 = E[:, 1].astype(f32) / area, E[:, 2].astype(f32) / area, E[:, 0].astype(f32) / area
        bary[k, ii, jj] = np.stack([l0, l1, l2], 1)
        if attrs is not None:
            a0, a1, a2 = (np.asarray(attrs, f32)[m, tri[:, t]] for t in range(3))
            with np.errstate(all="ignore"):
                attr[k, ii, jj] = rr.fma32(l2[:, None], a2, rr.fma32(l1[:, None], a1, (l0[:, None] * a0).astype(f32)))
        on = np.zeros(len(f), bool)
        if wire is not None and wire[0] > 0:
            on = wire_mask(E, A, Bc, wire[0])
            wire_out[k, ii, jj] = on
            image[k, ii[on], jj[on]] = np.asarray(wire[1], np.uint8)
        todo = ~on
        if wire is not None and wire[0] > 0 and wire[2]:
            todo[:] = False
        d0, d1, d2 = l0.astype(f64), l1.astype(f64), l2.astype(f64)
        with np.errstate(all="ignore"):
            if vcol is None and normals is None:
                v = v_face[m, f]
            else:
                I = I_face[m, f].copy()
                if normals is not None:
                    nr = np.asarray(normals, f32).astype(f64)
                    n0, n1, n2 = (nr[m, tri[:, t]] for t in range(3))
                    mm = (d0[:, None] * n0 + d1[:, None] * n1) + d2[:, None] * n2
                    q = (mm[:, 0] * mm[:, 0] + mm[:, 1] * mm[:, 1]) + mm[:, 2] * mm[:, 2]
                    use = (q > 0) & np.isfinite(q)
                    u = mm / np.sqrt(q)[:, None]
                    back = np.where(mirror[m], area2 < 0, area2 > 0)
                    u = np.where(back[:, None], -u, u)
                    Is = np.full(len(f), amb)
                    for l in li:
                        d = l[:3] / np.sqrt((l[:3] * l[:3]).sum())
                        dot = (u[:, 0] * d[0] + u[:, 1] * d[1]) + u[:, 2] * d[2]
                        Is = Is + l[3] * np.where(dot > 0, dot, 0.0)
                    I = np.where(use, Is, I)
                if vcol is not None:
                    c0, c1, c2 = (vcol[m, tri[:, t]] for t in range(3))
                    col = (d0[:, None] * c0 + d1[:, None] * c1) + d2[:, None] * c2
                else:
                    col = np.asarray(c["colours"], f32).astype(f64)[m]
                v = 255.0 * np.minimum(1.0, col * I[:, None]) + 0.5
        vout[k, ii[todo], jj[todo]] = v[todo]
        image[k, ii[todo], jj[todo]] = rr.bytes_of(v[todo])
    return dict(image=image, v=vout, bary=bary, attr=attr, wire=wire_out, covered=cov_out, status=status)
