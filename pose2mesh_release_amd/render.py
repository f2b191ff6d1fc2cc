"""Rendering on the GPU: a batched z-buffer rasteriser with flat shading and image overlay (p2m_mesh_render), the device
counterpart of the reference's demo/renderer.py + demo/run.py:24-67 (trimesh, pyrender, OpenGL / EGL, host compositing).

  MeshRenderer           meshes [B, nv, 3] + weak-perspective cameras [B, 4] -> image, mask, face_id, mesh_id, depth, one
                         image per mesh ("batch") or all meshes in one image ("scene")
  crop_cam_to_image      run.py's convert_crop_cam_to_orig_img: the camera of a crop as a camera of the original image
  project_vertices       the snapped 1/256-pixel coordinates of every vertex (p2m_mesh_project)
  vertex_normals         area-weighted unit vertex normals of a batch (p2m_vertex_normals), from a vertex_face_table
  MeshShader             a deferred pass over a MeshRenderer's visibility buffer (p2m_mesh_shade): smooth shading, vertex
                         colours, per-vertex attributes and barycentrics carried to the pixels, wireframe

Geometry follows the reference (px = W/2 (1 + sx (x + tx)), py = H/2 (1 + sy (y + ty)), depth = z, smaller is nearer);
shading is this project's (flat, ambient + up to 4 directional lights), NOT pyrender's metallic-roughness model.  The
definition is the comment of p2m_mesh_render in include/p2m.h, restated in float64 / exact integers in tests/render_ref.py.
Coverage is computed in exact integer arithmetic with the top-left rule, so a mesh is watertight and a render is reproducible
bit for bit.  The camera is an input: the demo's camera fit (optimize_cam_param) is not part of this module.  The launches
allocate and synchronise nothing, so a call can sit in a captured graph.  There is no CPU fallback: CPU tensors raise.
"""
import ctypes as _ct

import numpy as _np
import torch

from . import _lib

STATUS_CLAMPED, STATUS_BAD_INDEX = 1, 2
DEFAULT_LIGHTS = ((0.0, 0.0, -1.0, 0.7),)              # one head-light: the unit vector towards the light, and its k


def _p(t):
    return None if t is None else _ct.c_void_p(t.data_ptr())


def _stream():
    return _ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda(x, name, dtype=torch.float32):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.P2MError(f"{name}: the render kernels need a CUDA tensor (there is no CPU path)")
    return x.contiguous() if x.dtype == dtype else x.to(dtype).contiguous()


def crop_cam_to_image(cam, bbox, img_width, img_height):
    """run.py:24-43, convert_crop_cam_to_orig_img: cam [N, 3] = (s, tx, ty) of the crops, bbox [N, 4] = (x, y, w, h) of the
    crops in the original image -> [N, 4] = (sx, sy, tx, ty) in the original image.  Tensors (any device) or arrays; the
    result is of cam's kind, computed in its dtype."""
    if isinstance(cam, torch.Tensor):
        bbox = torch.as_tensor(bbox, dtype=cam.dtype, device=cam.device)
        stack = lambda v: torch.stack(v, dim=1)                                        # noqa: E731
    else:
        cam, bbox = _np.asarray(cam), _np.asarray(bbox)
        stack = lambda v: _np.stack(v, axis=1)                                         # noqa: E731
    x, y, w, h = bbox[:, 0], bbox[:, 1], bbox[:, 2], bbox[:, 3]
    cx, cy = x + w / 2, y + h / 2
    hw, hh = img_width / 2., img_height / 2.
    sx = cam[:, 0] * (1. / (img_width / h))
    sy = cam[:, 0] * (1. / (img_height / h))
    tx = ((cx - hw) / hw / sx) + cam[:, 1]
    ty = ((cy - hh) / hh / sy) + cam[:, 2]
    return stack([sx, sy, tx, ty])


def project_vertices(verts, cam, height, width):
    """(xy_fix int32 [B, nv, 2], status int32 [B]): every vertex's image position in 1/256-pixel units, as the renderer snaps
    it (include/p2m.h); status bit 0: a coordinate was clamped to +-2^23."""
    v, c = _cuda(verts, "verts"), _cuda(cam, "cam")
    if v.dim() != 3 or v.shape[2] != 3 or tuple(c.shape) != (v.shape[0], 4):
        raise ValueError(f"expected verts [B, nv, 3] and cam [B, 4], got {tuple(v.shape)}, {tuple(c.shape)}")
    B, nv = int(v.shape[0]), int(v.shape[1])
    xy = torch.zeros((B, nv, 2), device=v.device, dtype=torch.int32)
    status = torch.zeros((B,), device=v.device, dtype=torch.int32)
    with torch.cuda.device(v.device):
        _lib.check(_lib.hip().p2m_mesh_project(_p(v), _p(c), B, nv, int(height), int(width), _p(xy), _p(status), _stream()),
                   "p2m_mesh_project")
    return xy, status


class MeshRenderer:
    """r = MeshRenderer(faces, height, width, mode="batch" | "scene", order="list" | "depth", cull=True, ambient=0.3,
                        lights=((0, 0, -1, 0.7),), z_range=(-1.0, 1.0), num_vertex=None)
    out = r(verts [B, nv, 3], cam [B, 4], colours=(1, 1, 0.9) | [B, 3], background=None | uint8 [H, W, 3] | [B, H, W, 3])

    mode   "batch": mesh b is rendered into image b.  "scene": all meshes into one image (at most 255), order "list" - the
           reference's loop over people, a later mesh paints over an earlier one, the nearest fragment within a mesh - or
           "depth", the nearest fragment over all meshes.
    cam    (sx, sy, tx, ty) per mesh: the weak-perspective camera of renderer.py, in the image's own frame
           (crop_cam_to_image takes a crop's camera there).
    lights rows (x, y, z, k): the direction TOWARDS the light in mesh coordinates (the viewer looks along +z, so (0, 0, -1)
           is a head-light) and its weight; up to 4.  I = ambient + sum k max(0, n . l), rgb = floor(255 min(1, colour I) + .5).
    faces  [nf, 3] integer indices, validated against num_vertex here (or, without it, against nv at the first call).

    Returns a dict of device tensors - image uint8 [n, H, W, 3], mask bool [n, H, W], face_id int32 (-1: background), mesh_id
    int32 (the mesh's index in the call, -1: background), depth fp32 (+inf: background), n = B or 1, and status int32 [B]
    (bit 0: a vertex of the mesh was clamped to +-32768 pixels; bit 1: a face index out of range).  They are buffers reused
    per (B, nv), overwritten by the next call of that shape: no allocation after the first call of a shape and no sync."""

    def __init__(self, faces, height, width, mode="batch", order="list", cull=True, ambient=0.3, lights=DEFAULT_LIGHTS,
                 z_range=(-1.0, 1.0), num_vertex=None):
        f = _np.asarray(faces.cpu() if isinstance(faces, torch.Tensor) else faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or not _np.issubdtype(f.dtype, _np.integer):
            raise ValueError(f"faces: expected integer [nf >= 1, 3], got {f.dtype} {f.shape}")
        if mode not in ("batch", "scene") or order not in ("list", "depth"):
            raise ValueError(f"mode: batch | scene, order: list | depth; got {mode!r}, {order!r}")
        self.faces_host = _np.ascontiguousarray(f.astype(_np.int64))
        self.nf = int(f.shape[0])
        self._checked_nv = None
        if num_vertex is not None:
            self._check_faces(int(num_vertex))
        self.height, self.width, self.mode, self.order, self.cull = int(height), int(width), mode, order, bool(cull)
        self.ambient = float(ambient)
        li = _np.asarray(lights, dtype=_np.float32).reshape(-1, 4) if len(lights) else _np.zeros((0, 4), _np.float32)
        self.lights = li
        self._lights = (_ct.c_float * max(1, li.size))(*li.reshape(-1).tolist())
        self.z_range = (float(z_range[0]), float(z_range[1]))
        self.flags = (1 if self.cull else 0) | (2 if order == "depth" else 0)
        self._dev = None
        self._bufs = {}

    def _check_faces(self, nv):
        if self._checked_nv != nv:
            lo, hi = int(self.faces_host.min()), int(self.faces_host.max())
            if lo < 0 or hi >= nv:
                raise ValueError(f"faces: indices must lie in [0, {nv}), got [{lo}, {hi}]")
            self._checked_nv = nv

    def _buffers(self, B, nv, dev):
        if self._dev != dev:
            self._dev, self._bufs = dev, {}
            self._faces = torch.from_numpy(self.faces_host.astype(_np.int32)).to(dev)
        b = self._bufs.get((B, nv))
        if b is None:
            mode = 1 if self.mode == "scene" else 0
            n = _ct.c_int64(0)
            _lib.check(_lib.hip().p2m_mesh_render_workspace(B, self.nf, self.height, self.width, mode, _ct.byref(n)),
                       "p2m_mesh_render_workspace")
            ni, H, W = (1 if mode else B), self.height, self.width
            b = {"image": torch.zeros((ni, H, W, 3), device=dev, dtype=torch.uint8),
                 "mask": torch.zeros((ni, H, W), device=dev, dtype=torch.bool),
                 "face_id": torch.full((ni, H, W), -1, device=dev, dtype=torch.int32),
                 "mesh_id": torch.full((ni, H, W), -1, device=dev, dtype=torch.int32),
                 "depth": torch.full((ni, H, W), float("inf"), device=dev, dtype=torch.float32),
                 "status": torch.zeros((B,), device=dev, dtype=torch.int32),
                 "colours": torch.zeros((B, 3), device=dev, dtype=torch.float32),
                 "ws": torch.zeros((max(int(n.value), 16),), device=dev, dtype=torch.uint8)}
            self._bufs[(B, nv)] = b
        return b

    @torch.no_grad()
    def __call__(self, verts, cam, colours=(1.0, 1.0, 0.9), background=None):
        v, c = _cuda(verts, "verts"), _cuda(cam, "cam")
        if v.dim() != 3 or v.shape[2] != 3 or tuple(c.shape) != (v.shape[0], 4):
            raise ValueError(f"expected verts [B, nv, 3] and cam [B, 4], got {tuple(v.shape)}, {tuple(c.shape)}")
        B, nv = int(v.shape[0]), int(v.shape[1])
        self._check_faces(nv)
        H, W = self.height, self.width
        scene = self.mode == "scene"
        bg, per_mesh = None, 0
        if background is not None:
            bg = _cuda(background, "background", torch.uint8)
            if tuple(bg.shape) == (B, H, W, 3) and not scene:
                per_mesh = 1
            elif tuple(bg.shape) != (H, W, 3):
                raise ValueError(f"background: expected uint8 [{H}, {W}, 3]" + ("" if scene else f" or [{B}, {H}, {W}, 3]")
                                 + f", got {tuple(bg.shape)}")
        buf = self._buffers(B, nv, v.device)
        if isinstance(colours, torch.Tensor):
            col = _cuda(colours, "colours")
            if tuple(col.shape) not in ((3,), (B, 3)):
                raise ValueError(f"colours: expected [3] or [{B}, 3], got {tuple(col.shape)}")
            buf["colours"].copy_(col.expand(B, 3))
            buf["colours_key"] = None
            col = buf["colours"]
        else:
            ch = _np.asarray(colours, dtype=_np.float32)
            if ch.shape not in ((3,), (B, 3)):
                raise ValueError(f"colours: expected [3] or [{B}, 3], got {ch.shape}")
            key = ch.tobytes()
            if buf.get("colours_key") != key:           # (a host-to-device copy only when the values change)
                buf["colours"].copy_(torch.from_numpy(_np.ascontiguousarray(_np.broadcast_to(ch, (B, 3)))))
                buf["colours_key"] = key
            col = buf["colours"]
        with torch.cuda.device(v.device):
            _lib.check(_lib.hip().p2m_mesh_render(
                _p(v), _p(self._faces), self.nf, _p(c), _p(col), self._lights, len(self.lights), self.ambient, self.z_range[0],
                self.z_range[1], self.flags if scene else self.flags & 1, _p(bg), per_mesh, B, nv, H, W, 1 if scene else 0,
                _p(buf["image"]), _p(buf["face_id"]), _p(buf["mesh_id"]), _p(buf["depth"]), _p(buf["status"]), _p(buf["ws"]),
                _stream()), "p2m_mesh_render")
        torch.ge(buf["face_id"], 0, out=buf["mask"])
        return {k: buf[k] for k in ("image", "mask", "face_id", "mesh_id", "depth", "status")}


STATUS_DEGENERATE = 1                                  # vertex_normals: a zero or non-finite normal (status bit 0)


class VertexFaceTable:
    """vertex_face_table(faces, num_vertex): for each vertex the ids of its incident faces, ascending, as a CSR (ptr int32
    [nv + 1], idx int32 [3 nf]), built once per face list with numpy and kept on the device it is first used on."""

    def __init__(self, faces, num_vertex):
        f = _np.asarray(faces.cpu() if isinstance(faces, torch.Tensor) else faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or not _np.issubdtype(f.dtype, _np.integer):
            raise ValueError(f"faces: expected integer [nf >= 1, 3], got {f.dtype} {f.shape}")
        f = f.astype(_np.int64)
        nv = int(num_vertex)
        if int(f.min()) < 0 or int(f.max()) >= nv:
            raise ValueError(f"faces: indices must lie in [0, {nv}), got [{int(f.min())}, {int(f.max())}]")
        self.nv, self.nf = nv, int(f.shape[0])
        # one entry per (face, vertex) pair, a face that names a vertex twice listed once; sorted by vertex, then face id
        pairs = _np.unique(_np.stack([f.reshape(-1), _np.repeat(_np.arange(self.nf), 3)], 1), axis=0)
        self.ptr_host = _np.zeros(nv + 1, _np.int32)
        _np.cumsum(_np.bincount(pairs[:, 0], minlength=nv), out=self.ptr_host[1:])
        self.idx_host = _np.ascontiguousarray(pairs[:, 1].astype(_np.int32))
        self.faces_host = _np.ascontiguousarray(f.astype(_np.int32))
        self._dev = None

    def on(self, dev):
        if self._dev != dev:
            self._dev = dev
            self.faces, self.ptr, self.idx = (torch.from_numpy(a).to(dev) for a in (self.faces_host, self.ptr_host, self.idx_host))
        return self


def vertex_face_table(faces, num_vertex):
    return VertexFaceTable(faces, num_vertex)


@torch.no_grad()
def vertex_normals(verts, faces, out=None, status=None):
    """(normals fp32 [B, nv, 3], status int32 [B]): the area-weighted unit normal of every vertex (include/p2m.h,
    p2m_vertex_normals); a vertex without a normal (isolated, cancelling faces, NaN) gets (0, 0, 0) and status bit 0.
    faces: an integer [nf, 3] array or, to build the table once, a vertex_face_table(faces, nv).  out / status: buffers to write."""
    v = _cuda(verts, "verts")
    if v.dim() != 3 or v.shape[2] != 3:
        raise ValueError(f"expected verts [B, nv, 3], got {tuple(v.shape)}")
    B, nv = int(v.shape[0]), int(v.shape[1])
    t = faces if isinstance(faces, VertexFaceTable) else VertexFaceTable(faces, nv)
    if t.nv != nv:
        raise ValueError(f"the vertex-to-face table was built for {t.nv} vertices, verts has {nv}")
    t.on(v.device)
    normals = torch.empty((B, nv, 3), device=v.device, dtype=torch.float32) if out is None else out
    st = torch.zeros((B,), device=v.device, dtype=torch.int32) if status is None else status
    with torch.cuda.device(v.device):
        _lib.check(_lib.hip().p2m_vertex_normals(_p(v), _p(t.faces), _p(t.ptr), _p(t.idx), int(t.idx.numel()), B, nv, t.nf,
                                                 _p(normals), _p(st), _stream()), "p2m_vertex_normals")
    return normals, st


class MeshShader:
    """s = MeshShader(renderer, smooth=False, wire=None | (half_width_px, (r, g, b), only), attr_fill=0.0)
    res = s(out, verts, cam, colours=(1, 1, 0.9) | [B, 3]  or  vertex_colours=[B, nv, 3] | [nv, 3], normals=None | [B, nv, 3],
            attributes=None | [B, nv, C <= 16], background=None, bary=False, in_place=True)

    A second pass over `out`, the dict the renderer returned for the same verts and cam: every covered pixel is shaded from its
    own face (include/p2m.h, p2m_mesh_shade).  Faces, image size, mode, lights and ambient are the renderer's, so the two cannot
    disagree.  smooth=True interpolates vertex normals (computed here with p2m_vertex_normals unless `normals` is given);
    vertex_colours are interpolated over the face; wire draws the visible faces' edges, half_width_px wide on each side (in
    steps of 1 / 256 pixel), over the shading or - only=True - over the background.  attributes are any per-vertex floats carried
    to the pixels with the face's barycentric weights (`attr_fill` off the mesh); bary=True returns the weights themselves.

    Returns a dict: image uint8 [n, H, W, 3] - the renderer's own buffer unless in_place=False -, status int32 [B] (bit 1: a
    pixel of a hand-made buffer named no face), and when asked for bary fp32 [n, H, W, 3], attributes fp32 [n, H, W, C],
    normals [B, nv, 3] with normals_status (bit 0: a vertex without a normal).  Buffers are reused per shape; no allocation
    after the first call of a shape and no sync (capturable)."""

    def __init__(self, renderer, smooth=False, wire=None, attr_fill=0.0):
        self.renderer, self.smooth, self.attr_fill = renderer, bool(smooth), float(attr_fill)
        self.wire_T, self.wire_only = 0, 0
        self._wire_rgb = (_ct.c_uint8 * 3)(0, 0, 0)
        if wire is not None:
            width, rgb, only = wire
            T = int(round(float(width) * 256))
            if not 0 < T <= 1 << 16:
                raise ValueError(f"wire: the half width must lie in (0, 256] pixels, got {width}")
            rgb = [int(c) for c in rgb]
            if len(rgb) != 3 or min(rgb) < 0 or max(rgb) > 255:
                raise ValueError(f"wire: rgb must be three bytes, got {rgb}")
            self.wire_T, self.wire_only, self._wire_rgb = T, int(bool(only)), (_ct.c_uint8 * 3)(*rgb)
        self._table = None
        self._bufs = {}

    def _buffers(self, key, n, B, nv, C, dev):
        b = self._bufs.get(key)
        if b is None:
            H, W = self.renderer.height, self.renderer.width
            b = {"status": torch.zeros((B,), device=dev, dtype=torch.int32),
                 "colours": torch.zeros((B, 3), device=dev, dtype=torch.float32)}
            if self.smooth:
                b["normals"] = torch.zeros((B, nv, 3), device=dev, dtype=torch.float32)
                b["normals_status"] = torch.zeros((B,), device=dev, dtype=torch.int32)
            if C:
                b["attributes"] = torch.zeros((n, H, W, C), device=dev, dtype=torch.float32)
            self._bufs[key] = b
        return b

    @torch.no_grad()
    def __call__(self, out, verts, cam, colours=None, vertex_colours=None, normals=None, attributes=None, background=None,
                 bary=False, in_place=True):
        r = self.renderer
        v, c = _cuda(verts, "verts"), _cuda(cam, "cam")
        if v.dim() != 3 or v.shape[2] != 3 or tuple(c.shape) != (v.shape[0], 4):
            raise ValueError(f"expected verts [B, nv, 3] and cam [B, 4], got {tuple(v.shape)}, {tuple(c.shape)}")
        B, nv = int(v.shape[0]), int(v.shape[1])
        r._check_faces(nv)
        H, W, scene = r.height, r.width, r.mode == "scene"
        n = 1 if scene else B
        fid, mid = _cuda(out["face_id"], "face_id", torch.int32), _cuda(out["mesh_id"], "mesh_id", torch.int32)
        if tuple(fid.shape) != (n, H, W) or tuple(mid.shape) != (n, H, W):
            raise ValueError(f"face_id / mesh_id: expected [{n}, {H}, {W}], got {tuple(fid.shape)}, {tuple(mid.shape)}")
        if colours is not None and vertex_colours is not None:
            raise ValueError("colours or vertex_colours, not both")
        bg, per_mesh = None, 0
        if background is not None:
            bg = _cuda(background, "background", torch.uint8)
            if tuple(bg.shape) == (B, H, W, 3) and not scene:
                per_mesh = 1
            elif tuple(bg.shape) != (H, W, 3):
                raise ValueError(f"background: expected uint8 [{H}, {W}, 3]" + ("" if scene else f" or [{B}, {H}, {W}, 3]")
                                 + f", got {tuple(bg.shape)}")
        att, C = None, 0
        if attributes is not None:
            att = _cuda(attributes, "attributes")
            if att.dim() != 3 or tuple(att.shape[:2]) != (B, nv) or not 1 <= att.shape[2] <= 16:
                raise ValueError(f"attributes: expected [{B}, {nv}, 1..16], got {tuple(att.shape)}")
            C = int(att.shape[2])
        dev = v.device
        if r._dev != dev:
            raise ValueError("out: not what this renderer wrote on the device of verts")
        buf = self._buffers((B, nv, C, bool(bary), bool(in_place)), n, B, nv, C, dev)
        if bary and "bary" not in buf:
            buf["bary"] = torch.zeros((n, H, W, 3), device=dev, dtype=torch.float32)
        if in_place:
            image = out["image"]
            if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dtype == torch.uint8 and image.is_contiguous()
                    and tuple(image.shape) == (n, H, W, 3)):
                raise ValueError(f"image: expected a contiguous uint8 device tensor [{n}, {H}, {W}, 3]")
        else:
            if "image" not in buf:
                buf["image"] = torch.zeros((n, H, W, 3), device=dev, dtype=torch.uint8)
            image = buf["image"]
        col, vcol, shared = None, None, 0
        if vertex_colours is not None:
            vcol = _cuda(vertex_colours, "vertex_colours")
            if tuple(vcol.shape) == (nv, 3):
                shared = 1
            elif tuple(vcol.shape) != (B, nv, 3):
                raise ValueError(f"vertex_colours: expected [{B}, {nv}, 3] or [{nv}, 3], got {tuple(vcol.shape)}")
        else:
            colours = (1.0, 1.0, 0.9) if colours is None else colours
            if isinstance(colours, torch.Tensor):
                cc = _cuda(colours, "colours")
                if tuple(cc.shape) not in ((3,), (B, 3)):
                    raise ValueError(f"colours: expected [3] or [{B}, 3], got {tuple(cc.shape)}")
                buf["colours"].copy_(cc.expand(B, 3))
                buf["colours_key"] = None
            else:
                ch = _np.asarray(colours, dtype=_np.float32)
                if ch.shape not in ((3,), (B, 3)):
                    raise ValueError(f"colours: expected [3] or [{B}, 3], got {ch.shape}")
                key = ch.tobytes()
                if buf.get("colours_key") != key:       # (a host-to-device copy only when the values change)
                    buf["colours"].copy_(torch.from_numpy(_np.ascontiguousarray(_np.broadcast_to(ch, (B, 3)))))
                    buf["colours_key"] = key
            col = buf["colours"]
        res = {}
        nrm = None
        if normals is not None:
            nrm = _cuda(normals, "normals")
            if tuple(nrm.shape) != (B, nv, 3):
                raise ValueError(f"normals: expected [{B}, {nv}, 3], got {tuple(nrm.shape)}")
        elif self.smooth:
            if self._table is None or self._table.nv != nv:
                self._table = VertexFaceTable(r.faces_host, nv)
            nrm, _ = vertex_normals(v, self._table, out=buf["normals"], status=buf["normals_status"])
            res["normals"], res["normals_status"] = nrm, buf["normals_status"]
        with torch.cuda.device(dev):
            _lib.check(_lib.hip().p2m_mesh_shade(
                _p(fid), _p(mid), _p(v), _p(r._faces), r.nf, _p(c), _p(col), _p(vcol), shared, _p(nrm), r._lights, len(r.lights),
                r.ambient, _p(att), C, self.wire_T, self._wire_rgb, self.wire_only, _p(bg), per_mesh, self.attr_fill, B, nv, H, W,
                1 if scene else 0, _p(image), _p(buf["bary"]) if bary else None, _p(buf["attributes"]) if C else None,
                _p(buf["status"]), _stream()), "p2m_mesh_shade")
        res["image"], res["status"] = image, buf["status"]
        if bary:
            res["bary"] = buf["bary"]
        if C:
            res["attributes"] = buf["attributes"]
        return res
