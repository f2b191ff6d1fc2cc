"""Rendering on the GPU: a batched z-buffer rasteriser with flat shading and image overlay (p2m_mesh_render), the device
counterpart of the reference's demo/renderer.py + demo/run.py:24-67 (trimesh, pyrender, OpenGL / EGL, host compositing).

  MeshRenderer           meshes [B, nv, 3] + weak-perspective cameras [B, 4] -> image, mask, face_id, mesh_id, depth, one
                         image per mesh ("batch") or all meshes in one image ("scene")
  crop_cam_to_image      run.py's convert_crop_cam_to_orig_img: the camera of a crop as a camera of the original image
  project_vertices       the snapped 1/256-pixel coordinates of every vertex (p2m_mesh_project)

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
