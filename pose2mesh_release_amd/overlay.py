"""2D poses drawn on the GPU: batched anti-aliased lines, discs and rings blended into uint8 images (p2m_pose_overlay), the
device counterpart of the reference's lib/vis.py (vis_2d_keypoints / vis_2d_pose and vis_coco_skeleton, there OpenCV).

  PoseOverlay            poses [B, P, J, 2 | 3] (+ optional boxes [B, P, 4, 2]) drawn onto images [B, H, W, 3], in place or into out
  PoseOverlay.keypoints  the numbers of vis_2d_keypoints: thickness 2, filled radius-3 discs, kp_thre 0.4, rainbow per bone
  PoseOverlay.coco_skeleton  those of vis_coco_skeleton: thickness 2, rings of radius 2 and thickness 3, one colour per person
  rainbow_colours        matplotlib's `rainbow` map sampled as vis.py:79-81 does, without matplotlib

Which primitives are drawn, where and in which order follows the reference; the pixel arithmetic (coverage on a 1/16 grid from
exact integer distances, integer blending) is this project's, defined in the comment of p2m_pose_overlay in include/p2m.h and
restated in tests/overlay_ref.py: parity with OpenCV's LINE_AA pixels is not claimed.  The images stay in device memory - the
renderer's out["image"] can be drawn on directly - and a call launches two kernels that allocate and synchronise nothing, so it
can sit in a captured graph.  There is no CPU fallback: CPU tensors raise.
"""
import ctypes as _ct

import numpy as _np
import torch

from . import _lib

STATUS_BAD_JOINT, STATUS_BAD_BOX = 1, 2
MAX_JOINTS = MAX_PEOPLE = MAX_BONES = 64


def _p(t):
    return None if t is None else _ct.c_void_p(t.data_ptr())


def _stream():
    return _ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda(x, name, dtype=torch.float32):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.P2MError(f"{name}: the overlay kernels need a CUDA tensor (there is no CPU path)")
    return x.contiguous() if x.dtype == dtype else x.to(dtype).contiguous()


def rainbow_colours(n, order="bgr"):
    """uint8 [n, 3]: matplotlib's `rainbow` at np.linspace(0, 1, n), as vis.py:79-81 samples it.  The map is a 256-entry table:
    idx = 255 if x >= 1 else floor(256 x), u = np.linspace(0, 1, 256)[idx], (r, g, b) = (|2u - 1/2|, sin(pi u), cos(pi u / 2)) clipped to [0, 1],
    then rint(255 c).  order "bgr" (what vis.py hands to OpenCV) or "rgb"."""
    if order not in ("bgr", "rgb"):
        raise ValueError(f"order: bgr | rgb, got {order!r}")
    x = _np.linspace(0, 1, int(n))
    idx = _np.where(x >= 1.0, 255, _np.floor(256.0 * x)).astype(_np.int64)
    u = _np.linspace(0, 1, 256)[idx]            # (the table's own abscissae: 255 |2u - 1/2| is a tie in exact arithmetic)
    rgb = _np.stack([_np.abs(2.0 * u - 0.5), _np.sin(_np.pi * u), _np.cos(0.5 * _np.pi * u)], axis=1)
    out = _np.rint(255.0 * _np.clip(rgb, 0.0, 1.0)).astype(_np.uint8).reshape(-1, 3)
    return _np.ascontiguousarray(out[:, ::-1] if order == "bgr" else out)


def _pack_rgb(c):
    c = [int(v) for v in c]
    if len(c) != 3 or any(v < 0 or v > 255 for v in c):
        raise ValueError(f"a colour is three integers in [0, 255], got {c}")
    return c[0] | (c[1] << 8) | (c[2] << 16)


class PoseOverlay:
    """o = PoseOverlay(bones, height, width, line=2, mark=("disc", 3) | ("ring", 2, 3), thr=0.4, colours=None,
                       box_colour=(255, 255, 0), box=1)
    out = o(image uint8 [B, H, W, 3], poses [B, P, J, 2 | 3], colours=None | [B, P, 3], boxes=None | [B, P, 4, 2], alpha=1.0,
            out=None)

    bones   [L, 2] integer joint indices, checked here against the poses' J at the first call of a J (L = 0: boxes only).
    line    OpenCV's thickness of a bone, in pixels (half-pixel units of the kernel).
    mark    ("disc", radius): cv2.circle(thickness=-1);  ("ring", radius, thickness): cv2.circle(radius, thickness).
    thr     a joint with a confidence (C = 3) is drawn iff conf > thr; None: no threshold (every finite confidence passes).
    colours the per-bone palette, uint8 [L, 3] in the image's channel order; None: rainbow_colours(L) (BGR, as vis.py).
            Colours given to a CALL, [B, P, 3] or one (c0, c1, c2), are one colour per person (vis_coco_skeleton's given_color)
            and take the palette's place for that call; per_person=True (the coco_skeleton preset) makes them mandatory.
    boxes   the four corners per person, drawn first with box_colour and thickness `box` (vis_2d_keypoints' bbox).
    alpha   cv2.addWeighted's: 1 the drawing, 0 the image; rounded to 1/256.
    out     None: drawn in place on `image`; a uint8 tensor of image's shape: written completely, image untouched.

    Returns {"image": the tensor drawn on, "status": int32 [B, P]} - bit 0: a joint of the person was not finite or 16384
    pixels away or more (invisible); bit 1: such a corner, the person's box is skipped.  Workspace, status and the staged
    colours are buffers reused per (B, P), overwritten by the next call of that shape: no allocation after the first call
    of a shape and no sync.  A 3-dim image is B = 1; 3-dim poses [B, J, C] are P = 1."""

    def __init__(self, bones, height, width, line=2, mark=("disc", 3), thr=0.4, colours=None, box_colour=(255, 255, 0), box=1,
                 per_person=False):
        b = _np.asarray(bones.cpu() if isinstance(bones, torch.Tensor) else bones)
        if b.size == 0:
            b = _np.zeros((0, 2), _np.int64)
        if b.ndim != 2 or b.shape[1] != 2 or not _np.issubdtype(b.dtype, _np.integer):
            raise ValueError(f"bones: expected integer [L, 2], got {b.dtype} {b.shape}")
        if b.shape[0] > MAX_BONES:
            raise ValueError(f"bones: at most {MAX_BONES}, got {b.shape[0]}")
        if b.size and (int(b.min()) < 0 or int(b.max()) >= MAX_JOINTS):
            raise ValueError(f"bones: indices must lie in [0, {MAX_JOINTS}), got [{int(b.min())}, {int(b.max())}]")
        self.bones_host = _np.ascontiguousarray(b.astype(_np.int32))
        self.L = int(b.shape[0])
        self.height, self.width = int(height), int(width)
        if not (1 <= self.height <= 8192 and 1 <= self.width <= 8192):
            raise ValueError("height, width must lie in [1, 8192]")
        self.line_h2 = int(line)
        if mark[0] == "disc" and len(mark) == 2:
            self.mark_h2, self.mark_r16 = 2 * int(mark[1]), -1
        elif mark[0] == "ring" and len(mark) == 3:
            self.mark_h2, self.mark_r16 = int(mark[2]), 16 * int(mark[1])
        else:
            raise ValueError(f'mark: ("disc", radius) | ("ring", radius, thickness), got {mark!r}')
        self.box_h2 = int(box)
        if not all(0 <= h <= 64 for h in (self.line_h2, self.mark_h2, self.box_h2)) or not -1 <= self.mark_r16 <= 1024:
            raise ValueError("thicknesses must lie in [0, 64] half pixels (a disc's radius in [0, 32]), a ring's radius in [0, 64]")
        self.thr = float("-inf") if thr is None else float(thr)
        pal = rainbow_colours(self.L) if colours is None else _np.asarray(colours)
        if pal.shape != (self.L, 3) or (self.L and (pal.min() < 0 or pal.max() > 255)):
            raise ValueError(f"colours: expected uint8 [{self.L}, 3], got {pal.shape}")
        self.palette_host = _np.ascontiguousarray(pal.astype(_np.uint8))
        self.box_rgb = _pack_rgb(box_colour)
        self.per_person = bool(per_person)
        self._checked_J = None
        self._dev = None
        self._bufs = {}

    @classmethod
    def keypoints(cls, bones, height, width, **kw):
        """vis_2d_keypoints (vis.py:77-113): thickness 2, filled radius-3 discs, kp_thre 0.4, rainbow per bone, box thickness 1."""
        return cls(bones, height, width, **dict(dict(line=2, mark=("disc", 3), thr=0.4, box=1, box_colour=(255, 255, 0)), **kw))

    @classmethod
    def coco_skeleton(cls, bones, height, width, **kw):
        """vis_coco_skeleton (vis.py:10-74): thickness 2, rings of radius 2 and thickness 3, one colour per person (given to
        the call), no threshold."""
        return cls(bones, height, width, **dict(dict(line=2, mark=("ring", 2, 3), thr=None, per_person=True), **kw))

    def _check_bones(self, J):
        if self._checked_J != J:
            if not 1 <= J <= MAX_JOINTS:
                raise ValueError(f"poses: J must lie in [1, {MAX_JOINTS}], got {J}")
            if self.L and int(self.bones_host.max()) >= J:
                raise ValueError(f"bones: indices must lie in [0, {J}), got up to {int(self.bones_host.max())}")
            self._checked_J = J

    def _buffers(self, B, P, with_boxes, dev):
        if self._dev != dev:
            self._dev, self._bufs = dev, {}
            self._bones = torch.from_numpy(self.bones_host).to(dev) if self.L else None
            self._palette = torch.from_numpy(self.palette_host).to(dev) if self.L else None
        b = self._bufs.get((B, P, with_boxes))
        if b is None:
            n = _ct.c_int64(0)
            _lib.check(_lib.hip().p2m_pose_overlay_workspace(B, P, self.L, 1 if with_boxes else 0, _ct.byref(n)),
                       "p2m_pose_overlay_workspace")
            b = {"status": torch.zeros((B, P), device=dev, dtype=torch.int32),
                 "colours": torch.zeros((B, P, 3), device=dev, dtype=torch.uint8), "colours_key": None,
                 "ws": torch.zeros((max(int(n.value), 16),), device=dev, dtype=torch.uint8), "ws_bytes": int(n.value)}
            self._bufs[(B, P, with_boxes)] = b
        return b

    @torch.no_grad()
    def __call__(self, image, poses, colours=None, boxes=None, alpha=1.0, out=None):
        H, W = self.height, self.width
        if not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise _lib.P2MError("image: the overlay kernels need a CUDA tensor (there is no CPU path)")
        shape4 = (1, H, W, 3) if image.dim() == 3 else tuple(image.shape)
        if image.dtype != torch.uint8 or shape4[1:] != (H, W, 3) or tuple(image.shape)[-3:] != (H, W, 3):
            raise ValueError(f"image: expected uint8 [B, {H}, {W}, 3], got {image.dtype} {tuple(image.shape)}")
        if not image.is_contiguous():
            raise ValueError("image: must be contiguous (it is drawn on in place, or read as rows of 3 W bytes)")
        B = int(shape4[0])
        pz = _cuda(poses, "poses")
        if pz.dim() == 3:
            pz = pz.unsqueeze(1)
        if pz.dim() != 4 or pz.shape[0] != B or pz.shape[3] not in (2, 3) or not 1 <= pz.shape[1] <= MAX_PEOPLE:
            raise ValueError(f"poses: expected [{B}, P <= {MAX_PEOPLE}, J, 2 | 3], got {tuple(pz.shape)}")
        P, J, C = int(pz.shape[1]), int(pz.shape[2]), int(pz.shape[3])
        self._check_bones(J)
        bx = None
        if boxes is not None:
            bx = _cuda(boxes, "boxes")
            if tuple(bx.shape) != (B, P, 4, 2):
                raise ValueError(f"boxes: expected [{B}, {P}, 4, 2], got {tuple(bx.shape)}")
        elif self.L == 0:
            raise ValueError("no bones and no boxes: nothing to draw")
        dst = image
        if out is not None:
            if not isinstance(out, torch.Tensor) or not out.is_cuda:
                raise _lib.P2MError("out: the overlay kernels need a CUDA tensor (there is no CPU path)")
            if out.dtype != torch.uint8 or tuple(out.shape) != tuple(image.shape) or not out.is_contiguous():
                raise ValueError(f"out: expected contiguous uint8 {tuple(image.shape)}, got {out.dtype} {tuple(out.shape)}")
            dst = out
        a256 = int(round(float(alpha) * 256.0))
        if not 0 <= a256 <= 256:
            raise ValueError(f"alpha must lie in [0, 1], got {alpha}")
        buf = self._buffers(B, P, bx is not None, image.device)
        mode, col = 0, self._palette
        if colours is None:
            if self.per_person:
                raise ValueError("colours: this overlay draws one colour per person; give [B, P, 3] or one colour to the call")
        elif isinstance(colours, torch.Tensor):
            col = _cuda(colours, "colours", torch.uint8)
            if tuple(col.shape) != (B, P, 3):
                raise ValueError(f"colours: expected uint8 [{B}, {P}, 3], got {tuple(col.shape)}")
            mode = 1
        else:
            ch = _np.asarray(colours)
            if ch.shape not in ((3,), (B, P, 3)) or ch.min() < 0 or ch.max() > 255:
                raise ValueError(f"colours: expected [3] or [{B}, {P}, 3] in [0, 255], got {ch.shape}")
            ch = _np.ascontiguousarray(_np.broadcast_to(ch.astype(_np.uint8), (B, P, 3)))
            key = ch.tobytes()
            if buf["colours_key"] != key:                   # (a host-to-device copy only when the values change)
                buf["colours"].copy_(torch.from_numpy(ch))
                buf["colours_key"] = key
            mode, col = 1, buf["colours"]
        with torch.cuda.device(image.device):
            _lib.check(_lib.hip().p2m_pose_overlay(
                _p(pz), B, P, J, C, _p(self._bones), self.L, _p(col), mode, _p(bx), self.box_rgb, _p(image), _p(dst), H, W,
                self.thr, self.line_h2, self.mark_h2, self.mark_r16, self.box_h2, a256, _p(buf["status"]), _p(buf["ws"]),
                buf["ws_bytes"], _stream()), "p2m_pose_overlay")
        return {"image": dst, "status": buf["status"]}
