"""The demo's camera on the GPU: the batched 2D-pose preparation and the weak-perspective camera fit of demo/run.py's
optimize_cam_param (:149-197; lib/models/project_net.py) - csrc/camfit.hip, include/p2m.h "The demo's camera".

  prep = prepare_pose(joints_px)                       prep.pose2d (the network's input), prep.target, prep.bbox, prep.status
  fit = CameraFitter(crop=500)                         OptimzeCamLayer + L1Loss + Adam, 1500 steps, one wave per person
  out = fit(joints3d_m, prep.target)                   out.cam [B, 3] = (s, tx, ty) of the crop, out.loss [B], out.status [B]

Between the two sits infer.GraphedInference (its `joints` divided by its `scale` are joints3d_m); after them
render.crop_cam_to_image(out.cam, prep.bbox, W, H) and render.MeshRenderer.  Each call is one launch that allocates and
synchronises nothing once its buffers exist, so the chain can sit in a torch.cuda.graph.  Without cam0 the start is drawn
from the package's Philox stream (sample.NoiseStream, stage 10): sample b uses the global index stream.index + b, and a call
advances the index by B with a tensor add, so a replayed graph starts from fresh values.  A sample's result depends on that
sample alone and is bitwise reproducible.  There is no CPU fallback: CPU tensors raise P2MError.
"""
import ctypes as _ct
import types as _types

import torch

from . import _lib
from .sample import NoiseStream

MAX_JOINTS = 64
STATUS_INVALID, STATUS_MIRRORED = 1, 2
# the reference lowers the rate AFTER the steps with j == 500 and j == 1000 (run.py:184-189): zero-based first steps
DEFAULT_SCHEDULE = ((0, 0.1), (501, 0.05), (1001, 0.001))
DEFAULT_STEPS = 1500


def _p(t):
    return None if t is None else _ct.c_void_p(t.data_ptr())


def _stream():
    return _ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda(x, name, shape=None):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.P2MError(f"{name}: the camera kernels need a CUDA tensor (there is no CPU path)")
    if shape is not None and tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name}: expected {list(shape)}, got {list(x.shape)}")
    return x.contiguous() if x.dtype == torch.float32 else x.to(torch.float32).contiguous()


def _buffers(B, J, dev):
    z = lambda *sh, dt=torch.float32: torch.zeros(sh, device=dev, dtype=dt)  # noqa: E731
    return _types.SimpleNamespace(pose2d=z(B, J, 2), target=z(B, J, 2), bbox=z(B, 4), status=z(B, dt=torch.int32))


@torch.no_grad()
def prepare_pose(joints, input_shape=(384, 288), crop=500, out=None):
    """joints [B, J, 2] (pixels of the original image; further columns, a confidence say, are ignored) -> a namespace with
    pose2d [B, J, 2] (standardised, what the network takes), target [B, J, 2] (the joints in the crop x crop virtual crop),
    bbox [B, 4] (the reference's bbox1 as x, y, w, h) and status [B] int32 (bit 0: degenerate box, non-finite joint or zero
    std; that sample's outputs are zero).  input_shape = (H, W) as cfg.MODEL.input_shape.  out: a namespace from an earlier
    call of the same shape (then nothing is allocated)."""
    if not isinstance(joints, torch.Tensor) or not joints.is_cuda:
        raise _lib.P2MError("joints: the camera kernels need a CUDA tensor (there is no CPU path)")
    if joints.dim() != 3 or joints.shape[0] < 1 or joints.shape[2] < 2:
        raise ValueError(f"joints: expected [B >= 1, J, 2], got {list(joints.shape)}")
    B, J, dev = int(joints.shape[0]), int(joints.shape[1]), joints.device
    j = _cuda(joints[:, :, :2], "joints")
    if out is None:
        out = _buffers(B, J, dev)
    for k, sh in dict(pose2d=(B, J, 2), target=(B, J, 2), bbox=(B, 4)).items():
        t = getattr(out, k)
        if tuple(t.shape) != sh or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"out.{k}: expected a contiguous float32 tensor {list(sh)} on {dev}")
    if tuple(out.status.shape) != (B,) or out.status.dtype != torch.int32 or out.status.device != dev:
        raise ValueError(f"out.status: expected an int32 tensor [{B}] on {dev}")
    with torch.cuda.device(dev):
        _lib.check(_lib.hip().p2m_pose_prepare(_p(j), B, J, float(input_shape[1]), float(input_shape[0]), float(crop),
                                               _p(out.pose2d), _p(out.target), _p(out.bbox), _p(out.status), _stream()),
                   "p2m_pose_prepare")
    return out


class CameraFitter:
    """fit = CameraFitter(crop=500, steps=1500, schedule=((0, 0.1), (501, 0.05), (1001, 0.001)), betas=(0.9, 0.999), eps=1e-8,
                          seed=None | stream=NoiseStream)
    out = fit(joints3d [B, J, 3] (metres: GraphedInference's joints / scale), target [B, J, 2], weight=None | [B, J],
              cam0=None | [B, 3])

    schedule: up to 8 (first zero-based step, lr) pairs, the first at step 0, ascending.  cam0: the start (s, tx, ty) per
    sample; None: drawn from the stream (seed=, default 123, or a NoiseStream shared with other users), as the reference's
    torch.rand((1, 3)).  Returns a namespace of device tensors - cam [B, 3] after the last step, loss [B] the weighted L1
    objective at exactly that camera, status [B] int32 (bit 0: non-finite input or sum of weights <= 0, cam = loss = 0; bit
    1: s <= 0 at the end).  They are buffers kept per (B, J), overwritten by the next call of that shape: no allocation
    after the first call of a shape and no sync."""

    def __init__(self, crop=500, steps=DEFAULT_STEPS, schedule=DEFAULT_SCHEDULE, betas=(0.9, 0.999), eps=1e-8, seed=None,
                 stream=None):
        if seed is not None and stream is not None:
            raise ValueError("give seed or stream, not both")
        self.img_res = float(crop) / 2.0
        self.steps = int(steps)
        pairs = [(int(a), float(b)) for a, b in schedule]
        sc = _lib.FitSchedule()
        sc.n = len(pairs)
        for k, (a, b) in enumerate(pairs[:8]):
            sc.first_step[k], sc.lr[k] = a, b
        self.schedule, self._sched = tuple(pairs), sc
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.stream = stream
        self._seed = 123 if seed is None else seed
        self._bufs = {}

    def _state(self, dev):
        if self.stream is None:
            self.stream = NoiseStream(self._seed, 0, dev)
        if self.stream.state.device != dev:
            raise ValueError(f"the stream's state is on {self.stream.state.device}, the joints on {dev}")
        return self.stream

    @torch.no_grad()
    def __call__(self, joints3d, target, weight=None, cam0=None):
        if not isinstance(joints3d, torch.Tensor) or not joints3d.is_cuda:
            raise _lib.P2MError("joints3d: the camera kernels need a CUDA tensor (there is no CPU path)")
        if joints3d.dim() != 3 or joints3d.shape[0] < 1 or joints3d.shape[2] != 3:
            raise ValueError(f"joints3d: expected [B >= 1, J, 3], got {list(joints3d.shape)}")
        B, J, dev = int(joints3d.shape[0]), int(joints3d.shape[1]), joints3d.device
        j3 = _cuda(joints3d, "joints3d")
        tg = _cuda(target, "target", (B, J, 2))
        wt = None if weight is None else _cuda(weight, "weight", (B, J))
        c0 = None if cam0 is None else _cuda(cam0, "cam0", (B, 3))
        st = None if cam0 is not None else self._state(dev)
        buf = self._bufs.get((B, J, dev))
        if buf is None:
            buf = self._bufs[(B, J, dev)] = _types.SimpleNamespace(
                cam=torch.zeros((B, 3), device=dev), loss=torch.zeros((B,), device=dev),
                status=torch.zeros((B,), device=dev, dtype=torch.int32))
        with torch.cuda.device(dev):
            _lib.check(_lib.hip().p2m_camera_fit(
                _p(j3), _p(tg), _p(wt), _p(c0), None if st is None else _p(st.state), B, J, self._sched, self.steps,
                self.img_res, self.betas[0], self.betas[1], self.eps, _p(buf.cam), _p(buf.loss), _p(buf.status), _stream()),
                "p2m_camera_fit")
            if st is not None:
                st.advance(B)
        return buf
