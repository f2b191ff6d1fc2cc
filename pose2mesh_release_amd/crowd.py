"""The crowd demo's front end on the GPU: which detections of an image are people to show, and a colour for each - the head of
the crowd branch of demo/run.py (add_pelvis / add_neck :127-146, the score filter and the greedy duplicate suppression
:276-306, the random colour :314) - csrc/crowd.hip, include/p2m.h "The crowd demo's front end".

  sel = CrowdFilter()                                  midpoints=((11, 12), (5, 6)): pelvis, neck; 0.1, 1.5, 20 as run.py
  out = sel(dets, num=None)                            dets [B, P, J, 3] (x, y, conf) -> out.joints [B, P, J + 2, 3], out.count,
                                                       out.index, out.keep, out.reason, out.dup_of, out.score
  col = person_colours(n, stream=NoiseStream | seed=)  col.rgb [n, 3] fp32 (MeshRenderer's colours), col.u8 [n, 3] (PoseOverlay's)

The accepted people of an image are compacted to the front of out.joints in list order; every other slot is NaN, which the
modules behind understand as "nobody": camfit.prepare_pose zeroes such a sample (status bit 0), CameraFitter returns cam = 0
for it, the rasteriser skips its faces and PoseOverlay draws nothing of it.  So the number of people never has to visit the
host, and the whole chain from detections to picture can sit in one torch.cuda.graph.  Each call is one launch that allocates
and synchronises nothing once its buffers exist.  An image's result depends on that image alone and is bitwise reproducible.
There is no CPU fallback: CPU tensors raise P2MError.
"""
import ctypes as _ct
import types as _types

import torch

from . import _lib
from .sample import NoiseStream

MAX_PEOPLE = MAX_JOINTS = 64
MAX_MIDPOINTS = 8
REASON_ACCEPTED, REASON_LOW_SCORE, REASON_DUPLICATE, REASON_NON_FINITE, REASON_UNUSED = 0, 1, 2, 3, -1
COCO_MIDPOINTS = ((11, 12), (5, 6))          # pelvis = hips, neck = shoulders, in run.py's order


def _p(t):
    return None if t is None else _ct.c_void_p(t.data_ptr())


def _stream():
    return _ct.c_void_p(torch.cuda.current_stream().cuda_stream)


class CrowdFilter:
    """sel = CrowdFilter(midpoints=((11, 12), (5, 6)), pose_thr=0.1, score_thr=1.5, min_diff=20.0)
    out = sel(dets fp32 [B, P, J, 3], num=None | int32 [B] on the device)

    dets: (x, y, confidence) of up to P <= 64 detections per image in the detector's list order; num: how many of the P slots of
    each image are filled (None: all; the others are never read).  midpoints: pairs of input joints whose midpoint is appended
    (confidence = the product of the two), Jo = J + len(midpoints) <= 64.  A joint is valid iff conf > pose_thr; a person whose
    confidences sum to less than score_thr is dropped; a person whose masked mean distance to an ALREADY ACCEPTED person is
    below min_diff is dropped as its duplicate; a person with a non-finite input value is dropped (include/p2m.h has the exact
    arithmetic, all float64).  Returns a namespace of device tensors, buffers kept per (B, P, J) and overwritten by the next
    call of that shape (no allocation after the first call of a shape, no sync):
      joints [B, P, Jo, 3]  the accepted people compacted to the front in list order, NaN in every other slot
      count [B] int32, index [B, P] int32 (the input slot of compacted person k, -1 beyond count)
      per input slot: keep [B, P] bool, reason [B, P] int8 (REASON_*), dup_of [B, P] int32 (-1 unless a duplicate),
      score [B, P] float64 (NaN for a non-finite or unused slot)"""

    def __init__(self, midpoints=COCO_MIDPOINTS, pose_thr=0.1, score_thr=1.5, min_diff=20.0):
        pairs = [(int(a), int(b)) for a, b in midpoints]
        self.midpoints = tuple(pairs)
        flat = [v for ab in pairs for v in ab]
        self._mid = (_ct.c_int32 * max(1, len(flat)))(*flat)
        self.pose_thr, self.score_thr, self.min_diff = float(pose_thr), float(score_thr), float(min_diff)
        self._bufs = {}

    @torch.no_grad()
    def __call__(self, dets, num=None):
        if not isinstance(dets, torch.Tensor) or not dets.is_cuda:
            raise _lib.P2MError("dets: the crowd kernels need a CUDA tensor (there is no CPU path)")
        if dets.dim() != 4 or dets.shape[3] != 3:
            raise ValueError(f"dets: expected [B, P, J, 3], got {list(dets.shape)}")
        B, P, J, dev = int(dets.shape[0]), int(dets.shape[1]), int(dets.shape[2]), dets.device
        d = dets.contiguous() if dets.dtype == torch.float32 else dets.to(torch.float32).contiguous()
        if num is not None:
            if not isinstance(num, torch.Tensor) or not num.is_cuda:
                raise _lib.P2MError("num: the crowd kernels need a CUDA tensor (there is no CPU path)")
            if tuple(num.shape) != (B,) or num.dtype != torch.int32 or num.device != dev:
                raise ValueError(f"num: expected an int32 tensor [{B}] on {dev}")
            num = num.contiguous()
        n_mid = len(self.midpoints)
        buf = self._bufs.get((B, P, J, dev))
        if buf is None:
            Jo = max(J + n_mid, 0)
            buf = _types.SimpleNamespace(
                joints=torch.full((B, P, Jo, 3), float("nan"), device=dev), count=torch.zeros((B,), device=dev, dtype=torch.int32),
                index=torch.full((B, P), -1, device=dev, dtype=torch.int32), keep=torch.zeros((B, P), device=dev, dtype=torch.bool),
                reason=torch.full((B, P), -1, device=dev, dtype=torch.int8),
                dup_of=torch.full((B, P), -1, device=dev, dtype=torch.int32),
                score=torch.full((B, P), float("nan"), device=dev, dtype=torch.float64))
        with torch.cuda.device(dev):
            _lib.check(_lib.hip().p2m_crowd_select(
                _p(d), _p(num), B, P, J, self._mid, n_mid, self.pose_thr, self.score_thr, self.min_diff, _p(buf.joints),
                _p(buf.count), _p(buf.index), _p(buf.reason), _p(buf.dup_of), _p(buf.score), _p(buf.keep), _stream()),
                "p2m_crowd_select")
        self._bufs[(B, P, J, dev)] = buf                    # (kept only once the arguments have passed)
        return buf


@torch.no_grad()
def person_colours(n, stream=None, seed=None, s=0.5, v=1.0, out=None, advance=True, device="cuda"):
    """n colours as run.py:314's colorsys.hsv_to_rgb(np.random.rand(), 0.5, 1.0): a namespace with rgb fp32 [n, 3] (what
    MeshRenderer(colours=) takes) and u8 uint8 [n, 3] = round-half-even(255 rgb), in the same channel order (what
    PoseOverlay(colours=) takes; vis_coco_skeleton hands OpenCV the triple as it is).  The hues come from the package's Philox
    stream, stage 11: colour k uses the global index stream.index + k, and the call advances the index by n with a tensor add
    (advance=False: the caller does it), so a captured graph replays with fresh colours.  stream: a NoiseStream, possibly
    shared with CameraFitter and the sample kernels; or seed= (default 123) for a stream of its own starting at index 0.
    out: the namespace of an earlier call of the same n (then nothing is allocated)."""
    if seed is not None and stream is not None:
        raise ValueError("give seed or stream, not both")
    if stream is None:
        if torch.device(device).type != "cuda":
            raise _lib.P2MError("person_colours: the crowd kernels need a CUDA device (there is no CPU path)")
        stream = NoiseStream(123 if seed is None else seed, 0, device)
    dev = stream.state.device
    n = int(n)
    if out is None:
        out = _types.SimpleNamespace(rgb=torch.zeros((max(n, 0), 3), device=dev),
                                     u8=torch.zeros((max(n, 0), 3), device=dev, dtype=torch.uint8))
    for k, dt in (("rgb", torch.float32), ("u8", torch.uint8)):
        t = getattr(out, k)
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.P2MError(f"out.{k}: the crowd kernels need a CUDA tensor (there is no CPU path)")
        if tuple(t.shape) != (n, 3) or t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"out.{k}: expected a contiguous {dt} tensor [{n}, 3] on {dev}")
    with torch.cuda.device(dev):
        _lib.check(_lib.hip().p2m_person_colours(_p(stream.state), n, float(s), float(v), _p(out.rgb), _p(out.u8), _stream()),
                   "p2m_person_colours")
        if advance:
            stream.advance(n)
    return out
