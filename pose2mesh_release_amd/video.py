"""Video evaluation and the demo's temporal filter on the GPU: the second half of the reference's 3DPW protocol
(data/PW3D/dataset.py:383-417, its "temporal smoothing code"): One-Euro smoothing (lib/smooth_utils.py), the acceleration
error (lib/coord_utils.py:194-222) and MPJPE / PA-MPJPE of the smoothed joints per video.

  smooth_pose(pred_pose, min_cutoff, beta)       drop-in for smooth_utils.smooth_pose on a [T, ...] CUDA tensor; seq_ptr
                                                 filters many sequences in one launch (p2m_one_euro)
  OneEuroFilter                                  the streaming form: one new frame per track and call (or a chunk of frames),
                                                 state on the device, usable inside torch.cuda.graph - sits between
                                                 GraphedInference and MeshRenderer in the demo chain
  compute_error_accel, error_accel               drop-in / sync-free acceleration error (p2m_video_eval)
  VideoEvaluator                                 collects the Tester's joints on the device and evaluates every video in
                                                 one gather -> filter -> p2m_video_eval pass; summary() syncs once

The filter is fp32, op by op what the reference's numpy computes on float32 input: the output is bitwise the reference's
(include/p2m.h has the contract).  The metrics are accumulated in fp64 in fixed orders.  CUDA tensors only: there is no CPU
fallback, CPU tensors raise P2MError.
"""
import ctypes as _ct

import numpy as _np
import torch

from . import _lib


def _p(t):
    return None if t is None else _ct.c_void_p(t.data_ptr())


def _stream():
    return _ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda_f32(x, name):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.P2MError(f"{name}: the video kernels need a CUDA tensor (there is no CPU path)")
    return x.contiguous() if x.dtype == torch.float32 else x.float().contiguous()


def lookahead():
    """Frames the filter kernel loads ahead of its recurrence (p2m_one_euro_lookahead)."""
    return int(_lib.hip().p2m_one_euro_lookahead())


def sequence_tables(video_indices, n=None):
    """Host side of VideoEvaluator: a list of boolean masks or index arrays over the dataset order (what the dataset builds
    at data/PW3D/dataset.py:160-163) -> (rows int32 [N], seq_ptr int32 [S + 1], n): video s owns rows[seq_ptr[s] :
    seq_ptr[s + 1]], its dataset positions in order.  A video's frames need not be contiguous.  n: the dataset's length
    (default: the masks' length, or the largest index + 1); every position must lie in [0, n)."""
    rows, ptr, size = [], [0], None
    for k, v in enumerate(video_indices):
        v = _np.asarray(v)
        if v.dtype == _np.bool_:
            if v.ndim != 1 or (size is not None and v.shape[0] != size):
                raise ValueError(f"video_indices[{k}]: masks must be 1-D and of one length")
            size = v.shape[0]
            idx = _np.flatnonzero(v)
        else:
            if v.size and not _np.issubdtype(v.dtype, _np.integer):
                raise ValueError(f"video_indices[{k}]: a boolean mask or integer positions expected, got {v.dtype}")
            idx = v.astype(_np.int64).reshape(-1)
        rows.append(idx)
        ptr.append(ptr[-1] + idx.size)
    if not rows:
        raise ValueError("video_indices: at least one video expected")
    rows = _np.concatenate(rows)
    if n is None:
        n = size if size is not None else (int(rows.max()) + 1 if rows.size else 0)
    n = int(n)
    if (size is not None and size > n) or (rows.size and (rows.min() < 0 or rows.max() >= n)):
        raise ValueError(f"video_indices: positions outside [0, {n})")
    if ptr[-1] >= 1 << 31:
        raise ValueError("video_indices: 2^31 or more frames")
    return rows.astype(_np.int32), _np.asarray(ptr, dtype=_np.int32), n


def _dev_seq_ptr(seq_ptr, N, dev):
    """(device int32 tensor, S) of a host sequence or a CUDA tensor; None: the one sequence [0, N]."""
    if seq_ptr is None:
        return torch.tensor([0, N], dtype=torch.int32).to(dev), 1
    if isinstance(seq_ptr, torch.Tensor) and seq_ptr.is_cuda:
        sp = seq_ptr.to(torch.int32).contiguous().reshape(-1)
        return sp, sp.numel() - 1
    h = _np.asarray(seq_ptr, dtype=_np.int64).reshape(-1)
    if h.size < 2 or h[0] != 0 or h[-1] != N or (_np.diff(h) < 0).any():
        raise ValueError(f"seq_ptr: ascending from 0 to {N} expected")
    return torch.from_numpy(h.astype(_np.int32)).to(dev), h.size - 1


def _one_euro(x, sp, rows, N, S, C, mc, beta, dc, dt, state, y):
    sx, sdx, started = state if state is not None else (None, None, None)
    with torch.cuda.device(x.device):
        _lib.check(_lib.hip().p2m_one_euro(_p(x), _p(sp), _p(rows), N, S, C, float(mc), float(beta), float(dc), float(dt),
                                           _p(sx), _p(sdx), _p(started), _p(y), _stream()), "p2m_one_euro")


@torch.no_grad()
def smooth_pose(pred_pose, min_cutoff=0.004, beta=0.7, seq_ptr=None, out=None):
    """smooth_utils.smooth_pose on the GPU: pred_pose [T, ...] (any trailing shape) -> the filtered tensor of the same
    shape, fp32, bitwise what the reference returns for the same float32 input.  seq_ptr (host sequence or CUDA int32
    tensor, ascending from 0 to T): the frames are a batch of sequences, each filtered on its own, in one launch.  out: a
    contiguous fp32 CUDA tensor of the same shape to write into; it may be pred_pose itself (in place)."""
    x = _cuda_f32(pred_pose, "pred_pose")
    if x.dim() < 1:
        raise ValueError("pred_pose: [T, ...] expected")
    T = int(x.shape[0])
    C = int(x[0].numel()) if T else 0
    if out is None:
        out = torch.empty_like(x)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
              and out.shape == x.shape):
        raise ValueError("out: a contiguous fp32 CUDA tensor of pred_pose's shape expected")
    sp, S = _dev_seq_ptr(seq_ptr, T, x.device)
    if T == 0 or C == 0:
        return out
    _one_euro(x, sp, None, T, S, C, min_cutoff, beta, 1.0, 1.0, None, out)
    return out


class OneEuroFilter:
    """f = OneEuroFilter(min_cutoff=1.0, beta=0.0, d_cutoff=1.0, dt=1.0)
    y = f(x)                 x [B, ...]: one new frame for each of B tracks (e.g. [B, 6890, 3] from GraphedInference)
    y = f(x, chunk=True)     x [T, B, ...]: T frames per track; y has x's shape
    f.reset();  f.reset(track_ids);  f.reset(mask=m)

    The streaming form of the filter.  The first call fixes B and the per-track shape; the state (previous value and
    derivative per coordinate, a `started` flag per track) lives on the device, and a track's first frame after
    construction or reset() passes through unchanged and initialises it, as smooth_pose's first frame does.  Feeding a
    sequence frame by frame, or in chunks of any sizes, gives bitwise the one-shot smooth_pose(d_cutoff = 1, dt = 1).
    y is a static buffer per input shape, overwritten by the next call of that shape (pass out= to keep a result).  After
    one call of a shape (which allocates), a call launches two kernels on the current stream and nothing else: it can be
    captured in torch.cuda.graph.  reset() is a device-side fill; reset(track_ids) takes a host sequence (one small copy)
    or a CUDA index tensor (no copy); reset(mask=) a bool CUDA tensor [B] (a masked fill, capturable)."""

    def __init__(self, min_cutoff=1.0, beta=0.0, d_cutoff=1.0, dt=1.0):
        self.min_cutoff, self.beta, self.d_cutoff, self.dt = float(min_cutoff), float(beta), float(d_cutoff), float(dt)
        for v, n in ((self.min_cutoff, "min_cutoff"), (self.beta, "beta"), (self.d_cutoff, "d_cutoff"), (self.dt, "dt")):
            if not _np.isfinite(v):
                raise ValueError(f"{n}: finite value expected")
        if self.dt <= 0 or self.min_cutoff < 0 or self.d_cutoff < 0:
            raise ValueError("dt > 0, min_cutoff >= 0 and d_cutoff >= 0 expected")
        self._shape = None
        self._state = None
        self._bufs = {}

    def _init(self, shape, dev):
        self._shape, self._dev = tuple(shape), dev
        self.B = int(shape[0])
        self.C = 1
        for d in shape[1:]:
            self.C *= int(d)
        if self.B < 1 or self.C < 1:
            raise ValueError(f"x: at least one track and one coordinate expected, got {tuple(shape)}")
        self._state = (torch.zeros((self.B, self.C), device=dev, dtype=torch.float32),
                       torch.zeros((self.B, self.C), device=dev, dtype=torch.float32),
                       torch.zeros(self.B, device=dev, dtype=torch.int32))

    def _tables(self, T):
        b = self._bufs.get(T)
        if b is None:
            dev, B = self._dev, self.B
            b = {"seq_ptr": torch.arange(0, (B + 1) * T, T, device=dev, dtype=torch.int32)}
            if T > 1:           # sequence order is track-major: frame t of track b is input row t B + b
                t = torch.arange(T, device=dev, dtype=torch.int32)
                b["rows"] = (t[None, :] * B + torch.arange(B, device=dev, dtype=torch.int32)[:, None]).reshape(-1).contiguous()
            b["y"] = torch.empty((B * T, self.C), device=dev, dtype=torch.float32)
            self._bufs[T] = b
        return b

    @torch.no_grad()
    def __call__(self, x, chunk=False, out=None):
        x = _cuda_f32(x, "x")
        if x.dim() < (2 if chunk else 1):
            raise ValueError("x: [B, ...] (or [T, B, ...] with chunk=True) expected")
        per = tuple(x.shape[1:]) if chunk else tuple(x.shape)
        if self._shape is None:
            self._init(per, x.device)
        if per != self._shape or x.device != self._dev:
            raise ValueError(f"x: this filter holds tracks of shape {self._shape} on {self._dev}, got {per} on {x.device}")
        T = int(x.shape[0]) if chunk else 1
        if T == 0:
            return torch.empty_like(x)
        b = self._tables(T)
        _one_euro(x, b["seq_ptr"], b.get("rows"), self.B * T, self.B, self.C, self.min_cutoff, self.beta, self.d_cutoff,
                  self.dt, self._state, b["y"])
        y = b["y"].view((self.B, T) + self._shape[1:]).transpose(0, 1) if chunk else b["y"].view(self._shape)
        if out is not None:
            out.copy_(y)
            return out
        return y

    @torch.no_grad()
    def reset(self, track_ids=None, mask=None):
        """Restarts every track, or the given ones: their next frame passes through and initialises the filter.  mask: a bool
        CUDA tensor [B] instead of track_ids - the tracks where it is set restart (a masked fill: data-independent, no copy,
        capturable; track.PoseTracker's out.fresh.reshape(-1) is such a mask)."""
        if mask is not None:
            if track_ids is not None:
                raise ValueError("give track_ids or mask, not both")
            if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
                raise _lib.P2MError("mask: the video kernels need a CUDA tensor (there is no CPU path)")
            if self._state is None:
                return
            if mask.dtype != torch.bool or tuple(mask.shape) != (self.B,) or mask.device != self._dev:
                raise ValueError(f"mask: expected a bool tensor [{self.B}] on {self._dev}")
            self._state[2].masked_fill_(mask, 0)
            return
        if self._state is None:
            return
        started = self._state[2]
        if track_ids is None:
            started.zero_()
            return
        if isinstance(track_ids, torch.Tensor) and track_ids.is_cuda:
            ids = track_ids.reshape(-1).to(torch.int64)
        else:
            h = _np.asarray(track_ids, dtype=_np.int64).reshape(-1)
            if h.size and (h.min() < 0 or h.max() >= self.B):
                raise ValueError(f"track_ids outside [0, {self.B})")
            ids = torch.from_numpy(h).to(self._dev)
        started.index_fill_(0, ids, 0)


def _video_eval(pred, gt, sp, S, vis, want_pa):
    N, J = int(pred.shape[0]), int(pred.shape[1])
    dev = pred.device
    out = {"accel": torch.empty(N, device=dev, dtype=torch.float32),
           "valid": torch.empty(N, device=dev, dtype=torch.uint8),
           "mpjpe": torch.empty((N, J), device=dev, dtype=torch.float32),
           "pa_mpjpe": torch.empty((N, J), device=dev, dtype=torch.float32) if want_pa else None,
           "frame_sums": torch.empty((N, 4), device=dev, dtype=torch.float64),
           "stats": torch.empty((S + 1, 8), device=dev, dtype=torch.float64)}       # rows 0 .. S-1: seq_stats, row S: totals
    with torch.cuda.device(dev):
        _lib.check(_lib.hip().p2m_video_eval(_p(pred), _p(gt), _p(sp), _p(vis), N, S, J, int(want_pa), _p(out["accel"]),
                                             _p(out["valid"]), _p(out["mpjpe"]), _p(out["pa_mpjpe"]), _p(out["frame_sums"]),
                                             _p(out["stats"]), _p(out["stats"][S]), _stream()), "p2m_video_eval")
    return out


def _joints_pair(joints_gt, joints_pred):
    gt, pred = _cuda_f32(joints_gt, "joints_gt"), _cuda_f32(joints_pred, "joints_pred")
    if gt.dim() != 3 or gt.shape[-1] != 3 or gt.shape != pred.shape or not 1 <= gt.shape[1] <= 64:
        raise ValueError(f"joints: equal [N, J <= 64, 3] tensors expected, got {tuple(gt.shape)}, {tuple(pred.shape)}")
    return gt, pred


def _dev_vis(vis, N, dev):
    if vis is None:
        return None
    if isinstance(vis, torch.Tensor):
        v = (vis != 0).to(device=dev, dtype=torch.uint8).reshape(-1).contiguous()
    else:
        v = torch.from_numpy((_np.asarray(vis).reshape(-1) != 0).astype(_np.uint8)).to(dev)
    if v.numel() != N:
        raise ValueError(f"vis: {N} entries expected, got {v.numel()}")
    return v


@torch.no_grad()
def error_accel(joints_gt, joints_pred, vis=None, seq_ptr=None):
    """(accel [N] fp32, valid [N] bool) without a host sync: accel[i] is the acceleration error of the frames (i, i + 1,
    i + 2) - the mean over joints of |(p_i - 2 p_i+1 + p_i+2) - (g_i - 2 g_i+1 + g_i+2)|, computed in fp64 - where the three
    lie in one sequence and are visible, else 0 with valid[i] False.  joints [N, J <= 64, 3] CUDA tensors."""
    gt, pred = _joints_pair(joints_gt, joints_pred)
    N = int(gt.shape[0])
    if N == 0:
        return gt.new_zeros(0), torch.zeros(0, device=gt.device, dtype=torch.bool)
    sp, S = _dev_seq_ptr(seq_ptr, N, gt.device)
    out = _video_eval(pred, gt, sp, S, _dev_vis(vis, N, gt.device), False)
    return out["accel"], out["valid"].bool()


def compute_error_accel(joints_gt, joints_pred, vis=None):
    """coord_utils.compute_error_accel, drop-in: the [N - 2] acceleration errors of one sequence, compacted to the triples
    whose three frames are visible when vis [N] is given.  Without vis nothing syncs; with vis the compaction's size is
    data-dependent, which costs ONE host sync (use error_accel for a loop without one)."""
    accel, valid = error_accel(joints_gt, joints_pred, vis)
    n = max(int(accel.shape[0]) - 2, 0)
    return accel[:n] if vis is None else accel[:n][valid[:n]]


class VideoEvaluator:
    """ve = VideoEvaluator(video_indices, J, min_cutoff=0.004, beta=0.005, smooth=True, pa=True, n=None)
    ve.put(first, pred_joints, gt_joints)        per Tester batch
    res = ve.summary()

    The smoothed block of data/PW3D/dataset.py:383-417 for the whole dataset.  video_indices: the dataset's list of boolean
    masks (or index arrays) over the dataset order, one per video; turned into a row table and sequence offsets once
    (sequence_tables).  A video's frames need not be contiguous: the reference's are not for two-person videos, whose
    datalist is sorted by person_id first.
    put: root-centred evaluation joints [b, J, 3] (CUDA) of dataset positions first .. first + b - 1, copied into device
    buffers (no sync).  Positions never put stay zero.
    summary: gathers each video's frames, filters the prediction (smooth=True: smooth_pose(min_cutoff, beta) per video;
    the filter kernel gathers through the row table itself), runs p2m_video_eval and syncs once.  Returns
      accel_error  unweighted mean over videos of the per-video mean acceleration error
      mpjpe        unweighted mean over videos of the per-video MPJPE
      pa_mpjpe     mean pooled over all frames and joints (pa=True)
      per_video    {"frames", "accel_frames", "accel_error", "mpjpe", "pa_mpjpe"}: arrays of one entry per video
      videos, videos_without_accel, empty_videos, frames
    which is the reference's aggregation, except that a video without a valid acceleration triple (NaN in per_video) is
    left out of accel_error and counted in videos_without_accel instead of turning the total into NaN, and an empty video
    is left out of mpjpe likewise.  The per-frame device tensors of the last summary() are in ve.last."""

    def __init__(self, video_indices, J, min_cutoff=0.004, beta=0.005, smooth=True, pa=True, n=None):
        self.J = int(J)
        if not 1 <= self.J <= 64:
            raise ValueError("J outside 1..64")
        self.rows, self.seq_ptr, self.n = sequence_tables(video_indices, n)
        self.S = len(self.seq_ptr) - 1
        self.N = int(self.seq_ptr[-1])
        self.min_cutoff, self.beta, self.smooth, self.pa = float(min_cutoff), float(beta), bool(smooth), bool(pa)
        self._dev = None
        self.last = None

    def _buffers(self, dev):
        if self._dev is None:
            self._dev = dev
            self._pred = torch.zeros((self.n, self.J, 3), device=dev, dtype=torch.float32)
            self._gt = torch.zeros((self.n, self.J, 3), device=dev, dtype=torch.float32)
            self._rows = torch.from_numpy(self.rows).to(dev)
            self._sp = torch.from_numpy(self.seq_ptr).to(dev)
        elif dev != self._dev:
            raise ValueError(f"this evaluator's buffers are on {self._dev}, got a tensor on {dev}")

    @torch.no_grad()
    def put(self, first, pred_joints, gt_joints):
        pred, gt = _cuda_f32(pred_joints, "pred_joints"), _cuda_f32(gt_joints, "gt_joints")
        if pred.dim() != 3 or tuple(pred.shape[1:]) != (self.J, 3) or pred.shape != gt.shape:
            raise ValueError(f"pred_joints / gt_joints: expected equal [b, {self.J}, 3], got {tuple(pred.shape)}, "
                             f"{tuple(gt.shape)}")
        first, b = int(first), int(pred.shape[0])
        if first < 0 or first + b > self.n:
            raise ValueError(f"put: positions {first} .. {first + b - 1} outside the dataset's [0, {self.n})")
        self._buffers(pred.device)
        self._pred[first:first + b].copy_(pred)
        self._gt[first:first + b].copy_(gt)

    @torch.no_grad()
    def summary(self):
        if self._dev is None:
            raise ValueError("summary() before any put()")
        if self.N == 0:
            nan = float("nan")
            z = _np.zeros(self.S)
            return {"accel_error": nan, "mpjpe": nan, "pa_mpjpe": nan, "videos": self.S, "videos_without_accel": self.S,
                    "empty_videos": self.S, "frames": 0,
                    "per_video": {"frames": z, "accel_frames": z, "accel_error": z + nan, "mpjpe": z + nan, "pa_mpjpe": z + nan}}
        rows64 = self._rows.long()
        gt = self._gt.index_select(0, rows64)
        if self.smooth:
            pred = torch.empty((self.N, self.J, 3), device=self._dev, dtype=torch.float32)
            _one_euro(self._pred, self._sp, self._rows, self.N, self.S, self.J * 3, self.min_cutoff, self.beta, 1.0, 1.0,
                      None, pred)
        else:
            pred = self._pred.index_select(0, rows64)
        out = _video_eval(pred, gt, self._sp, self.S, None, self.pa)
        stats = out["stats"].cpu().numpy()                      # the one sync
        seq, tot = stats[:self.S], stats[self.S]
        self.last = {"pred": pred, "gt": gt, "accel": out["accel"], "valid": out["valid"].bool(), "mpjpe": out["mpjpe"],
                     "pa_mpjpe": out["pa_mpjpe"], "seq_stats": out["stats"][:self.S], "totals": out["stats"][self.S]}
        with _np.errstate(invalid="ignore", divide="ignore"):
            pa_pv = seq[:, 4] / seq[:, 5]
        return {"accel_error": float(tot[0]), "mpjpe": float(tot[1]), "pa_mpjpe": float(tot[2]) if self.pa else float("nan"),
                "videos": self.S, "videos_without_accel": int(tot[4]), "empty_videos": int(tot[6]),
                "frames": int(tot[7]),
                "per_video": {"frames": seq[:, 0].copy(), "accel_frames": seq[:, 1].copy(), "accel_error": seq[:, 2].copy(),
                              "mpjpe": seq[:, 3].copy(), "pa_mpjpe": pa_pv}}
