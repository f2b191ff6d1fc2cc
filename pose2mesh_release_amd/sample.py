"""Training samples on the GPU: mesh + camera in, the tensors of the train step out (TrainSampleBuilder), and the synthetic
2D detector errors that every released recipe of the reference puts in place of the clean input joints (use_gt_input:
False) on their own - csrc/sample.hip, include/p2m.h "training-sample noise" and "training samples".

  build = TrainSampleBuilder(reg_regressor, input_regressor, midpoints, roots, flip_pairs, noise="coco")
  s = build(verts, focal, princpt)                     s.pose2d, s.mesh, s.lift_pose3d, s.reg_pose3d, s.*_valid, s.status

  stream = NoiseStream(seed=123)                       the device words {seed, first sample index} of the Philox stream
  out, kind = noise_coco(joints, area, stream)         synthesize_pose (lib/noise_utils.py:17-285), COCO joint set
  out = noise_table(pose, mean, std, weight, stream)   generate_syn_error (data/AMASS/dataset.py:77-89, 327-329)

Sample b of a call uses the global index stream.index + b, and a call advances the index by B with an ordinary tensor add:
results depend on (seed, global index) alone, never on how the samples were batched, and a call - the advance included -
can sit in a torch.cuda.graph and replays with fresh numbers.  Nothing allocates once `out` is given.  There is no CPU
fallback: CPU tensors raise P2MError.
"""
import ctypes as _ct
import types as _types

import numpy as _np
import torch

from . import _lib

# the 17 published COCO OKS sigmas / 10 (nose, eyes, ears, shoulders, elbows, wrists, hips, knees, ankles)
COCO_SIGMAS = tuple(s / 10.0 for s in (.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89))
KIND_JITTER, KIND_MISS, KIND_INVERSION, KIND_GOOD, KIND_ZEROED = 0, 1, 2, 4, -1
MAX_TABLE_JOINTS = 32


def _p(t):
    return None if t is None else _ct.c_void_p(t.data_ptr())


def _cur_stream():
    return _ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda(x, name, shape, dtype=torch.float32):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.P2MError(f"{name}: the sample kernels need a CUDA tensor (there is no CPU path)")
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name}: expected {list(shape)}, got {list(x.shape)}")
    return x.contiguous() if x.dtype == dtype else x.to(dtype).contiguous()


def _out(x, name, shape, dtype, dev):
    if x is None:
        return torch.empty(shape, device=dev, dtype=dtype)
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.P2MError(f"{name}: the sample kernels need a CUDA tensor (there is no CPU path)")
    if tuple(x.shape) != tuple(shape) or x.dtype != dtype or not x.is_contiguous() or x.device != dev:
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor {list(shape)} on {dev}")
    return x


class NoiseStream:
    """The two device words of the stream: state[0] = seed, state[1] = global index of the next sample (an int64 tensor: the
    kernels read the same bits as uint64, and an int64 add wraps the same way)."""

    def __init__(self, seed=123, first_index=0, device="cuda"):
        if torch.device(device).type != "cuda":
            raise _lib.P2MError("NoiseStream: the state words live in device memory (there is no CPU path)")
        self.state = torch.tensor([self._s64(seed), self._s64(first_index)], dtype=torch.int64, device=device)

    def advance(self, n):
        """index += n, on the current stream (capturable)."""
        self.state[1:2].add_(int(n))

    @property
    def index(self):
        return int(self.state[1].item()) & 0xFFFFFFFFFFFFFFFF

    def seek(self, first_index):
        self.state[1:2].fill_(NoiseStream._s64(first_index))

    @staticmethod
    def _s64(v):
        v = int(v) & 0xFFFFFFFFFFFFFFFF
        return v - (1 << 64) if v >= 1 << 63 else v


_sigma_cache = {}


def _sigmas(sigmas, dev):
    key = (dev, tuple(float(s) for s in (COCO_SIGMAS if sigmas is None else _np.asarray(sigmas).reshape(-1).tolist())))
    if len(key[1]) != 17:
        raise ValueError(f"sigmas: expected 17 values, got {len(key[1])}")
    t = _sigma_cache.get(key)
    if t is None:
        t = _sigma_cache[key] = torch.tensor(key[1], dtype=torch.float32, device=dev)
    return t


@torch.no_grad()
def noise_coco(joints, area, stream, sigmas=None, out=None, kind=None, advance=True):
    """joints [B, 17, 3] (x, y, valid), area [B] -> out [B, 17, 3], kind [B, 17] int8 (KIND_*).  sigmas: 17 values or a CUDA
    tensor (default COCO_SIGMAS).  out / kind: the caller's static tensors (out must not be joints).  One launch, then the
    stream's index advances by B (advance=False: the caller does it)."""
    if not isinstance(joints, torch.Tensor) or not joints.is_cuda:
        raise _lib.P2MError("joints: the sample kernels need a CUDA tensor (there is no CPU path)")
    if joints.dim() != 3 or joints.shape[0] < 1:
        raise ValueError(f"joints: expected [B >= 1, 17, 3], got {list(joints.shape)}")
    B, dev = int(joints.shape[0]), joints.device
    joints = _cuda(joints, "joints", (B, 17, 3))
    area = _cuda(area, "area", (B,))
    sg = _cuda(sigmas, "sigmas", (17,)) if isinstance(sigmas, torch.Tensor) else _sigmas(sigmas, dev)
    out = _out(out, "out", (B, 17, 3), torch.float32, dev)
    kind = _out(kind, "kind", (B, 17), torch.int8, dev)
    if stream.state.device != dev:
        raise ValueError(f"the stream's state is on {stream.state.device}, joints on {dev}")
    with torch.cuda.device(dev):
        _lib.check(_lib.hip().p2m_pose_noise_coco(_p(joints), _p(area), _p(sg), _p(stream.state), _p(out), _p(kind), B,
                                                  _cur_stream()), "p2m_pose_noise_coco")
        if advance:
            stream.advance(B)
    return out, kind


@torch.no_grad()
def noise_table(pose, mean, std, weight, stream, input_shape=(384, 288), out=None, advance=True):
    """pose [B, J, 2] -> out [B, J, 2] = pose + [weight > u] * N(mean, std) / 256 * (W, H), with input_shape = (H, W) as in
    cfg.MODEL.input_shape.  mean, std [J, 2], weight [J]: CUDA tensors (the error table, uploaded once by the caller);
    J <= 32.  out may be pose itself."""
    if not isinstance(pose, torch.Tensor) or not pose.is_cuda:
        raise _lib.P2MError("pose: the sample kernels need a CUDA tensor (there is no CPU path)")
    if pose.dim() != 3 or pose.shape[0] < 1 or pose.shape[2] != 2:
        raise ValueError(f"pose: expected [B >= 1, J, 2], got {list(pose.shape)}")
    B, J, dev = int(pose.shape[0]), int(pose.shape[1]), pose.device
    pose = _cuda(pose, "pose", (B, J, 2))
    mean, std, weight = _cuda(mean, "mean", (J, 2)), _cuda(std, "std", (J, 2)), _cuda(weight, "weight", (J,))
    out = _out(out, "out", (B, J, 2), torch.float32, dev)
    if stream.state.device != dev:
        raise ValueError(f"the stream's state is on {stream.state.device}, pose on {dev}")
    with torch.cuda.device(dev):
        _lib.check(_lib.hip().p2m_pose_noise_table(_p(pose), _p(mean), _p(std), _p(weight), J, float(input_shape[1]),
                                                   float(input_shape[0]), _p(stream.state), _p(out), B, _cur_stream()),
                   "p2m_pose_noise_table")
        if advance:
            stream.advance(B)
    return out


NOISE_MODES = {None: 0, "none": 0, "coco": 1, "table": 2}


def _csr(R, nv_name):
    R = _np.asarray(R, _np.float32)
    if R.ndim != 2 or R.shape[0] < 1:
        raise ValueError(f"{nv_name}: expected a dense [J, nv] matrix, got {list(R.shape)}")
    ptr, idx, val = [0], [], []
    for row in R:
        nz = _np.flatnonzero(row)
        idx.extend(nz.tolist())
        val.extend(row[nz].tolist())
        ptr.append(len(idx))
    return _np.asarray(ptr, _np.int32), _np.asarray(idx, _np.int32), _np.asarray(val, _np.float32)


def _iarr(pairs, name):
    a = _np.asarray(list(pairs), _np.int32).reshape(-1, 2) if len(pairs) else _np.zeros((0, 2), _np.int32)
    return _np.ascontiguousarray(a)


class TrainSampleBuilder:
    """The dataset chain of the reference (data/AMASS/dataset.py:246-330 and its siblings) for a batch on the device:
    p2m_train_sample, include/p2m.h "training samples".

    reg_regressor [Jr, nv] (dense, numpy): the h36m regressor; input_regressor [Ji, nv] or None (the input set is the reg
    set); midpoints: pairs (a, b) of input rows appended as (a + b) / 2 (pelvis, neck); roots = (reg_root, input_root);
    flip_pairs over the J = Ji + len(midpoints) input joints; input_shape = (H, W); noise "coco" | "table" | None; sigmas: 17
    values (coco); table = (mean [J, 2], std [J, 2], weight [J]) (table); rotate_factor / flip: cfg.AUG's, used when a call
    gives no rot / flip; fit_thr: Human36M's fitting_thr for calls with given=.  The builder owns the stream's device words
    and advances the index by B after each call with a tensor add: a call can sit in a torch.cuda.graph."""

    def __init__(self, reg_regressor, input_regressor=None, midpoints=(), roots=(0, 0), flip_pairs=(), input_shape=(384, 288),
                 noise="coco", sigmas=None, table=None, rotate_factor=0, flip=False, seed=123, fit_thr=0.0, device="cuda"):
        if torch.device(device).type != "cuda":
            raise _lib.P2MError("TrainSampleBuilder: the sample kernels need a CUDA device (there is no CPU path)")
        if noise not in NOISE_MODES:
            raise ValueError(f"noise: expected 'coco', 'table' or None, got {noise!r}")
        self.device = torch.device(device)
        self.noise_mode = NOISE_MODES[noise]
        rr = _csr(reg_regressor, "reg_regressor")
        self.nv, self.Jr = int(_np.asarray(reg_regressor).shape[1]), int(_np.asarray(reg_regressor).shape[0])
        self._rr = [torch.from_numpy(a).to(self.device) for a in rr]
        self._ir, self.Ji = [None, None, None], self.Jr
        self._mid = _iarr(midpoints, "midpoints")
        if input_regressor is not None:
            if _np.asarray(input_regressor).shape[1] != self.nv:
                raise ValueError("input_regressor: another vertex count than reg_regressor")
            self.Ji = int(_np.asarray(input_regressor).shape[0])
            self._ir = [torch.from_numpy(a).to(self.device) for a in _csr(input_regressor, "input_regressor")]
        self.J = self.Ji + len(self._mid) if input_regressor is not None else self.Jr
        self._pairs = _iarr(flip_pairs, "flip_pairs")
        self.reg_root, self.input_root = int(roots[0]), int(roots[1])
        self.H, self.W = float(input_shape[0]), float(input_shape[1])
        self.rotate_factor, self.flip, self.fit_thr = float(rotate_factor), bool(flip), float(fit_thr)
        self._sigmas = self._table = None
        if self.noise_mode == 1:
            self._sigmas = _cuda(sigmas, "sigmas", (17,)) if isinstance(sigmas, torch.Tensor) else _sigmas(sigmas, self.device)
        if self.noise_mode == 2:
            if table is None:
                raise ValueError("noise='table' needs table=(mean [J, 2], std [J, 2], weight [J])")
            shapes = ((self.J, 2), (self.J, 2), (self.J,))
            self._table = [torch.as_tensor(_np.asarray(t, _np.float32)).reshape(sh).contiguous().to(self.device)
                           if not isinstance(t, torch.Tensor) else _cuda(t, "table", sh) for t, sh in zip(table, shapes)]
        self.stream = NoiseStream(seed, 0, self.device)
        self._bufs = {}

    def buffers(self, B):
        """Freshly allocated output tensors for a batch of B (what out= takes)."""
        d, f = self.device, torch.float32
        e = lambda *sh, dt=f: torch.zeros(sh, device=d, dtype=dt)  # noqa: E731
        return _types.SimpleNamespace(
            pose2d=e(B, self.J, 2), mesh=e(B, self.nv, 3), lift_pose3d=e(B, self.J, 3), reg_pose3d=e(B, self.Jr, 3),
            mesh_valid=e(B, self.nv), lift_valid=e(B, self.J), reg_valid=e(B, self.Jr), status=e(B, dt=torch.int32),
            fit_err=e(B), kind=e(B, 17, dt=torch.int8), rot_flip=e(B, 2))

    @torch.no_grad()
    def __call__(self, verts, focal, princpt, trans=None, mesh_scale=1000.0, out=None, rot=None, flip=None, given=None):
        """verts [B, nv, 3], focal / princpt [B, 2], trans [B, 3] -> the namespace of buffers().  rot [B] degrees / flip [B]
        int32: given, else drawn.  given = (reg_cam [B, Jr, 3], reg_img [B, Jr, 2] or None): annotated reg joints."""
        if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
            raise _lib.P2MError("verts: the sample kernels need a CUDA tensor (there is no CPU path)")
        if verts.dim() != 3 or verts.shape[0] < 1 or tuple(verts.shape[1:]) != (self.nv, 3):
            raise ValueError(f"verts: expected [B >= 1, {self.nv}, 3], got {list(verts.shape)}")
        B, dev = int(verts.shape[0]), verts.device
        if dev != self.stream.state.device:
            raise ValueError(f"verts on {dev}, the builder on {self.stream.state.device}")
        verts = _cuda(verts, "verts", (B, self.nv, 3))
        focal, princpt = _cuda(focal, "focal", (B, 2)), _cuda(princpt, "princpt", (B, 2))
        trans = None if trans is None else _cuda(trans, "trans", (B, 3))
        rot = None if rot is None else _cuda(rot, "rot", (B,))
        flip = None if flip is None else _cuda(flip, "flip", (B,), torch.int32)
        gcam = gimg = None
        if given is not None:
            gcam = _cuda(given[0], "given reg_cam", (B, self.Jr, 3))
            gimg = None if given[1] is None else _cuda(given[1], "given reg_img", (B, self.Jr, 2))
        if out is None:
            out = self._bufs.get(B)
            if out is None:
                out = self._bufs[B] = self.buffers(B)
        shapes = dict(pose2d=(B, self.J, 2), mesh=(B, self.nv, 3), lift_pose3d=(B, self.J, 3), reg_pose3d=(B, self.Jr, 3),
                      mesh_valid=(B, self.nv), lift_valid=(B, self.J), reg_valid=(B, self.Jr))
        for k, sh in shapes.items():
            _out(getattr(out, k), k, sh, torch.float32, dev)
        _out(out.status, "status", (B,), torch.int32, dev)
        opt = {k: getattr(out, k, None) for k in ("fit_err", "kind", "rot_flip")}
        for k, (sh, dt) in dict(fit_err=((B,), torch.float32), kind=((B, 17), torch.int8), rot_flip=((B, 2), torch.float32)).items():
            if opt[k] is not None:
                _out(opt[k], k, sh, dt, dev)
        lib = _lib.hip()
        work = self._bufs.get(("work", B))
        if work is None:
            work = self._bufs[("work", B)] = torch.zeros(int(lib.p2m_train_sample_workspace(B)) // 4, device=dev)
        tab = self._table or [None, None, None]
        hp = lambda a: a.ctypes.data_as(_ct.c_void_p) if a.size else None  # noqa: E731
        with torch.cuda.device(dev):
            _lib.check(lib.p2m_train_sample(
                _p(verts), _p(trans), float(mesh_scale), _p(focal), _p(princpt), B, self.nv, *[_p(t) for t in self._rr], self.Jr,
                self.reg_root, *[_p(t) for t in self._ir], self.Ji, hp(self._mid), len(self._mid), self.input_root, _p(gcam),
                _p(gimg), self.fit_thr, _p(rot), _p(flip), self.rotate_factor, int(self.flip), self.noise_mode,
                _p(self._sigmas), _p(tab[0]), _p(tab[1]), _p(tab[2]), hp(self._pairs), len(self._pairs), self.W, self.H,
                _p(self.stream.state), _p(work), work.numel() * 4, _p(out.pose2d), _p(out.mesh), _p(out.lift_pose3d),
                _p(out.reg_pose3d), _p(out.mesh_valid), _p(out.lift_valid), _p(out.reg_valid), _p(out.status), _p(opt["fit_err"]),
                _p(opt["kind"]) if self.noise_mode == 1 else None, _p(opt["rot_flip"]), _cur_stream()), "p2m_train_sample")
            self.stream.advance(B)
        return out
