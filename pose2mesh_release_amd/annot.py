"""Dataset annotations to camera-frame body parameters on the GPU, and a bank of body models chosen per sample by gender:
what get_smpl_coord / get_mano_coord of the reference's datasets do per sample in numpy and transforms3d on a dataloader
worker, for a batch of row indices - csrc/annot.hip, include/p2m.h "dataset annotations".

  src = AnnotationSource(pose, betas, trans, cam_R, cam_t, focal=f, princpt=c, gender=g, models=bank, preset="human36m")
  batch = src(idx)                                   batch.pose, .betas, .trans, .focal, .princpt, .gender, .given_cam,
                                                     .given_img, .status: one p2m_annot_gather launch
  bank = GenderedBody([male, female, neutral])       BodyModels of one shape
  verts, joints[, extra] = bank(batch.pose, batch.betas, batch.trans, batch.gender)

The tables are uploaded once; a call reads idx on the device, allocates and synchronises nothing once the buffers of a batch
size exist, and so sits in a torch.cuda.graph together with the bank, TrainSampleBuilder and the train step.  There is no CPU
fallback: CPU tensors raise P2MError.

Two deliberate differences from the reference (include/p2m.h has the arithmetic): a zero root pose is the identity rotation
(the reference divides 0 / 0 and feeds NaNs to the body model), and the root compensation of Human3.6M uses the rest root
joint folded from the model tables in float64 (the reference subtracts the root joint its layer returned in fp32; the two
differ by fp32 rounding of a metre-sized value).
"""
import ctypes as _ct
import types as _types

import numpy as _np
import torch

from . import _lib
from .body import BodyModel

MAX_MODELS = 4
MAX_GIVEN_JOINTS = 32
STATUS_BAD_INDEX, STATUS_BAD_GENDER, STATUS_BETA_RESET, STATUS_NON_FINITE = 1, 2, 4, 8

# the flag sets of the reference's seven datasets (what each get_smpl_coord / get_mano_coord does to the parameters)
PRESETS = {
    # data/Human36M/dataset.py:264 (reset), :267-273 (root rotation), :286-291 (R trans + t / 1000 - J0 + R J0)
    "human36m": dict(rotate_root=True, beta_reset=True, compensate_root=True, t_scale=1e-3),
    # data/AMASS/dataset.py:189-196 (root rotation), :206-207 (+ t in metres; no trans table)
    "amass": dict(rotate_root=True, beta_reset=False, compensate_root=False, t_scale=1.0),
    # data/FreiHAND/dataset.py:120-126 (root rotation), :117, :130 (t goes in as the layer's translation)
    "freihand": dict(rotate_root=True, beta_reset=False, compensate_root=False, t_scale=1.0),
    # data/PW3D/dataset.py:86-93: pose, shape and trans as annotated, the layer picked by gender
    "pw3d": dict(rotate_root=False, beta_reset=False, compensate_root=False, t_scale=1.0),
    # data/SURREAL/dataset.py:64-69: the same
    "surreal": dict(rotate_root=False, beta_reset=False, compensate_root=False, t_scale=1.0),
    # data/MuCo/dataset.py:198-205: as annotated, but :202 resets far-off shapes
    "muco": dict(rotate_root=False, beta_reset=True, compensate_root=False, t_scale=1.0),
    # data/COCO/dataset.py:147-166: the same, the reset at :154
    "coco": dict(rotate_root=False, beta_reset=True, compensate_root=False, t_scale=1.0),
}


def _p(t):
    return None if t is None else _ct.c_void_p(t.data_ptr())


def _cur_stream():
    return _ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _host(x, dtype=_np.float32):
    """An array or tensor (any device) -> a C-contiguous numpy array of `dtype` (None stays None)."""
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return _np.ascontiguousarray(_np.asarray(x), dtype)


def _out(x, name, shape, dtype, dev):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.P2MError(f"{name}: the annotation kernels need a CUDA tensor (there is no CPU path)")
    if tuple(x.shape) != tuple(shape) or x.dtype != dtype or not x.is_contiguous() or x.device != dev:
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor {list(shape)} on {dev}")
    return x


class GenderedBody:
    """bank = GenderedBody(models);  verts, joints[, extra] = bank(pose, betas, trans, gender)

    models: a list, or a dict (its values in order; the keys are kept as bank.names), of at most 4 BodyModels with equal V,
    NJ, JX, J and nb.  gender [B] int32 on the device picks the model per sample (outside [0, G): model 0) - what
    self.mesh_model.layer[gender] does in Human36M, 3DPW and SURREAL.  A call runs EACH model's forward on the whole batch and
    then one p2m_body_select launch into the bank's own buffers (reused per batch size, as BodyModel's): G forwards, the
    price of leaving the forward kernels as they are (DESIGN.md has the measured cost).  With one model the call is that
    model's forward and returns its buffers; nothing else is launched."""

    def __init__(self, models):
        if isinstance(models, dict):
            self.names, models = list(models.keys()), list(models.values())
        else:
            models = list(models)
            self.names = list(range(len(models)))
        if not 1 <= len(models) <= MAX_MODELS:
            raise ValueError(f"models: expected 1 to {MAX_MODELS} BodyModels, got {len(models)}")
        for m in models:
            if not isinstance(m, BodyModel):
                raise TypeError("models: every entry must be a BodyModel")
        m0 = models[0]
        for k in ("V", "NJ", "JX", "J", "nb"):
            vals = [getattr(m, k) for m in models]
            if any(v != vals[0] for v in vals):
                raise ValueError(f"models: unequal {k} {vals} - a bank's models share V, NJ, JX, J and nb")
        self.models = models
        self.G, self.V, self.NJ, self.JX, self.J, self.nb = len(models), m0.V, m0.NJ, m0.JX, m0.J, m0.nb
        self._bufs = {}

    def root_tables(self):
        """(root_template [G, 3], root_shapedirs [G, 3, nb]) fp32: the root joint's rows of the models' folded rest-joint
        tables, what AnnotationSource(models=...) uploads for compensate_root."""
        return (_np.stack([_np.asarray(m._host["jt"][0], _np.float32) for m in self.models]),
                _np.stack([_np.asarray(m._host["js"][0], _np.float32).reshape(3, self.nb) for m in self.models]))

    def _buffers(self, B, dev):
        b = self._bufs.get((B, dev))
        if b is None:
            b = [torch.zeros((B, n, 3), device=dev, dtype=torch.float32) for n in (self.V, self.NJ, self.JX) if n]
            self._bufs[(B, dev)] = b
        return b

    @torch.no_grad()
    def __call__(self, pose, betas=None, trans=None, gender=None):
        if self.G == 1:
            return self.models[0](pose, betas, trans)
        if not isinstance(gender, torch.Tensor) or not gender.is_cuda:
            raise _lib.P2MError("gender: the bank needs a CUDA int32 tensor [B] (there is no CPU path)")
        outs = [m(pose, betas, trans) for m in self.models]
        B, dev = int(outs[0][0].shape[0]), outs[0][0].device
        if tuple(gender.shape) != (B,) or gender.device != dev:
            raise ValueError(f"gender: expected [{B}] on {dev}, got {list(gender.shape)} on {gender.device}")
        gender = gender.contiguous() if gender.dtype == torch.int32 else gender.to(torch.int32).contiguous()
        buf = self._buffers(B, dev)
        ptrs = [(_ct.c_void_p * self.G)(*[o[k].data_ptr() for o in outs]) for k in range(len(buf))]
        with torch.cuda.device(dev):
            _lib.check(_lib.hip().p2m_body_select(
                ptrs[0], ptrs[1], ptrs[2] if self.JX else None, self.G, _p(gender), B, self.V, self.NJ, self.JX, _p(buf[0]),
                _p(buf[1]), _p(buf[2]) if self.JX else None, _cur_stream()), "p2m_body_select")
        return tuple(buf)


class AnnotationSource:
    """src = AnnotationSource(pose [N, 3 J], betas [N, nb], trans=None, cam_R=None, cam_t=None, focal= [N, 2], princpt= [N, 2],
                             gender=None, given_cam=None, given_img=None, models=None, preset=None, rotate_root=False,
                             beta_reset=False, compensate_root=False, t_scale=1.0, beta_limit=3.0, device="cuda")
    batch = src(idx, out=None)

    Arrays or tensors, one row per annotated frame, uploaded once: trans [N, 3] (None: zeros), cam_R [N, 3, 3] or [N, 9]
    (None: identity), cam_t [N, 3] (None: zeros), gender [N] integers (None: all 0), given_cam [N, Jr, 3] / given_img [N, Jr,
    2]: the annotated joints TrainSampleBuilder takes as given= (None: skipped).  models: a GenderedBody, a BodyModel or a
    pair (root_template [G, 3], root_shapedirs [G, 3, nb]) - the root tables of compensate_root and the number of models a
    gender may name; None: one model, no tables.  preset: a key of PRESETS; explicit flags override it.

    idx [B]: an int32 or int64 CUDA tensor of row indices (a slice of torch.randperm).  The result is a namespace of the
    static buffers of that batch size - pose, betas, trans, focal, princpt, gender (int32), given_cam, given_img (None when
    not given), status (int32; STATUS_* bits) - overwritten by the next call of the same size; out= takes the caller's
    (buffers(B) makes a set).  An index outside [0, N) gives a zero sample with status bit 0, never a read at it."""

    def __init__(self, pose, betas, trans=None, cam_R=None, cam_t=None, focal=None, princpt=None, gender=None, given_cam=None,
                 given_img=None, models=None, preset=None, rotate_root=None, beta_reset=None, compensate_root=None,
                 t_scale=None, beta_limit=3.0, device="cuda"):
        flags = dict(rotate_root=False, beta_reset=False, compensate_root=False, t_scale=1.0)
        if preset is not None:
            if preset not in PRESETS:
                raise ValueError(f"preset: one of {sorted(PRESETS)}, got {preset!r}")
            flags.update(PRESETS[preset])
        for k, v in dict(rotate_root=rotate_root, beta_reset=beta_reset, compensate_root=compensate_root, t_scale=t_scale).items():
            if v is not None:
                flags[k] = v
        self.rotate_root, self.beta_reset = bool(flags["rotate_root"]), bool(flags["beta_reset"])
        self.compensate_root, self.t_scale, self.beta_limit = bool(flags["compensate_root"]), float(flags["t_scale"]), float(beta_limit)
        if focal is None or princpt is None:
            raise ValueError("focal and princpt are required ([N, 2] each)")
        h = {"pose": _host(pose), "betas": _host(betas)}
        if h["pose"].ndim != 2 or h["pose"].shape[0] < 1 or h["pose"].shape[1] % 3 or not 3 <= h["pose"].shape[1] <= 192:
            raise ValueError(f"pose: expected [N >= 1, 3 J] with J in [1, 64], got {list(h['pose'].shape)}")
        N, self.J = int(h["pose"].shape[0]), int(h["pose"].shape[1]) // 3
        if h["betas"] is None:
            h["betas"] = _np.zeros((N, 0), _np.float32)
        if h["betas"].ndim != 2 or h["betas"].shape[0] != N or h["betas"].shape[1] > 64:
            raise ValueError(f"betas: expected [{N}, nb <= 64], got {list(h['betas'].shape)}")
        self.N, self.nb = N, int(h["betas"].shape[1])
        for name, x, shape in (("trans", trans, (N, 3)), ("cam_t", cam_t, (N, 3)), ("focal", focal, (N, 2)),
                               ("princpt", princpt, (N, 2))):
            h[name] = _host(x)
            if h[name] is not None and h[name].shape != shape:
                raise ValueError(f"{name}: expected {list(shape)}, got {list(h[name].shape)}")
        h["cam_R"] = _host(cam_R)
        if h["cam_R"] is not None:
            if h["cam_R"].shape not in ((N, 3, 3), (N, 9)):
                raise ValueError(f"cam_R: expected [{N}, 3, 3] or [{N}, 9], got {list(h['cam_R'].shape)}")
            h["cam_R"] = h["cam_R"].reshape(N, 9)
        h["gender"] = None
        if gender is not None:
            gnd = _host(gender, _np.int64)
            if gnd.shape != (N,) or gnd.min() < 0 or gnd.max() > 255:
                raise ValueError(f"gender: expected [{N}] integers in [0, 255], got {list(gnd.shape)}")
            h["gender"] = gnd.astype(_np.uint8)
        self.Jr = 0
        h["given_cam"], h["given_img"] = _host(given_cam), _host(given_img)
        for name, c in (("given_cam", 3), ("given_img", 2)):
            x = h[name]
            if x is None:
                continue
            if x.ndim != 3 or x.shape[0] != N or x.shape[2] != c or not 1 <= x.shape[1] <= MAX_GIVEN_JOINTS:
                raise ValueError(f"{name}: expected [{N}, Jr <= {MAX_GIVEN_JOINTS}, {c}], got {list(x.shape)}")
            if self.Jr and x.shape[1] != self.Jr:
                raise ValueError(f"given_img: {x.shape[1]} joints, given_cam {self.Jr}")
            self.Jr = int(x.shape[1])
        self.G = 1
        h["root_template"] = h["root_shapedirs"] = None
        if models is not None:
            if isinstance(models, BodyModel):
                models = GenderedBody([models])
            rt, rs = models.root_tables() if isinstance(models, GenderedBody) else models
            rt, rs = _host(rt), _host(rs)
            if rt.ndim != 2 or rt.shape[1] != 3 or not 1 <= rt.shape[0] <= MAX_MODELS:
                raise ValueError(f"root_template: expected [G <= {MAX_MODELS}, 3], got {list(rt.shape)}")
            self.G = int(rt.shape[0])
            if rs.shape != (self.G, 3, self.nb):
                raise ValueError(f"root_shapedirs: expected [{self.G}, 3, {self.nb}] (the tables' nb), got {list(rs.shape)}")
            if isinstance(models, GenderedBody) and models.J != self.J:
                raise ValueError(f"models: {models.J} joints, the pose table {self.J}")
            h["root_template"] = rt
            h["root_shapedirs"] = rs if rs.size else _np.zeros(1, _np.float32)      # nb = 0: a stand-in no kernel reads
        elif self.compensate_root:
            raise ValueError("compensate_root needs models= (the root joint's tables)")
        if torch.device(device).type != "cuda":
            raise _lib.P2MError("AnnotationSource: the tables live in device memory (there is no CPU path)")
        self.device = torch.device(device)
        self._t = {k: None if v is None or v.size == 0 else torch.from_numpy(v).to(self.device) for k, v in h.items()}
        self.device = self._t["pose"].device
        self._bufs = {}

    def buffers(self, B):
        """Freshly allocated output tensors for a batch of B (what out= takes)."""
        d, f = self.device, torch.float32
        e = lambda *sh, dt=f: torch.zeros(sh, device=d, dtype=dt)  # noqa: E731
        t = self._t
        return _types.SimpleNamespace(
            pose=e(B, 3 * self.J), betas=e(B, self.nb), trans=e(B, 3), focal=e(B, 2), princpt=e(B, 2),
            gender=e(B, dt=torch.int32), status=e(B, dt=torch.int32),
            given_cam=e(B, self.Jr, 3) if t["given_cam"] is not None else None,
            given_img=e(B, self.Jr, 2) if t["given_img"] is not None else None)

    @torch.no_grad()
    def __call__(self, idx, out=None):
        if not isinstance(idx, torch.Tensor) or not idx.is_cuda:
            raise _lib.P2MError("idx: the annotation kernels need a CUDA tensor (there is no CPU path)")
        if idx.dim() != 1 or idx.shape[0] < 1 or idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"idx: expected an int32 or int64 tensor [B >= 1], got {idx.dtype} {list(idx.shape)}")
        dev, B = self.device, int(idx.shape[0])
        if idx.device != dev:
            raise ValueError(f"idx on {idx.device}, the tables on {dev}")
        idx = idx.contiguous()
        if out is None:
            out = self._bufs.get(B)
            if out is None:
                out = self._bufs[B] = self.buffers(B)
        t = self._t
        f, i4 = torch.float32, torch.int32
        for k, sh, dt in (("pose", (B, 3 * self.J), f), ("betas", (B, self.nb), f), ("trans", (B, 3), f), ("focal", (B, 2), f),
                          ("princpt", (B, 2), f), ("gender", (B,), i4), ("status", (B,), i4)):
            _out(getattr(out, k), k, sh, dt, dev)
        gc = _out(out.given_cam, "given_cam", (B, self.Jr, 3), f, dev) if t["given_cam"] is not None else None
        gi = _out(out.given_img, "given_img", (B, self.Jr, 2), f, dev) if t["given_img"] is not None else None
        with torch.cuda.device(dev):
            _lib.check(_lib.hip().p2m_annot_gather(
                _p(t["pose"]), _p(t["betas"]), _p(t["trans"]), _p(t["cam_R"]), _p(t["cam_t"]), _p(t["focal"]), _p(t["princpt"]),
                _p(t["gender"]), _p(t["given_cam"]), _p(t["given_img"]), self.N, self.J, self.nb, self.Jr, _p(idx),
                int(idx.dtype == torch.int64), B, _p(t["root_template"]), _p(t["root_shapedirs"]), self.G,
                int(self.rotate_root), int(self.beta_reset), int(self.compensate_root), self.beta_limit, self.t_scale,
                _p(out.pose), _p(out.betas) if self.nb else None, _p(out.trans), _p(out.focal), _p(out.princpt), _p(out.gender),
                _p(gc), _p(gi), _p(out.status), _cur_stream()), "p2m_annot_gather")
        return out
