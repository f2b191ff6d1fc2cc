"""Evaluation on the GPU: the Tester's per-batch errors and dataset.evaluate()'s metrics (MPJPE, PA-MPJPE, MPVPE,
PA-MPVPE) without copying meshes to the host (lib/core/base.py:196-230, data/PW3D/dataset.py:273-286,322-375,
data/Human36M/dataset.py:514-572, lib/coord_utils.py:127-149).

  rigid_transform_3D(A, B), rigid_align(A, B)   batched similarity alignment of [N, 3] / [nb, N, 3] CUDA tensors
                                                (p2m_rigid_align).  LiftTester's evaluate_joint needs no mesh: its
                                                PA-MPJPE is rigid_align on the [nb, 14, 3] root-centred joint subsets.
  MeshEvaluator                                 per-sample metrics of a batch in one launch (p2m_mesh_eval) and running
                                                fp64 totals on the device; summary() syncs once.
  compute_both_err                              drop-in for the datasets' compute_both_err (two floats per batch).

Everything is accumulated in fp64 on the device, in fixed orders (bitwise reproducible), and the launches allocate and
synchronise nothing, so an evaluator call can sit in a captured graph.  There is no CPU fallback: CPU tensors raise.
"""
import ctypes as _ct

import numpy as _np
import torch

from . import _lib
from . import loss as _loss

KEYS = ("mpjpe_E", "pa_mpjpe_E", "mpjpe_A", "mpvpe", "pa_mpvpe")     # column order of sample_means / totals[:, 1:]


def _p(t):
    return None if t is None else _ct.c_void_p(t.data_ptr())


def _stream():
    return _ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda_f32(x, name):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.P2MError(f"{name}: the evaluation kernels need a CUDA tensor (there is no CPU path)")
    return x.contiguous() if x.dtype == torch.float32 else x.float().contiguous()


def rigid_transform_3D(A, B):
    """coord_utils.rigid_transform_3D, batched: A, B [N, 3] or [nb, N, 3] -> (c, R, t) of shapes [] / [nb], [3, 3] /
    [nb, 3, 3], [3] / [nb, 3] (fp32, computed in fp64): B ~ c R A + t."""
    c, R, t, _ = _rigid(A, B, False)
    return c, R, t


def rigid_align(A, B):
    """coord_utils.rigid_align, batched: c R A + t for A, B [N, 3] or [nb, N, 3]."""
    return _rigid(A, B, True)[3]


def _rigid(A, B, want_a2):
    A, B = _cuda_f32(A, "A"), _cuda_f32(B, "B")
    if A.shape != B.shape or A.dim() not in (2, 3) or A.shape[-1] != 3 or A.shape[-2] < 1:
        raise ValueError(f"A, B: expected equal [N, 3] or [nb, N, 3] shapes, got {tuple(A.shape)}, {tuple(B.shape)}")
    single = A.dim() == 2
    nb, N = (1, A.shape[0]) if single else (A.shape[0], A.shape[1])
    dev = A.device
    c = torch.empty(nb, device=dev, dtype=torch.float32)
    R = torch.empty((nb, 3, 3), device=dev, dtype=torch.float32)
    t = torch.empty((nb, 3), device=dev, dtype=torch.float32)
    A2 = torch.empty_like(A) if want_a2 else None
    with torch.cuda.device(dev):
        _lib.check(_lib.hip().p2m_rigid_align(_p(A), _p(B), nb, N, _p(c), _p(R), _p(t), _p(A2), _stream()),
                   "p2m_rigid_align")
    if single:
        return c[0], R[0], t[0], A2
    return c, R, t, A2


def _subset(sub, J, name):
    if sub is None:
        return None
    s = _np.asarray(sub, dtype=_np.int64).reshape(-1)
    if s.size < 1 or s.size > 64 or s.min() < 0 or s.max() >= J:
        raise ValueError(f"{name}: 1..64 joint indices in [0, {J}) expected")
    return s.astype(_np.int32)


class MeshEvaluator:
    """ev = MeshEvaluator(nv, regressor_A, root_A, sub_A=None, regressor_E=None, root_E=0, sub_E=None, pa_mesh=False,
                          gt_mesh_scale=1.0, n_groups=32)
    out = ev(pred_mesh, gt_mesh, gt_joints_A=None, gt_joints_E=None, B_real=None, group=None)
    totals = ev.summary();  ev.reset()

    Per sample, in the reference's order (the p2m_mesh_eval comment in include/p2m.h has the details):
      stage A  joints = regressor_A @ mesh (the ground truth's may be given: gt_joints_A), both meshes and joint sets centred
               on their own joint root_A -> mpjpe_A [B, |sub_A|], mpvpe [B]
      stage E  (regressor_E) joints of the A-centred meshes (the ground truth's may be given: gt_joints_E, the annotation's
               joint_cam), re-centred on root_E, subset sub_E -> mpjpe_E, pa_mpjpe_E [B, |sub_E|]
      pa_mesh  the A-centred prediction aligned onto the ground truth -> pa_mpvpe [B]
    pred_mesh / gt_mesh: [B, nv, 3] CUDA tensors in mesh-model order (what GraphedInference, MeshEpilogue and
    set_inference(perm_reverse=...) return); gt_mesh is read times gt_mesh_scale (the Tester's x 1000); given joints are
    used as they are.  Regressors: dense [J, nv] arrays (at most 64 joints), or None for stage A when every call passes
    both pred_joints_A and gt_joints_A.  B_real: rows >= B_real are padding (their outputs are 0 and they are not
    counted).  group: per-sample ids in [0, n_groups) (a host sequence or a CUDA tensor of >= B_real entries); other ids
    count in the overall totals only.

    A call launches on the current stream and returns a dict of per-sample device tensors (the keys of the metrics
    computed, plus "sample_means" [B, 5] fp64 in KEYS order).  Like GraphedInference's outputs, they are buffers reused
    per batch size, overwritten by the next call of the same size.  The call also adds the batch to running fp64 totals
    on the device (no host sync)."""

    def __init__(self, nv, regressor_A, root_A, sub_A=None, regressor_E=None, root_E=0, sub_E=None, pa_mesh=False,
                 gt_mesh_scale=1.0, n_groups=32):
        self.nv, self.root_A, self.root_E = int(nv), int(root_A), int(root_E)
        self.pa_mesh, self.gt_mesh_scale, self.n_groups = bool(pa_mesh), float(gt_mesh_scale), int(n_groups)
        self._host = {}
        self.JA = None
        if regressor_A is not None:
            ra = _np.asarray(regressor_A, dtype=_np.float32)
            if ra.ndim != 2 or ra.shape[1] != self.nv or not 1 <= ra.shape[0] <= 64:
                raise ValueError(f"regressor_A: expected [J <= 64, {self.nv}], got {ra.shape}")
            self.JA = int(ra.shape[0])
            t = _loss._regressor_tables(ra, self.nv)
            self._host.update(ra_ptr=t["jr_ptr"], ra_idx=t["jr_idx"], ra_val=t["jr_val"])
            self._sub_A = _subset(sub_A, self.JA, "sub_A")
        else:
            self._sub_A = None if sub_A is None else _np.asarray(sub_A, dtype=_np.int32).reshape(-1)
        self.JE = 0
        if regressor_E is not None:
            re = _np.asarray(regressor_E, dtype=_np.float32)
            if re.ndim != 2 or re.shape[1] != self.nv or not 1 <= re.shape[0] <= 64:
                raise ValueError(f"regressor_E: expected [J <= 64, {self.nv}], got {re.shape}")
            self.JE = int(re.shape[0])
            if not 0 <= self.root_E < self.JE:
                raise ValueError("root_E out of range")
            t = _loss._regressor_tables(re, self.nv)
            self._host.update(re_ptr=t["jr_ptr"], re_idx=t["jr_idx"], re_val=t["jr_val"])
            self._sub_E = _subset(sub_E, self.JE, "sub_E")
            if self._sub_E is not None:
                self._host["sub_E"] = self._sub_E
        if self._sub_A is not None:
            self._host["sub_A"] = self._sub_A
        self._dev = None
        self._bufs = {}
        self.totals = None

    def _device_tables(self, dev):
        if self._dev is None or self._dev[0] != dev:
            d = {k: torch.from_numpy(_np.ascontiguousarray(v)).to(dev) for k, v in self._host.items()}
            self._dev = (dev, d)
            self.totals = torch.zeros((self.n_groups + 1, 6), device=dev, dtype=torch.float64)
            self._bufs = {}
        return self._dev[1]

    def reset(self):
        """Clears the running totals (a device-side fill on the current stream)."""
        if self.totals is not None:
            self.totals.zero_()

    def _buffers(self, B, JA, dev):
        key = (B, JA)
        b = self._bufs.get(key)
        if b is None:
            nsA = len(self._sub_A) if self._sub_A is not None else JA
            nsE = (len(self._sub_E) if self._sub_E is not None else self.JE) if self.JE else 0

            def f(*shape):
                return torch.zeros(shape, device=dev, dtype=torch.float32)
            b = {"mpjpe_A": f(B, nsA), "mpvpe": f(B)}
            if self.JE:
                b["mpjpe_E"], b["pa_mpjpe_E"] = f(B, nsE), f(B, nsE)
            if self.pa_mesh:
                b["pa_mpvpe"] = f(B)
            b["sample_means"] = torch.zeros((B, 5), device=dev, dtype=torch.float64)
            b["group"] = torch.full((B,), -1, device=dev, dtype=torch.int32)
            self._bufs[key] = b
        return b

    @torch.no_grad()
    def __call__(self, pred_mesh, gt_mesh, gt_joints_A=None, gt_joints_E=None, B_real=None, group=None, pred_joints_A=None):
        pred, gt = _cuda_f32(pred_mesh, "pred_mesh"), _cuda_f32(gt_mesh, "gt_mesh")
        if pred.dim() != 3 or tuple(pred.shape[1:]) != (self.nv, 3) or pred.shape != gt.shape:
            raise ValueError(f"pred_mesh / gt_mesh: expected [B, {self.nv}, 3], got {tuple(pred.shape)}, {tuple(gt.shape)}")
        B = int(pred.shape[0])
        B_real = B if B_real is None else int(B_real)
        if not 0 <= B_real <= B:
            raise ValueError(f"B_real = {B_real} outside [0, {B}]")
        dev = pred.device
        t = self._device_tables(dev)
        JA = self.JA
        pja = gja = gje = None
        if pred_joints_A is not None:
            pja = _cuda_f32(pred_joints_A, "pred_joints_A")
            JA = int(pja.shape[1]) if JA is None else JA
        if gt_joints_A is not None:
            gja = _cuda_f32(gt_joints_A, "gt_joints_A")
            JA = int(gja.shape[1]) if JA is None else JA
        if JA is None or (self.JA is None and (pja is None or gja is None)):
            raise ValueError("without regressor_A, pred_joints_A and gt_joints_A are both required")
        for x, n in ((pja, "pred_joints_A"), (gja, "gt_joints_A")):
            if x is not None and tuple(x.shape) != (B, JA, 3):
                raise ValueError(f"{n}: expected [{B}, {JA}, 3], got {tuple(x.shape)}")
        if self.JA is None and self._sub_A is not None:
            _subset(self._sub_A, JA, "sub_A")
        if not 0 <= self.root_A < JA:
            raise ValueError("root_A out of range")
        if gt_joints_E is not None:
            if not self.JE:
                raise ValueError("gt_joints_E given without regressor_E")
            gje = _cuda_f32(gt_joints_E, "gt_joints_E")
            if tuple(gje.shape) != (B, self.JE, 3):
                raise ValueError(f"gt_joints_E: expected [{B}, {self.JE}, 3], got {tuple(gje.shape)}")
        buf = self._buffers(B, JA, dev)
        grp = None
        if group is not None:
            grp = buf["group"]
            if isinstance(group, torch.Tensor) and group.is_cuda:
                g = group.reshape(-1)[:B].to(torch.int32)
            else:
                g = torch.as_tensor(_np.asarray(group, dtype=_np.int32).reshape(-1)[:B]).to(dev, non_blocking=True)
            if g.numel() < B_real:
                raise ValueError(f"group: need >= {B_real} ids, got {g.numel()}")
            grp[:g.numel()].copy_(g)
        nsA = len(self._sub_A) if self._sub_A is not None else 0
        nsE = len(self._sub_E) if self.JE and self._sub_E is not None else 0
        with torch.cuda.device(dev):
            _lib.check(_lib.hip().p2m_mesh_eval(
                _p(pred), _p(gt), B, B_real, self.nv, self.gt_mesh_scale,
                _p(t.get("ra_ptr")), _p(t.get("ra_idx")), _p(t.get("ra_val")), JA, self.root_A, _p(t.get("sub_A")), nsA,
                _p(pja), _p(gja),
                _p(t.get("re_ptr")), _p(t.get("re_idx")), _p(t.get("re_val")), self.JE, self.root_E, _p(t.get("sub_E")), nsE,
                _p(gje), int(self.pa_mesh), _p(buf["mpjpe_A"]), _p(buf["mpvpe"]), _p(buf.get("mpjpe_E")),
                _p(buf.get("pa_mpjpe_E")), _p(buf.get("pa_mpvpe")), _p(buf["sample_means"]), _p(grp), self.n_groups,
                _p(self.totals), _stream()), "p2m_mesh_eval")
        return {k: v for k, v in buf.items() if k != "group"}

    def _present(self):
        return [k for k in KEYS if (k in ("mpjpe_A", "mpvpe")) or (k.endswith("_E") and self.JE) or
                (k == "pa_mpvpe" and self.pa_mesh)]

    def summary(self):
        """Syncs once.  {"samples": n, <metric>: dataset mean, ..., "groups": {g: {"samples": n_g, <metric>: mean}}} over
        every sample since the last reset(): mpjpe_E / pa_mpjpe_E (MPJPE, PA-MPJPE on the E joints), mpjpe_A, mpvpe,
        pa_mpvpe - those this evaluator computes.  "groups" lists the groups that received samples."""
        if self.totals is None:
            return {"samples": 0}
        tot = self.totals.cpu().numpy()
        keys = self._present()

        def row(r):
            n = tot[r, 0]
            d = {"samples": int(n)}
            for k in keys:
                d[k] = float(tot[r, 1 + KEYS.index(k)] / n) if n > 0 else float("nan")
            return d
        out = row(0)
        groups = {g: row(g + 1) for g in range(self.n_groups) if tot[g + 1, 0] > 0}
        if groups:
            out["groups"] = groups
        return out


_both_err_cache = {}


def compute_both_err(pred_mesh, target_mesh, pred_joint, target_joint, eval_joint):
    """data/PW3D/dataset.py:273-286 (and Human36M's twin): both meshes centred on joint 0 of their own joint set, errors of
    the eval_joint subset of the joints and of every vertex -> (joint_mean_error, mesh_mean_error) as Python floats (one
    sync, as the reference's numpy round trip has).  pred_mesh / target_mesh [B, nv, 3], pred_joint / target_joint
    [B, J, 3] CUDA tensors (the Tester passes them already in mm).  For a loop without a sync per batch, use MeshEvaluator
    and summary()."""
    B, nv = int(pred_mesh.shape[0]), int(pred_mesh.shape[1])
    J = int(pred_joint.shape[1])
    key = (nv, J, tuple(int(j) for j in eval_joint))
    ev = _both_err_cache.get(key)
    if ev is None:
        ev = MeshEvaluator(nv, None, 0, sub_A=key[2])
        _both_err_cache[key] = ev
    out = ev(pred_mesh, target_mesh, gt_joints_A=target_joint, pred_joints_A=pred_joint)
    ev.reset()
    m = out["sample_means"][:, 2:4].mean(dim=0).cpu()
    return float(m[0]), float(m[1])
