"""Evaluation on the GPU: the Tester's per-batch errors and dataset.evaluate()'s metrics (MPJPE, PA-MPJPE, MPVPE,
PA-MPVPE) without copying meshes to the host (lib/core/base.py:196-230, data/PW3D/dataset.py:273-286,322-375,
data/Human36M/dataset.py:514-572, lib/coord_utils.py:127-149).

  rigid_transform_3D(A, B), rigid_align(A, B)   batched similarity alignment of [N, 3] / [nb, N, 3] CUDA tensors
                                                (p2m_rigid_align).  LiftTester's evaluate_joint needs no mesh: its
                                                PA-MPJPE is rigid_align on the [nb, 14, 3] root-centred joint subsets.
  MeshEvaluator                                 per-sample metrics of a batch in one launch (p2m_mesh_eval) and running
                                                fp64 totals on the device; summary() syncs once.
  compute_both_err                              drop-in for the datasets' compute_both_err (two floats per batch).
  FScoreEvaluator                               FreiHAND's F@5 mm / F@15 mm per sample (p2m_mesh_fscore): nearest-vertex
                                                distances both ways between prediction and ground truth, centred and / or
                                                similarity-aligned (PA-MPVPE's alignment), thresholded counts, F, running
                                                fp64 totals; summary() syncs once.  The reference ships no F-score code:
                                                the definition is the one in include/p2m.h, restated in float64 in
                                                tests/fscore_ref.py.
  nearest_distances(A, B)                       the bare two-way nearest-point search between [N, 3] / [nb, N, 3] and
                                                [M, 3] / [nb, M, 3] CUDA tensors (p2m_point_nn): chamfer distances,
                                                per-vertex error heat maps.
  ErrorProfile                                  where the error sits and how it is distributed (p2m_error_profile): per-point
                                                errors between corresponding points, raw or similarity-aligned, binned against
                                                an fp64 threshold table; running per-group and per-point sums, counts and
                                                histograms; summary() syncs once and derives means, PCK curves and their AUC
                                                (FreiHAND's AUC columns, PCK@150 mm, per-joint tables, the dataset-mean
                                                per-vertex error map).  Defined in include/p2m.h, restated in float64 in
                                                tests/profile_ref.py.

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


def _workspace(nb, nA, nB, dev):
    n = int(_lib.hip().p2m_nn_workspace(nb, nA, nB))
    if n < 0:
        raise ValueError(f"bad point-set shape ({nb}, {nA}, {nB})")
    return torch.empty(max(n, 16), device=dev, dtype=torch.uint8), n


def nearest_distances(A, B):
    """(d_ab, d_ba): d_ab[..., i] = min_j |A_i - B_j| and d_ba[..., j] = min_i |B_j - A_i| for A [N, 3] or [nb, N, 3] and B
    [M, 3] or [nb, M, 3] CUDA tensors (N != M allowed), fp32.  The points are staged about each pair's centroid of B (fp64
    subtraction before the fp32 rounding), so the error scales with the sets' extent, not their position: at most
    (2 sqrt(3) max|coordinate - centroid| + 6 d) 2^-24 per distance."""
    if not (isinstance(A, torch.Tensor) and isinstance(B, torch.Tensor)) or A.dim() != B.dim() or A.dim() not in (2, 3) or \
            A.shape[-1] != 3 or B.shape[-1] != 3 or A.shape[-2] < 1 or B.shape[-2] < 1 or \
            (A.dim() == 3 and A.shape[0] != B.shape[0]):
        raise ValueError(f"A, B: expected [N, 3] and [M, 3] or [nb, N, 3] and [nb, M, 3] tensors, got "
                         f"{tuple(getattr(A, 'shape', ()))}, {tuple(getattr(B, 'shape', ()))}")
    A, B = _cuda_f32(A, "A"), _cuda_f32(B, "B")
    single = A.dim() == 2
    nb = 1 if single else int(A.shape[0])
    nA, nB = int(A.shape[-2]), int(B.shape[-2])
    dev = A.device
    d_ab = torch.empty((nb, nA), device=dev, dtype=torch.float32)
    d_ba = torch.empty((nb, nB), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        ws, n = _workspace(nb, nA, nB, dev)
        _lib.check(_lib.hip().p2m_point_nn(_p(A), _p(B), nb, nA, nB, _p(d_ab), _p(d_ba), _p(ws), n, _stream()),
                   "p2m_point_nn")
    return (d_ab[0], d_ba[0]) if single else (d_ab, d_ba)


class FScoreEvaluator:
    """fs = FScoreEvaluator(nv, regressor=None, root=0, thresholds=(5.0, 15.0), centred=True, aligned=True,
                            gt_mesh_scale=1.0, n_groups=32)
    out = fs(pred_mesh, gt_mesh, pred_root=None, gt_root=None, B_real=None, group=None)
    totals = fs.summary();  fs.reset()

    Per sample (include/p2m.h, p2m_mesh_fscore, has the definition): d_pred[i] = distance of prediction vertex i to the
    NEAREST ground-truth vertex, d_gt[j] the other way; near_pred / near_gt = the share of them strictly below a threshold;
    F = their harmonic mean (0 when both are 0).
      centred  both meshes minus their own centre point: row `root` of `regressor` ([J, nv] dense) applied to each mesh, or
               pred_root / gt_root [B, 3] given per call (used as they are; both or neither), or - without a regressor and
               without roots - nothing: the meshes are compared where they are
      aligned  the centred prediction similarity-aligned onto the centred ground truth over all vertices (MeshEvaluator's
               pa_mesh transform): the published FreiHAND F-scores
    pred_mesh / gt_mesh: [B, nv, 3] CUDA tensors; gt_mesh is read times gt_mesh_scale; thresholds (1..4) are in the unit of
    the prediction.  B_real, group: as MeshEvaluator's.

    A call launches on the current stream and returns per-sample device tensors: f, near_pred, near_gt [B, T] (fp64) and
    d_pred, d_gt [B, nv] (fp32) for the centred variant, the same with a pa_ prefix for the aligned one, and counts
    [B, variants, 2, T] (int32).  They are buffers reused per batch size, overwritten by the next call of the same size, and
    the call adds the batch to running fp64 totals on the device: no allocation after the first call of a size and no sync,
    so a call can sit in a single-stream captured graph."""

    def __init__(self, nv, regressor=None, root=0, thresholds=(5.0, 15.0), centred=True, aligned=True, gt_mesh_scale=1.0,
                 n_groups=32):
        self.nv, self.root, self.n_groups = int(nv), int(root), int(n_groups)
        self.centred, self.aligned, self.gt_mesh_scale = bool(centred), bool(aligned), float(gt_mesh_scale)
        if self.nv < 1:
            raise ValueError("nv < 1")
        if not (self.centred or self.aligned):
            raise ValueError("at least one of centred, aligned")
        th = [float(t) for t in _np.asarray(thresholds, dtype=_np.float64).reshape(-1)]
        if not 1 <= len(th) <= 4 or not all(_np.isfinite(t) and t > 0 for t in th):
            raise ValueError(f"thresholds: 1..4 positive finite values expected, got {thresholds}")
        self.thresholds = tuple(th)
        self._th = (_ct.c_float * len(th))(*th)
        self._host = {}
        if regressor is not None:
            r = _np.asarray(regressor, dtype=_np.float32)
            if r.ndim != 2 or r.shape[1] != self.nv or not 0 <= self.root < r.shape[0]:
                raise ValueError(f"regressor: expected [J > root, {self.nv}], got {r.shape}")
            t = _loss._regressor_tables(r[self.root:self.root + 1], self.nv)       # only the centre's row is read
            self._host.update(r_ptr=t["jr_ptr"], r_idx=t["jr_idx"], r_val=t["jr_val"])
        self.variants = (1 if self.centred else 0) | (2 if self.aligned else 0)
        self._prefixes = ([""] if self.centred else []) + (["pa_"] if self.aligned else [])
        self._dev = None
        self._bufs = {}
        self.totals = None

    @property
    def _ncol(self):
        return 1 + len(self._prefixes) * 3 * len(self.thresholds)

    def _device_tables(self, dev):
        if self._dev is None or self._dev[0] != dev:
            d = {k: torch.from_numpy(_np.ascontiguousarray(v)).to(dev) for k, v in self._host.items()}
            self._dev = (dev, d)
            self.totals = torch.zeros((self.n_groups + 1, self._ncol), device=dev, dtype=torch.float64)
            self._bufs = {}
        return self._dev[1]

    def reset(self):
        """Clears the running totals (a device-side fill on the current stream)."""
        if self.totals is not None:
            self.totals.zero_()

    def _buffers(self, B, dev):
        b = self._bufs.get(B)
        if b is None:
            nvar, T = len(self._prefixes), len(self.thresholds)
            b = {"counts": torch.zeros((B, nvar, 2, T), device=dev, dtype=torch.int32),
                 "scores": torch.zeros((B, nvar, 3, T), device=dev, dtype=torch.float64),
                 "group": torch.full((B,), -1, device=dev, dtype=torch.int32)}
            for pre in self._prefixes:
                b[pre + "d_pred"] = torch.zeros((B, self.nv), device=dev, dtype=torch.float32)
                b[pre + "d_gt"] = torch.zeros((B, self.nv), device=dev, dtype=torch.float32)
            b["ws"], b["ws_bytes"] = _workspace(B, self.nv, self.nv, dev)
            self._bufs[B] = b
        return b

    @torch.no_grad()
    def __call__(self, pred_mesh, gt_mesh, pred_root=None, gt_root=None, B_real=None, group=None):
        for x in (pred_mesh, gt_mesh):
            if not isinstance(x, torch.Tensor) or x.dim() != 3 or tuple(x.shape[1:]) != (self.nv, 3) or \
                    x.shape != pred_mesh.shape:
                raise ValueError(f"pred_mesh / gt_mesh: expected equal [B, {self.nv}, 3] tensors, got "
                                 f"{tuple(getattr(x, 'shape', ()))}")
        B = int(pred_mesh.shape[0])
        B_real = B if B_real is None else int(B_real)
        if not 0 <= B_real <= B:
            raise ValueError(f"B_real = {B_real} outside [0, {B}]")
        if (pred_root is None) != (gt_root is None):
            raise ValueError("pred_root and gt_root: both or neither")
        if pred_root is not None:
            for x, n in ((pred_root, "pred_root"), (gt_root, "gt_root")):
                if not isinstance(x, torch.Tensor) or tuple(x.shape) != (B, 3):
                    raise ValueError(f"{n}: expected a [{B}, 3] tensor, got {tuple(getattr(x, 'shape', ()))}")
        pred, gt = _cuda_f32(pred_mesh, "pred_mesh"), _cuda_f32(gt_mesh, "gt_mesh")
        pr = gr = None
        if pred_root is not None:
            pr, gr = _cuda_f32(pred_root, "pred_root"), _cuda_f32(gt_root, "gt_root")
        dev = pred.device
        t = self._device_tables(dev)
        buf = self._buffers(B, dev)
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
        with torch.cuda.device(dev):
            _lib.check(_lib.hip().p2m_mesh_fscore(
                _p(pred), _p(gt), B, B_real, self.nv, self.gt_mesh_scale, _p(t.get("r_ptr")), _p(t.get("r_idx")),
                _p(t.get("r_val")), 1, 0, _p(pr), _p(gr), self.variants, self._th, len(self.thresholds), _p(buf["ws"]),
                buf["ws_bytes"], _p(buf.get("d_pred")), _p(buf.get("d_gt")), _p(buf.get("pa_d_pred")), _p(buf.get("pa_d_gt")),
                _p(buf["counts"]), _p(buf["scores"]), _p(grp), self.n_groups, _p(self.totals), _stream()), "p2m_mesh_fscore")
        out = {"counts": buf["counts"]}
        for v, pre in enumerate(self._prefixes):
            out[pre + "near_pred"], out[pre + "near_gt"], out[pre + "f"] = (buf["scores"][:, v, k] for k in range(3))
            out[pre + "d_pred"], out[pre + "d_gt"] = buf[pre + "d_pred"], buf[pre + "d_gt"]
        return out

    def _columns(self):
        """Names of totals[:, 1:], in the layout of the scores: [variant][near_pred, near_gt, f][threshold]."""
        return [f"{pre}{k}@{th:g}" for pre in self._prefixes for k in ("near_pred", "near_gt", "f") for th in self.thresholds]

    def summary(self):
        """Syncs once.  {"samples": n, "f@5": dataset mean of the per-sample F, "near_pred@5", "near_gt@5", ..., "pa_f@5",
        ..., "groups": {g: {"samples": n_g, ...}}} over every sample since the last reset() (thresholds formatted with :g).
        "groups" lists the groups that received samples."""
        if self.totals is None:
            return {"samples": 0}
        tot = self.totals.cpu().numpy()
        cols = self._columns()

        def row(r):
            n = tot[r, 0]
            d = {"samples": int(n)}
            for i, k in enumerate(cols):
                d[k] = float(tot[r, 1 + i] / n) if n > 0 else float("nan")
            return d
        out = row(0)
        groups = {g: row(g + 1) for g in range(self.n_groups) if tot[g + 1, 0] > 0}
        if groups:
            out["groups"] = groups
        return out


def _threshold_table(thresholds):
    """(lo, hi, steps) - a sequence of three whose last entry is a Python / numpy integer - is np.linspace(lo, hi, steps);
    anything else is taken as the table itself.  Returns a float64 array, checked: 2..256 finite ascending values."""
    if not isinstance(thresholds, _np.ndarray) and hasattr(thresholds, "__len__") and len(thresholds) == 3 and \
            isinstance(thresholds[2], (int, _np.integer)) and not isinstance(thresholds[2], bool):
        lo, hi, steps = float(thresholds[0]), float(thresholds[1]), int(thresholds[2])
        if not 2 <= steps <= 256:
            raise ValueError(f"thresholds: 2..256 steps expected, got {steps}")
        t = _np.linspace(lo, hi, steps)
    else:
        t = _np.array(thresholds, dtype=_np.float64).reshape(-1)
    if not 2 <= t.size <= 256:
        raise ValueError(f"thresholds: a table of 2..256 values expected, got {t.size}")
    if not _np.isfinite(t).all() or not (_np.diff(t) > 0).all():
        raise ValueError("thresholds: finite, strictly ascending values expected")
    return _np.ascontiguousarray(t)


def profile_curves(total, count, hist, t):
    """The derived figures of error totals (host, float64): total [...], count [...], hist [..., K + 1] ->
    mean [...] = total / count, pck [..., K] = cumsum(hist)[..., :K] / count (the share of points with e <= t[k]) and
    auc [...] = sum_k (pck[k] + pck[k + 1]) / 2 * (t[k + 1] - t[k]) / (t[K - 1] - t[0]).  count == 0 gives NaN."""
    total, count = _np.asarray(total, _np.float64), _np.asarray(count)
    hist, t = _np.ascontiguousarray(hist), _np.asarray(t, _np.float64)
    with _np.errstate(invalid="ignore", divide="ignore"):
        n = count.astype(_np.float64)
        mean = total / n
        pck = _np.ascontiguousarray(_np.cumsum(hist, axis=-1)[..., :-1] / n[..., None])
        auc = _np.sum((pck[..., :-1] + pck[..., 1:]) / 2 * _np.diff(t), axis=-1) / (t[-1] - t[0])
    return mean, pck, auc


class ErrorProfile:
    """ep = ErrorProfile(n_points, thresholds=(0.0, 50.0, 100), align=False, root=None, per_point=True, gt_scale=1.0,
                         n_groups=32)
    out = ep(pred, gt, valid=None, B_real=None, group=None)
    totals = ep.summary();  ep.reset()

    Where the error sits and how it is distributed: per-point distances between corresponding points (joints or vertices),
    binned against a threshold table, accumulated per group and per point (p2m_error_profile; include/p2m.h has the
    definition, tests/profile_ref.py restates it in float64).  Per sample, in fp64: `root` (a point index or None) - both
    sets minus their own point `root`; `align` - the prediction similarity-aligned onto the ground truth over the valid
    points (MeshEvaluator's pa_mesh solve); e_i = |p_i - g_i|; bin_i = the first k with e_i <= thresholds[k], K if there is
    none.  pred, gt: [B, n_points, 3] CUDA tensors, gt read times gt_scale; valid: [B, n_points] (non-zero = counted), any
    dtype; B_real, group: as MeshEvaluator's.  thresholds: (lo, hi, steps) with an integer `steps` (np.linspace(lo, hi, steps),
    uploaded bit for bit) or an ascending table of 2..256 values, in the unit of the prediction.

    A call launches on the current stream and returns per-sample device tensors: "error" [B, n_points] fp64 (0 where not
    counted), "sample_mean" [B] fp64 and "sample_pck" [B, K + 1] int32 (the sample's points per bin; its cumulative sum over
    the points counted is the sample's PCK curve).  They are buffers reused per batch size, overwritten by the next call of
    the same size.  The call adds the batch to running totals on the device (fp64 sums in sample order, int64 counts and
    bins), per group and - with per_point - per point: no allocation after the first call of a size and no sync, so a call
    can sit in a single-stream captured graph."""

    def __init__(self, n_points, thresholds=(0.0, 50.0, 100), align=False, root=None, per_point=True, gt_scale=1.0,
                 n_groups=32):
        self.n_points, self.n_groups = int(n_points), int(n_groups)
        self.align, self.per_point, self.gt_scale = bool(align), bool(per_point), float(gt_scale)
        if self.n_points < 1:
            raise ValueError("n_points < 1")
        if not 0 <= self.n_groups <= 65535:
            raise ValueError("n_groups outside 0..65535")
        self.root = -1 if root is None else int(root)
        if root is not None and not 0 <= self.root < self.n_points:
            raise ValueError(f"root: None or a point index in [0, {self.n_points}), got {root}")
        self.thresholds = _threshold_table(thresholds)
        self.K = int(self.thresholds.size)
        self._dev = None
        self._bufs = {}
        self.state = None

    def _layout(self):
        """Offsets (in 8-byte words) of the running totals inside self.state: one buffer, so reset() is one fill and summary()
        one copy."""
        G, K, N = self.n_groups + 1, self.K, self.n_points if self.per_point else 0
        sizes = (("group_sum", G), ("group_count", G), ("group_hist", G * (K + 1)), ("point_sum", N), ("point_count", N),
                 ("point_hist", N * (K + 1)))
        off, o = {}, 0
        for k, n in sizes:
            off[k] = (o, n)
            o += n
        return off, o

    def _device_tables(self, dev):
        if self._dev is None or self._dev[0] != dev:
            off, n = self._layout()
            self.state = torch.zeros(n, device=dev, dtype=torch.int64)
            views = {k: self.state[o:o + m] for k, (o, m) in off.items() if m}
            for k in ("group_sum", "point_sum"):
                if k in views:
                    views[k] = views[k].view(torch.float64)
            self._dev = (dev, views, torch.from_numpy(self.thresholds).to(dev))
            self._bufs = {}
        return self._dev[1], self._dev[2]

    def reset(self):
        """Clears the running totals (a device-side fill on the current stream)."""
        if self.state is not None:
            self.state.zero_()

    def _buffers(self, B, dev):
        b = self._bufs.get(B)
        if b is None:
            n = int(_lib.hip().p2m_error_profile_workspace(B, self.n_points))
            b = {"error": torch.zeros((B, self.n_points), device=dev, dtype=torch.float64),
                 "sample_mean": torch.zeros((B,), device=dev, dtype=torch.float64),
                 "sample_pck": torch.zeros((B, self.K + 1), device=dev, dtype=torch.int32),
                 "group": torch.full((B,), -1, device=dev, dtype=torch.int32),
                 "valid": torch.zeros((B, self.n_points), device=dev, dtype=torch.uint8),
                 "ws": torch.empty(max(n, 16), device=dev, dtype=torch.uint8), "ws_bytes": n}
            self._bufs[B] = b
        return b

    @torch.no_grad()
    def __call__(self, pred, gt, valid=None, B_real=None, group=None):
        for x in (pred, gt):
            if not isinstance(x, torch.Tensor) or x.dim() != 3 or tuple(x.shape[1:]) != (self.n_points, 3) or \
                    x.shape != pred.shape:
                raise ValueError(f"pred / gt: expected equal [B, {self.n_points}, 3] tensors, got "
                                 f"{tuple(getattr(x, 'shape', ()))}")
        B = int(pred.shape[0])
        B_real = B if B_real is None else int(B_real)
        if not 0 <= B_real <= B:
            raise ValueError(f"B_real = {B_real} outside [0, {B}]")
        if valid is not None and (not isinstance(valid, torch.Tensor) or tuple(valid.shape) != (B, self.n_points)):
            raise ValueError(f"valid: expected a [{B}, {self.n_points}] tensor, got {tuple(getattr(valid, 'shape', ()))}")
        pred, gt = _cuda_f32(pred, "pred"), _cuda_f32(gt, "gt")
        dev = pred.device
        if valid is not None and not valid.is_cuda:
            raise _lib.P2MError("valid: the evaluation kernels need a CUDA tensor (there is no CPU path)")
        views, th = self._device_tables(dev)
        buf = self._buffers(B, dev)
        val = None
        if valid is not None:
            val = buf["valid"]
            torch.ne(valid, 0, out=val.view(torch.bool))
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
        with torch.cuda.device(dev):
            _lib.check(_lib.hip().p2m_error_profile(
                _p(pred), _p(gt), _p(val), B, B_real, self.n_points, self.gt_scale, self.root, int(self.align), _p(th), self.K,
                _p(buf["ws"]), buf["ws_bytes"], _p(buf["error"]), _p(buf["sample_mean"]), _p(buf["sample_pck"]), _p(grp),
                self.n_groups, _p(views["group_sum"]), _p(views["group_count"]), _p(views["group_hist"]),
                _p(views.get("point_sum")), _p(views.get("point_count")), _p(views.get("point_hist")), _stream()),
                "p2m_error_profile")
        return {k: buf[k] for k in ("error", "sample_mean", "sample_pck")}

    def totals(self):
        """Syncs once.  The raw running totals as host arrays: group_sum [n_groups + 1] fp64, group_count [n_groups + 1] and
        group_hist [n_groups + 1, K + 1] int64 (row 0: overall) and, with per_point, point_sum [n_points] fp64, point_count
        [n_points] and point_hist [n_points, K + 1] int64; None before the first call."""
        if self.state is None:
            return None
        host = self.state.cpu().numpy()
        off, _ = self._layout()
        out = {}
        for k, (o, n) in off.items():
            if n:
                a = host[o:o + n]
                out[k] = a.view(_np.float64) if k.endswith("_sum") else a
                if k.endswith("_hist"):
                    out[k] = out[k].reshape(-1, self.K + 1)
        return out

    def summary(self):
        """Syncs once.  Over every sample since the last reset():
          {"thresholds": t [K], "count": points counted, "mean": their mean error, "pck": [K] the share with e <= t[k],
           "auc": the area under that curve over t[0] .. t[K - 1] (trapezoids, normalised to 1),
           "groups": {g: {"count", "mean", "pck", "auc"}} for the groups that counted points,
           "points": {"count" [N], "mean" [N], "pck" [N, K], "auc" [N]} and "auc_points": the mean of points.auc over the
           points with count > 0 (FreiHAND's per-keypoint AUC; equal to "auc" when every point is always valid) - with
           per_point}
        Nothing counted gives NaN means, curves and areas.  pck_at(summary, x) reads the curve at a threshold of the table."""
        t = self.thresholds
        tot = self.totals()
        if tot is None:
            return {"thresholds": t, "count": 0}
        mean, pck, auc = profile_curves(tot["group_sum"], tot["group_count"], tot["group_hist"], t)

        def row(r):
            return {"count": int(tot["group_count"][r]), "mean": float(mean[r]), "pck": pck[r], "auc": float(auc[r])}
        out = dict(row(0), thresholds=t)
        groups = {g: row(g + 1) for g in range(self.n_groups) if tot["group_count"][g + 1] > 0}
        if groups:
            out["groups"] = groups
        if self.per_point:
            pm, pp, pa = profile_curves(tot["point_sum"], tot["point_count"], tot["point_hist"], t)
            out["points"] = {"count": tot["point_count"], "mean": pm, "pck": pp, "auc": pa}
            seen = tot["point_count"] > 0
            out["auc_points"] = float(_np.mean(pa[seen])) if seen.any() else float("nan")
        return out


def pck_at(summary, threshold):
    """PCK at one threshold of the table, e.g. pck_at(ep.summary(), 150.0) for PCK@150 mm: the entry of summary["pck"] whose
    threshold equals `threshold` (KeyError when the table has no such entry - the curve is not interpolated)."""
    hit = _np.flatnonzero(_np.asarray(summary["thresholds"]) == float(threshold))
    if hit.size != 1:
        raise KeyError(f"{threshold} is not a threshold of the table")
    return float(summary["pck"][int(hit[0])])
