"""Body-model layer on the GPU: the batched forward of smplpytorch's SMPL_Layer (smpl_layer.py:65-158) and manopth's
ManoLayer (manolayer.py:109-273, as lib/_mano.py:33 builds it: use_pca=False, axis-angle root) - what every dataset calls
once per sample on a dataloader worker to make its target mesh (get_smpl_coord / get_mano_coord).

  BodyModel(v_template, shapedirs, posedirs, J_regressor, weights, parents, ...)   from arrays
  BodyModel.from_layer(layer)                                                       from a constructed reference layer
  verts, joints[, extra] = model(pose, betas=None, trans=None)                      one p2m_body_forward call

  layer = BodyLayer(model);  verts, joints[, extra] = layer(pose, betas, trans)      the same forward, differentiable

BodyModel is forward only, fp32, on the current stream; the launch path allocates and synchronises nothing once the buffers
of a batch size exist, so a call can sit in a captured graph.  BodyLayer is the opt-in differentiable entry: new output
tensors per call and one p2m_body_backward call for the gradients of pose, betas and trans.  There is no CPU fallback: CPU
tensors raise.
"""
import ctypes as _ct

import numpy as _np
import torch

from . import _lib
from . import loss as _loss

SAMPLE_TILE = 8        # samples per block of the skinning kernel (p2m_body_sample_tile)
VERTEX_TILE = 64       # vertices per block (p2m_body_vertex_tile)
MAX_JOINTS = 64
MAX_COEFFS = 640
MANO_TIPS = {"right": (745, 317, 444, 556, 673), "left": (745, 317, 445, 556, 673)}               # manolayer.py:252-255
MANO_JOINT_ORDER = (0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20)     # manolayer.py:259


def _p(t):
    return None if t is None else _ct.c_void_p(t.data_ptr())


def _betas_arg(t, betas):
    """The betas pointer of a call: the input, or the model's stored betas.  With nb = 0 the input [B, 0] has no element and
    so no address; the stored table's one-element stand-in goes instead (the kernels read nb values of it: none)."""
    return _p(t["betas"] if betas is None or betas.numel() == 0 else betas)


def _stream():
    return _ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda_f32(x, name, shape, grad_ok=False):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.P2MError(f"{name}: the body-model kernels need a CUDA tensor (there is no CPU path)")
    if x.requires_grad and not grad_ok:
        raise _lib.P2MError(f"{name}: requires grad, and BodyModel is forward only (BodyLayer is the differentiable entry)")
    if tuple(x.shape) != shape:
        raise ValueError(f"{name}: expected {list(shape)}, got {list(x.shape)}")
    return x.contiguous() if x.dtype == torch.float32 else x.float().contiguous()


def repack_dirs(shapedirs, posedirs):
    """shapedirs [V, 3, nb], posedirs [V, 3, P] -> the kernel's coefficient-major table [nb + P, 3 V] (fp32): row k holds
    direction k of every vertex component, so a wave reads 64 consecutive floats per coefficient."""
    sd, pd = _np.asarray(shapedirs, _np.float32), _np.asarray(posedirs, _np.float32)
    V = sd.shape[0]
    return _np.ascontiguousarray(_np.concatenate([sd.reshape(V * 3, -1), pd.reshape(V * 3, -1)], axis=1).T)


def unpack_dirs(dirs, nb):
    """Inverse of repack_dirs: [K, 3 V] -> (shapedirs [V, 3, nb], posedirs [V, 3, K - nb])."""
    d = _np.asarray(dirs)
    V = d.shape[1] // 3
    return (_np.ascontiguousarray(d[:nb].T).reshape(V, 3, nb), _np.ascontiguousarray(d[nb:].T).reshape(V, 3, d.shape[0] - nb))


def check_parents(parents, J):
    """The chain is walked in index order: parents[j] < j for j >= 1 (parents[0] is ignored).  Returns int32 [J]."""
    p = [int(x) for x in _np.asarray(parents).reshape(-1).tolist()]
    if len(p) != J:
        raise ValueError(f"parents: expected {J} entries, got {len(p)}")
    for j in range(1, J):
        if not 0 <= p[j] < j:
            raise ValueError(f"parents[{j}] = {p[j]}: the kinematic chain needs 0 <= parents[j] < j")
    return _np.asarray([0] + p[1:], dtype=_np.int32)


class BodyModel:
    """model = BodyModel(v_template [V, 3], shapedirs [V, 3, nb], posedirs [V, 3, 9 (J - 1)], J_regressor [J, V],
                         weights [V, J], parents [J], betas=None, hands_mean=None, tip_vertices=None, joint_order=None,
                         scale=1.0, center_idx=None, extra_regressor=None)
    verts, joints[, extra] = model(pose, betas=None, trans=None)

    pose [B, 3 J] axis-angle (MANO: 3 root + 45 joint values, to which hands_mean is added), betas [B, nb], trans [B, 3]:
    CUDA tensors.  verts [B, V, 3]; joints [B, NJ, 3]: the posed chain joints, then the vertices tip_vertices, reordered by
    joint_order (SMPL: the 24 chain joints; MANO: 21); both times `scale` (MANO: 1000, mm).  With extra_regressor
    ([J' <= 64, V]) a third output extra = extra_regressor @ verts [B, J', 3] - the product every dataset applies next.

    The reference's semantics line by line (rotations through batch_rodrigues' quaternion and its + 1e-8, dense skinning
    weights, the chain walked over `parents`), with one deliberate difference: the reference picks "centre on center_idx"
    or "add trans" by testing torch.norm(th_trans) == 0 over the whole batch, and "stored betas" by torch.norm(th_betas)
    == 0 - a host sync each.  Here trans=None centres (when center_idx is set) and a trans tensor is ALWAYS added;
    betas=None takes the model's stored betas and a betas tensor is always used.  So a batch whose translations are all
    exactly zero, with center_idx set, is centred by the reference and not here.  center_idx must name a chain joint
    (centring on an appended tip vertex is not supported).  nb = 0, a model without a shape space, is allowed (J >= 2, so
    that there is a coefficient at all): betas is then None or [B, 0], and BodyLayer's gradient for it is an empty [B, 0].

    The outputs are buffers reused per batch size, overwritten by the next call of the same size (as MeshEvaluator's
    are); clone what must outlive it.  Device tables are uploaded once per device.  Rest joints use J_regressor folded
    into the template and the shape directions in float64 on the host, so they cost nb FMAs per coordinate."""

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, weights, parents, betas=None, hands_mean=None,
                 tip_vertices=None, joint_order=None, scale=1.0, center_idx=None, extra_regressor=None):
        f8 = _np.float64
        tmpl = _np.asarray(v_template, _np.float32)
        if tmpl.ndim == 3 and tmpl.shape[0] == 1:
            tmpl = tmpl[0]
        sd, pd = _np.asarray(shapedirs, _np.float32), _np.asarray(posedirs, _np.float32)
        jr, w = _np.asarray(J_regressor, _np.float32), _np.asarray(weights, _np.float32)
        if tmpl.ndim != 2 or tmpl.shape[1] != 3 or tmpl.shape[0] < 1:
            raise ValueError(f"v_template: expected [V >= 1, 3], got {tmpl.shape}")
        V = self.V = int(tmpl.shape[0])
        if jr.ndim != 2 or jr.shape[1] != V or not 1 <= jr.shape[0] <= MAX_JOINTS:
            raise ValueError(f"J_regressor: expected [1 <= J <= {MAX_JOINTS}, {V}], got {jr.shape}")
        J = self.J = int(jr.shape[0])
        if sd.ndim != 3 or sd.shape[:2] != (V, 3):
            raise ValueError(f"shapedirs: expected [{V}, 3, nb], got {sd.shape}")
        nb = self.nb = int(sd.shape[2])
        if pd.shape != (V, 3, 9 * (J - 1)):
            raise ValueError(f"posedirs: expected [{V}, 3, {9 * (J - 1)}], got {pd.shape}")
        if w.shape != (V, J):
            raise ValueError(f"weights: expected [{V}, {J}], got {w.shape}")
        if not 1 <= nb + 9 * (J - 1) <= MAX_COEFFS:
            raise ValueError(f"nb + 9 (J - 1) = {nb + 9 * (J - 1)} outside [1, {MAX_COEFFS}]")
        par = check_parents(parents, J)
        self.scale = float(scale)
        b0 = _np.zeros(nb, _np.float32) if betas is None else _np.asarray(betas, _np.float32).reshape(-1)
        if b0.shape != (nb,):
            raise ValueError(f"betas: expected {nb} values, got {b0.shape}")
        tips = [] if tip_vertices is None else [int(t) for t in tip_vertices]
        if len(tips) > MAX_JOINTS or any(not 0 <= t < V for t in tips):
            raise ValueError(f"tip_vertices: at most {MAX_JOINTS} indices in [0, {V})")
        order = list(range(J + len(tips))) if joint_order is None else [int(o) for o in joint_order]
        if not order or len(set(order)) != len(order) or min(order) < 0 or max(order) >= J + len(tips):
            raise ValueError(f"joint_order: distinct indices in [0, {J + len(tips)}) expected")
        self.NJ = len(order)
        jslot = _np.full(J, -1, _np.int32)
        tip_vert, tip_slot = [], []
        for slot, src in enumerate(order):
            if src < J:
                jslot[src] = slot
            else:
                tip_vert.append(tips[src - J])
                tip_slot.append(slot)
        self.center_joint = -1
        if center_idx is not None:
            if not 0 <= int(center_idx) < self.NJ:
                raise ValueError(f"center_idx = {center_idx} outside [0, {self.NJ})")
            if order[int(center_idx)] >= J:
                raise ValueError("center_idx names an appended tip vertex: only chain joints can be the centre")
            self.center_joint = order[int(center_idx)]
        self.center_idx = center_idx
        host = {"tmpl": tmpl.reshape(-1), "dirs": repack_dirs(sd, pd), "wt": _np.ascontiguousarray(w.T),
                "jt": (jr.astype(f8) @ tmpl.astype(f8)).astype(_np.float32),
                "js": _np.einsum("jv,vcn->jcn", jr.astype(f8), sd.astype(f8)).astype(_np.float32),
                "parents": par, "jslot": jslot, "betas": b0}
        if hands_mean is not None:
            hm = _np.asarray(hands_mean, _np.float32).reshape(-1)
            if hm.shape != (3 * (J - 1),):
                raise ValueError(f"hands_mean: expected {3 * (J - 1)} values, got {hm.shape}")
            host["pose_mean"] = _np.concatenate([_np.zeros(3, _np.float32), hm])
        self.n_tips = len(tip_vert)
        if tip_vert:
            host["tip_vert"], host["tip_slot"] = _np.asarray(tip_vert, _np.int32), _np.asarray(tip_slot, _np.int32)
        self.JX = 0
        if extra_regressor is not None:
            xr = _np.asarray(extra_regressor, _np.float32)
            if xr.ndim != 2 or xr.shape[1] != V or not 1 <= xr.shape[0] <= MAX_JOINTS:
                raise ValueError(f"extra_regressor: expected [J' <= {MAX_JOINTS}, {V}], got {xr.shape}")
            self.JX = int(xr.shape[0])
            t = _loss._regressor_tables(xr, V)
            host.update(xr_ptr=t["jr_ptr"], xr_idx=t["jr_idx"], xr_val=t["jr_val"])
            if t["jr_val"].size == 0:                                      # an all-zero regressor: keep the tables non-empty
                host.update(xr_idx=_np.zeros(1, _np.int32), xr_val=_np.zeros(1, _np.float32))
            # the same regressor by column, for the backward (BodyLayer): the entries of a vertex, joints ascending
            self._host_grad = {"xc_ptr": t["vj_ptr"], "xc_idx": _np.concatenate([t["vj_idx"], _np.zeros(1, _np.int32)]),
                               "xc_val": _np.concatenate([t["vj_val"], _np.zeros(1, _np.float32)])}
        else:
            self._host_grad = {}
        self._host = host
        self._dev = None
        self._dev_grad = None
        self._bufs = {}

    @classmethod
    def from_layer(cls, layer, extra_regressor=None):
        """From an already constructed reference SMPL_Layer or ManoLayer (anything carrying their th_* buffers,
        kintree_parents and center_idx): BodyModel.from_layer(self.mesh_model.layer[gender]).  A ManoLayer must be what
        lib/_mano.py builds - use_pca=False, joint_rot_mode = root_rot_mode = 'axisang'; other modes raise ValueError."""
        def arr(name):
            return getattr(layer, name).detach().cpu().numpy()
        kw = dict(betas=arr("th_betas").reshape(-1), center_idx=getattr(layer, "center_idx", None),
                  extra_regressor=extra_regressor)
        if hasattr(layer, "use_pca") or hasattr(layer, "th_hands_mean"):
            if getattr(layer, "use_pca", False):
                raise ValueError("ManoLayer(use_pca=True): PCA pose coefficients are not supported")
            if getattr(layer, "joint_rot_mode", "axisang") != "axisang" or getattr(layer, "root_rot_mode", "axisang") != "axisang":
                raise ValueError("ManoLayer: only joint_rot_mode = root_rot_mode = 'axisang' is supported")
            side = getattr(layer, "side", "right")
            if side not in MANO_TIPS:
                raise ValueError(f"ManoLayer.side = {side!r}")
            kw.update(hands_mean=arr("th_hands_mean").reshape(-1), tip_vertices=MANO_TIPS[side], joint_order=MANO_JOINT_ORDER,
                      scale=1000.0)
        return cls(arr("th_v_template"), arr("th_shapedirs"), arr("th_posedirs"), arr("th_J_regressor"), arr("th_weights"),
                   list(layer.kintree_parents), **kw)

    def _device_tables(self, dev):
        if self._dev is None or self._dev[0] != dev:
            # a table without an element (nb = 0: the stored betas, the rest joints' shape directions) goes up as one zero
            # that no kernel reads: an empty tensor has no address, and the C entries reject a null table
            self._dev = (dev, {k: torch.from_numpy(_np.ascontiguousarray(v) if v.size else _np.zeros(1, v.dtype)).to(dev)
                               for k, v in self._host.items()})
            self._bufs = {}
        return self._dev[1]

    def _grad_tables(self, dev):
        """What only the backward reads, uploaded on the first differentiable call: the direction table vertex-major
        [3 V][K rounded up to 4] (the reference's own [V, 3, .] layout; SMPL: + 18 MB) and the extra regressor by column."""
        if self._dev_grad is None or self._dev_grad[0] != dev:
            d = self._host["dirs"]
            dt = _np.zeros((d.shape[1], (d.shape[0] + 3) // 4 * 4), _np.float32)
            dt[:, :d.shape[0]] = d.T
            g = {k: torch.from_numpy(_np.ascontiguousarray(v)).to(dev) for k, v in self._host_grad.items()}
            g["dirs_t"] = torch.from_numpy(dt).to(dev)
            self._dev_grad = (dev, g)
        return self._dev_grad[1]

    def _buffers(self, B, dev):
        b = self._bufs.get(B)
        if b is None:
            nbytes = int(_lib.hip().p2m_body_workspace(B, self.J, self.nb))
            if nbytes < 0:
                raise _lib.P2MError("p2m_body_workspace: bad shape")
            b = {"verts": torch.zeros((B, self.V, 3), device=dev, dtype=torch.float32),
                 "joints": torch.zeros((B, self.NJ, 3), device=dev, dtype=torch.float32),
                 "ws": torch.zeros(nbytes // 4, device=dev, dtype=torch.float32)}
            if self.JX:
                b["extra"] = torch.zeros((B, self.JX, 3), device=dev, dtype=torch.float32)
            self._bufs[B] = b
        return b

    @torch.no_grad()
    def __call__(self, pose, betas=None, trans=None, root_palm=False, share_betas=False):
        if root_palm or share_betas:
            raise ValueError("root_palm / share_betas are not supported")
        if not isinstance(pose, torch.Tensor) or not pose.is_cuda:
            raise _lib.P2MError("pose: the body-model kernels need a CUDA tensor (there is no CPU path)")
        if pose.dim() != 2 or pose.shape[0] < 1:
            raise ValueError(f"pose: expected axis-angle [B >= 1, {3 * self.J}] (rotation-matrix and 6-D poses are not "
                             f"supported), got {list(pose.shape)}")
        B = int(pose.shape[0])
        pose = _cuda_f32(pose, "pose", (B, 3 * self.J))
        if betas is not None:
            betas = _cuda_f32(betas, "betas", (B, self.nb))
        if trans is not None:
            trans = _cuda_f32(trans, "trans", (B, 3))
        dev = pose.device
        for x, n in ((betas, "betas"), (trans, "trans")):
            if x is not None and x.device != dev:
                raise ValueError(f"{n} is on {x.device}, pose on {dev}")
        t = self._device_tables(dev)
        buf = self._buffers(B, dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.hip().p2m_body_forward(
                _p(pose), _p(t.get("pose_mean")), _betas_arg(t, betas), int(betas is not None),
                _p(trans), -1 if trans is not None else self.center_joint, self.scale, B, self.V, self.J, self.nb,
                _p(t["tmpl"]), _p(t["dirs"]), _p(t["wt"]), _p(t["jt"]), _p(t["js"]), _p(t["parents"]), _p(t["jslot"]), self.NJ,
                _p(t.get("tip_vert")), _p(t.get("tip_slot")), self.n_tips, _p(t.get("xr_ptr")), _p(t.get("xr_idx")),
                _p(t.get("xr_val")), self.JX, _p(buf["ws"]), buf["ws"].numel() * 4, _p(buf["verts"]), _p(buf["joints"]),
                _p(buf.get("extra")), _stream()), "p2m_body_forward")
        if self.JX:
            return buf["verts"], buf["joints"], buf["extra"]
        return buf["verts"], buf["joints"]


class _BodyFunction(torch.autograd.Function):
    """One p2m_body_forward call into fresh tensors; the backward is one p2m_body_backward call.  The forward workspace
    (coefficient rows, skinning matrices, offsets) and the inputs are saved per call."""

    @staticmethod
    def forward(ctx, model, pose, betas, trans):
        B, dev = int(pose.shape[0]), pose.device
        t = model._device_tables(dev)
        nbytes = int(_lib.hip().p2m_body_workspace(B, model.J, model.nb))
        if nbytes < 0:
            raise _lib.P2MError("p2m_body_workspace: bad shape")
        ws = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
        verts = torch.empty((B, model.V, 3), device=dev, dtype=torch.float32)
        joints = torch.empty((B, model.NJ, 3), device=dev, dtype=torch.float32)
        extra = torch.empty((B, model.JX, 3), device=dev, dtype=torch.float32) if model.JX else None
        with torch.cuda.device(dev):
            _lib.check(_lib.hip().p2m_body_forward(
                _p(pose), _p(t.get("pose_mean")), _betas_arg(t, betas), int(betas is not None),
                _p(trans), -1 if trans is not None else model.center_joint, model.scale, B, model.V, model.J, model.nb,
                _p(t["tmpl"]), _p(t["dirs"]), _p(t["wt"]), _p(t["jt"]), _p(t["js"]), _p(t["parents"]), _p(t["jslot"]), model.NJ,
                _p(t.get("tip_vert")), _p(t.get("tip_slot")), model.n_tips, _p(t.get("xr_ptr")), _p(t.get("xr_idx")),
                _p(t.get("xr_val")), model.JX, _p(ws), ws.numel() * 4, _p(verts), _p(joints), _p(extra), _stream()),
                "p2m_body_forward")
        ctx.model, ctx.ws = model, ws
        ctx.save_for_backward(pose, betas, trans)
        ctx.set_materialize_grads(False)
        return (verts, joints, extra) if model.JX else (verts, joints)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_verts, g_joints, g_extra=None):
        model, ws = ctx.model, ctx.ws
        pose, betas, trans = ctx.saved_tensors
        need = list(ctx.needs_input_grad[1:])
        ups = [None if g is None else (g if g.dtype == torch.float32 else g.float()).contiguous()
               for g in (g_verts, g_joints, g_extra)]
        if not any(need) or all(g is None for g in ups):
            return None, None, None, None
        g_none = None
        if need[1] and model.nb == 0:                        # no shape space: the gradient of [B, 0] betas has no element,
            g_none, need[1] = torch.zeros_like(betas), False  # so the kernels are asked for the other gradients only
            if not any(need):
                return None, None, g_none, None
        B, dev = int(pose.shape[0]), pose.device
        t, tg = model._device_tables(dev), model._grad_tables(dev)
        nbytes = int(_lib.hip().p2m_body_backward_workspace(B, model.V, model.J, model.nb))
        if nbytes < 0:
            raise _lib.P2MError("p2m_body_backward_workspace: bad shape")
        part = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
        outs = [torch.empty_like(x) if n else None for x, n in zip((pose, betas, trans), need)]
        with torch.cuda.device(dev):
            _lib.check(_lib.hip().p2m_body_backward(
                _p(pose), _p(t.get("pose_mean")), _betas_arg(t, betas), int(betas is not None),
                int(trans is not None), -1 if trans is not None else model.center_joint, model.scale, B, model.V, model.J,
                model.nb, _p(t["tmpl"]), _p(t["dirs"]), _p(tg["dirs_t"]), _p(t["wt"]), _p(t["jt"]), _p(t["js"]),
                _p(t["parents"]), _p(t["jslot"]), model.NJ, _p(t.get("tip_vert")), _p(t.get("tip_slot")), model.n_tips,
                _p(tg.get("xc_ptr")), _p(tg.get("xc_idx")), _p(tg.get("xc_val")), model.JX, _p(ws), ws.numel() * 4,
                _p(ups[0]), _p(ups[1]), _p(ups[2]), _p(part), part.numel() * 4, _p(outs[0]), _p(outs[1]), _p(outs[2]),
                _stream()), "p2m_body_backward")
        return None, outs[0], outs[1] if g_none is None else g_none, outs[2]


class BodyLayer(torch.nn.Module):
    """layer = BodyLayer(model);  verts, joints[, extra] = layer(pose, betas=None, trans=None)

    The differentiable entry of a BodyModel: the same inputs, input rules and forward kernels (the values are bitwise those
    of model(pose, betas, trans)), but the outputs are new tensors per call, attached to one autograd function whose backward
    is one p2m_body_backward call.  Gradients reach pose, betas and trans - whichever require grad; the model tables are
    not trainable and the layer has no parameters.  betas=None takes the stored betas, trans=None centres on center_idx.
    Any subset of the outputs may be used downstream.  Double backward is not supported.  Every launch is on the current
    stream without a host synchronisation and all memory comes from torch's allocator, so forward plus backward can be
    captured with torch.cuda.graph.  The first differentiable call uploads a vertex-major copy of the direction table (as
    large as the table itself: 18 MB at SMPL size)."""

    def __init__(self, model):
        super().__init__()
        if not isinstance(model, BodyModel):
            raise TypeError("BodyLayer wraps a BodyModel")
        self.model = model

    def forward(self, pose, betas=None, trans=None):
        m = self.model
        if not isinstance(pose, torch.Tensor) or not pose.is_cuda:
            raise _lib.P2MError("pose: the body-model kernels need a CUDA tensor (there is no CPU path)")
        if pose.dim() != 2 or pose.shape[0] < 1:
            raise ValueError(f"pose: expected axis-angle [B >= 1, {3 * m.J}] (rotation-matrix and 6-D poses are not "
                             f"supported), got {list(pose.shape)}")
        B = int(pose.shape[0])
        pose = _cuda_f32(pose, "pose", (B, 3 * m.J), grad_ok=True)
        if betas is not None:
            betas = _cuda_f32(betas, "betas", (B, m.nb), grad_ok=True)
        if trans is not None:
            trans = _cuda_f32(trans, "trans", (B, 3), grad_ok=True)
        for x, n in ((betas, "betas"), (trans, "trans")):
            if x is not None and x.device != pose.device:
                raise ValueError(f"{n} is on {x.device}, pose on {pose.device}")
        return _BodyFunction.apply(m, pose, betas, trans)
