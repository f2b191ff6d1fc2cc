"""Test infrastructure: ReLU-kink-resolved gradient comparison against the float64 oracle.

Why.  In train mode the network is (conv -> BatchNorm -> ReLU) x 14-20.  An element whose pre-activation lies within
fp32 rounding of 0 gets mask 0 under one evaluation order and mask 1 under another; the forward value is unaffected
(|y| ~ 1e-6) but the backward loses / gains that element's WHOLE gradient path, which moves every upstream gradient by
~1e-3 relative.  The reference's own fp32 CPU arithmetic does this too: the fp32 oracle differs from the float64 oracle
by 2-4e-3 on all upstream tensors (1.3e-2 on bn.8.bias) for human36 B=3, and by 1e-6 when no element happens to flip
(tools/probes/grad_diag.py).  A plain tolerance therefore either hides real errors (2e-2) or is
flaky (1e-4).

What this does instead: it ACCOUNTS for the flips.  The implementation under test reports, for every ReLU layer, the
mask it actually used (the module's `_tap` test hook hands out the raw conv output and the BatchNorm scale / shift; the
mask fmaf(y, scale, shift) > 0 is reproduced exactly in float64, because an fp32 x fp32 product is exact in double and
one rounding never changes a sign).  The float64 oracle is then run with THOSE masks.  What must hold:
  * every element whose mask differs from the oracle's own (y64 > 0) is a genuine kink element: |y64| <= 1e-4
    (a wrong mask from a real bug would sit at O(1));
  * the number of such elements is reported (typically 0-10 of millions);
  * with the masks aligned, every gradient tensor agrees with float64 to fp32 round-off (1e-5 rel-L2).

Two fp32 results that used DIFFERENT masks (the kernels against the reference's fixture, one kernel set against another)
are compared by the same accounting taken one step further (accounted_difference, assert_accounted): the float64 oracle
runs once with each mask set, D = G64(masks_a) - G64(masks_b) is what the differing bits do to every gradient, and
(A - B) - D must be round-off, whatever the number of differing bits.  The reference's masks are rebuilt from the
fixture's record of its near-kink elements (masks_from_record).  PoseNet's BatchNorm-ReLU pairs are handled the same way
(posenet_hip_masks, posenet_masked_reference); flat_masked_oracle_gradients runs the whole model and its five losses.
"""
import collections

import torch

import loss_oracle as lo
import meshnet_oracle as mo

# Gradient bound with the ReLU masks aligned: 3x the largest per-tensor rel-L2 measured on MI355X (1.5e-5 at MANO B=256,
# 1.1e-5 at SMPL-like B=32, 2-4e-6 at B=2..5; DESIGN.md section 5 quotes the maxima).
ALIGNED_GRAD_TOL = 5e-5
KINK_WINDOW = 1e-4            # a flipped element must have |pre-activation| below this in float64 (activations are O(1))


class _MaskedReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        return x * mask

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * mask, None


def new_stats():
    return {"n_relu_elements": 0, "n_flips": 0, "max_abs_preact_at_flip": 0.0, "flips_per_layer": {},
            "n_watch_bits": 0, "max_abs_preact_at_watch_bit": 0.0, "call_dims": []}


def _layer_mask(masks, lid, x):
    """masks may arrive bit-unpacked from a child process (padded to a multiple of 8 elements): never by more."""
    m = torch.as_tensor(masks[lid]).flatten()
    assert x.numel() <= m.numel() < x.numel() + 8, (lid, tuple(x.shape), m.numel())
    return m[:x.numel()].reshape(x.shape).bool()


class _FProxy:
    """torch.nn.functional with relu replaced (only inside the oracle module, only during one call).  `watch`: a second
    mask set; the bits in which it differs from `masks` are counted, with the largest |pre-activation| among them."""

    def __init__(self, masks, stats, watch=None, keep_own=None):
        self._masks, self._stats, self._n, self._watch, self._keep_own = masks, stats, 0, watch, keep_own

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    def relu(self, x, inplace=False):
        lid = self._n
        self._n += 1
        st = self._stats
        own = x.detach() > 0
        if self._keep_own is not None:
            self._keep_own.append(own)
        m = own if self._masks is None else _layer_mask(self._masks, lid, x)
        diff = m != own
        n = int(diff.sum())
        st["n_relu_elements"] += x.numel()
        st["n_flips"] += n
        st.setdefault("call_dims", []).append(x.dim())
        if n:
            st["max_abs_preact_at_flip"] = max(st["max_abs_preact_at_flip"], float(x.detach().abs()[diff].max()))
            st["flips_per_layer"][lid] = n
            st.setdefault("max_abs_preact_per_layer", {})[lid] = float(x.detach().abs()[diff].max())
        if self._watch is not None:
            wd = m != _layer_mask(self._watch, lid, x)
            nw = int(wd.sum())
            if nw:
                st["n_watch_bits"] += nw
                st["max_abs_preact_at_watch_bit"] = max(st["max_abs_preact_at_watch_bit"],
                                                        float(x.detach().abs()[wd].max()))
        return _MaskedReLU.apply(x, m)


def hip_masks(tap):
    """tap: list of (conv index, y_raw [M, F], scale [F], shift [F]) from Pose2Mesh._tap -> list of bool CPU tensors in
    layer order.  Exactly the kernels' fmaf(y, scale, shift) > 0 (k_bn_act_fwd / k_bn_bwd_*), see the module docstring."""
    out = []
    for ci, y, sc, sh in sorted(tap, key=lambda t: t[0]):
        out.append(((y.double() * sc.double() + sh.double()) > 0).cpu())
    return out


def _state64(sd32, dtype):
    sd = {k: (v.detach().to(dtype).clone() if v.dtype.is_floating_point else v.detach().clone()) for k, v in sd32.items()}
    names = [k for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k]
    return sd, names


def masked_oracle_gradients(sd32, graph_L_torch32, x32, mano, w32, masks, dtype=torch.float64, training=True, watch=None):
    """Float64 oracle forward + backward with the ReLU masks forced to `masks` (None: its own).
    Returns (out, grads dict incl. '__input__', stats)."""
    sd, names = _state64(sd32, dtype)
    for k in names:
        sd[k].requires_grad_(True)
    x = x32.to(dtype).clone().requires_grad_(True)
    stats = new_stats()
    old_F = mo.F
    mo.F = proxy = _FProxy(masks, stats, watch)
    try:
        out = mo.meshnet_forward(sd, [g.to(dtype) for g in graph_L_torch32], x, mano, training)
    finally:
        mo.F = old_F
    assert masks is None or proxy._n == len(masks), (proxy._n, len(masks))
    (out * w32.to(dtype)).sum().backward()
    grads = {k: sd[k].grad for k in names}
    grads["__input__"] = x.grad
    return out.detach(), grads, stats


def oracle_own_masks(sd32, graph_L_torch32, x32, mano, training=True, dtype=torch.float64):
    """The float64 oracle's own masks (y64 > 0 of its unforced forward), one bool tensor [B, V, F] per ReLU call."""
    sd, _ = _state64(sd32, dtype)
    own = []
    old_F = mo.F
    mo.F = _FProxy(None, new_stats(), keep_own=own)
    try:
        with torch.no_grad():
            mo.meshnet_forward(sd, [g.to(dtype) for g in graph_L_torch32], x32.to(dtype), mano, training)
    finally:
        mo.F = old_F
    return own


def masks_from_record(own_masks, layer, index, bit):
    """The float64 oracle's own masks overridden at the recorded elements: `layer` is the ReLU call order (what _FProxy
    counts), `index` the flat index into that call's [B, V, F] tensor, `bit` the recorded y > 0 (the fixtures'
    {mode}_kink_layer / _index / _bit: every element the reference saw within KINK_WINDOW of 0)."""
    out = [m.clone() for m in own_masks]
    layer = torch.as_tensor(layer).long()
    index = torch.as_tensor(index).long()
    bit = torch.as_tensor(bit).bool()
    assert layer.shape == index.shape == bit.shape
    for lid in layer.unique().tolist():
        sel = layer == lid
        assert int(index[sel].max()) < out[lid].numel(), lid
        out[lid].view(-1)[index[sel]] = bit[sel]
    return out


def count_mask_bits(masks_a, masks_b):
    assert len(masks_a) == len(masks_b)
    n = 0
    for a, b in zip(masks_a, masks_b):
        a, b = torch.as_tensor(a).flatten(), torch.as_tensor(b).flatten()
        k = min(a.numel(), b.numel())
        assert max(a.numel(), b.numel()) < k + 8
        n += int((a[:k].bool().cpu() != b[:k].bool().cpu()).sum())
    return n


Accounted = collections.namedtuple("Accounted", "D n_bits max_abs_y G_a G_b out_a out_b flips_a flips_b")


def accounted_difference(sd, glt, x, mano, w, masks_a, masks_b, training=True):
    """What the bits in which two mask sets differ do to every gradient, in float64:
    D = G64(masks_a) - G64(masks_b) per tensor ('__input__' included), the number of differing bits and the largest
    |y64| at one of them.  Identical mask sets: one oracle run, D = 0.  Also returned: both gradient sets (G_b carries the
    scale of the comparison), both outputs, and each set's flips against the oracle's own masks."""
    n_bits = count_mask_bits(masks_a, masks_b)
    out_b, G_b, st_b = masked_oracle_gradients(sd, glt, x, mano, w, masks_b, training=training)
    if n_bits == 0:
        D = {k: torch.zeros_like(v) for k, v in G_b.items()}
        return Accounted(D, 0, 0.0, G_b, G_b, out_b, out_b, st_b["n_flips"], st_b["n_flips"])
    out_a, G_a, st_a = masked_oracle_gradients(sd, glt, x, mano, w, masks_a, training=training, watch=masks_b)
    assert st_a["n_watch_bits"] == n_bits, (st_a["n_watch_bits"], n_bits)
    D = {k: G_a[k] - G_b[k] for k in G_b}
    return Accounted(D, n_bits, st_a["max_abs_preact_at_watch_bit"], G_a, G_b, out_a, out_b, st_a["n_flips"],
                     st_b["n_flips"])


def assert_accounted(A, B, acc, tol, skip=None, norms=None, what=""):
    """Two fp32 gradient sets A (masks_a) and B (masks_b) of acc = accounted_difference(..., masks_a, masks_b): per tensor
        || (A - B) - D ||  <=  tol * || G64(masks_b) ||,
    and every differing bit lies within KINK_WINDOW of the kink.  Tensors are the keys of B (skip(k) true: left out);
    `norms`: name -> ||B|| for tensors of which only the norm is known: | ||A - D|| - ||B|| | <= tol * ||B||  (A - D is
    what A would have been with B's masks).  Returns {"n_bits", "max_abs_y", "worst", "at", "per"}: residual / scale."""
    assert acc.max_abs_y <= KINK_WINDOW, (what, acc.n_bits, acc.max_abs_y)
    per = {}
    for k, b in B.items():
        if skip is not None and skip(k):
            continue
        a = torch.as_tensor(A[k]).detach().cpu().double()
        b = torch.as_tensor(b).detach().cpu().double()
        assert a.shape == b.shape == acc.D[k].shape, (k, a.shape, b.shape)
        per[k] = float(((a - b) - acc.D[k]).norm() / (acc.G_b[k].norm() + 1e-30))
    for k, nb in (norms or {}).items():
        if k in per or (skip is not None and skip(k)):
            continue
        a = torch.as_tensor(A[k]).detach().cpu().double()
        per[k] = abs(float((a - acc.D[k]).norm()) - float(nb)) / (float(nb) + 1e-30)
    at = max(per, key=per.get)
    res = {"n_bits": acc.n_bits, "max_abs_y": acc.max_abs_y, "worst": per[at], "at": at, "per": per}
    bad = {k: v for k, v in per.items() if not v <= tol}
    assert not bad, f"{what}: accounted residual above {tol:g} with {acc.n_bits} mask bits subtracted: {bad}"
    return res


# ---------------------------------------------------------------------------------------------
# PoseNet (lib/models/posenet.py:25-38, 77-87): two BatchNorm-ReLU pairs per stage
# ---------------------------------------------------------------------------------------------
def posenet_small_batch_factor(B):
    """Factor on the PoseNet tolerances for batches of a handful of samples, where BatchNorm1d itself is ill-conditioned: a
    channel on which the 2-5 samples nearly agree is divided by sqrt(var + 1e-5), so fp32 round-off of z is amplified up to
    316 x - in the reference's own fp32 arithmetic just the same."""
    return 1.0 if B >= 30 else (20.0 if B >= 5 else 200.0)


def posenet_hip_masks(tap, Br):
    """The masks the stage kernels used, reproduced exactly: xhat = (z - mean) * invstd in fp32 (two roundings, as in
    k_pn_stage_fwd / _bwd), then the sign of fmaf(xhat, gamma, beta) - one rounding never changes a sign, so the product and
    sum are formed exactly in float64."""
    out = []
    for _, z, mu, istd, ga, be in sorted(tap, key=lambda t: t[0]):
        xh = (z[:Br] - mu) * istd
        out.append(((xh.double() * ga.double() + be.double()) > 0).cpu())
    return out


def posenet_masked_reference(sd, x, training, masks=None, p=0.0, dtype=torch.float64, relu_masks=None, kinks=None):
    """posenet.py:77-87 + :25-38 restated with optional dropout masks (uniform numbers: keep where u >= p, scale 1/(1-p)).
    relu_masks: one bool tensor per BatchNorm-ReLU (stage order) to use INSTEAD of the restatement's own y > 0; `kinks`
    (a dict) then receives how many elements differ and the largest |pre-activation| among them."""
    F = torch.nn.functional
    calls = [0]
    sd = {k: (v.to(dtype).clone() if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
    names = [k for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k and not k.startswith("batch_norm1")]
    for k in names:
        sd[k].requires_grad_(True)
    x = x.to(dtype)

    def lin(n, t):
        return F.linear(t, sd[n + ".weight"], sd[n + ".bias"])

    def stage(n, t, u):
        t = F.batch_norm(t, sd[n + ".running_mean"], sd[n + ".running_var"], sd[n + ".weight"], sd[n + ".bias"],
                         training, 0.1, 1e-5)
        if relu_masks is None:
            t = F.relu(t)
        else:
            m = relu_masks[calls[0]]
            diff = m != (t.detach() > 0)
            if kinks is not None:
                kinks["flips"] = kinks.get("flips", 0) + int(diff.sum())
                kinks["elements"] = kinks.get("elements", 0) + t.numel()
                if diff.any():
                    kinks["max_abs"] = max(kinks.get("max_abs", 0.0), float(t.detach().abs()[diff].max()))
            t = _MaskedReLU.apply(t, m.to(dtype))
        calls[0] += 1
        if u is not None:
            t = torch.where(u.to(dtype) >= p, t / (1.0 - p), torch.zeros_like(t))
        return t
    y = lin("w1", x)
    s = 0
    while f"linear_stages.{s}.w1.weight" in sd:
        q = f"linear_stages.{s}."
        z = lin(q + "w1", stage(q + "batch_norm1", y, None if masks is None else masks[2 * s]))
        z = lin(q + "w2", stage(q + "batch_norm2", z, None if masks is None else masks[2 * s + 1]))
        y = y + z
        s += 1
    return lin("w2", y), sd, names


# ---------------------------------------------------------------------------------------------
# the whole model: FlatPose2Mesh (lib/models/pose2mesh_net.py:16-22) + the train step's losses (lib/core/base.py:130-143)
# ---------------------------------------------------------------------------------------------
def flat_masked_oracle_gradients(sd32, graph_L_torch32, pose2d, mano, masks, loss_args, dtype=torch.float64,
                                 with_edge=True):
    """mo.flat_forward in train mode (dropout off) under _FProxy, then loss_oracle.train_losses and backward().
    masks: PoseNet's ReLU calls first (posenet_hip_masks order: two per stage), MeshNet's after them in call order
    (hip_masks) - the order is checked by counting the calls: the lifter's act on [B, hid], MeshNet's on [B, V, F].
    loss_args: (perm_reverse, nv, faces, J_regressor, gt_mesh, gt_reg3dpose, gt_lift3dpose, val_mesh, val_reg3dpose,
    val_lift3dpose) as train_losses takes them.  Returns (loss, {name: float64 gradient or None}, stats)."""
    sd, names = _state64(sd32, dtype)
    for k in names:
        sd[k].requires_grad_(True)
    stats = new_stats()
    n_lift = 2 * sum(1 for k in sd if k.startswith("pose_lifter.linear_stages.") and k.endswith(".w1.weight"))
    old_F = mo.F
    mo.F = proxy = _FProxy(masks, stats)
    try:
        mesh, lift = mo.flat_forward(sd, [g.to(dtype) for g in graph_L_torch32], pose2d.to(dtype), mano, True)
    finally:
        mo.F = old_F
    assert masks is None or proxy._n == len(masks), (proxy._n, len(masks))
    assert stats["call_dims"] == [2] * n_lift + [3] * (proxy._n - n_lift), stats["call_dims"]
    perm_reverse, nv, faces, jreg = loss_args[:4]
    rest = [torch.as_tensor(t).to(dtype) for t in loss_args[4:]]
    loss, _ = lo.train_losses(mesh, lift, perm_reverse, nv, faces, torch.as_tensor(jreg).to(dtype), *rest,
                              with_edge=with_edge)
    loss.backward()
    return loss.detach(), {k: sd[k].grad for k in names}, stats
