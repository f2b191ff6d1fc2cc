"""Float64 restatement of one PoseNet stage (csrc/posenet.hip: k_pn_stage_fwd / k_pn_stage_bwd; lib/models/posenet.py:25-38,
79-87: sum of the contraction's partials + bias + residual, BatchNorm1d in train or eval mode, ReLU, dropout from GIVEN uniform
numbers), forward and backward, the restated row walk of the two kernels, and the table of cases that
tests/test_gpu_posenet_edges.py runs.  No GPU and no library: tests/test_posenet_ref_cpu.py checks the backward against torch's
float64 autograd of the forward, audits which trip of pass 1, which pass of the transposed-store tile and which column quads
every case reaches, and counts the elements at the ReLU kink.

The functions take tensors on any device and return float64 tensors on the same device, over the B_real rows that hold samples.

How the kernels move rows (restated below): a block owns PN_COLS = 32 columns, a thread 4 of them and the rows ty, ty + 32, ...
(PN_RG = 32 row groups).  Pass 1 takes 4 rows per trip (r, r + 32, r + 64, r + 96; r += 128): a row past B is clamped to B - 1
and a `break` decides which of the four loaded rows is stored and summed.  Pass 2 and the transposed store go through an LDS
tile of PN_TROWS = 256 rows, refilled between two barriers for B > 256.  F % 4 == 0 is all the C entry asks, so the last block
holds 1 .. 8 live column quads next to dead ones, and the dead threads still take part in the column sums."""
import math

import torch

EPS, MOMENTUM = 1e-5, 0.1
PN_COLS, PN_Q, PN_RG, PN_TROWS = 32, 8, 32, 256
TRIP_ROWS = 4 * PN_RG            # rows of one trip of pass 1, over the whole block
KINK = 1e-5                      # |pre-activation| below this: the element may take either ReLU mask in fp32
KINK_CAP = 2                     # at most this many such elements per (case, nch, variant)

# (bias, residual / addend, BatchNorm: None / "train" / "eval", p_drop)
PN_VARIANTS = [(True, True, "train", 0.5), (True, False, "eval", 0.0), (False, True, "train", 0.0), (True, True, None, 0.0),
               (False, False, "eval", 0.5)]


# ---- inputs ------------------------------------------------------------------------------------------------------------------

def pn_inputs(B, F, nch, seed):
    """The tensors of one stage, forward and backward, seeded, on the CPU: B rows, all of them drawn."""
    gen = torch.Generator().manual_seed(seed)
    return {"P": torch.randn(nch, B, F, generator=gen), "bias": torch.randn(F, generator=gen),
            "resid": torch.randn(B, F, generator=gen), "rnd": torch.rand(B, F, generator=gen),
            "gamma": torch.rand(F, generator=gen) + 0.5, "beta": 0.2 * torch.randn(F, generator=gen),
            "rm": 0.1 * torch.randn(F, generator=gen), "rv": torch.rand(F, generator=gen) + 0.5,
            "G": torch.randn(nch, B, F, generator=gen), "addend": torch.randn(B, F, generator=gen)}


ROW_TENSORS = ("P", "resid", "rnd", "G", "addend")     # [.., B, F]: what has padding rows


def pad_rows(d, B):
    """The inputs of pn_inputs(B_real, ...) with the row tensors padded to B rows.  The padding holds 0.75: a kernel that lets a
    padding row into a statistic or a sum shows it even without the poison."""
    out = dict(d)
    for k in ROW_TENSORS:
        t = d[k]
        Br = t.shape[-2]
        if B > Br:
            out[k] = torch.cat([t, torch.full(t.shape[:-2] + (B - Br, t.shape[-1]), 0.75)], -2)
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def z_ref(P, Br, bias=None, resid=None):
    """z = sum of the partials + bias + residual over the first Br rows ([nch, B, F] -> [Br, F])."""
    z = P.double().sum(0)[:Br]
    if bias is not None:
        z = z + bias.double()
    if resid is not None:
        z = z + resid.double()[:Br]
    return z


def _affine(z, gamma, beta):
    one, zero = torch.ones(z.shape[1], dtype=z.dtype, device=z.device), torch.zeros(z.shape[1], dtype=z.dtype, device=z.device)
    return (one if gamma is None else gamma.to(z.dtype)), (zero if beta is None else beta.to(z.dtype))


def stats_ref(z, bn, rm=None, rv=None, eps=EPS):
    """(mean, variance used to normalise, invstd): the batch's (biased variance) in train mode, the running ones in eval mode."""
    if bn == "train":
        mu, var = z.mean(0), z.var(0, unbiased=False)
    else:
        mu, var = rm.to(z.dtype), rv.to(z.dtype)
    return mu, var, 1.0 / torch.sqrt(var + eps)


def running_ref(rm, rv, mu, var, Br, momentum=MOMENTUM):
    """nn.BatchNorm1d's update: (1 - momentum) * running + momentum * batch statistic, with the UNBIASED variance (one sample:
    the kernel's factor 1)."""
    ub = Br / (Br - 1.0) if Br > 1 else 1.0
    return (1.0 - momentum) * rm.double() + momentum * mu, (1.0 - momentum) * rv.double() + momentum * var * ub


def act_ref(z, bn, gamma=None, beta=None, rm=None, rv=None, rnd=None, p_drop=0.0, eps=EPS):
    """a = dropout(relu(batch_norm(z))) (bn None: a = z), in z's dtype, differentiable in z, gamma and beta.  rnd: uniform
    numbers [>= Br, F]: keep where u >= p_drop, scale 1 / (1 - p_drop).  Returns (a, pre-activation or None, mean, var, invstd)."""
    if bn is None:
        return z, None, None, None, None
    Br = z.shape[0]
    mu, var, istd = stats_ref(z, bn, rm, rv, eps)
    ga, be = _affine(z, gamma, beta)
    pre = (z - mu) * istd * ga + be
    a = torch.relu(pre)
    if rnd is not None and p_drop > 0:
        a = torch.where(rnd[:Br] >= p_drop, a / (1.0 - p_drop), torch.zeros_like(a))
    return a, pre, mu, var, istd


def near_kink(pre):
    """Elements whose pre-activation is within KINK of the ReLU kink (none without BatchNorm)."""
    return pre.detach().abs() < KINK


def bwd_ref(z, ga, bn, gamma=None, beta=None, rm=None, rv=None, rnd=None, p_drop=0.0, addend=None, eps=EPS):
    """Backward of act_ref in closed form.  z [Br, F] float64: the stage's saved z; ga [Br, F]: the gradient w.r.t. a.
    g_u = g_a * dropout mask * relu mask; dbeta = sum g_u, dgamma = sum g_u xhat; train: g_z = gamma invstd (g_u - mean(g_u) -
    xhat mean(g_u xhat)), eval: g_z = gamma invstd g_u; no BatchNorm: g_z = g_a; + addend.  dbias = column sums of g_z (the bias
    gradient of the Linear that produced z).  Returns (gz, dgamma, dbeta, dbias, near): dgamma / dbeta None without BatchNorm."""
    z, ga = z.double(), ga.double()
    Br = z.shape[0]
    dgamma = dbeta = None
    near = torch.zeros_like(z, dtype=torch.bool)
    if bn is None:
        gz = ga
    else:
        mu, var, istd = stats_ref(z, bn, rm, rv, eps)
        gam, bet = _affine(z, gamma, beta)
        xh = (z - mu) * istd
        pre = xh * gam + bet
        near = near_kink(pre)
        gu = ga
        if rnd is not None and p_drop > 0:
            gu = torch.where(rnd[:Br] >= p_drop, gu / (1.0 - p_drop), torch.zeros_like(gu))
        gu = torch.where(pre > 0, gu, torch.zeros_like(gu))
        dbeta, dgamma = gu.sum(0), (gu * xh).sum(0)
        if bn == "train":
            gz = gam * istd * (gu - dbeta / Br - xh * (dgamma / Br))
        else:
            gz = gam * istd * gu
    if addend is not None:
        gz = gz + addend.double()[:Br]
    return gz, dgamma, dbeta, gz.sum(0), near


def stage_ref(d, Br, bias, resid, bn, p_drop, gamma=True, beta=True, dtype=torch.float64):
    """One whole stage on the inputs of pn_inputs, forward and backward (the backward on the restatement's own z): a dict of z,
    a, pre, mean, invstd, rm, rv (the running statistics afterwards), gz, dgamma, dbeta, dbias, near.  dtype float32: the same
    lines in torch's fp32, forward only (what a bar is measured against)."""
    z = z_ref(d["P"], Br, d["bias"] if bias else None, d["resid"] if resid else None)
    gam, bet = (d["gamma"] if gamma else None), (d["beta"] if beta else None)
    rnd = d["rnd"] if (bn and p_drop > 0) else None
    if dtype != torch.float64:
        z32 = d["P"].to(dtype).sum(0)[:Br]
        if bias:
            z32 = z32 + d["bias"].to(dtype)
        if resid:
            z32 = z32 + d["resid"].to(dtype)[:Br]
        a32 = act_ref(z32, bn, gam, bet, d["rm"], d["rv"], rnd, p_drop)[0]
        return {"z": z32, "a": a32}
    a, pre, mu, var, istd = act_ref(z, bn, gam, bet, d["rm"], d["rv"], rnd, p_drop)
    out = {"z": z, "a": a, "pre": pre, "mean": mu, "invstd": istd, "rm": d["rm"].double(), "rv": d["rv"].double()}
    if bn == "train":
        out["rm"], out["rv"] = running_ref(d["rm"], d["rv"], mu, var, Br)
    ga = d["G"].double().sum(0)[:Br]
    out["gz"], out["dgamma"], out["dbeta"], out["dbias"], out["near"] = bwd_ref(
        z, ga, bn, gam, bet, d["rm"], d["rv"], rnd, p_drop, d["addend"] if resid else None)
    return out


# ---- the row walk of the kernels, restated -----------------------------------------------------------------------------------

def trips(B, ty):
    """Trips of pass 1 (`for (r = ty; r < B; r += 128)`) of the threads of row group ty: ceil((B - ty) / 128)."""
    return max(0, -(-(B - ty) // TRIP_ROWS))


def last_trip(B, Br):
    """(trips of the block = those of ty = 0, row groups that make that many, the set of live-row counts 1 .. 4 - the u before
    the `break` - on that trip, clamped loads on it, padding rows >= Br on it)."""
    t = trips(B, 0)
    groups = [ty for ty in range(PN_RG) if trips(B, ty) == t]
    live, clamped, pad = set(), 0, 0
    for ty in groups:
        rows = [ty + (t - 1) * TRIP_ROWS + u * PN_RG for u in range(4)]
        n = sum(r < B for r in rows)
        assert rows[0] < B and all(r < B for r in rows[:n]) and all(r >= B for r in rows[n:])
        live.add(n)
        clamped += 4 - n
        pad += sum(Br <= r < B for r in rows)
    return t, len(groups), live, clamped, pad


def tile_passes(B):
    """(passes of the PN_TROWS-row tile: ceil(B / 256), rows of the last one)."""
    n = -(-B // PN_TROWS)
    return n, B - (n - 1) * PN_TROWS


def quads(F):
    """(blocks, live column quads of the last block, dead ones)."""
    nb = -(-F // PN_COLS)
    live = (F - (nb - 1) * PN_COLS) // 4
    return nb, live, PN_Q - live


# ---- the case table ----------------------------------------------------------------------------------------------------------
# (B, B_real, F); B_real = 0: all B rows hold samples.  Every case runs with nch in NCH and the five PN_VARIANTS.
EDGE_CASES = [
    (128, 0, 32),        # one trip, exactly full (all four rows live, nothing clamped)
    (129, 0, 36),        # odd B; a second trip with only u = 0 live; a full block plus one live quad
    (132, 129, 36),      # the same 129 samples, padded: 3 padding rows on the second trip
    (256, 0, 32),        # exactly one tile pass, two trips
    (257, 0, 4),         # a second tile pass of one row; one live quad in the only block; odd aT stride
    (260, 257, 68),      # a second tile pass of 4 rows (1 real, 3 padding); third trip clamped
    (516, 513, 36),      # three tile passes; fifth trip
    (64, 0, 28),         # 7 live quads, 1 dead
    (40, 37, 4),         # one live quad, with padding
]
NCH = (1, 3)
# input seeds per (B_real, F, nch), default 1: chosen on the CPU so that the float64 restatement alone has at most KINK_CAP
# elements within KINK of the ReLU kink in every variant (tests/test_posenet_ref_cpu.py counts them).  Seed 1 gives 0 or 1 per
# variant; the four entries below are the shapes where it gives 1, and with them every count is 0 - so no element can take
# the other mask in fp32 and move a column sum.
EDGE_SEEDS = {(128, 32, 3): 2, (257, 68, 1): 2, (257, 68, 3): 3, (513, 36, 3): 2}
ARM_SHAPES = [(132, 129, 36), (260, 257, 68)]     # where the arms no other test calls are run


# The arms of the two C entries that no other test calls, run at ARM_SHAPES:
# name -> (nch, bias, residual / addend, BatchNorm, p_drop, gamma / beta given, B_real instead of the shape's or None)
ARMS = {
    "no_z_train":        (1, False, False, "train", 0.5, True, None),    # z == NULL: P is the tensor itself
    "no_z_eval":         (1, False, False, "eval", 0.0, True, None),
    "no_z_plain":        (1, False, False, None, 0.0, True, None),
    "null_affine_train": (3, True, True, "train", 0.5, False, None),     # NULL gamma / beta: the kernels' 1 / 0
    "null_affine_eval":  (3, True, False, "eval", 0.0, False, None),
    "no_running":        (3, True, True, "train", 0.0, True, None),      # training without running statistics
    "single_outputs":    (3, True, True, "train", 0.5, True, None),      # a only, aT only; backward without gzT, without sums
    "eval_addend":       (3, True, True, "eval", 0.5, True, None),       # eval-mode backward with an addend
    "one_sample_eval":   (3, True, True, "eval", 0.5, True, 1),
    "one_sample_train":  (3, True, True, "train", 0.5, True, 1),         # var = 0: invstd = 1 / sqrt(eps), a = dropout(relu(beta))
}


def case_inputs(B, B_real, F, nch):
    """Inputs of a case of EDGE_CASES: B_real (or B) drawn rows - so (129, 0, 36) and (132, 129, 36) hold the same 129 samples -
    padded to B rows."""
    Br = B_real or B
    return pad_rows(pn_inputs(Br, F, nch, EDGE_SEEDS.get((Br, F, nch), 1)), B)


def arm_inputs(name, B, B_real, F):
    """(inputs, rows that hold samples) of an arm of ARMS at a shape of ARM_SHAPES: the case's inputs for three chunks, cut to
    the arm's chunk count."""
    nch, Br = ARMS[name][0], ARMS[name][6] or B_real or B
    d = case_inputs(B, B_real, F, 3)
    d["P"], d["G"] = d["P"][:nch].contiguous(), d["G"][:nch].contiguous()
    return d, Br


def arm_ref(name, d, Br):
    """The float64 stage of an arm on arm_inputs' tensors (any device)."""
    _, bias, resid, bn, p_drop, affine, _ = ARMS[name]
    return stage_ref(d, Br, bias, resid, bn, p_drop, gamma=affine, beta=affine)


def sum_bar(B, ref):
    """The bar of dgamma / dbeta / dbias: 1e-5 sqrt(B) max(1, max |ref|)."""
    return 1e-5 * math.sqrt(B) * max(1.0, float(ref.abs().max()))
