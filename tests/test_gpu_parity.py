"""-m gpu: the HIP path (through the C ABI) against (1) golden vectors produced by the real reference,
(2) the CPU oracle on the same seeded inputs, and (3) size-independent properties at BASELINE sizes.
Parity bar (BASELINE.json): per-vertex L2 <= 1e-4 on the output mesh."""
import numpy as np
import pytest
import torch

import helpers
import kinks
import meshnet_oracle as mo
from pose2mesh_release_amd import synth
from test_gpu_parity_full import ORACLE_THREADS, _record

pytestmark = pytest.mark.gpu
VERTEX_TOL = 1e-4
# the reference fixture's own distance from the float64 oracle on the same masks: the bounds that
# tests/test_oracle.py::test_meshnet_oracle_vs_golden asserts on the CPU (3 x measured, see there)
REFERENCE_CPU_BOUND = {("eval", "mano"): 3 * 1.34e-6, ("eval", "human36"): 3 * 2.86e-6,
                       ("train", "mano"): 3 * 2.02e-6, ("train", "human36"): 3 * 3.63e-6}


def _net(joint_set, gL, seed=1, flat=False):
    from pose2mesh_release_amd import meshnet, pose2mesh_net
    mano = joint_set == "mano"
    J = gL[-1].shape[0]
    net = pose2mesh_net.get_model(J, gL, mano=mano) if flat else meshnet.get_model(5, 3, gL, mano=mano)
    net.load_state_dict(helpers.numpy_state(net.state_dict(), seed))
    return net.cuda()


@pytest.mark.parametrize("joint_set", ["mano", "human36"])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_meshnet_vs_reference_golden(hip_libs, joint_set, mode):
    z = helpers.golden(f"meshnet_{joint_set}.npz")
    gL, _, _ = helpers.golden_graphs(joint_set)
    B, J = int(z["B"]), int(z["J"])
    train = mode == "train"
    net = _net(joint_set, gL).train(train)
    x = helpers.meshnet_input(B, J, seed=7).cuda().requires_grad_(True)
    net._tap = []                         # (the hook is live in eval() too: the BatchNorm is then the fixed affine map)
    y = net(x)
    err = helpers.max_vertex_l2(y.detach().cpu(), z[f"{mode}_out"])
    assert err <= VERTEX_TOL, f"max per-vertex L2 {err:.3e}"
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(3))
    (y * w.cuda()).sum().backward()
    masks_hip = kinks.hip_masks(net._tap)
    net._tap = None
    # What the reference fixture pins exactly: a conv bias in front of a train-mode BatchNorm has a true gradient of
    # exactly 0, and everything is finite.
    P = dict(net.named_parameters())
    assert torch.isfinite(x.grad).all()

    def zero_bias(k):
        return train and k.startswith("cl.") and k.endswith("bias") and f"bn.{k.split('.')[1]}.weight" in P
    for k in z[f"{mode}_grad_names"]:
        k = str(k)
        assert torch.isfinite(P[k].grad).all(), k
        if zero_bias(k):
            assert float(P[k].grad.norm()) < 1e-3 * max(1.0, float(P[k.replace("bias", "weight")].grad.norm()))
    # The reference's OWN gradients (x.grad, every stored full gradient, the norm of every gradient), with the ReLU kinks
    # accounted for exactly (tests/kinks.py): A = the kernels' gradients on the kernels' masks, B = the fixture's on the
    # reference's masks (the float64 oracle's, overridden at the fixture's record of the reference's near-kink elements),
    # D = G64(kernels' masks) - G64(reference's masks); (A - B) - D is round-off of the kernels (ALIGNED_GRAD_TOL) plus
    # round-off of the reference (the CPU bound of tests/test_oracle.py::test_meshnet_oracle_vs_golden).
    torch.set_num_threads(ORACLE_THREADS)
    sd = helpers.numpy_state(mo.init_state(J, mo.trim_graph_list(gL), bool(z["mano"])), 1)
    glt, xc = helpers.oracle_graphs(gL), helpers.meshnet_input(B, J, seed=7)
    own = kinks.oracle_own_masks(sd, glt, xc, bool(z["mano"]), train)
    masks_ref = kinks.masks_from_record(own, z[f"{mode}_kink_layer"], z[f"{mode}_kink_index"], z[f"{mode}_kink_bit"])
    acc = kinks.accounted_difference(sd, glt, xc, bool(z["mano"]), w, masks_hip, masks_ref, train)
    A = {k: p.grad for k, p in P.items()}
    A["__input__"] = x.grad
    Bf = {"__input__": z[f"{mode}_gin"]}
    Bf.update({k[len(mode) + 7:]: z[k] for k in z.files if k.startswith(f"{mode}_grad::")})
    norms = {str(k): float(n) for k, n in zip(z[f"{mode}_grad_names"], z[f"{mode}_grad_norms"])}
    assert set(norms) == set(P) and len(Bf) > 20
    tol = kinks.ALIGNED_GRAD_TOL + REFERENCE_CPU_BOUND[(mode, joint_set)]
    res = kinks.assert_accounted(A, Bf, acc, tol, skip=zero_bias, norms=norms, what=f"{joint_set} {mode} vs fixture")
    _record(f"g_meshnet_{joint_set}_{mode}_vs_reference_fixture",
            {"mask_bits_differing": acc.n_bits, "max_abs_y64_at_a_differing_bit": acc.max_abs_y,
             "flips_vs_float64_kernels": acc.flips_a, "flips_vs_float64_reference": acc.flips_b,
             "worst_accounted_residual": res["worst"], "at": res["at"], "tensors": len(res["per"]), "bound": tol})
    assert max(acc.flips_a, acc.flips_b) <= max(20, 4e-6 * sum(m.numel() for m in own)), (acc.flips_a, acc.flips_b)
    if mode == "train":
        for k, v in net.state_dict().items():
            if "running" in k:
                assert np.abs(v.cpu().numpy() - z[f"train_state::{k}"]).max() < 1e-4, k
            if "num_batches_tracked" in k:
                assert int(v) == 1


@pytest.mark.parametrize("joint_set", ["mano", "coco"])
def test_flat_model_vs_reference_golden(hip_libs, joint_set):
    z = helpers.golden(f"flat_{joint_set}.npz")
    gL, _, _ = helpers.golden_graphs(joint_set)
    B, J = int(z["B"]), int(z["J"])
    from pose2mesh_release_amd import ops
    net = _net(joint_set, gL, seed=2, flat=True).eval()
    ops.TIMER = ops.KernelTimer()
    try:
        with torch.no_grad():
            mesh, pose3d = net(synth.pose2d_batch(B, J, seed=11).cuda())
        summ = ops.TIMER.summary()
    finally:
        ops.TIMER = None
    # the fixture's batch is 2 / 4: since round 6 such batches run on posenet.hip too (zero-padded), not on stock modules
    assert summ.get("pn_gemm", {}).get("launches", 0) == 6, summ.keys()
    assert helpers.max_vertex_l2(mesh.cpu(), z["cam_mesh"]) <= VERTEX_TOL
    # the bound tests/test_gpu_posenet.py asserts for the same kernels against float64 (the fixture is 1.4e-7 from float64)
    d = float(np.abs(pose3d.cpu().numpy() - z["pose3d"]).max())
    bound = 5e-5 * max(1.0, float(np.abs(z["pose3d"]).max()))
    _record(f"g_flat_{joint_set}_pose3d_vs_reference_fixture", {"max_abs_diff": d, "bound": bound})
    assert d <= bound, d


def test_graph_conv_cheby_vs_reference_golden(hip_libs):
    from pose2mesh_release_amd.cheby_graph_conv import graph_conv_cheby
    z = helpers.golden("chebconv.npz")
    gL, _, _ = helpers.golden_graphs("mano")
    ci = 0
    while f"c{ci}_meta" in z:
        lvl, Fin, Fout, has_bn, B = [int(v) for v in z[f"c{ci}_meta"]]
        L = gL[lvl]
        rng = np.random.default_rng(100 + ci)
        x = torch.from_numpy(rng.standard_normal((B, L.shape[0], Fin)).astype(np.float32)).cuda().requires_grad_(True)
        cl = torch.nn.Linear(Fin * 3, Fout)
        bn = torch.nn.BatchNorm1d(Fout) if has_bn else None
        with torch.no_grad():
            cl.weight.copy_(torch.from_numpy(rng.uniform(-0.1, 0.1, cl.weight.shape).astype(np.float32)))
            cl.bias.copy_(torch.from_numpy(rng.uniform(-0.1, 0.1, cl.bias.shape).astype(np.float32)))
            if bn is not None:
                bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, (Fout,)).astype(np.float32)))
                bn.bias.copy_(torch.from_numpy(rng.uniform(-0.2, 0.2, (Fout,)).astype(np.float32)))
        cl = cl.cuda()
        bn = bn.cuda() if bn is not None else None
        y = graph_conv_cheby(x, cl, bn, L, Fout, 3)
        w = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32)).cuda()
        (y * w).sum().backward()
        assert np.abs(y.detach().cpu().numpy() - z[f"c{ci}_y"]).max() < 2e-5
        assert helpers.rel_l2(x.grad.cpu(), z[f"c{ci}_dx"]) < 1e-4
        assert helpers.rel_l2(cl.weight.grad.cpu(), z[f"c{ci}_dW"]) < 1e-4
        if has_bn:
            assert helpers.rel_l2(bn.weight.grad.cpu(), z[f"c{ci}_dgamma"]) < 1e-4
            assert helpers.rel_l2(bn.bias.grad.cpu(), z[f"c{ci}_dbeta"]) < 1e-4
            assert np.abs(bn.running_mean.cpu().numpy() - z[f"c{ci}_rm"]).max() < 1e-5
            assert np.abs(bn.running_var.cpu().numpy() - z[f"c{ci}_rv"]).max() < 1e-5
        else:
            assert helpers.rel_l2(cl.bias.grad.cpu(), z[f"c{ci}_db"]) < 1e-4
        ci += 1


def test_graph_conv_cheby_low_orders_and_inputs(hip_libs):
    """K=1,2 (zero-padded planes) against the oracle; torch-sparse L as the reference passes it."""
    from pose2mesh_release_amd.cheby_graph_conv import graph_conv_cheby
    gL, _, _ = helpers.golden_graphs("mano")
    L = gL[3]
    Lt = mo.scipy_to_torch_coo(L)
    for K in (1, 2):
        x = torch.randn(2, L.shape[0], 32, generator=torch.Generator().manual_seed(K))
        cl = torch.nn.Linear(32 * K, 64)
        ref = mo.graph_conv_cheby(x, cl.weight.detach(), cl.bias.detach(), None, Lt, K, False)
        y = graph_conv_cheby(x.cuda(), cl.cuda(), None, Lt, 64, K)
        assert (y.cpu() - ref).abs().max() < 1e-5


@pytest.mark.parametrize("K", [4, 6])
def test_graph_conv_cheby_higher_orders_vs_oracle(hip_libs, K):
    """cheby_graph_conv.py:27-30 is generic in K: orders above 3 (which Pose2Mesh never uses) run the recurrence on the HIP
    L-product; forward, BatchNorm statistics and every gradient against the oracle's sparse-mm form."""
    from pose2mesh_release_amd.cheby_graph_conv import graph_conv_cheby
    gL, _, _ = helpers.golden_graphs("mano")
    L = gL[3]
    Lt = mo.scipy_to_torch_coo(L)
    gen = torch.Generator().manual_seed(40 + K)
    x = torch.randn(3, L.shape[0], 16, generator=gen)
    cl = torch.nn.Linear(16 * K, 24)
    bn = torch.nn.BatchNorm1d(24)
    w = torch.randn(3, L.shape[0], 24, generator=gen)
    xr = x.clone().requires_grad_(True)
    wr, br = cl.weight.detach().clone().requires_grad_(True), cl.bias.detach().clone().requires_grad_(True)
    bnd = {"weight": bn.weight.detach().clone().requires_grad_(True), "bias": bn.bias.detach().clone().requires_grad_(True),
           "running_mean": bn.running_mean.clone(), "running_var": bn.running_var.clone()}
    ref = mo.graph_conv_cheby(xr, wr, br, bnd, Lt, K, True)
    (ref * w).sum().backward()
    cl, bn = cl.cuda(), bn.cuda().train()
    xg = x.cuda().requires_grad_(True)
    y = graph_conv_cheby(xg, cl, bn, Lt, 24, K)
    (y * w.cuda()).sum().backward()
    assert (y.detach().cpu() - ref.detach()).abs().max() < 2e-5
    assert helpers.rel_l2(xg.grad.cpu(), xr.grad) < 1e-4
    assert helpers.rel_l2(cl.weight.grad.cpu(), wr.grad) < 1e-4
    assert helpers.rel_l2(bn.weight.grad.cpu(), bnd["weight"].grad) < 1e-4
    assert (bn.running_var.cpu() - bnd["running_var"]).abs().max() < 1e-5


@pytest.mark.parametrize("joint_set,B", [("mano", 5), ("human36", 3)])
def test_meshnet_vs_oracle_fresh_inputs(hip_libs, joint_set, B):
    """Different seeds / batch sizes than the goldens, against the CPU oracle (eval and train)."""
    gL, _, _ = helpers.golden_graphs(joint_set)
    J = gL[-1].shape[0]
    mano = joint_set == "mano"
    glt = helpers.oracle_graphs(gL)
    for training in (False, True):
        net = _net(joint_set, gL, seed=21).train(training)
        sd = helpers.numpy_state(net.state_dict(), 21)
        x = helpers.meshnet_input(B, J, seed=99)
        ref, _, _ = helpers.oracle_run(sd, glt, x, mano, training)
        with torch.no_grad():
            out = net(x.cuda())
        assert helpers.max_vertex_l2(out.cpu(), ref) <= VERTEX_TOL


def test_properties_at_baseline_batch(hip_libs):
    """BASELINE sizes (B=256 MANO / B=64 SMPL are too slow for the CPU oracle) -> size-independent properties:
    eval-mode samples are independent, the result is deterministic, and fake vertices never leak into real ones."""
    gL, perm0, _ = helpers.golden_graphs("mano")
    J = gL[-1].shape[0]
    net = _net("mano", gL, seed=5).eval()
    x = helpers.meshnet_input(256, J, seed=4).cuda()
    with torch.no_grad():
        big = net(x)
        again = net(x)
        small = net(x[37:41])
    assert torch.equal(big, again)                                    # deterministic (no atomics)
    assert (big[37:41] - small).abs().max() < 1e-6                    # sample independence in eval()
    glt = helpers.oracle_graphs(gL)
    ref, _, _ = helpers.oracle_run(helpers.numpy_state(net.state_dict(), 5), glt, x[:2].cpu(), True, False)
    assert helpers.max_vertex_l2(big[:2].cpu(), ref) <= VERTEX_TOL
    # train(): BatchNorm output statistics over all B*V rows of the first layer are (0,1) before affine
    gS, _, _ = helpers.golden_graphs("human36")
    netS = _net("human36", gS, seed=6).eval()
    with torch.no_grad():
        o = netS(helpers.meshnet_input(64, 17, seed=8).cuda())      # configs[1]: batch 64 SMPL fwd
    assert o.shape == (64, gS[0].shape[0], 3) and torch.isfinite(o).all()


def test_edge_cases(hip_libs):
    from pose2mesh_release_amd import meshnet
    from pose2mesh_release_amd._lib import P2MError
    gL, _, _ = helpers.golden_graphs("mano")
    J = gL[-1].shape[0]
    net = _net("mano", gL, seed=3).eval()
    x1 = helpers.meshnet_input(1, J, seed=2)
    with torch.no_grad():
        a = net(x1.cuda())                                            # B = 1 (demo path)
        b = net(x1.view(1, J * 5).cuda())                             # flat input, as x.view(-1, J, 5) accepts
        c = net(x1.cuda().transpose(1, 2).contiguous().transpose(1, 2))   # non-contiguous input
    assert torch.equal(a, b) and torch.equal(a, c)
    ref, _, _ = helpers.oracle_run(helpers.numpy_state(net.state_dict(), 3), helpers.oracle_graphs(gL), x1, True, False)
    assert helpers.max_vertex_l2(a.cpu(), ref) <= VERTEX_TOL
    # caller's list is not mutated (the reference deletes graph_L[-2] in place, meshnet.py:35)
    lst = list(gL)
    meshnet.get_model(5, 3, lst, mano=True)
    assert len(lst) == len(gL)
    with pytest.raises(ValueError):
        meshnet.get_model(5, 3, gL[:-1], mano=True)                   # wrong number of levels
    with pytest.raises(P2MError):
        net(x1)                                                       # CPU tensor: no silent fallback
    # state dict round trip with the reference's key set
    keys = set(net.state_dict().keys())
    assert "fc.weight" in keys and "cl.14.weight" in keys and "bn.13.running_var" in keys and "bn.14.weight" not in keys


def test_fake_vertex_split_network_equivalence(hip_libs):
    """The real/fake row-set launches (ops.SPLIT_FAKE) give the same network output and gradients as the unsplit
    kernels (SMPL-like levels: 41 % padding vertices at the finest level).  Two fp32 evaluations, each within
    ALIGNED_GRAD_TOL of float64 on its own masks: the ReLU masks of both runs are tapped, what their differing bits do to
    every gradient is subtracted in float64 (tests/kinks.py), and the rest is held to 2 x ALIGNED_GRAD_TOL."""
    from pose2mesh_release_amd import ops
    gL, _, _ = helpers.golden_graphs("human36")
    x = helpers.meshnet_input(2, 17, seed=5)
    outs, grads, masks = [], [], []
    old = ops.SPLIT_FAKE
    try:
        for flag in (True, False):
            ops.SPLIT_FAKE = flag
            net = _net("human36", gL, seed=4).train()
            assert any(g.split for g in net._graph_cache.on(torch.device("cuda", 0))) == flag
            xg = x.cuda().requires_grad_(True)
            net._tap = []
            y = net(xg)
            w = torch.randn(y.shape, generator=torch.Generator().manual_seed(9))
            (y * w.cuda()).sum().backward()
            masks.append(kinks.hip_masks(net._tap))
            net._tap = None
            outs.append(y.detach())
            grads.append({k: p.grad.clone() for k, p in net.named_parameters()})
            grads[-1]["__input__"] = xg.grad.clone()
    finally:
        ops.SPLIT_FAKE = old
    assert helpers.max_vertex_l2(outs[0].cpu(), outs[1].cpu()) <= 2e-5
    torch.set_num_threads(ORACLE_THREADS)
    sd = helpers.numpy_state(mo.init_state(17, mo.trim_graph_list(gL), False), 4)
    acc = kinks.accounted_difference(sd, helpers.oracle_graphs(gL), x, False, w, masks[0], masks[1], True)
    # exactly-zero gradients in front of train-mode BatchNorm (round-off only) are left out
    res = kinks.assert_accounted(grads[0], grads[1], acc, 2 * kinks.ALIGNED_GRAD_TOL, what="split vs unsplit",
                                 skip=lambda k: k.startswith("cl.") and k.endswith("bias") and k != "cl.20.bias")
    _record("g_fake_vertex_split_vs_unsplit",
            {"mask_bits_differing": acc.n_bits, "max_abs_y64_at_a_differing_bit": acc.max_abs_y,
             "worst_accounted_residual": res["worst"], "at": res["at"], "bound": 2 * kinks.ALIGNED_GRAD_TOL})
