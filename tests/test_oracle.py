"""CPU: the oracle (oracle/*.py) against the golden vectors produced by the real reference, and -- when
/root/reference is present -- against the live reference itself."""
import numpy as np
import pytest
import torch

import coarsen_oracle as co
import helpers
import meshnet_oracle as mo
import ref_loader
from pose2mesh_release_amd import synth


def test_compute_perm_known_answer():
    """The reference's only golden vector (lib/coarsening.py:261-262)."""
    got = co.tree_permutations([np.array([4, 1, 1, 2, 2, 3, 0, 0, 3]), np.array([2, 1, 0, 1, 0])])
    assert got == [[3, 4, 0, 9, 1, 2, 5, 8, 6, 7, 10, 11], [2, 4, 1, 3, 0, 5], [0, 1, 2]]


@pytest.mark.parametrize("joint_set", ["mano", "human36"])
def test_coarsen_oracle_vs_golden(joint_set):
    J, skel, flip, levels = synth.JOINT_SETS[joint_set]
    _, faces = synth.hull_mesh(778 if joint_set == "mano" else 6890, 0)
    _, gL, perms, rev = co.build_coarse_graphs(faces, J, skel, flip, levels)
    ref_L, perm0, perm_rev = helpers.golden_graphs(joint_set)
    assert list(perms[0]) == list(perm0) and list(rev) == list(perm_rev)
    for a, b in zip(gL, ref_L):
        assert a.shape == b.shape and a.nnz == b.nnz
        assert abs(a - b).max() < 1e-10            # ARPACK start-vector wobble only
        assert abs(a - a.T).max() < 1e-12          # coarsening.py:23


@pytest.mark.parametrize("joint_set", ["mano", "human36"])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_meshnet_oracle_vs_golden(joint_set, mode):
    z = helpers.golden(f"meshnet_{joint_set}.npz")
    gL, _, _ = helpers.golden_graphs(joint_set)
    B, J, mano = int(z["B"]), int(z["J"]), bool(z["mano"])
    glt = helpers.oracle_graphs(gL)
    sd = helpers.numpy_state(mo.init_state(J, mo.trim_graph_list(gL), mano), 1)
    x = helpers.meshnet_input(B, J, seed=7)
    out, grads, sd2 = helpers.oracle_run(sd, glt, x, mano, mode == "train", grad_seed=3)
    assert helpers.max_vertex_l2(out, z[f"{mode}_out"]) < (2e-5 if mode == "train" else 2e-6)
    flips = None
    if mode == "train":
        # The fp32 oracle and the reference take different ReLU masks at a handful of kink elements (unaligned, the worst
        # tensor is 7.2e-3 apart at human36).  So: the float64 oracle, forced to the masks the reference used - its own,
        # overridden at the fixture's record of the reference's near-kink elements (tests/kinks.py).
        import kinks
        w = torch.randn(out.shape, generator=torch.Generator().manual_seed(3))
        own = kinks.oracle_own_masks(sd, glt, x, mano, True)
        masks = kinks.masks_from_record(own, z["train_kink_layer"], z["train_kink_index"], z["train_kink_bit"])
        _, grads, st = kinks.masked_oracle_gradients(sd, glt, x, mano, w, masks, training=True)
        flips = (st["n_flips"], st["max_abs_preact_at_flip"])
        assert st["n_flips"] == kinks.count_mask_bits(own, masks)
        # every flip is a genuine kink element, and there is only a handful (the GPU tests' rule; identical padding rows
        # flip together)
        assert st["max_abs_preact_at_flip"] <= kinks.KINK_WINDOW, st
        assert st["n_flips"] <= max(20, 4e-6 * st["n_relu_elements"]), st
    # Bounds: 3 x the worst value measured, per mode and joint set (worst full tensor incl. gin, rel-L2; the norms,
    # relative, stay below it).
    #   eval, fp32 oracle vs fixture.  The fp32 sums depend on torch's thread count, which is the host's: measured with
    #   1, 2, 3, 5, 8, 16, 32 and 64 threads, full tensors / norms
    #     mano     1.34e-6 / 7.5e-7 (1 thread), 4.4e-7 / 2.2e-7 (16), 5.4e-7 / 2.6e-7 (32), 0 / 0 (8: the fixture's own count)
    #     human36  2.86e-6 / 1.26e-6 (1 thread), 6.1e-7 / 1.7e-7 (16), 6.3e-7 / 1.9e-7 (32), 0 / 0 (8)
    #   (output and gin are bitwise equal at every count; bitwise equality is not asserted.)
    #   train, float64 oracle on the reference's masks vs fixture (thread-independent):
    #     mano     2.02e-6 (bn.12.weight), norms 2.3e-7;  0 flips
    #     human36  3.63e-6 (bn.16.weight), norms 8.2e-7; 44 flips, |y64| <= 4.8e-6
    bound = {("eval", "mano"): 3 * 1.34e-6, ("eval", "human36"): 3 * 2.86e-6,
             ("train", "mano"): 3 * 2.02e-6, ("train", "human36"): 3 * 3.63e-6}[(mode, joint_set)]
    worst = {"full": (0.0, None), "norm": (0.0, None)}

    def note(kind, e, k):
        if e > worst[kind][0]:
            worst[kind] = (e, k)
    note("full", helpers.rel_l2(grads["__input__"], z[f"{mode}_gin"]), "__input__")
    names, norms = z[f"{mode}_grad_names"], z[f"{mode}_grad_norms"]
    n_full = 0
    for k, n in zip(names, norms):
        k = str(k)
        if mode == "train" and k.endswith("bias") and k.startswith("cl.") and f"bn.{k.split('.')[1]}.weight" in sd:
            continue                               # conv bias before BN: true gradient is 0 (round-off only)
        note("norm", abs(float(grads[k].double().norm()) - n) / n, k)
        if f"{mode}_grad::{k}" in z:
            n_full += 1
            note("full", helpers.rel_l2(grads[k], z[f"{mode}_grad::{k}"]), k)
    print(f"{joint_set} {mode}: worst full tensor {worst['full']}, worst norm {worst['norm']}, bound {bound:.2e}, "
          f"{n_full} full tensors, flips (count, max |y64|) {flips}")
    assert n_full >= 20
    assert worst["full"][0] <= bound, worst
    assert worst["norm"][0] <= bound, worst
    if mode == "train":
        for k in sd2:
            if "running" in k:
                assert np.abs(sd2[k].numpy() - z[f"train_state::{k}"]).max() < 1e-5


def test_chebconv_oracle_vs_golden():
    z = helpers.golden("chebconv.npz")
    gL, _, _ = helpers.golden_graphs("mano")
    ci = 0
    while f"c{ci}_meta" in z:
        lvl, Fin, Fout, has_bn, B = [int(v) for v in z[f"c{ci}_meta"]]
        L = gL[lvl]
        rng = np.random.default_rng(100 + ci)
        x = torch.from_numpy(rng.standard_normal((B, L.shape[0], Fin)).astype(np.float32)).requires_grad_(True)
        W = torch.from_numpy(rng.uniform(-0.1, 0.1, (Fout, Fin * 3)).astype(np.float32)).requires_grad_(True)
        b = torch.from_numpy(rng.uniform(-0.1, 0.1, (Fout,)).astype(np.float32)).requires_grad_(True)
        bn = None
        if has_bn:
            bn = {"weight": torch.from_numpy(rng.uniform(0.5, 1.5, (Fout,)).astype(np.float32)).requires_grad_(True),
                  "bias": torch.from_numpy(rng.uniform(-0.2, 0.2, (Fout,)).astype(np.float32)).requires_grad_(True),
                  "running_mean": torch.zeros(Fout), "running_var": torch.ones(Fout)}
        y = mo.graph_conv_cheby(x, W, b, bn, mo.scipy_to_torch_coo(L), 3, True)
        w = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
        (y * w).sum().backward()
        assert np.abs(y.detach().numpy() - z[f"c{ci}_y"]).max() < 1e-5
        assert helpers.rel_l2(x.grad, z[f"c{ci}_dx"]) < 1e-5
        assert helpers.rel_l2(W.grad, z[f"c{ci}_dW"]) < 1e-5
        if has_bn:
            assert helpers.rel_l2(bn["weight"].grad, z[f"c{ci}_dgamma"]) < 1e-5
            assert np.abs(bn["running_var"].numpy() - z[f"c{ci}_rv"]).max() < 1e-6
        ci += 1
    assert ci == 5


@pytest.mark.parametrize("joint_set", ["mano", "coco"])
def test_flat_oracle_vs_golden(joint_set):
    z = helpers.golden(f"flat_{joint_set}.npz")
    gL, _, _ = helpers.golden_graphs(joint_set)
    B, J = int(z["B"]), int(z["J"])
    from pose2mesh_release_amd import pose2mesh_net
    shapes = pose2mesh_net.get_model(J, gL, mano=(joint_set == "mano")).state_dict()
    sd = helpers.numpy_state(shapes, 2)
    pose2d = synth.pose2d_batch(B, J, seed=11)
    with torch.no_grad():
        mesh, pose3d = mo.flat_forward(sd, helpers.oracle_graphs(gL), pose2d, joint_set == "mano", False)
    assert helpers.max_vertex_l2(mesh, z["cam_mesh"]) < 5e-6
    # pose3d (|max| 0.34 / 0.33): 3 x the measured float64-oracle-vs-fixture difference, 1.285e-7 (mano) and 1.394e-7 (coco)
    # absolute - the fixture's own fp32 rounding.  (The fp32 oracle is bitwise equal at 1 ... 64 threads.)
    sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
    with torch.no_grad():
        _, pose64 = mo.flat_forward(sd64, [g.double() for g in helpers.oracle_graphs(gL)], pose2d.double(),
                                    joint_set == "mano", False)
    d64, d32 = np.abs(pose64.numpy() - z["pose3d"]).max(), np.abs(pose3d.numpy() - z["pose3d"]).max()
    print(f"{joint_set}: pose3d vs fixture: float64 oracle {d64:.3e}, fp32 oracle {d32:.3e}")
    bound = 3 * {"mano": 1.285e-7, "coco": 1.394e-7}[joint_set]
    assert d64 <= bound and d32 <= bound, (d64, d32)


def test_feature_axis_interpolation_closed_forms():
    """64->256 lerp and 256->128 pair-mean are what F.interpolate(mode='linear') computes."""
    x = torch.randn(3, 7, 64)
    assert (mo.interp_feature_axis(x, 256) - torch.nn.functional.interpolate(x, size=256, mode="linear")).abs().max() < 1e-6
    x = torch.randn(3, 7, 256)
    pm = 0.5 * (x[..., 0::2] + x[..., 1::2])
    assert (pm - torch.nn.functional.interpolate(x, size=128, mode="linear")).abs().max() < 1e-6


def test_oracle_vs_live_reference_mano():
    """The oracle against the real reference's MANO Pose2Mesh in eval(): against that model's output stored in
    tests/golden/live_mano.npz (make_golden.py), and against the live reference itself where its tree is present."""
    z = helpers.golden("live_mano.npz")
    gL, _, _ = helpers.golden_graphs("mano")
    J = synth.JOINT_SETS["mano"][0]
    sd = helpers.numpy_state(mo.init_state(J, mo.trim_graph_list(gL), True), 9)
    x = helpers.meshnet_input(3, J, seed=1)
    out, _, _ = helpers.oracle_run(sd, helpers.oracle_graphs(gL), x, True, False)
    assert helpers.max_vertex_l2(out, z["eval_out"]) < 2e-6
    if not ref_loader.available():
        return
    ns = ref_loader.load("mano")
    J, skel, flip, levels = synth.JOINT_SETS["mano"]
    _, faces = synth.hull_mesh(778, 0)
    _, gL, _, _ = ref_loader.build_coarse_graphs(faces, J, skel, flip, levels)
    net = ns.meshnet.get_model(5, 3, [L.copy() for L in gL])
    sd = helpers.numpy_state(net.state_dict(), 9)
    net.load_state_dict(sd)
    net.eval()
    x = helpers.meshnet_input(3, J, seed=1)
    with torch.no_grad(), ref_loader.cpu_cuda_shim():
        ref = net(x.clone())
    out, _, _ = helpers.oracle_run(sd, helpers.oracle_graphs(gL), x, True, False)
    assert helpers.max_vertex_l2(out, ref) < 2e-6
    ref_loader.load("human36")


# ---------------------------------------------------------------------------------------------
# loss / epilogue oracle and demo-preprocessing oracle vs goldens made by the REAL reference
# ---------------------------------------------------------------------------------------------
import demo_oracle as do
import loss_oracle as lo


@pytest.mark.parametrize("joint_set", ["mano", "coco", "human36"])
@pytest.mark.parametrize("with_edge", [True, False])
def test_loss_oracle_vs_reference_golden(joint_set, with_edge):
    """oracle/loss_oracle.py against lib/core/loss.py driven as lib/core/base.py:130-143 does (values + gradients);
    human36 with the reference's own J_regressor_h36m_correct.npy (embedded in the fixture)."""
    z = helpers.golden(f"loss_{joint_set}.npz")
    c = helpers.loss_case(joint_set, jreg=helpers.golden_regressor() if joint_set == "human36" else None)
    tag = "edge" if with_edge else "noedge"
    cam = c["cam_mesh"].clone().requires_grad_(True)
    lift = c["lift_pose"].clone().requires_grad_(True)
    total, parts = lo.train_losses(cam, lift, c["perm_reverse"], c["nv"], c["faces"], c["J_regressor"], c["gt_mesh"],
                                   c["gt_reg3dpose"], c["gt_lift3dpose"], c["val_mesh"], c["val_reg3dpose"],
                                   c["val_lift3dpose"], with_edge=with_edge)
    total.backward()
    for a, b in zip(parts, z[f"{tag}_losses"]):
        assert abs(float(a) - b) <= 1e-6 * max(1.0, abs(b))
    assert abs(float(total) - float(z[f"{tag}_total"])) <= 1e-6 * max(1.0, abs(float(z[f"{tag}_total"])))
    assert helpers.rel_l2(cam.grad, z[f"{tag}_grad_cam"]) < 1e-6
    assert helpers.rel_l2(lift.grad, z[f"{tag}_grad_lift"]) < 1e-6
    fake = np.setdiff1d(np.arange(c["V0"]), c["perm_reverse"][:c["nv"]])
    assert float(cam.grad[:, fake].abs().max()) == 0.0


def test_demo_preprocessing_oracle_vs_reference_golden():
    """configs[0]: demo/h36m_joint_input.npy through the numpy restatement == the real get_bbox / process_bbox /
    j2d_processing (SURVEY A7 lists the expected first rows)."""
    z = helpers.golden("demo_h36m.npz")
    x, bbox, bbox2 = do.demo_model_input(z["joint_input"].copy())
    assert z["joint_input"].dtype == np.int64 and z["joint_input"].shape == (17, 2)
    assert np.array_equal(bbox, z["bbox"]) and np.allclose(bbox2, z["bbox2"], rtol=0, atol=1e-12)
    assert np.abs(x - z["model_input"][0]).max() < 1e-6
    assert np.allclose(x[:4], [[0.1489, 0.2843], [-0.3839, 0.2843], [-1.9158, 0.8613], [-2.1156, 1.9963]], atol=1e-4)
    # the model + epilogue part of the fixture: oracle forward on the golden input
    gL, _, rev = helpers.golden_graphs("human36")
    from pose2mesh_release_amd import pose2mesh_net
    sd = helpers.numpy_state(pose2mesh_net.get_model(17, gL, mano=False).state_dict(), 2)
    with torch.no_grad():
        cam_mesh, pose3d = mo.flat_forward(sd, helpers.oracle_graphs(gL), torch.from_numpy(x[None]), False, False)
    assert helpers.max_vertex_l2(cam_mesh, z["cam_mesh"]) < 5e-6
    mesh, joints = do.demo_mesh_epilogue(cam_mesh.numpy(), rev, 6890, helpers.golden_regressor("demo_h36m.npz"))
    assert mesh.shape == (1, 6890, 3) and np.abs(mesh - z["mesh"]).max() < 5e-6
    assert np.abs(joints - z["joints"]).max() < 5e-6


@pytest.mark.parametrize("joint_set", ["mano", "human36", "coco"])
def test_state_dict_inventory_matches_real_reference(joint_set):
    """Keys, shapes and dtypes of FlatPose2Mesh.state_dict() == the REAL reference module's;
    a state dict with exactly the reference's key set loads with strict=True."""
    from pose2mesh_release_amd import pose2mesh_net
    z = helpers.golden(f"state_{joint_set}.npz")
    gL, _, _ = helpers.golden_graphs(joint_set)
    net = pose2mesh_net.get_model(int(gL[-1].shape[0]), gL, mano=(joint_set == "mano"))
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in z["keys"]]
    for (k, v), shp, dt in zip(sd.items(), z["shapes"], z["dtypes"]):
        assert ",".join(str(d) for d in v.shape) == str(shp), k
        assert str(v.dtype) == str(dt), k
    assert sum(p.numel() for p in net.parameters()) == int(z["num_params"])
    # a checkpoint-shaped dict with the reference's keys (module. prefix stripped as check_data_pararell does)
    ref_sd = {}
    for i, k in enumerate(z["keys"]):
        k = str(k)
        shp = tuple(int(d) for d in str(z["shapes"][i]).split(",") if d != "")
        ref_sd[k] = torch.from_numpy(z[f"t{i}"]) if f"t{i}" in z else torch.zeros(shp, dtype=sd[k].dtype)
    missing = net.load_state_dict(ref_sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    i = [str(k) for k in z["keys"]].index("pose2mesh.cl.0.weight")
    assert np.array_equal(net.state_dict()["pose2mesh.cl.0.weight"].numpy(), z[f"t{i}"])
    # same init distribution as the reference (meshnet.py:46-50): uniform with the same bound, zero bias
    ours = pose2mesh_net.get_model(int(gL[-1].shape[0]), gL, mano=(joint_set == "mano")).state_dict()
    for name in ("pose2mesh.cl.3.weight", "pose2mesh.fc.weight"):
        j = [str(k) for k in z["keys"]].index(name)
        n = ours[name].numel()
        ref_absmean = float(z[f"c{j}"][1]) / n if f"c{j}" in z else float(np.abs(z[f"t{j}"]).mean())
        assert abs(float(ours[name].abs().mean()) - ref_absmean) < 0.05 * ref_absmean, name


def test_kink_accounting_counts_a_planted_flip():
    """tests/kinks.py (the ReLU-kink accounting of the GPU gradient-parity tests): with the oracle's own masks nothing is
    flipped and the gradient is the plain float64 gradient; with one mask bit flipped at the element closest to the
    kink the flip is counted, located, and the gradient changes far above round-off."""
    import kinks
    gL, _, _ = helpers.golden_graphs("mano")
    J = int(gL[-1].shape[0])
    glt = helpers.oracle_graphs(gL)
    sd = helpers.numpy_state(mo.init_state(J, mo.trim_graph_list(gL), True), 21)
    x = helpers.meshnet_input(2, J, seed=99)
    w = torch.randn(2, gL[0].shape[0], 3, generator=torch.Generator().manual_seed(5))
    out, g0, st0 = kinks.masked_oracle_gradients(sd, glt, x, True, w, None)
    assert st0["n_flips"] == 0 and st0["n_relu_elements"] > 500000
    ref, gref, _ = helpers.oracle_run(sd, glt, x, True, True, grad_seed=5)       # plain fp32 oracle
    assert helpers.max_vertex_l2(out, ref) < 2e-5
    # harvest the oracle's own masks, flip the element closest to zero in layer 6
    masks, pre = [], []

    class Rec(kinks._FProxy):
        def relu(self, t, inplace=False):
            pre.append(t.detach().clone())
            masks.append(t.detach() > 0)
            return super().relu(t)
    old = mo.F
    mo.F = Rec(None, {"n_relu_elements": 0, "n_flips": 0, "max_abs_preact_at_flip": 0.0, "flips_per_layer": {}})
    try:
        with torch.no_grad():
            mo.meshnet_forward({k: v.double() if v.dtype.is_floating_point else v.clone() for k, v in sd.items()},
                               [g.double() for g in glt], x.double(), True, True)
    finally:
        mo.F = old
    i = int(pre[6].abs().reshape(-1).argmin())
    masks[6].view(-1)[i] ^= True
    _, g1, st1 = kinks.masked_oracle_gradients(sd, glt, x, True, w, masks)
    assert st1["n_flips"] == 1 and st1["flips_per_layer"] == {6: 1}
    assert st1["max_abs_preact_at_flip"] == float(pre[6].abs().reshape(-1)[i])
    assert helpers.rel_l2(g1["bn.6.bias"], g0["bn.6.bias"]) > 1e-5
    # downstream of the flip only the forward value moved, by |y| ~ 1e-7: gradients there are untouched
    assert helpers.rel_l2(g1["cl.9.weight"], g0["cl.9.weight"]) < 1e-6


def test_kink_accounting_between_two_mask_sets_and_planted_faults():
    """tests/kinks.py, the comparison of two fp32 results that used DIFFERENT masks (kernels vs the reference's fixture, one
    kernel set vs another), mano B=2: one planted flip at the near-zero element of layer 6 is reported as 1 bit, D is what
    that bit does to the gradients ((g1 - g0) - D at float64 round-off, g0 / g1 from runs of their own), and two stand-in
    fp32 results pass the accounted compare at ALIGNED_GRAD_TOL although they differ by far more; a planted VALUE fault
    (32 consecutive elements of one tensor x 1.001) fails it, and a planted MASK fault at an element with |y| of order 1
    fails on the kink window."""
    import kinks
    gL, _, _ = helpers.golden_graphs("mano")
    J = int(gL[-1].shape[0])
    glt = helpers.oracle_graphs(gL)
    sd = helpers.numpy_state(mo.init_state(J, mo.trim_graph_list(gL), True), 21)
    x = helpers.meshnet_input(2, J, seed=99)
    w = torch.randn(2, gL[0].shape[0], 3, generator=torch.Generator().manual_seed(5))
    own = kinks.oracle_own_masks(sd, glt, x, True, True)
    pre = []

    class Rec(kinks._FProxy):
        def relu(self, t, inplace=False):
            pre.append(t.detach().clone())
            return super().relu(t)
    old = mo.F
    mo.F = Rec(None, kinks.new_stats())
    try:
        with torch.no_grad():
            mo.meshnet_forward({k: v.double() if v.dtype.is_floating_point else v.clone() for k, v in sd.items()},
                               [g.double() for g in glt], x.double(), True, True)
    finally:
        mo.F = old
    assert all(torch.equal(m, p > 0) for m, p in zip(own, pre))
    i = int(pre[6].abs().reshape(-1).argmin())
    y_i = float(pre[6].abs().reshape(-1)[i])
    assert y_i <= kinks.KINK_WINDOW
    # the planted flip, written as a fixture would record it
    flipped = kinks.masks_from_record(own, np.array([6], np.int16), np.array([i], np.int64),
                                      np.array([not bool(own[6].reshape(-1)[i])]))
    assert kinks.count_mask_bits(flipped, own) == 1
    # identical sets: one oracle run, D = 0
    same = kinks.accounted_difference(sd, glt, x, True, w, own, [m.clone() for m in own], True)
    assert same.n_bits == 0 and same.max_abs_y == 0.0 and all(float(d.abs().max()) == 0.0 for d in same.D.values())
    acc = kinks.accounted_difference(sd, glt, x, True, w, flipped, own, True)
    assert acc.n_bits == 1 and acc.max_abs_y == y_i and (acc.flips_a, acc.flips_b) == (1, 0)
    _, g0, _ = kinks.masked_oracle_gradients(sd, glt, x, True, w, own)
    _, g1, _ = kinks.masked_oracle_gradients(sd, glt, x, True, w, flipped)
    assert set(acc.D) == set(g0) and "__input__" in acc.D
    for k in g0:
        assert float(((g1[k] - g0[k]) - acc.D[k]).norm()) <= 1e-12 * float(g0[k].norm()), k
    assert helpers.rel_l2(g1["bn.6.bias"], g0["bn.6.bias"]) > 1e-5          # what a plain tolerance would have to swallow
    # two stand-in fp32 results, one per mask set
    A = {k: v.float() for k, v in g1.items()}
    B = {k: v.float() for k, v in g0.items()}
    res = kinks.assert_accounted(A, B, acc, kinks.ALIGNED_GRAD_TOL, what="stand-in")
    assert res["n_bits"] == 1 and res["worst"] <= 2e-7, res               # two fp32 roundings
    norms = {k: float(v.double().norm()) for k, v in B.items()}
    res = kinks.assert_accounted(A, {"__input__": B["__input__"]}, acc, kinks.ALIGNED_GRAD_TOL, norms=norms, what="norms")
    assert len(res["per"]) == len(B) and res["worst"] <= 2e-7, res
    # a value fault: 32 consecutive elements of one gradient tensor off by one part in a thousand
    bad = dict(A)
    bad["bn.6.bias"] = A["bn.6.bias"].clone()
    bad["bn.6.bias"][:32] *= 1.001
    with pytest.raises(AssertionError, match="bn.6.bias"):
        kinks.assert_accounted(bad, B, acc, kinks.ALIGNED_GRAD_TOL, what="value fault")
    with pytest.raises(AssertionError, match="bn.6.bias"):
        kinks.assert_accounted(bad, {"__input__": B["__input__"]}, acc, kinks.ALIGNED_GRAD_TOL, norms=norms, what="value fault")
    # a mask fault: a differing bit at an element of order 1 is no kink, whatever the gradients say
    j = int(pre[6].abs().reshape(-1).argmax())
    assert float(pre[6].abs().reshape(-1)[j]) > 1.0
    wrong = kinks.masks_from_record(own, [6], [j], [not bool(own[6].reshape(-1)[j])])
    accw = kinks.accounted_difference(sd, glt, x, True, w, wrong, own, True)
    assert accw.n_bits == 1 and accw.max_abs_y == float(pre[6].abs().reshape(-1)[j])
    Aw = {k: v.float() for k, v in accw.G_a.items()}
    with pytest.raises(AssertionError, match="mask fault"):
        kinks.assert_accounted(Aw, B, accw, kinks.ALIGNED_GRAD_TOL, what="mask fault")


def test_whole_model_masked_oracle_call_order_and_plain_gradients():
    """tests/kinks.py flat_masked_oracle_gradients (the float64 side of the train-step gradient check, mano B=4): with no
    masks forced it is plain float64 autograd of flat_forward + train_losses; the lifter's four ReLU calls come first and
    MeshNet's follow (counted); handing it its own masks in that order changes nothing, and a mask list in another order is
    refused."""
    import kinks
    c = helpers.loss_case("mano")
    gL, _, _ = helpers.golden_graphs("mano")
    from pose2mesh_release_amd import pose2mesh_net
    sd = helpers.numpy_state(pose2mesh_net.get_model(c["J"], gL, mano=True).state_dict(), 2)
    glt = helpers.oracle_graphs(gL)
    pose2d = synth.pose2d_batch(c["B"], c["J"], seed=11)
    largs = (c["perm_reverse"], c["nv"], c["faces"], c["J_regressor"], c["gt_mesh"], c["gt_reg3dpose"], c["gt_lift3dpose"],
             c["val_mesh"], c["val_reg3dpose"], c["val_lift3dpose"])
    loss, g, st = kinks.flat_masked_oracle_gradients(sd, glt, pose2d, True, None, largs)
    n = len(st["call_dims"])
    assert st["call_dims"] == [2] * 4 + [3] * (n - 4) and n == 4 + 14 and st["n_flips"] == 0
    # plain float64 autograd, no proxy
    sd64 = {k: (v.double().clone().requires_grad_(v.dtype.is_floating_point and "running" not in k)
                if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
    mesh, lift = mo.flat_forward(sd64, [t.double() for t in glt], pose2d.double(), True, True)
    ref, _ = lo.train_losses(mesh, lift, largs[0], largs[1], largs[2], largs[3].double(), *[t.double() for t in largs[4:]])
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-12 * abs(float(ref))
    none = [k for k, v in g.items() if v is None]
    assert none and all(k.startswith("pose_lifter.batch_norm1.") for k in none)
    for k, v in g.items():
        if v is not None:
            assert float((v - sd64[k].grad).norm()) <= 1e-12 * float(v.norm()) + 1e-300, k
    # its own masks, in call order
    own = []
    old = mo.F
    mo.F = kinks._FProxy(None, kinks.new_stats(), keep_own=own)
    try:
        with torch.no_grad():
            mo.flat_forward({k: v.double() if v.dtype.is_floating_point else v.clone() for k, v in sd.items()},
                            [t.double() for t in glt], pose2d.double(), True, True)
    finally:
        mo.F = old
    assert [m.dim() for m in own] == st["call_dims"]
    loss2, g2, st2 = kinks.flat_masked_oracle_gradients(sd, glt, pose2d, True, own, largs)
    assert st2["n_flips"] == 0 and float(loss2) == float(loss)
    with pytest.raises(AssertionError):
        kinks.flat_masked_oracle_gradients(sd, glt, pose2d, True, own[4:] + own[:4], largs)


def test_posenet_pretrained_contract(tmp_path, monkeypatch, capsys):
    """lib/models/pose2mesh_net.py:13 + lib/models/posenet.py:74-75,89-92: FlatPose2Mesh reads cfg.MODEL.posenet_pretrained at
    construction and, when set (every training yaml sets it), loads checkpoint['model_state_dict'] of cfg.MODEL.posenet_path
    into the lifter through funcs_utils.load_checkpoint; a missing file raises ValueError("No checkpoint exists!") as
    lib/funcs_utils.py:122-128 does.  Outside the reference's scripts (no core.config) the default stays random init, and
    the same is reachable through explicit keyword arguments."""
    import sys
    import types
    from pose2mesh_release_amd import pose2mesh_net, posenet
    gL, _, _ = helpers.golden_graphs("mano")
    J = int(gL[-1].shape[0])
    torch.manual_seed(5)
    donor = posenet.get_model(J, 4096, 2, 0.5)
    sd = {k: (v + 0.25 if v.dtype.is_floating_point else v + 3) for k, v in donor.state_dict().items()}
    ckpt = tmp_path / "final.pth.tar"
    torch.save({"model_state_dict": sd, "epoch": 7}, str(ckpt))

    def cfg_modules(pretrained, path):
        cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(posenet_pretrained=pretrained, posenet_path=str(path)),
                                    DATASET=types.SimpleNamespace(target_joint_set="mano"))
        core, cc = types.ModuleType("core"), types.ModuleType("core.config")
        cc.cfg = cfg
        core.config = cc
        return core, cc

    def same(net):
        got = net.pose_lifter.state_dict()
        return all(torch.equal(got[k], v) for k, v in sd.items())
    # 1. no reference config loaded: random init (config.py:56 default False)
    for k in ("core", "core.config", "funcs_utils"):
        monkeypatch.delitem(sys.modules, k, raising=False)
    assert not same(pose2mesh_net.get_model(J, gL, mano=True))
    # 2. inside the reference's scripts: cfg.MODEL.posenet_pretrained = True -> the checkpoint is loaded
    core, cc = cfg_modules(True, ckpt)
    monkeypatch.setitem(sys.modules, "core", core)
    monkeypatch.setitem(sys.modules, "core.config", cc)
    net = pose2mesh_net.get_model(J, gL)
    assert same(net) and net.pose2mesh.mano
    out = capsys.readouterr().out
    assert "Loading pretrained posenet..." in out and "Fetch model weight from" in out
    # ... through the reference's own loader when funcs_utils is imported (lib/models/posenet.py:3)
    calls = []
    fu = types.ModuleType("funcs_utils")

    def load_checkpoint(load_dir, epoch=0, pick_best=False):
        calls.append((load_dir, pick_best))
        return torch.load(load_dir, map_location="cpu")
    fu.load_checkpoint = load_checkpoint
    monkeypatch.setitem(sys.modules, "funcs_utils", fu)
    assert same(pose2mesh_net.get_model(J, gL)) and calls == [(str(ckpt), True)]
    monkeypatch.delitem(sys.modules, "funcs_utils")
    # 3. cfg says False -> untouched; a missing file -> the reference's error
    cc.cfg.MODEL.posenet_pretrained = False
    assert not same(pose2mesh_net.get_model(J, gL))
    cc.cfg.MODEL.posenet_pretrained = True
    cc.cfg.MODEL.posenet_path = str(tmp_path / "nope.pth.tar")
    with pytest.raises(ValueError, match="No checkpoint exists!"):
        pose2mesh_net.get_model(J, gL)
    # 4. explicit arguments, no config
    monkeypatch.delitem(sys.modules, "core")
    monkeypatch.delitem(sys.modules, "core.config")
    assert same(pose2mesh_net.get_model(J, gL, mano=True, posenet_pretrained=True, posenet_path=str(ckpt)))
    with pytest.raises(ValueError, match="posenet_path"):
        pose2mesh_net.get_model(J, gL, mano=True, posenet_pretrained=True)
