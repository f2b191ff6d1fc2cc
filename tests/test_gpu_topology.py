"""-m gpu: topology generality at NETWORK level (VERDICT r2 "next round" 5).  The real SMPL / MANO faces are not
available, so what protects a user who has them is correctness as a function of (V, nnz, degree): train-mode forward +
backward against the float64 oracle, ReLU kinks accounted for (tests/kinks.py), on meshes that are NOT the two hull meshes
every other test uses:
  * hull(6890, seed 3)   same sizes as the bench mesh, different connectivity / coarsening tree;
  * hull(7000)           padded level sizes of another shape (not 11776 ... 92);
  * a UV sphere          two poles of degree 72: their merged rows (pole + ring + second ring) exceed the tile caps, so
                         the levels they sit on get NO tile plan (p2m_graph_plan_info == 0), no paired operator, and the
                         class plan is refused (Pose2Mesh._class_plan -> None): the row kernels and the fine-resolution
                         backward run INSIDE the network;
  * a UV sphere          whose poles just FIT the caps (degree 59: merged row 2 * 59 + 1 = 119 <= 120 union rows): the finest
                         level keeps all three tile plans, with rows of 119 / 120 entries beside rows of ~19 - the tile
                         kernels run inside the network on the longest rows a plan can hold (tests/tile_plan_ref.py).
Graphs are built by the package's own build_coarse_graphs (C++ HEM), which tests/test_graph_prep.py pins to the
reference's lib/graph_utils.py:75-95 / lib/coarsening.py:214-258."""
import numpy as np
import pytest
import torch

import helpers
import kinks
import meshnet_oracle as mo
from pose2mesh_release_amd import graph_utils, synth

pytestmark = pytest.mark.gpu


def _uv_sphere_faces(nlat, nlon):
    """Closed triangle mesh: 2 poles + nlat rings of nlon vertices; pole degree = nlon."""
    f = []
    ring = lambda i, j: 2 + i * nlon + (j % nlon)           # noqa: E731
    for j in range(nlon):
        f.append((0, ring(0, j), ring(0, j + 1)))
        f.append((1, ring(nlat - 1, j + 1), ring(nlat - 1, j)))
    for i in range(nlat - 1):
        for j in range(nlon):
            f.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    return np.asarray(f, dtype=np.int64)


def _graphs(kind):
    J, skel, flip, levels = synth.JOINT_SETS["human36"]
    if kind == "hull6890_seed3":
        _, faces = synth.hull_mesh(6890, 3)
    elif kind == "hull7000":
        _, faces = synth.hull_mesh(7000, 0)
    elif kind == "uv_sphere_poles_fit":
        faces = _uv_sphere_faces(60, 59)                   # 3542 vertices, poles of degree 59
    else:
        faces = _uv_sphere_faces(60, 72)                   # 4322 vertices, poles of degree 72
    _, gL, _, _ = graph_utils.build_coarse_graphs(faces, J, skel, flip, levels=levels)
    return gL, J


def _run(kind, B, expect):
    from pose2mesh_release_amd import meshnet
    gL, J = _graphs(kind)
    net = meshnet.get_model(5, 3, gL, mano=False)
    sd = helpers.numpy_state(net.state_dict(), 5)
    net.load_state_dict(sd)
    net = net.cuda().train()
    net._tap = []
    x = helpers.meshnet_input(B, J, seed=12)
    xg = x.cuda().requires_grad_(True)
    y = net(xg)
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(4))
    (y * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    graphs = net._graph_cache.on(xg.device)
    info = {"levels": [g.V for g in graphs], "split": [g.split for g in graphs],
            "plans": [g.plan_tiles for g in graphs], "classes": [g.classes for g in graphs]}
    expect(info)
    masks = kinks.hip_masks(net._tap)
    net._tap = None
    torch.set_num_threads(16)
    sd_o = helpers.numpy_state(mo.init_state(J, mo.trim_graph_list(gL), False), 5)
    out64, g64, st = kinks.masked_oracle_gradients(sd_o, helpers.oracle_graphs(gL), x, False, w, masks)
    err = helpers.max_vertex_l2(y.detach().cpu(), out64)
    assert err <= 1e-4, (kind, err)
    assert st["max_abs_preact_at_flip"] <= 1e-4 and st["n_flips"] <= max(20, 4e-6 * st["n_relu_elements"]), st
    grads = {k: p.grad for k, p in net.named_parameters()}
    grads["__input__"] = xg.grad
    names = set(g64)
    for k, r in g64.items():
        if k.startswith("cl.") and k.endswith("bias") and f"bn.{k.split('.')[1]}.weight" in names:
            continue                                        # exactly-zero gradient in front of a train-mode BatchNorm
        e = helpers.rel_l2(grads[k].cpu(), r)
        assert e <= 5e-5, (kind, k, e)
    return info


def test_other_coarsening_tree_same_sizes(hip_libs):
    def expect(info):
        assert info["levels"][0] == 11776 or info["levels"][0] % 2 == 0
        assert any(info["split"]) and any(info["classes"])          # the default shortcuts are all active
    _run("hull6890_seed3", 2, expect)


def test_other_padded_sizes(hip_libs):
    ref = [g.shape[0] for g in helpers.golden_graphs("human36")[0]]

    def expect(info):
        assert info["levels"][0] != ref[0]                           # not the 11776 ... 92 shape
        assert any(info["split"]) and any(info["classes"])
    _run("hull7000", 2, expect)


def test_high_degree_vertices_take_the_no_plan_paths_inside_the_network(hip_libs):
    def expect(info):
        split_lv = [i for i, s in enumerate(info["split"]) if s]
        assert split_lv, info
        # the finest level carries the poles: their merged rows (145 entries) exceed the tile caps, so that level has no
        # tile plan for its own resolution and no paired operator -> row kernels, fine-resolution backward, no classes
        assert any(info["plans"][i][0] == 0 and info["plans"][i][2] == 0 for i in split_lv), str(info["plans"])
        assert not any(info["classes"]), str(info["classes"])
    _run("uv_sphere", 3, expect)


def test_high_degree_vertices_that_fit_the_caps_take_the_tile_kernels(hip_libs):
    import tile_plan_ref as tp
    gL, _ = _graphs("uv_sphere_poles_fit")
    want = tp.Plans(gL[0])                                  # the planner restated on the CPU: what the level should get
    assert all(t > 0 for t in want.plan_tiles) and min(int(r.max()) for r in want.row_len) >= 100, want.describe()

    def expect(info):
        assert info["split"][0], info
        # the finest level carries the poles (merged rows of 119 entries, 120 in the paired operator) and keeps every plan
        assert info["plans"][0] == want.plan_tiles and all(t > 0 for t in info["plans"][0]), str(info["plans"])
    _run("uv_sphere_poles_fit", 3, expect)
