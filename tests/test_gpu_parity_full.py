"""-m gpu: parity at the quantities and sizes that matter ("next round" 1):
  (a) FULL-tensor gradients of every parameter and of the input against the CPU oracle on fresh inputs;
  (b) the bench's own scale against the oracle where the oracle still finishes in seconds
      (MANO B=256 train, SMPL-like B=32 train);
  (c) BASELINE configs[2] itself (SMPL-like coco graph, B=256, train): the default kernel set against an INDEPENDENT
      kernel set (native f32 MFMA, no fake-vertex split, row-per-wave basis kernel, 4-wave GEMM) in a child process,
      plus eval slices of the same batch against the oracle;
  (c') the train-mode FORWARD of configs[2] (B=256) and configs[4] (MANO B=512) against the fp32 AND the float64 oracle under
      no_grad (full-batch BatchNorm statistics) -- BASELINE's "vertex L2 vs ref at batch 256", oracle-anchored;
  (d) three optimizer steps of the bench's TrainStep against oracle + torch.optim.Adam;
  (e) train-mode bitwise repeatability.
All through the C ABI.  The BASELINE-size oracle tests (c', c'') run in BOTH slice arithmetics (round 6): bf16x3 - the exact fp32
emulation bench.py quotes, whose policy picks other tile-kernel instantiations at B = 256 than at the small sizes - and f16x2,
the import-time default of the package that every other test here runs on.  Achieved maxima are written to
gpurun_out/parity_maxima.json (DESIGN.md section 5 quotes them)."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers
import kinks
import meshnet_oracle as mo

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VERTEX_TOL = 1e-4
ORACLE_THREADS = 16          # torch's CPU sparse path collapses when a 256-thread host is used fully


def _record(key, value, name=None):
    path = os.path.join(ROOT, "gpurun_out", "parity_maxima.json")
    if name is not None:         # another test file's figures (test_gpu_stream_order.py): same directory, its own file
        path = os.path.join(os.path.dirname(path), name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    try:
        d = json.load(open(path))
    except Exception:
        d = {}
    d[key] = value
    json.dump(d, open(path, "w"), indent=1, sort_keys=True)


@contextlib.contextmanager
def _arith(name):
    """Run a block in another contraction arithmetic (what `P2M_GEMM_ARITH=...` selects at import; bench.py --arith)."""
    from pose2mesh_release_amd import ops
    old = ops.GEMM_ARITH
    ops.GEMM_ARITH = name
    ops.bump_weight_epoch()
    try:
        yield
    finally:
        ops.GEMM_ARITH = old
        ops.bump_weight_epoch()


def _atag(arith):
    return "" if arith == "f16x2" else f"_{arith}"          # (the f16x2 keys keep their round-5 names)


def _zero_grad_bias(k, names):
    """conv bias in front of a train-mode BatchNorm: the true gradient is exactly 0 (round-off only)."""
    return k.startswith("cl.") and k.endswith("bias") and f"bn.{k.split('.')[1]}.weight" in names


def _compare_grads(hip, ref, tol, tag, train):
    """hip/ref: dict name -> tensor/array.  Per-tensor rel-L2; returns the maxima."""
    names = set(ref.keys())
    worst, worst_k = 0.0, None
    per = {}
    for k, r in ref.items():
        h = hip[k]
        h = torch.as_tensor(h).detach().cpu()
        r = torch.as_tensor(r).detach().cpu()
        if train and _zero_grad_bias(k, names):
            wk = k.replace("bias", "weight")
            assert float(h.norm()) <= 1e-3 * max(1.0, float(torch.as_tensor(hip[wk]).norm())), k
            continue
        e = helpers.rel_l2(h, r)
        per[k] = e
        if e > worst:
            worst, worst_k = e, k
    _record(tag, {"max_rel_l2": worst, "at": worst_k})
    bad = {k: v for k, v in per.items() if v > tol}
    assert not bad, f"{tag}: gradient rel-L2 above {tol:g}: {bad}"
    return worst


def _hip_run(joint_set, B, mode, wseed, xseed, gseed, tap=False):
    sys.path.insert(0, HERE)
    import _child_meshnet_run as child
    return child.run(joint_set, B, mode, wseed, xseed, gseed, keep_on_gpu=True, tap=tap)


def _oracle_inputs(joint_set, B, wseed, xseed, gseed):
    torch.set_num_threads(ORACLE_THREADS)
    gL, _, _ = helpers.golden_graphs(joint_set)
    J = int(gL[-1].shape[0])
    mano = joint_set == "mano"
    sd = helpers.numpy_state(mo.init_state(J, mo.trim_graph_list(gL), mano), wseed)
    x = helpers.meshnet_input(B, J, seed=xseed)
    w = torch.randn(B, gL[0].shape[0], 3, generator=torch.Generator().manual_seed(gseed))
    return sd, helpers.oracle_graphs(gL), x, mano, w


def _oracle(joint_set, B, mode, wseed, xseed, gseed):
    sd, glt, x, mano, _ = _oracle_inputs(joint_set, B, wseed, xseed, gseed)
    return helpers.oracle_run(sd, glt, x, mano, mode == "train", grad_seed=gseed)


# the gradient bound with the ReLU masks aligned, and the window a flipped element must lie in: tests/kinks.py
ALIGNED_GRAD_TOL = kinks.ALIGNED_GRAD_TOL
KINK_WINDOW = kinks.KINK_WINDOW


def _accounted_record(tag, acc, res, tol):
    _record(tag, {"mask_bits_differing": acc.n_bits, "max_abs_y64_at_a_differing_bit": acc.max_abs_y,
                  "worst_accounted_residual": res["worst"], "at": res["at"], "bound": tol})


def _kink_resolved_check(tag, joint_set, B, wseed, xseed, gseed, dtype=torch.float64):
    """HIP forward + backward (default kernels) against the float64 oracle run with the masks the kernels used."""
    hip = _hip_run(joint_set, B, "train", wseed, xseed, gseed, tap=True)
    masks = [hip[k].cpu() for k in sorted((k for k in hip if k.startswith("mask::")), key=lambda k: int(k[6:]))]
    sd, glt, x, mano, w = _oracle_inputs(joint_set, B, wseed, xseed, gseed)
    out64, g64, st = kinks.masked_oracle_gradients(sd, glt, x, mano, w, masks, dtype=dtype)
    err = helpers.max_vertex_l2(hip["out"].cpu(), out64)
    _record(f"{tag}_vertex_l2", err)
    assert err <= VERTEX_TOL
    _record(f"{tag}_kinks", {"relu_elements": st["n_relu_elements"], "flipped": st["n_flips"],
                             "max_abs_preact_at_flip": st["max_abs_preact_at_flip"],
                             "flips_per_relu_layer": {str(k): v for k, v in st["flips_per_layer"].items()}})
    # every mask difference is a genuine kink element, and there are only a handful of them
    assert st["max_abs_preact_at_flip"] <= KINK_WINDOW, st
    assert st["n_flips"] <= max(20, 4e-6 * st["n_relu_elements"]), st
    _compare_grads({k[6:]: v for k, v in hip.items() if k.startswith("grad::")}, g64, ALIGNED_GRAD_TOL,
                   f"{tag}_grads_masks_aligned", True)
    return hip, st


INDEPENDENT_SET = dict(P2M_GEMM_ARITH="f32", P2M_SPLIT_FAKE="0", P2M_BASIS_TILED="0")


def _child_run(tmp_path, env, joint_set, B, mode, wseed, xseed, gseed):
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_meshnet_run.py"), out, joint_set, str(B), mode,
                        str(wseed), str(xseed), str(gseed)], env=dict(os.environ, P2M_TEST_TAP="1", **env),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(out)


def _kink_resolved_check_child(tag, tmp_path, env, joint_set, B, wseed, xseed, gseed):
    """The same float64 comparison for a NON-DEFAULT kernel set: the network runs in a child process under `env`, its
    ReLU masks come back bit-packed, the float64 oracle runs with those masks."""
    res = _child_run(tmp_path, env, joint_set, B, "train", wseed, xseed, gseed)
    keys = sorted((k for k in res.files if k.startswith("mask::")), key=lambda k: int(k[6:]))
    masks = [torch.from_numpy(np.unpackbits(res[k]).astype(bool)) for k in keys]
    sd, glt, x, mano, w = _oracle_inputs(joint_set, B, wseed, xseed, gseed)
    out64, g64, st = kinks.masked_oracle_gradients(sd, glt, x, mano, w, masks)
    err = helpers.max_vertex_l2(res["out"], out64)
    _record(f"{tag}_vertex_l2", err)
    assert err <= VERTEX_TOL
    assert st["max_abs_preact_at_flip"] <= KINK_WINDOW, st
    assert st["n_flips"] <= max(20, 4e-6 * st["n_relu_elements"]), st
    _compare_grads({k[6:]: res[k] for k in res.files if k.startswith("grad::")}, g64, ALIGNED_GRAD_TOL,
                   f"{tag}_grads_masks_aligned", True)


def test_independent_kernel_set_vs_oracle_train(hip_libs, tmp_path):
    """The INDEPENDENT kernel set of test (c) -- native f32 MFMA, unsplit rows (every fake row computed, backward at the
    fine resolution), row-per-wave basis kernel, 4-wave contractions -- pinned to the float64 oracle at NETWORK level
    (human36, B=3, train, every gradient tensor, kinks accounted for), so that the B=256 / B=512 default-vs-independent
    comparisons stand on a leg that is itself tied to the reference arithmetic."""
    _kink_resolved_check_child("a_independent_human36_B3", tmp_path, INDEPENDENT_SET, "human36", 3, 21, 99, 5)


def test_basis_inside_the_contraction_network_vs_oracle_train(hip_libs, tmp_path):
    """The opt-in P2M_TILE_GEMM=1 path (p2m_cheb_tile_gemm on every split level: forward, plain and paired backward)
    inside the whole network against the float64 oracle, kinks accounted for."""
    _kink_resolved_check_child("a_tile_gemm_human36_B3", tmp_path, {"P2M_TILE_GEMM": "1"}, "human36", 3, 21, 99, 5)


@pytest.mark.parametrize("env,tag", [({"P2M_GEMM_ARITH": "f16x2"}, "a_f16x2_human36_B3"),
                                     ({"P2M_GEMM_ARITH": "f16x2", "P2M_TILE_GEMM": "1"}, "a_f16x2_tile_human36_B3"),
                                     ({"P2M_GEMM_ARITH": "bf16x3"}, "a_bf16x3_human36_B3"),
                                     # the bench's headline path: k_cheb_tile_gemm in three bf16 slices on every plan (at B = 256
                                     # the policy picks it by itself), LDS-staged epilogue, planes out, activation on load
                                     ({"P2M_GEMM_ARITH": "bf16x3", "P2M_TILE_GEMM": "1"}, "a_bf16x3_tile_human36_B3")])
def test_slice_arithmetics_network_vs_oracle_train(hip_libs, tmp_path, env, tag):
    """The whole network in each slice arithmetic of the contractions (include/p2m.h P2M_ARITH_*: two scaled fp16 slices with
    the amax words travelling with the tensors, three exact bf16 slices), with and without the basis inside the
    contraction, against the float64 oracle: vertices, and every gradient with the ReLU kinks resolved."""
    _kink_resolved_check_child(tag, tmp_path, env, "human36", 3, 21, 99, 5)


@pytest.mark.parametrize("joint_set,B", [("mano", 5), ("human36", 3), ("coco", 2)])
def test_full_gradients_vs_oracle_train(hip_libs, joint_set, B):
    """(a) every parameter gradient and the input gradient, FULL tensors, train mode, fresh inputs, against float64
    with the ReLU kinks accounted for element by element (tests/kinks.py); running statistics against the fp32 oracle."""
    hip, _ = _kink_resolved_check(f"a_{joint_set}_B{B}", joint_set, B, 21, 99, 5)
    _, _, ref_sd = _oracle(joint_set, B, "train", 21, 99, 5)
    for k, v in ref_sd.items():
        if "running" in k:
            assert (hip[f"state::{k}"].cpu() - v).abs().max() < 1e-4, k


def test_full_gradients_vs_oracle_eval(hip_libs):
    """(a') eval mode (running statistics): gradients flow through BN as a fixed affine map - and through ReLU kinks as
    in train mode: the float64 oracle in eval mode, run with the masks the kernels used (tests/kinks.py)."""
    hip = _hip_run("mano", 5, "eval", 22, 98, 6, tap=True)
    masks = [hip[k].cpu() for k in sorted((k for k in hip if k.startswith("mask::")), key=lambda k: int(k[6:]))]
    sd, glt, x, mano, w = _oracle_inputs("mano", 5, 22, 98, 6)
    out64, g64, st = kinks.masked_oracle_gradients(sd, glt, x, mano, w, masks, training=False)
    assert helpers.max_vertex_l2(hip["out"].cpu(), out64) <= VERTEX_TOL
    _record("a_mano_eval_kinks", {"relu_elements": st["n_relu_elements"], "flipped": st["n_flips"],
                                  "max_abs_preact_at_flip": st["max_abs_preact_at_flip"]})
    assert st["max_abs_preact_at_flip"] <= KINK_WINDOW, st
    assert st["n_flips"] <= max(20, 4e-6 * st["n_relu_elements"]), st
    _compare_grads({k[6:]: v for k, v in hip.items() if k.startswith("grad::")}, g64, ALIGNED_GRAD_TOL,
                   "a_mano_eval_grads", False)


@pytest.mark.parametrize("joint_set,B", [("mano", 256), ("human36", 32), ("coco", 32)])
def test_bench_scale_vs_oracle_train(hip_libs, joint_set, B):
    """(b) MANO B=256 (the MANO config's row-set tiling, 256 x tiles-per-sample) and SMPL-like B=32 (BASELINE.md
    section 2: 8.8 GB on the CPU in fp32) forward + backward against the float64 oracle, kinks accounted for; coco
    (J=19) is the bench's own graph (BASELINE configs[2])."""
    _kink_resolved_check(f"b_{joint_set}_B{B}", joint_set, B, 31, 77, 8)


@pytest.mark.parametrize("joint_set,B,seeds", [("coco", 256, (41, 55, 9)), ("mano", 512, (42, 56, 10))])
def test_baseline_sizes_default_vs_independent_kernel_set(hip_libs, tmp_path, joint_set, B, seeds):
    """(c) BASELINE configs[2] (SMPL-like coco graph, B=256, train) and configs[4] (MANO-like, B=512, train): a
    CROSS-CHECK since round 5 - the oracle-anchored backward at these sizes is
    test_baseline_sizes_backward_vs_float64_oracle (float64 needs ~140 GB of host memory for configs[2]; it runs where the
    host has them).  Here the default kernel set (f16x2 contraction on
    the FP16 pipe, fake-vertex split, LDS-tiled basis, wave-specialised GEMM) is compared with an INDEPENDENT one (native
    f32 MFMA, unsplit rows, row-per-wave gather, 4-wave GEMM) that test_independent_kernel_set_vs_oracle_train pins to the
    float64 oracle at network level.  Forward: per-vertex L2.  Backward: the two runs' ReLU masks are compared bit by
    bit -- the handful of differing elements (fp32 kinks) is counted; plus 4 eval samples of the SAME batch against the
    oracle.  The gradient bound stays the unaccounted 1e-2 HERE AND ONLY HERE: subtracting what the differing bits do
    (tests/kinks.py accounted_difference, as every smaller comparison of two kernel sets does) takes two float64 oracle
    backward passes, which at B = 256 do not fit most hosts (~140 GB each); test_baseline_sizes_backward_vs_float64_oracle
    is the anchor at these sizes where the memory is there, and test_independent_kernel_set_vs_oracle_train /
    test_algebraic_shortcuts_against_their_plain_forms hold the same kernel sets to 5e-5 / 1e-4 at human36 B=3."""
    ws, xs, gs = seeds
    ind = _child_run(tmp_path, INDEPENDENT_SET, joint_set, B, "train", ws, xs, gs)
    hip = _hip_run(joint_set, B, "train", ws, xs, gs, tap=True)
    tag = f"c_{joint_set}_B{B}"
    err = helpers.max_vertex_l2(hip["out"].cpu(), ind["out"])
    _record(f"{tag}_vertex_l2_default_vs_independent", err)
    assert err <= 5e-5                    # two fp32 evaluation orders of a 21-layer network, |y| ~ 3; the bar is 1e-4
    nflip, nel = 0, 0
    for k in (k for k in hip if k.startswith("mask::")):
        a = np.packbits(hip[k].cpu().numpy().reshape(-1))
        nflip += int(np.unpackbits(a ^ ind[k]).sum())
        nel += hip[k].numel()
    _record(f"{tag}_mask_bits_differing", {"flipped": nflip, "relu_elements": nel})
    assert nflip <= 4e-6 * nel, (nflip, nel)          # ~1 element per million sits within fp32 rounding of the kink
    grads_h = {k[6:]: v for k, v in hip.items() if k.startswith("grad::")}
    grads_i = {k[6:]: ind[k] for k in ind.files if k.startswith("grad::")}
    # each differing mask bit moves the upstream gradients by ~1/sqrt(rows x features) of their norm; the sum over the
    # counted flips stays below 1e-2 (measured: see gpurun_out/parity_maxima.json).  With the masks ALIGNED the same
    # kernels agree with float64 to 3e-5 (tests (a), (b)).
    _compare_grads(grads_h, grads_i, 1e-2, f"{tag}_grads_default_vs_independent", True)
    for k in ind.files:
        if k.startswith("state::"):
            assert np.abs(hip[k].cpu().numpy() - ind[k]).max() < 1e-5, k
    del hip, grads_h
    torch.cuda.empty_cache()
    # eval slices of the same batch vs the oracle (eval-mode samples are independent)
    from pose2mesh_release_amd import meshnet
    gL, _, _ = helpers.golden_graphs(joint_set)
    mano = joint_set == "mano"
    net = meshnet.get_model(5, 3, gL, mano=mano)
    sd = helpers.numpy_state(net.state_dict(), ws)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    x = helpers.meshnet_input(B, int(gL[-1].shape[0]), seed=xs)
    with torch.no_grad():
        big = net(x.cuda())
    idx = [0, B // 3, 2 * B // 3, B - 1]
    torch.set_num_threads(ORACLE_THREADS)
    ref, _, _ = helpers.oracle_run(sd, helpers.oracle_graphs(gL), x[idx], mano, False)
    err = helpers.max_vertex_l2(big[idx].cpu(), ref)
    _record(f"{tag}_eval_slices_vertex_l2", err)
    assert err <= VERTEX_TOL


def _host_mem_available_gb():
    try:
        for ln in open("/proc/meminfo"):
            if ln.startswith("MemAvailable:"):
                return int(ln.split()[1]) / 1048576.0
    except OSError:
        pass
    return 0.0


# float64 oracle, forward + BACKWARD, peak host memory: ~0.55 GB per SMPL-like mesh (saved activations of the reference's
# operator sequence: 8.8 GB in fp32 at B = 32) -> ~140 GB at B = 256; ~0.03 GB per MANO-like mesh
@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("joint_set,B,seeds,need_gb", [("coco", 256, (41, 55, 9), 200.0), ("mano", 512, (42, 56, 10), 40.0)])
def test_baseline_sizes_backward_vs_float64_oracle(hip_libs, joint_set, B, seeds, need_gb, arith):
    """(c'') VERDICT r4 item 4: the BACKWARD of BASELINE configs[2] (SMPL-like coco graph, B=256, train) and configs[4]
    (MANO-like, B=512) anchored on the ORACLE, not on a second HIP kernel set: every parameter gradient and the input
    gradient of the default kernels against the float64 oracle run with the ReLU masks the kernels used (tests/kinks.py),
    at BASELINE's own batch.  The float64 oracle needs ~140 GB of host memory at B=256: the GPU host (256-thread EPYC) is
    asked through /proc/meminfo; with less than `need_gb` available the fp32 oracle is NOT substituted (its own BatchNorm
    rounding noise at 3 M rows per channel is 3e-4, test_baseline_sizes_train_forward_vs_oracle) - the test skips and says
    so, and test_baseline_sizes_default_vs_independent_kernel_set remains the cross-check.
    Round 6: in bf16x3 (the arithmetic of bench.py's headline: other tile-kernel instantiations, grid shapes and the
    LDS-staged epilogue at this batch) AND in f16x2.  The float64 oracle's backward is run per arithmetic, because it is run
    with the masks THAT run's kernels used (they differ in a few hundred kink elements of 1.9 G)."""
    have = _host_mem_available_gb()
    _record(f"c_{joint_set}_B{B}_host_mem_available_gb", round(have, 1))
    if have < need_gb:
        pytest.skip(f"float64 oracle backward at {joint_set} B={B} needs ~{need_gb:.0f} GB of host memory, "
                    f"{have:.0f} GB available")
    ws, xs, gs = seeds
    with _arith(arith):
        _kink_resolved_check(f"c_{joint_set}_B{B}{_atag(arith)}", joint_set, B, ws, xs, gs)


@pytest.mark.parametrize("joint_set,B,seeds", [("coco", 256, (41, 55, 9)), ("mano", 512, (42, 56, 10))])
def test_baseline_sizes_train_forward_vs_oracle(hip_libs, joint_set, B, seeds):
    """(c') BASELINE's own parity figure, oracle-anchored: the TRAIN-mode forward (full-batch BatchNorm statistics,
    lib/models/backbones/cheby_graph_conv.py:39, lib/models/meshnet.py:80-117) of configs[2] (SMPL-like coco graph, B=256)
    and configs[4] (MANO-like, B=512) on the default kernel set against the CPU oracle run under no_grad (no saved
    activations) - in fp32, the reference's own CPU arithmetic, AND in float64, the same operator sequence without its
    rounding noise.  At B=256 the BatchNorm statistics run over 3.0 M rows per channel; the reference's fp32 CPU path
    (torch's per-thread fp32 accumulation) is itself ~3e-4 away from the float64 result there (measured, recorded), so
    "within 1e-4 of the reference" is asserted the only way that is well defined:
      * HIP vs float64 oracle             <= 1e-4  (per-vertex L2, max over B x V)          -- the bar;
      * HIP vs fp32 oracle                <= 1e-4 + (fp32 oracle vs float64 oracle)         -- no further away from the
        reference's fp32 result than that result's own rounding error allows;
      * running statistics vs the float64 oracle's (rounded to fp32)."""
    ws, xs, gs = seeds
    got = {}
    for arith in ("bf16x3", "f16x2"):          # the credited arithmetic and the package default, against ONE oracle evaluation
        with _arith(arith):
            hip = _hip_run(joint_set, B, "train", ws, xs, gs)
        got[arith] = (hip["out"].cpu(), {k[7:]: v.cpu() for k, v in hip.items() if k.startswith("state::")})
        del hip
        torch.cuda.empty_cache()
    assert not torch.equal(got["bf16x3"][0], got["f16x2"][0])          # two arithmetics really ran
    sd, glt, x, mano, _ = _oracle_inputs(joint_set, B, ws, xs, gs)
    ref32, _, _ = helpers.oracle_run(sd, glt, x, mano, True, grad_seed=None)
    sd64 = {k: (v.double().clone() if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        ref64 = mo.meshnet_forward(sd64, [g.double() for g in glt], x.double(), mano, True)
    noise = helpers.max_vertex_l2(ref32, ref64)
    for arith, (out, state) in got.items():
        tag = f"c_{joint_set}_B{B}{_atag(arith)}_train_fwd"
        e64, e32 = helpers.max_vertex_l2(out, ref64), helpers.max_vertex_l2(out, ref32)
        _record(f"{tag}_vertex_l2_vs_float64_oracle", e64)
        _record(f"{tag}_vertex_l2_vs_fp32_oracle", e32)
        _record(f"{tag}_fp32_oracle_vs_float64_oracle", noise)
        _record(f"{tag}_vertex_l2_mean_vs_float64_oracle", float((out.double() - ref64).norm(dim=-1).mean()))
        assert e64 <= VERTEX_TOL, (arith, e64, e32, noise)
        assert e32 <= VERTEX_TOL + noise, (arith, e64, e32, noise)
        worst = 0.0
        for k, v in sd64.items():
            if "running" in k:
                d = float((state[k].double() - v).abs().max())
                worst = max(worst, d)
                assert d < 1e-4, (arith, k, d)
        _record(f"{tag}_running_stats_max_abs_vs_float64_oracle", worst)


@pytest.mark.parametrize("env,fwd_bitwise", [({"P2M_CLASSES": "0"}, False), ({"P2M_PAIR_BWD": "0"}, True),
                                             ({"P2M_TILE_GEMM": "1"}, False), ({"P2M_TILE_GEMM": "0"}, False),
                                             ({"P2M_FOLD_ACT": "0"}, False)])
def test_algebraic_shortcuts_against_their_plain_forms(hip_libs, tmp_path, env, fwd_bitwise):
    """The default path's exact algebraic shortcuts -- classes of identical fake rows (only one representative of a run of
    identical padding rows is computed), the backward of un-pooled convs at the coarse resolution -- and the opt-in
    basis-inside-the-contraction kernel everywhere (1) / nowhere (0) instead of on the big levels' forward only (auto),
    the BatchNorm + ReLU between the two convs of a block as its own pass (P2M_FOLD_ACT=0) instead of applied where the second
    conv loads its input (same operand values, but the amax word of the folded operand is a bound, not the exact maximum:
    the fp16 slices are cut at another binade) - each against the same network with the knob flipped (child process; human36, B=3, train).  P2M_PAIR_BWD=0 also switches the classes off (they need the paired operator)."""
    out = str(tmp_path / "plain.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_child_meshnet_run.py"), out, "human36", "3", "train",
                        "13", "21", "5"], env=dict(os.environ, P2M_TEST_TAP="1", **env), capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ref = np.load(out)
    hip = _hip_run("human36", 3, "train", 13, 21, 5, tap=True)
    o = hip["out"].cpu().numpy()
    if fwd_bitwise and "P2M_PAIR_BWD" not in env:
        assert np.array_equal(o, ref["out"])                 # the forward is untouched by a backward-only knob
    assert helpers.max_vertex_l2(hip["out"].cpu(), ref["out"]) <= 1e-5
    keys = sorted((k for k in hip if k.startswith("mask::")), key=lambda k: int(k[6:]))
    masks_h = [hip[k].cpu() for k in keys]
    masks_r = [torch.from_numpy(np.unpackbits(ref[k]).astype(bool)) for k in keys]
    grads_h = {k[6:]: v for k, v in hip.items() if k.startswith("grad::")}
    grads_r = {k[6:]: ref[k] for k in ref.files if k.startswith("grad::")}
    # two fp32 evaluations, each within ALIGNED_GRAD_TOL of float64 on its own masks: what the differing mask bits do is
    # subtracted in float64 (tests/kinks.py), the rest is round-off whatever the number of bits
    sd, glt, x, mano, w = _oracle_inputs("human36", 3, 13, 21, 5)
    acc = kinks.accounted_difference(sd, glt, x, mano, w, masks_h, masks_r, True)
    names = set(grads_r)
    tag = "ab_" + "_".join(f"{k}={v}" for k, v in env.items())
    res = kinks.assert_accounted(grads_h, grads_r, acc, 2 * ALIGNED_GRAD_TOL, skip=lambda k: _zero_grad_bias(k, names),
                                 what=tag)
    _accounted_record(tag, acc, res, 2 * ALIGNED_GRAD_TOL)
    for k in names:
        if _zero_grad_bias(k, names):
            wk = k.replace("bias", "weight")
            assert float(torch.as_tensor(grads_h[k]).norm()) <= 1e-3 * max(1.0, float(torch.as_tensor(grads_h[wk]).norm())), k
    for k in ref.files:
        if k.startswith("state::"):
            assert np.abs(hip[k].cpu().numpy() - ref[k]).max() < 1e-5, k


def test_fused_batchnorm_backward_reduction_against_the_separate_pass(hip_libs, tmp_path):
    """Round 6: in bf16x3 the BatchNorm-backward reduction of a block's first conv is summed, for the real-vertex rows, by the
    tile kernel that stores the gradient it reduces (p2m_cheb_tile_gemm bnr_*), the fake-vertex rows by
    p2m_bn_bwd_reduce_fake - instead of one stand-alone pass over g and y (P2M_BN_FUSE=0).  Same network, knob flipped (two
    child processes; human36, B=3, train, tile kernel on every level that has a plan): the forward is bitwise the same, so
    are the ReLU masks; every gradient agrees to fp32 round-off (the sums are taken in another order); and the fused form
    really ran (on every block whose second conv's dX is <= 128 wide)."""
    env = dict(P2M_GEMM_ARITH="bf16x3", P2M_TILE_GEMM="1")
    fused = dict(_child_run(tmp_path, dict(env, P2M_BN_FUSE="1"), "human36", 3, "train", 13, 21, 5))     # (read fully: the
    plain = dict(_child_run(tmp_path, dict(env, P2M_BN_FUSE="0"), "human36", 3, "train", 13, 21, 5))     # file is reused)
    assert int(fused["meta::bnr_fused"]) >= 3 and int(plain["meta::bnr_fused"]) == 0, (fused["meta::bnr_fused"],)
    assert np.array_equal(fused["out"], plain["out"])
    for k in fused:
        if k.startswith("mask::"):
            assert np.array_equal(fused[k], plain[k]), k
    _compare_grads({k[6:]: fused[k] for k in fused if k.startswith("grad::")},
                   {k[6:]: plain[k] for k in plain if k.startswith("grad::")}, 2e-6, "ab_bn_fuse", True)


def test_train_mode_is_bitwise_repeatable(hip_libs):
    """(e) BN partial merge + side-stream dW + row-set split: two identical fwd+bwd give identical bits."""
    a = _hip_run("human36", 4, "train", 7, 8, 9)
    b = _hip_run("human36", 4, "train", 7, 8, 9)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_three_adam_steps_vs_oracle(hip_libs):
    """(d) bench.TrainStep (FlatPose2Mesh fwd, fused epilogue + losses, bwd, FlatAdam on the flat buffers), MANO B=8,
    dropout off, three steps.

    Adam's first updates are lr * g / (|g| + 1e-8) = +-lr for ANY |g| >> 1e-8: an element whose gradient is within
    rounding noise (or within a ReLU-kink perturbation, tests/kinks.py) of 0 takes a full step of arbitrary sign in
    either implementation, and after that step the two trajectories are different optimisation problems (measured:
    2.6 % of the elements are > 1e-4 apart after 3 steps, loss 7.9866 vs 7.9771).  "All parameters within 1e-5 after 3
    steps" is therefore not a property of the reference arithmetic.  What is checked instead, without loosening:
      1. step 1 against the float64 oracle of the WHOLE model - lifter, MeshNet, the five losses - run with the ReLU masks
         the kernels used (both modules' `_tap` hooks; tests/kinks.py flat_masked_oracle_gradients), then float64 Adam:
         (a) the loss agrees to 1e-5 and every tensor of the flat gradient buffer, as the optimizer is about to read it, is
             within ALIGNED_GRAD_TOL rel-L2 of float64 - the end-to-end gradient check: PoseNet, MeshNet, the fused
             epilogue, five losses, the flat layout (exactly-zero biases in front of a train-mode BatchNorm left out);
         (b) every element whose float64 gradient is not tiny (|g64| >= 5 % of its tensor's rms) lands within 1e-6 of the
             float64 oracle's updated parameter.  The only other thing such an element may do is step the other way
             because its HIP gradient has the opposite SIGN; that takes |g_hip - g64| >= 0.05 rms, so (a) caps the
             number of such elements of a tensor of n elements at tol^2 n / 0.0025 (about 1e-6 n: none below a million
             elements) - asserted per tensor - and each of them must sit within 1e-6 of what stock Adam makes of the
             HIP gradient.
      2. steps 1-3 against torch.optim.Adam fed with the SAME (HIP) gradients: FlatAdam's moments, bias correction and
         flat-buffer layout over several steps, all elements within 2e-6."""
    import bench
    torch.set_num_threads(ORACLE_THREADS)
    B = 8
    step = bench.TrainStep(torch.device("cuda", 0), B, "mano", 1)
    for m in step.model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    sd = {k: v.detach().cpu().clone() for k, v in step.model.state_dict().items()}
    names = [k for k, _ in step.model.named_parameters()]
    # shadow optimizer: stock torch Adam on a copy of the flat buffer, fed with the gradients the HIP step produced
    shadow = step.opt.flat_param.detach().clone().requires_grad_(True)
    shadow_opt = torch.optim.Adam([shadow], lr=1e-3)
    real_step = step.opt.step
    flat_grads, masks = [], []

    def step_both(grad_scale=1.0):
        shadow.grad = step.opt.flat_grad.detach().clone()          # the gradients as the optimizer is about to read them
        flat_grads.append(shadow.grad)
        if step.model.pose_lifter._tap is not None:
            # the masks the kernels used, formed BEFORE the optimizer moves the lifter's gamma and beta: its tap hands out
            # the parameters themselves
            masks.extend(kinks.posenet_hip_masks(step.model.pose_lifter._tap, B) + kinks.hip_masks(step.model.pose2mesh._tap))
            step.model.pose2mesh._tap = step.model.pose_lifter._tap = None
        shadow_opt.step()
        return real_step(grad_scale)
    step.opt.step = step_both
    # ---- step 1, both sides
    step.model.pose2mesh._tap = []
    step.model.pose_lifter._tap = []
    hip_loss = float(step().detach())
    assert step.model.pose_lifter._tap is None and len(masks) == 4 + 14
    shadow1 = shadow.detach().clone().cpu()
    glt = helpers.oracle_graphs(step.graph_L)
    one = step.one.cpu()
    ref_loss, g64, st = kinks.flat_masked_oracle_gradients(
        sd, glt, step.pose2d.cpu(), True, masks,
        (step.perm_rev, step.nv, step.faces, step.Jreg.cpu(), step.gt_mesh.cpu(), step.gt_reg.cpu(), step.gt_lift.cpu(),
         one, one, one))
    ref_loss = float(ref_loss)
    assert abs(hip_loss - ref_loss) <= 1e-5 * abs(ref_loss), (hip_loss, ref_loss)
    # every mask difference is a genuine kink element, in the lifter's four layers and in MeshNet's
    n_lift = st["call_dims"].count(2)
    per_layer = st.get("max_abs_preact_per_layer", {})
    y_lift = max([v for l, v in per_layer.items() if l < n_lift], default=0.0)
    y_mesh = max([v for l, v in per_layer.items() if l >= n_lift], default=0.0)
    print(f"step 1: loss {hip_loss:.8f} vs float64 {ref_loss:.8f}; flips per ReLU call {st['flips_per_layer']}, "
          f"max |y64| at a flip: lifter {y_lift:.3e}, MeshNet {y_mesh:.3e}")
    assert n_lift == 4 and y_mesh <= KINK_WINDOW and y_lift <= KINK_WINDOW, st
    assert st["n_flips"] <= max(20, 4e-6 * st["n_relu_elements"]), st
    got = dict(step.model.named_parameters())
    where = {id(p): o for p, o in zip(step.opt.params, step.opt.offsets)}
    flat1 = flat_grads[0].cpu()

    def zero_grad_param(k):          # exactly-zero true gradient (a bias in front of a train-mode BatchNorm): pure noise
        if k.startswith("pose2mesh.cl.") and k.endswith("bias"):
            return k.replace("cl.", "bn.").replace("bias", "weight") in got
        return k.startswith("pose_lifter.linear_stages.") and k.endswith(".w1.bias")
    live = [k for k in names if g64[k] is not None and not zero_grad_param(k) and float(g64[k].abs().max()) > 0.0]
    # float64 Adam on the float64 gradients
    p64 = {k: sd[k].double().clone().requires_grad_(True) for k in live}
    for k in live:
        p64[k].grad = g64[k]
    torch.optim.Adam([p64[k] for k in live], lr=1e-3).step()
    tol = ALIGNED_GRAD_TOL
    n_checked, worst, n_opposite, n_cap, rel = 0, 0.0, 0, 0, {}
    for k in live:
        o, n = where[id(got[k])], got[k].numel()
        gh = flat1[o:o + n].view_as(g64[k]).double()
        rel[k] = helpers.rel_l2(gh, g64[k])                                             # (a)
        g = g64[k]
        rms = float(g.pow(2).mean().sqrt())
        big = g.abs() >= 0.05 * rms                                                     # (b)
        d = (got[k].detach().cpu().double() - p64[k].detach()).abs()
        n_checked += int(big.sum())
        other = big & (d > 1e-6)
        if int(other.sum()):
            cap = int(tol * tol * n / 0.0025)
            assert int(other.sum()) <= cap, (k, int(other.sum()), cap, n)
            assert bool(((gh * g)[other] < 0).all()), (k, "off its float64 Adam update without an opposite-sign gradient")
            ds = (got[k].detach().cpu() - shadow1[o:o + n].view_as(g)).abs()
            assert float(ds[other].max()) <= 1e-6, (k, float(ds[other].max()))
            n_opposite += int(other.sum())
        n_cap += int(tol * tol * n / 0.0025)
        if bool((big & ~other).any()):
            worst = max(worst, float(d[big & ~other].max()))
    at = max(rel, key=rel.get)
    print("flat gradient vs float64, masks aligned, worst tensors:",
          sorted(((round(v, 9), k) for k, v in rel.items()), reverse=True)[:8],
          f"; opposite-sign elements {n_opposite} (cap {n_cap}), max |p - p64| {worst:.3e} over {n_checked}")
    _record("d_adam_step1_vs_oracle", {"elements_checked": n_checked, "max_param_diff": worst,
                                       "opposite_sign_elements": n_opposite, "opposite_sign_cap_all_tensors": n_cap,
                                       "flat_grad_worst_rel_l2_masks_aligned": rel[at], "at": at, "tensors": len(rel),
                                       "relu_elements": st["n_relu_elements"], "flipped": st["n_flips"],
                                       "max_abs_preact_at_flip_lifter": y_lift, "max_abs_preact_at_flip_meshnet": y_mesh,
                                       "of_total": sum(p.numel() for p in got.values())})
    bad = {k: v for k, v in rel.items() if v > tol}
    assert not bad, f"flat gradient vs float64, masks aligned, above {tol:g}: {bad}"
    assert n_checked > 0.9 * sum(g64[k].numel() for k in live)
    # nothing else is left out: the zero-gradient biases, and the lifter's batch_norm1, which its forward never applies
    assert all(zero_grad_param(k) or k.startswith("pose_lifter.batch_norm1.") for k in names if k not in live)
    # ---- steps 2, 3 on the HIP side; FlatAdam vs stock Adam on identical gradients
    losses = [hip_loss] + [float(step().detach()) for _ in range(2)]
    assert losses[2] < losses[1] < losses[0]
    d = float((step.opt.flat_param - shadow.detach()).abs().max())
    _record("d_flat_adam_vs_torch_adam_same_grads_3_steps", d)
    assert d <= 2e-6, d
    assert step.opt.step_count == 3


@pytest.mark.parametrize("joint_set", ["mano", "coco", "human36"])
@pytest.mark.parametrize("with_edge", [True, False])
def test_fused_mesh_loss_vs_reference_golden(hip_libs, joint_set, with_edge):
    """p2m_mesh_loss (perm-reverse gather + J-regression + 4 losses + gradient) against fixtures
    made by the REAL lib/core/loss.py driven as lib/core/base.py:130-143 does; masks in the reference's shapes.
    human36 runs with the reference's own regressor file (J_regressor_h36m_correct.npy, 107 nnz, embedded in the fixture)."""
    from pose2mesh_release_amd import loss as L
    z = helpers.golden(f"loss_{joint_set}.npz")
    c = helpers.loss_case(joint_set, jreg=helpers.golden_regressor() if joint_set == "human36" else None)
    tag = "edge" if with_edge else "noedge"
    fused = L.FusedMeshLoss(c["faces"], c["perm_reverse"], c["J_regressor"].numpy(), w_normal=1e-1,
                            w_edge=20.0 if with_edge else 0.0, w_joint=1e-3)
    cam = c["cam_mesh"].cuda().requires_grad_(True)
    total, comp = fused(cam, c["gt_mesh"].cuda(), c["gt_reg3dpose"].cuda(), c["val_mesh"].cuda(),
                        c["val_reg3dpose"].cuda())
    total.backward()
    want = z[f"{tag}_losses"]
    for got, ref in zip(comp.tolist(), [want[0], want[1], want[2], want[3]]):
        assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref)), (comp.tolist(), want)
    e = helpers.rel_l2(cam.grad.cpu(), z[f"{tag}_grad_cam"])
    _record(f"f_loss_{joint_set}_{tag}_grad_rel_l2", e)
    assert e <= 1e-5
    fake = np.setdiff1d(np.arange(c["V0"]), c["perm_reverse"][:c["nv"]])
    assert float(cam.grad[:, torch.as_tensor(fake, device="cuda")].abs().max()) == 0.0
    # mask shapes: [B], [B,1,1] give the same result as the reference's [B,nv,1] / [B,J,1]
    vm, vr = c["val_mesh"][:, 0, 0].cuda(), c["val_reg3dpose"][:, 0, 0].cuda()
    for shp in ((-1,), (-1, 1, 1)):
        t2, c2 = fused(cam.detach(), c["gt_mesh"].cuda(), c["gt_reg3dpose"].cuda(), vm.view(*shp), vr.view(*shp))
        assert torch.equal(c2, comp)
    with pytest.raises(ValueError):
        fused(cam.detach(), c["gt_mesh"].cuda(), c["gt_reg3dpose"].cuda(), torch.ones(c["B"], c["nv"], 3).cuda(), None)


def test_disabled_edge_loss_cannot_inject_nan(hip_libs):
    """w_edge = 0 with a zero-length predicted edge must give a finite gradient (the reference does not
    evaluate the edge loss before cfg.TRAIN.edge_loss_start, lib/core/base.py:141-143)."""
    from pose2mesh_release_amd import loss as L
    c = helpers.loss_case("mano")
    fused = L.FusedMeshLoss(c["faces"], c["perm_reverse"], c["J_regressor"].numpy(), w_edge=0.0)
    cam = c["cam_mesh"].clone()
    f0 = c["faces"][0]
    pr = c["perm_reverse"]
    cam[:, pr[f0[1]]] = cam[:, pr[f0[0]]]          # degenerate edge
    cam = cam.cuda().requires_grad_(True)
    total, _ = fused(cam, c["gt_mesh"].cuda(), c["gt_reg3dpose"].cuda(), None, None)
    total.backward()
    assert torch.isfinite(total) and torch.isfinite(cam.grad).all()


@pytest.mark.parametrize("scale", [1000.0, 1.0])
def test_mesh_epilogue_vs_oracle(hip_libs, scale):
    """SURVEY 8(f1) for the Tester / demo: p2m_mesh_epilogue == lib/core/base.py:200-204 (x1000) / demo/run.py:169-171."""
    import loss_oracle as lo
    from pose2mesh_release_amd import loss as L
    c = helpers.loss_case("coco", B=3)
    epi = L.MeshEpilogue(c["perm_reverse"], c["nv"], c["J_regressor"].numpy(), scale=scale)
    mesh, joints = epi(c["cam_mesh"].cuda())
    rm, rj = lo.test_epilogue(c["cam_mesh"], c["perm_reverse"], c["nv"], c["J_regressor"])
    if scale == 1.0:
        rm, rj = rm / 1000, rj / 1000
    assert (mesh.cpu() - rm).abs().max() <= 1e-6 * float(rm.abs().max())
    assert (joints.cpu() - rj).abs().max() <= 1e-5 * float(rj.abs().max())
