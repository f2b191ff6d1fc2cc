"""-m gpu: the data-parallel path on the REAL model, provable on a 1-GPU box (VERDICT r1 "next round" 6):
two ranks share cuda:0 over gloo (P2M_DIST_BACKEND=gloo; RCCL needs one GPU per rank and remains unmeasured).
SURVEY 8(e)'s parity definition: the N-rank averaged gradient == the mean of the reference's (here: the oracle's)
gradients computed on each shard separately; BatchNorm statistics stay per rank (nn.DataParallel semantics)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers
import meshnet_oracle as mo

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

WORKER = r'''
import os, sys
sys.path[:0] = [{root!r}, {root!r} + "/oracle", {root!r} + "/tests"]
import numpy as np, torch
import helpers
from pose2mesh_release_amd import dist as pd, loss as L, optim, pose2mesh_net, synth
rank, world, local = pd.init_from_env()
assert world == 2 and torch.distributed.get_backend() == "gloo"
dev = torch.device("cuda", local)
gL, _, rev = helpers.golden_graphs("mano")
c = helpers.loss_case("mano", B=8, seed=23)
def build_net():
    net = pose2mesh_net.get_model(21, gL, mano=True)
    net.load_state_dict(helpers.numpy_state(net.state_dict(), 4))
    net = net.to(dev).train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return net
# test-only knobs (tests/stream_skew.py): which rank gets its weight-gradient stream delayed right before each backward(),
# and which rank its main stream before red.finish(); unset (the default): no skew, nothing below runs
skew_side = os.environ.get("P2M_TEST_SKEW_SIDE_RANK", "") == str(rank)
skew_main = os.environ.get("P2M_TEST_SKEW_MAIN_RANK", "") == str(rank)
late_side = late_main = lambda: None
if skew_side or skew_main:
    import time
    import stream_skew as sk
    from pose2mesh_release_amd import ops
    torch.cuda.set_device(dev)
    sk.reset_budget()
    sk.calibrate()
    main_st = torch.cuda.current_stream()
    side_st = sk.distinct_stream(main_st)
    ops._side_streams[(local, 0)] = side_st
    assert sk.bites(main_st, side_st) and sk.bites(side_st, main_st), sk.last_bite
    # t_step of an unskewed step on a throw-away copy of the model (second pass), then D = max(20 ms, 3 t_step)
    probe = build_net()
    px = synth.pose2d_batch(8, 21, seed=31)[:4].to(dev)
    for _ in range(2):
        torch.cuda.synchronize()
        e0, e1, t0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), time.perf_counter()
        e0.record()
        pm, pl = probe(px)
        (pm.square().mean() + pl.square().mean()).backward()
        e1.record()
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
    t_step = max(host_ms, e0.elapsed_time(e1))
    D = max(20.0, 3.0 * t_step)
    assert D <= sk.CAP_CALL_MS, (t_step, D)
    del probe, pm, pl
    print(f"SKEW rank {{rank}}: side late {{skew_side}}, main late {{skew_main}}, bites both ways, t_step {{t_step:.3f}} ms, "
          f"D {{D:.3f}} ms", flush=True)
    if skew_side:
        late_side = lambda: sk.delay(side_st, D)
    if skew_main:
        late_main = lambda: sk.delay(main_st, D)
net = build_net()
opt = optim.FlatAdam(net.parameters(), lr=1e-3)
# the bench's configuration: MeshNet gradients accumulate in place and are reported to the reducer per layer from inside
# the backward (autograd's hooks only fire once the whole backward has returned); small buckets so that several of them
# lie inside the MeshNet slice
net.pose2mesh.accumulate_grads_in_place(True)
red = pd.BucketedAllReduce(opt.params, opt.offsets, opt.flat_grad, bucket_bytes=1 << 20)
net.pose2mesh.set_grad_sink(red.notify)
fused = L.FusedMeshLoss(c["faces"], c["perm_reverse"], c["J_regressor"].numpy())
stock = L.get_loss(c["faces"])
sl = slice(rank * 4, rank * 4 + 4)
pose2d = synth.pose2d_batch(8, 21, seed=31)[sl].to(dev)
opt.zero_grad()
mesh, lift = net(pose2d)
total, _ = fused(mesh, c["gt_mesh"][sl].to(dev), c["gt_reg3dpose"][sl].to(dev), c["val_mesh"][sl].to(dev),
                 c["val_reg3dpose"][sl].to(dev))
lift_l = 1e-3 * stock[4](lift, c["gt_lift3dpose"][sl].to(dev), c["val_lift3dpose"][sl].to(dev))
late_side()
lift_l.backward()
late_side()
total.backward()
# overlap by construction: a bucket made of MeshNet parameters only was launched while gradients were still arriving
mesh_ids = {{id(p) for p in net.pose2mesh.parameters()}}
mesh_only = [b for b, (_, _, idx) in enumerate(red.buckets) if all(id(opt.params[i]) in mesh_ids for i in idx)]
log, seen_total = list(red.launch_log), red._seen
early = [seen for b, seen in log if b in mesh_only]
assert len(mesh_only) >= 2 and early and min(early) <= seen_total - 10, (mesh_only, log, seen_total)
late_main()
scale = red.finish()
assert abs(scale - 0.5) < 1e-12 and len(red.buckets) >= 2
grads = {{k: (p.grad * scale).cpu().numpy() for k, p in net.named_parameters()}}
stats = {{k: v.cpu().numpy() for k, v in net.state_dict().items() if "running" in k}}
np.savez({out!r} + f"_r{{rank}}.npz", **{{"g::" + k: v for k, v in grads.items()}}, **{{"s::" + k: v for k, v in stats.items()}})
opt.step(scale)          # identical update on both ranks
np.save({out!r} + f"_p{{rank}}.npy", opt.flat_param.cpu().numpy())
torch.distributed.barrier()
torch.distributed.destroy_process_group()
'''


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(nproc, argv, extra_env=None, timeout=900):
    env = dict(os.environ, P2M_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.update(extra_env or {})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port())] + argv
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)


def _run_worker(folder, tag, extra_env=None):
    """One two-rank gloo run of WORKER; returns (prefix of the files it wrote, its stdout)."""
    out = str(folder / tag)
    script = folder / f"worker_{tag}.py"
    script.write_text(WORKER.format(root=ROOT, out=out))
    r = _launch(2, [str(script)], extra_env=extra_env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return out, r.stdout


@pytest.fixture(scope="module")
def plain_run(hip_libs, tmp_path_factory):
    """The unskewed two-rank run, once for the tests that read it."""
    return _run_worker(tmp_path_factory.mktemp("dp"), "dp")


def test_two_ranks_real_model_gradient_is_mean_of_oracle_shard_gradients(hip_libs, plain_run):
    import loss_oracle as lo
    out, _ = plain_run
    z = [np.load(out + f"_r{k}.npz") for k in range(2)]
    # both ranks hold the same averaged gradient and, after the step, the same parameters
    for k in z[0].files:
        if k.startswith("g::"):
            assert np.array_equal(z[0][k], z[1][k]), k
    assert np.array_equal(np.load(out + "_p0.npy"), np.load(out + "_p1.npy"))
    # oracle on each shard separately
    torch.set_num_threads(16)
    from pose2mesh_release_amd import pose2mesh_net, synth
    gL, _, _ = helpers.golden_graphs("mano")
    c = helpers.loss_case("mano", B=8, seed=23)
    sd0 = helpers.numpy_state(pose2mesh_net.get_model(21, gL, mano=True).state_dict(), 4)
    glt = helpers.oracle_graphs(gL)
    pose2d = synth.pose2d_batch(8, 21, seed=31)
    mean_g, stats = None, []
    for rank in range(2):
        sl = slice(rank * 4, rank * 4 + 4)
        sd = {k: v.clone() for k, v in sd0.items()}
        names = [k for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k]
        for k in names:
            sd[k].requires_grad_(True)
        mesh, lift = mo.flat_forward(sd, glt, pose2d[sl], True, True)
        loss, _ = lo.train_losses(mesh, lift, c["perm_reverse"], c["nv"], c["faces"], c["J_regressor"], c["gt_mesh"][sl],
                                  c["gt_reg3dpose"][sl], c["gt_lift3dpose"][sl], c["val_mesh"][sl],
                                  c["val_reg3dpose"][sl], c["val_lift3dpose"][sl], with_edge=True)
        loss.backward()
        # (the outer pose_lifter.batch_norm1 exists in the state dict but is never applied, posenet.py:77-87: no grad)
        g = {k: sd[k].grad.clone() for k in names if sd[k].grad is not None}
        mean_g = g if mean_g is None else {k: 0.5 * (mean_g[k] + g[k]) for k in g}
        stats.append({k: v.detach() for k, v in sd.items() if "running" in k})
    worst = 0.0
    assert float(np.abs(z[0]["g::pose_lifter.batch_norm1.weight"]).max()) == 0.0
    for k, ref in mean_g.items():
        got = z[0]["g::" + k]
        if k.startswith("pose2mesh.cl.") and k.endswith("bias") and k.replace("cl.", "bn.").replace("bias", "weight") in mean_g:
            continue                                       # zero gradient in front of train-mode BatchNorm
        if k.startswith("pose_lifter.linear_stages.") and k.endswith(".w1.bias"):
            continue                                       # same: w1 feeds batch_norm2 (posenet.py:32-35)
        e = helpers.rel_l2(got, ref)
        worst = max(worst, e)
        # fp32 ReLU kinks (tests/kinks.py): a flipped mask bit moves upstream gradients by ~1e-3; the aligned-mask
        # comparison against float64 lives in test_gpu_parity_full.py, here the point is the AVERAGING across ranks
        assert e < 1e-2, (k, e)
    # BatchNorm running statistics are per rank (each rank saw only its shard), as under nn.DataParallel
    for rank in range(2):
        for k, v in stats[rank].items():
            assert np.abs(z[rank]["s::" + k] - v.numpy()).max() < 1e-4 * max(1.0, float(v.abs().max())), (rank, k)
    assert not np.array_equal(z[0]["s::pose2mesh.bn.0.running_mean"], z[1]["s::pose2mesh.bn.0.running_mean"])


def test_two_ranks_skewed_write_the_bytes_of_the_unskewed_run(hip_libs, plain_run, tmp_path):
    """The same two-rank gloo step with rank 0's weight-gradient stream late before each backward() and rank 1's main
    stream late before red.finish(): the communication stream must wait for EVERY stream that wrote a bucket, on both
    ranks.  A two-rank sum is order-free, so the averaged gradients and the updated parameters are the unskewed run's, byte
    for byte.  The worker installs a side stream that bites against its main stream (tests/stream_skew.py) and sizes the
    delay from its own measured step."""
    runs = {}
    skewed = _run_worker(tmp_path, "skewed", {"P2M_TEST_SKEW_SIDE_RANK": "0", "P2M_TEST_SKEW_MAIN_RANK": "1"})
    for tag, (out, stdout), lines in (("plain", plain_run, 0), ("skewed", skewed, 2)):
        skew_lines = [ln for ln in stdout.splitlines() if ln.startswith("SKEW rank")]
        print("\n".join(skew_lines))
        assert len(skew_lines) == lines, stdout[-2000:]
        runs[tag] = ([np.load(out + f"_r{k}.npz") for k in range(2)], [np.load(out + f"_p{k}.npy") for k in range(2)])
    for k in range(2):
        za, zb = runs["plain"][0][k], runs["skewed"][0][k]
        names = [n for n in za.files if n.startswith("g::")]
        assert len(names) >= 60 and sorted(za.files) == sorted(zb.files)
        for n in names:
            assert za[n].tobytes() == zb[n].tobytes(), (k, n)
        assert runs["plain"][1][k].tobytes() == runs["skewed"][1][k].tobytes(), k
    assert float(np.abs(runs["plain"][0][0]["g::pose2mesh.cl.5.weight"]).max()) > 0.0


def test_bench_two_ranks_on_one_gpu(hip_libs):
    """`torchrun --nproc-per-node 2 bench.py --gpus 2` exactly as the driver launches it (gloo instead of RCCL because
    both ranks share the only GPU): one JSON line from rank 0 with the whole-job aggregate."""
    r = _launch(2, ["bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "16", "--no-kernel-timing"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 2 and j["scaling"] == "weak"
    assert j["config"]["global_batch"] == 32 and j["config"]["parallelism"] == "dp2"
    assert 300 < j["config"]["grad_allreduce_MB"] < 310          # 76.0 M parameters x 4 B
    assert j["value"] > 0 and "cpu_baseline" not in j


def test_bench_self_launches_its_ranks(hip_libs):
    """`python bench.py --gpus 2` with NO launcher around it (WORLD_SIZE unset - the form the driver uses for N=1) starts its
    two ranks itself and prints rank 0's single line; with the gloo override (both ranks share the only GPU) the line says
    it is not a valid scaling point.  Without the override on a 1-GPU box the ranks refuse: no line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(P2M_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    argv = [sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "16", "--no-kernel-timing"]
    r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["config"]["parallelism"] == "dp2" and j["config"]["valid_scaling_point"] is False
    assert j["config"]["backend"] == "gloo" and j["value"] > 0
    if torch.cuda.device_count() < 2:
        env.pop("P2M_DIST_BACKEND")
        r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode != 0 and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")], r.stdout[-2000:]


ONE_RANK_RCCL = r'''
import os, sys
sys.path[:0] = [{root!r}, {root!r} + "/oracle", {root!r} + "/tests"]
import torch, torch.distributed as dist
import helpers
from pose2mesh_release_amd import dist as pd, loss as L, optim, pose2mesh_net, synth
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT={port!r}, RANK="0", WORLD_SIZE="1")
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1)          # "nccl" IS RCCL on ROCm: loads librccl, one communicator
assert dist.get_backend() == "nccl"
dev = torch.device("cuda", 0)
gL, _, rev = helpers.golden_graphs("mano")
c = helpers.loss_case("mano", B=8, seed=23)
pose2d = synth.pose2d_batch(8, 21, seed=31).to(dev)
finals = []
for use_rccl in (False, True):
    net = pose2mesh_net.get_model(21, gL, mano=True)
    net.load_state_dict(helpers.numpy_state(net.state_dict(), 4))
    net = net.to(dev).train()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    opt = optim.FlatAdam(net.parameters(), lr=1e-3)
    net.pose2mesh.accumulate_grads_in_place(True)
    red = None
    if use_rccl:
        red = pd.BucketedAllReduce(opt.params, opt.offsets, opt.flat_grad, bucket_bytes=4 << 20, always=True)
        net.pose2mesh.set_grad_sink(red.notify)
        assert red.active and red.world == 1
    fused = L.FusedMeshLoss(c["faces"], c["perm_reverse"], c["J_regressor"].numpy())
    stock = L.get_loss(c["faces"])
    for step in range(3):                 # no host synchronisation between the steps: the ordering is the streams' job
        opt.zero_grad()
        mesh, lift = net(pose2d)
        total, _ = fused(mesh, c["gt_mesh"].to(dev), c["gt_reg3dpose"].to(dev), c["val_mesh"].to(dev),
                         c["val_reg3dpose"].to(dev))
        lift_l = 1e-3 * stock[4](lift, c["gt_lift3dpose"].to(dev), c["val_lift3dpose"].to(dev))
        lift_l.backward()
        total.backward()
        scale = 1.0
        if red is not None:
            n_launched_in_backward = len(red.launch_log)
            scale = red.finish()
            assert scale == 1.0 and n_launched_in_backward >= 3
            assert red.launch_log == []               # one step's entries only (reset() clears them)
        opt.step(scale)
    torch.cuda.synchronize()
    finals.append((opt.flat_param.clone(), opt.exp_avg.clone()))
# a sum over ONE rank is the identity: with the collectives (async Work objects, waited on by the stream, issued from the
# communication stream) in the step, three updates are bit for bit those of the plain loop
assert torch.equal(finals[0][0], finals[1][0]) and torch.equal(finals[0][1], finals[1][1])
# ... and the overlap by TIME, not only by launch order (HIP events around every collective on the communication stream,
# around finish()'s wait on the main stream): one more step at a batch whose backward takes milliseconds
seen = pd.ranks_seen()
assert seen["backend"] == "nccl" and seen["ranks"] == [0] and seen["local_devices"] == [0] and seen["rccl_version"]
red.timing = True
big = synth.pose2d_batch(64, 21, seed=32).to(dev)
cb = helpers.loss_case("mano", B=64, seed=24)
tgt = [cb[k].to(dev) for k in ("gt_mesh", "gt_reg3dpose", "val_mesh", "val_reg3dpose", "gt_lift3dpose", "val_lift3dpose")]
for _ in range(2):
    opt.zero_grad()
    red.mark_step_start()
    mesh, lift = net(big)
    total, _ = fused(mesh, tgt[0], tgt[1], tgt[2], tgt[3])
    (1e-3 * stock[4](lift, tgt[4], tgt[5])).backward()
    total.backward()
    red.finish()
rep = red.timing_report()
assert rep is not None and len(rep["buckets"]) == len(red.buckets) and rep["allreduce_ms_total"] > 0
mesh_ids = {{id(p) for p in net.pose2mesh.parameters()}}
early = [x for x in rep["buckets"] if all(id(opt.params[i]) in mesh_ids for i in red.buckets[x["bucket"]][2])]
# the PoseNet buckets (270 MB, back-propagated first) finish while the MeshNet backward is still running, and at least one
# MeshNet-only bucket is complete before the main stream reaches the end of its backward work
pose_b = [x for x in rep["buckets"] if not any(id(opt.params[i]) in mesh_ids for i in red.buckets[x["bucket"]][2])]
assert pose_b and max(x["end_ms"] for x in pose_b) < rep["backward_end_ms"], rep
assert early and min(x["end_ms"] for x in early) < rep["backward_end_ms"], rep
assert rep["hidden_frac"] is not None and 0.0 <= rep["hidden_frac"] <= 1.0 and rep["exposed_ms"] < rep["backward_end_ms"], rep
print("TIMING", rep["backward_end_ms"], rep["exposed_ms"], rep["hidden_frac"])
dist.destroy_process_group()
print("ONE_RANK_RCCL_OK")
'''


def test_one_rank_rccl_group_runs_the_bucketed_all_reduce(hip_libs, tmp_path):
    """VERDICT r2 "next round" 7(a): what one GPU can prove about the RCCL path.  A 1-rank `nccl` process group (librccl
    loaded, a real communicator), the real FlatPose2Mesh train step with the bucketed all-reduce forced on: the nccl
    backend's asynchronous Work.wait() (the stream waits, not the host - unlike gloo's blocking wait) must order the
    optimizer step after the collectives; three steps without host synchronisation == the loop without collectives."""
    script = tmp_path / "one_rank.py"
    script.write_text(ONE_RANK_RCCL.format(root=ROOT, port=str(_free_port())))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "ONE_RANK_RCCL_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
