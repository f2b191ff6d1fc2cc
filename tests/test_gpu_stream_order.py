"""-m gpu: WHICH STREAM a launch runs on and WHAT IT WAITS FOR - the one thing no kernel test sees.

The package orders its streams by hand: MeshNet's weight gradients on ops.side_stream (meshnet.py `side_ctx`: a
side.wait_stream(main) at every entry, a `keep` list, one main.wait_stream(side) join), amax chunks zeroed on whichever
stream rolls them over (ops.new_amax: an event every other stream waits for), GraphedTrainStep's private warm-up stream,
GraphedInference's warm-up stream.  In their natural timing a missing wait is invisible - the producer happens to finish
first.  Here the streams are skewed on purpose with a bounded spin (tests/stream_skew.py) and every result must be the
serial one BIT FOR BIT: the same kernels run on the same operands whatever the timing.

Every scenario first installs a weight-gradient stream that provably `bites` against the test's main stream (a delay on
one really lets the other run ahead - pooled streams can share a hardware queue, and the skew would then be vacuous), and
sizes its delays from a measurement: t_step = max(device time, host enqueue time) of the unskewed run,
D = max(20 ms, 3 t_step) for a whole-stream delay, d = max(5 ms, t_step) per call.  The figures are printed and written to
stream_skew.json next to test_gpu_parity_full.py's parity_maxima.json (DESIGN.md section "Stream ordering and how it is tested" quotes them).

Anchor: MANO, B = 5, train mode, seeds (21, 99, 5) - the configuration test_full_gradients_vs_oracle_train ties to the
float64 oracle.  "Equal" is torch.equal on out, every grad::* and every state::*."""
import json
import time

import pytest
import torch

import stream_skew as sk

pytestmark = pytest.mark.gpu

ANCHOR = ("mano", 5, "train", 21, 99, 5)
SPIED = ("gemm_tn_rows", "gemm_tn", "weight_grad_unpack", "weight_grad_unpack2")       # the weight-gradient launches
PRODUCERS = ("bn_relu_bwd", "conv_split", "conv_pair")           # main-stream launches whose outputs the side stream reads
AMAX_WORDS = 256             # words per chunk of ops.new_amax
_cache = {}
_figures = {}                # scenario -> the figures recorded in this run


def _record(scenario, **figures):
    """Keep a scenario's figures in stream_skew.json, next to test_gpu_parity_full's parity_maxima.json."""
    import test_gpu_parity_full as parity
    _figures.setdefault(scenario, {}).update(figures)
    parity._record(scenario, _figures[scenario], name="stream_skew.json")
    print(f"stream_skew[{scenario}]", json.dumps(figures, sort_keys=True))


def _delays(scenario, t_step):
    """D (whole-stream delay: still behind when the other stream has finished everything it was given) and d (per call)."""
    D, d = max(20.0, 3.0 * t_step), max(5.0, t_step)
    _record(scenario, t_step_ms=round(t_step, 3), D_ms=round(D, 3), d_ms=round(d, 3),
            cycles_per_ms=round(sk.calibrate(), 1))
    assert D <= sk.CAP_CALL_MS, f"{scenario}: D = {D:.1f} ms exceeds the {sk.CAP_CALL_MS:.0f} ms cap - the configuration is too big"
    return D, d


@pytest.fixture
def streams(hip_libs, monkeypatch):
    """(main, side): the test's main stream and a weight-gradient stream installed in ops that bites against it."""
    from pose2mesh_release_amd import ops
    sk.reset_budget()
    sk.calibrate()
    main = torch.cuda.current_stream()
    if "side" not in _cache:
        _cache["side"] = sk.distinct_stream(main)
    side = _cache["side"]
    fwd = sk.bites(main, side)
    ev_fwd = sk.last_bite
    bwd = sk.bites(side, main)
    print(f"bites(main {main.cuda_stream:#x}, side {side.cuda_stream:#x}) = {fwd} {ev_fwd}; "
          f"bites(side, main) = {bwd} {sk.last_bite}")
    assert fwd and bwd, (ev_fwd, sk.last_bite)
    monkeypatch.setitem(ops._side_streams, (main.device.index, 0), side)
    saved = ops.DW_SIDE_STREAM
    try:
        yield main, side
    finally:
        ops.DW_SIDE_STREAM = saved
        torch.cuda.synchronize()


# ---- the anchor run, with hooks --------------------------------------------------------------------------------------
def _anchor(side_mode, flat=False, passes=1, before_backward=None, after_forward=None, timing=None):
    """_child_meshnet_run.run(*ANCHOR) with room for a skew: `passes` forward + backward passes with no zero_grad between
    them, before_backward() right before each backward(), and the results READ ON THE MAIN STREAM AS SOON AS backward()
    HAS RETURNED, with no device synchronisation in between.  flat: gradients accumulate in place into a FlatAdam's
    flat_grad (compared too), then opt.step() and flat_param.  timing: dict that receives t_step_ms."""
    import helpers
    from pose2mesh_release_amd import meshnet, ops, optim
    joint_set, B, mode, wseed, xseed, gseed = ANCHOR
    ops.DW_SIDE_STREAM = bool(side_mode)
    gL, _, _ = helpers.golden_graphs(joint_set)
    J = int(gL[-1].shape[0])
    net = meshnet.get_model(5, 3, gL, mano=(joint_set == "mano"))
    net.load_state_dict(helpers.numpy_state(net.state_dict(), wseed))
    net = net.cuda().train(mode == "train")
    x = helpers.meshnet_input(B, J, seed=xseed).cuda().requires_grad_(True)
    w = torch.randn((B, int(gL[0].shape[0]), 3), generator=torch.Generator().manual_seed(gseed)).cuda()
    opt = None
    if flat:
        opt = optim.FlatAdam(net.parameters(), lr=1e-3)
        net.accumulate_grads_in_place(True)
        opt.zero_grad()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(passes):
        y = net(x)
        assert y.shape == w.shape
        if after_forward is not None:
            after_forward()
        loss = (y * w).sum()
        if before_backward is not None:
            before_backward()
        loss.backward()
    # no synchronisation here: these clones are enqueued on the main stream right behind the backward's join
    out = {"out": y.detach().clone(), "grad::__input__": x.grad.clone()}
    for k, p in net.named_parameters():
        out[f"grad::{k}"] = p.grad.clone()
    if flat:
        out["flat_grad"] = opt.flat_grad.clone()
        opt.step()
        out["flat_param"] = opt.flat_param.clone()
    for k, v in net.state_dict().items():
        if "running" in k:
            out[f"state::{k}"] = v.clone()
    e1.record()
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    if timing is not None:
        timing.update(host_ms=host_ms, device_ms=e0.elapsed_time(e1), t_step_ms=max(host_ms, e0.elapsed_time(e1)))
    return out


def _assert_equal(got, ref, what):
    assert set(got) == set(ref), (what, set(got) ^ set(ref))
    bad = [k for k in ref if not torch.equal(got[k], ref[k])]
    assert not bad, f"{what}: {len(bad)} of {len(ref)} tensors differ from the serial run, e.g. " + ", ".join(
        f"{k} (max |diff| {float((got[k].double() - ref[k].double()).abs().max()):.3e})" for k in bad[:4])


def _serial(flat=False, passes=1):
    """The serial form (weight gradients on the main stream), unskewed: computed once per variant and left unchanged."""
    key = ("serial", flat, passes)
    if key not in _cache:
        _cache[key] = _anchor(False, flat=flat, passes=passes)
    return _cache[key]


def _median(ts):
    """of three timings (dicts with t_step_ms): one visit of another tenant of the machine does not size the delays"""
    ts = sorted(ts, key=lambda t: t["t_step_ms"])
    return ts[len(ts) // 2]


def _anchor_delays():
    """t_step of the unskewed side-stream anchor (the median of three runs after a first one: graph handles and allocator
    pools exist), D and d."""
    if "delays" not in _cache:
        ts = [{} for _ in range(3)]
        _anchor(True)
        for t in ts:
            _anchor(True, timing=t)
        t = _median(ts)
        print(f"anchor: host {t['host_ms']:.3f} ms, device {t['device_ms']:.3f} ms (t_step of the three runs: "
              f"{[round(u['t_step_ms'], 3) for u in ts]})")
        _cache["delays"] = _delays("anchor", t["t_step_ms"])
    return _cache["delays"]


def _late_main(monkeypatch, main, d):
    """Scenario D: every main-stream producer of the backward is preceded by a spin of d on main - the side stream gets
    ahead wherever nothing orders it."""
    from pose2mesh_release_amd import ops
    count = [0, False]                   # producers delayed so far; armed (the forward calls conv_split too: not delayed)

    def wrap(real):
        def late(*a, **kw):
            if count[1]:
                count[0] += 1
                sk.delay(main, d)
            return real(*a, **kw)
        return late
    for name in PRODUCERS:
        monkeypatch.setattr(ops, name, wrap(getattr(ops, name)))
    return count, lambda: count.__setitem__(1, True)


# ---- A: serial form == side-stream form ------------------------------------------------------------------------------
def test_serial_form_equals_side_stream_form(streams):
    """ops.DW_SIDE_STREAM = False (P2M_DW_STREAM=main; the way bench.py toggles it) against True, no skew: the same bits -
    and the hooked anchor run of this file is the run of _child_meshnet_run."""
    import _child_meshnet_run as child
    from pose2mesh_release_amd import ops
    ops.DW_SIDE_STREAM = False
    ser = child.run(*ANCHOR, keep_on_gpu=True)
    ops.DW_SIDE_STREAM = True
    par = child.run(*ANCHOR, keep_on_gpu=True)
    assert sum(k.startswith("grad::") for k in ser) > 50 and sum(k.startswith("state::") for k in ser) >= 28
    _assert_equal(par, ser, "side-stream form")
    _assert_equal(_serial(), ser, "hooked anchor, serial")
    _assert_equal(_anchor(True), ser, "hooked anchor, side stream")


# ---- B: structure ----------------------------------------------------------------------------------------------------
def _tensors(obj, path):
    """(path, tensor) of every CUDA tensor inside an argument (lists and tuples walked)"""
    if isinstance(obj, torch.Tensor):
        return [(path, obj)] if obj.is_cuda else []
    if isinstance(obj, (list, tuple)):
        return [pt for i, o in enumerate(obj) for pt in _tensors(o, f"{path}[{i}]")]
    return []


def _detail(name, args, kwargs):
    """row set / number of G planes (which side_ctx site this is), and a WEAK reference to the memory of every tensor the
    launch was given: whatever a side-stream kernel reads must still be allocated when the main stream joins."""
    from torch.multiprocessing.reductions import StorageWeakRef
    d = {"mem": [(f"{name} {path}", StorageWeakRef(t.untyped_storage()))
                 for key, val in list(enumerate(args)) + sorted(kwargs.items()) for path, t in _tensors(val, f"arg {key}")]}
    if name == "gemm_tn_rows":
        d.update(row_set=int(args[1]), planes=len(args[6]))
    if name == "gemm_tn":
        d.update(planes=len(args[3]) if isinstance(args[3], (list, tuple)) else 1)
    return d


@pytest.mark.parametrize("flat", [False, True], ids=["autograd", "in_place"])
def test_backward_stream_structure(streams, monkeypatch, flat):
    """Side mode: all three side_ctx sites are reached; every run of side-stream launches is preceded, since the last
    main-stream launch, by side.wait_stream(main); the backward's last ordering call is main.wait_stream(side).  Main
    mode: nothing runs on, waits for or is awaited by the side stream."""
    main, side = streams
    M, S = main.cuda_stream, side.cuda_stream
    _serial(flat)                        # (outside the spy)
    from pose2mesh_release_amd import ops

    def freed_at_join(kind, a, b):
        """at main.wait_stream(side): operands of side-stream launches whose memory has already gone back to the allocator
        (the main stream's next allocation may overwrite it while the side stream has not read it yet)"""
        if (kind, a, b) != ("wait_stream", M, S):
            return None
        return [what for e in spy.launches() if e[1] == S and e[0] in SPIED for what, ref in e[2]["mem"] if ref.expired()]
    spy = sk.StreamSpy(monkeypatch, ops, SPIED + PRODUCERS, _detail, at_ordering=freed_at_join)
    mark = {}
    got = _anchor(True, flat=flat, after_forward=lambda: mark.setdefault("fwd", len(spy.events)),
                  before_backward=lambda: mark.setdefault("bwd", len(spy.events)))
    _assert_equal(got, _serial(flat), "spied side-stream run")
    ev = spy.events[mark["bwd"]:]
    # the backward ends at its join: what follows (the clones, the optimizer step) launches nothing that is spied
    joins = [i for i, e in enumerate(ev) if e[:3] == ("wait_stream", M, S)]
    assert joins, "no main.wait_stream(side) in the backward"
    bwd = ev[:joins[-1] + 1]
    launches = [e for e in bwd if e[0] not in spy.ORDERING]
    on_side = [e for e in launches if e[1] == S]
    assert all(e[1] in (M, S) for e in launches), {hex(e[1]) for e in launches}
    sites = {"paired (row set 3)": [e for e in on_side if e[0] == "gemm_tn_rows" and e[2]["row_set"] == 3],
             "split (row set 1)": [e for e in on_side if e[0] == "gemm_tn_rows" and e[2]["row_set"] == 1],
             "un-split (gemm_tn, 3 G planes)": [e for e in on_side if e[0] == "gemm_tn" and e[2]["planes"] == 3]}
    print("side_ctx sites reached:", {k: len(v) for k, v in sites.items()}, "| side launches", len(on_side),
          "| main launches", len(launches) - len(on_side))
    assert all(sites.values()), {k: len(v) for k, v in sites.items()}
    assert not [e for e in spy.events[:mark["bwd"]] if e[0] not in spy.ORDERING and e[1] == S], "side launch in the forward"
    # every launch on the side stream is ordered after everything main has been given so far
    ordered, runs = False, 0
    for e in bwd:
        if e[:3] == ("wait_stream", S, M):
            ordered = True
        elif e[0] in spy.ORDERING:
            continue
        elif e[1] == M:
            ordered = False
        else:
            assert ordered, f"{e} runs on the side stream with no side.wait_stream(main) since the last main-stream launch"
    for i, e in enumerate(bwd):
        runs += e[:3] == ("wait_stream", S, M)
    assert runs >= len(sites["paired (row set 3)"]) + len(sites["split (row set 1)"]) + len(sites["un-split (gemm_tn, 3 G planes)"])
    # the LAST ordering call of the backward is the join, and no weight-gradient launch follows it
    assert [e for e in ev if e[0] in ("wait_stream", "wait_event")][-1][:3] == ("wait_stream", M, S)
    assert not [e for e in ev[joins[-1] + 1:] if e[0] in SPIED], "weight-gradient launch after the join"
    # ... and everything the side stream was given to read is still allocated there (`keep`, or owned by someone who lives on)
    freed = [v for i, v in spy.probes if i == mark["bwd"] + joins[-1]][0]
    assert freed == [], f"freed before the join although the side stream reads them: {freed}"
    # in place: the unpack kernels ADD into the parameters' .grad on the side stream
    if flat:
        assert [e for e in on_side if e[0] in ("weight_grad_unpack", "weight_grad_unpack2")]
    # main mode
    spy.clear()
    got = _anchor(False, flat=flat)
    _assert_equal(got, _serial(flat), "spied serial run")
    assert not [e for e in spy.launches() if e[1] == S], "a launch on the side stream with DW_SIDE_STREAM off"
    assert not [e for e in spy.events if e[0] == "wait_stream" and S in e[1:3]], "a wait on the side stream with DW_SIDE_STREAM off"
    assert len(spy.launches()) == len([e for e in spy.launches() if e[1] == M]) > 0


# ---- C: side stream late ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [1, 2], ids=["one_backward", "two_backwards_accumulate"])
@pytest.mark.parametrize("flat", [False, True], ids=["autograd", "in_place"])
def test_side_stream_late(streams, flat, passes):
    """delay(side, D) right before every backward(): the gradients read on main as soon as backward() returns are the
    serial ones (the join), also accumulated in place into FlatAdam.flat_grad, also over two backwards with no zero_grad
    (the second one's side-stream adds come after the first one's)."""
    main, side = streams
    D, _ = _anchor_delays()
    ref = _serial(flat, passes)
    got = _anchor(True, flat=flat, passes=passes, before_backward=lambda: sk.delay(side, D))
    print(f"side late: D = {D:.2f} ms x {passes}, spun {sk.spent_ms():.1f} ms in this test")
    _assert_equal(got, ref, f"side stream {D:.1f} ms late")
    if passes == 2:
        assert not torch.equal(ref["grad::cl.5.weight"], _serial(flat, 1)["grad::cl.5.weight"])


# ---- D: main stream late ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flat", [False, True], ids=["autograd", "in_place"])
def test_main_stream_late(streams, monkeypatch, flat):
    """delay(main, d) in front of every bn_relu_bwd / conv_split / conv_pair of the backward: the side stream may only
    read what main has produced (side.wait_stream(main) at every side_ctx entry, the `keep` list)."""
    main, side = streams
    _, d = _anchor_delays()
    ref = _serial(flat)
    count, arm = _late_main(monkeypatch, main, d)
    got = _anchor(True, flat=flat, before_backward=arm)
    print(f"main late: d = {d:.2f} ms x {count[0]} producers, spun {sk.spent_ms():.1f} ms in this test")
    assert count[0] >= 14                # one BatchNorm backward per conv in front of a BatchNorm, at the least
    _assert_equal(got, ref, f"main stream {d:.1f} ms late per producer")


# ---- E: amax chunk across streams ------------------------------------------------------------------------------------
def _spy_amax(monkeypatch, log):
    """Every ops.new_amax draw as (current stream handle, the chunk's buffer, index of the word in it).  The buffer OBJECT is
    kept in the log: its identity names the chunk."""
    from pose2mesh_release_amd import ops
    real = ops.new_amax

    def new_amax(device):
        w = real(device)
        key = torch.device(device).index
        ent = ops._amax_chunks[torch.cuda.current_device() if key is None else key]
        log.append((torch.cuda.current_stream().cuda_stream, ent[0], ent[1] - 1))
        return w
    monkeypatch.setattr(ops, "new_amax", new_amax)
    return real


def _draw(new_amax, k):
    dev = torch.device("cuda", torch.cuda.current_device())
    for _ in range(k):
        new_amax(dev)


def _crossings(log, M, S):
    """chunks created (word 0 drawn) while the side stream was current and drawn from on main afterwards"""
    out = []
    for i, (st, buf, idx) in enumerate(log):
        if idx == 0 and st == S and any(b is buf and s == M for s, b, _ in log[i + 1:]):
            out.append(i)
    return out


def _amax_sweep(monkeypatch, M, S):
    """The sweep, from the draws of one unskewed side-stream run (nf words drawn by the forward, nb by the backward):
    slot -> (k words drawn on main between forward and backward, words drawn after them with the SIDE stream current).
      bwd_first / bwd_middle / bwd_last   k = 256 - nf - j: the chunk rolls over at the backward's own draw number j
      rolled_on_side                      k = 256 - nf fills the chunk, one more word is drawn with the side stream current:
                                          the new chunk is created and zeroed THERE (behind the delay when the side stream
                                          is late) and every word the backward draws on main comes out of it
    In this configuration the backward itself draws every word on the MAIN stream (the operands of the weight-gradient
    launches come tagged, or their words are passed in): its own draws cannot create a chunk on the side stream, whatever
    k - the positions are printed and recorded - which is why the side-stream rollover is made by the test."""
    if "sweep" in _cache:
        return _cache["sweep"]
    from pose2mesh_release_amd import ops
    assert ops.f16x2(), "scenario E is about the default arithmetic"
    log, mark = [], {}
    with monkeypatch.context() as mp:
        _spy_amax(mp, log)
        _anchor(True, after_forward=lambda: mark.setdefault("nf", len(log)))
    nf = mark["nf"]
    bwd = [st for st, _, _ in log[nf:]]
    nb = len(bwd)
    assert 0 < nf < AMAX_WORDS - nb and nb >= 3 and all(idx == i for i, (_, _, idx) in enumerate(log)), (nf, nb)
    on_side = [j for j, st in enumerate(bwd) if st == S]
    print(f"amax draws: forward {nf}, backward {nb}, of these with the side stream current: {on_side}")
    full = AMAX_WORDS - nf
    sweep = {"rolled_on_side": (full, 1), "bwd_first": (full, 0), "bwd_middle": (full - nb // 2, 0),
             "bwd_last": (full - (nb - 1), 0)}
    for j in on_side[:1] + on_side[-1:]:            # (none today) the backward's own side-stream draws, when it has any
        sweep[f"bwd_side_draw_{j}"] = (full - j, 0)
    _cache["sweep"] = (sweep, nf, nb, on_side)
    return _cache["sweep"]


E_SLOTS = ("rolled_on_side", "bwd_first", "bwd_middle", "bwd_last")


def _pre_draw(spied_new_amax, real_new_amax, side, k, on_side):
    _draw(real_new_amax, k)
    with torch.cuda.stream(side):
        _draw(spied_new_amax, on_side)


def test_amax_sweep_reaches_a_side_stream_chunk_drawn_on_main(streams, monkeypatch):
    """For at least one entry of the sweep the spy shows a chunk created while the side stream is current and a later word
    of it drawn on main - the case the event in ops.new_amax exists for.  Unskewed, every entry: the serial bits."""
    from pose2mesh_release_amd import ops
    main, side = streams
    M, S = main.cuda_stream, side.cuda_stream
    sweep, nf, nb, on_side = _amax_sweep(monkeypatch, M, S)
    hits = {}
    for slot, (k, ks) in sweep.items():
        log = []
        with monkeypatch.context() as mp:
            real = _spy_amax(mp, log)
            got = _anchor(True, after_forward=lambda: _pre_draw(ops.new_amax, real, side, k, ks))
        _assert_equal(got, _serial(), f"amax sweep, {slot} (k = {k}), unskewed")
        cross = _crossings(log, M, S)
        hits[slot] = {"k": k, "drawn_on_side": ks, "chunks": len({id(b) for _, b, _ in log}),
                      "main_draws_from_side_chunk": sum(b is log[i][1] and s == M for i in cross for s, b, _ in log[i + 1:])}
    print(f"amax sweep: {hits}")
    _record("amax", forward_draws=nf, backward_draws=nb, backward_draws_on_side=on_side, sweep=hits)
    assert all(h["chunks"] == 2 for h in hits.values()), hits
    assert any(h["main_draws_from_side_chunk"] for h in hits.values()), (
        f"no entry of the sweep shows a chunk created on the side stream with a later draw on main: {hits} - scenario E "
        f"does not bite in this configuration")
    assert hits["rolled_on_side"]["main_draws_from_side_chunk"] == nb


@pytest.mark.parametrize("skew", ["side_late", "main_late"])
@pytest.mark.parametrize("slot", E_SLOTS)
def test_amax_chunk_rolls_over_under_skew(streams, monkeypatch, slot, skew):
    """Words drawn between forward and backward so that the 256-word chunk rolls over during the backward (three positions),
    or on the side stream right before it with the backward drawing all its words from that chunk on main - under skew C
    (the side stream D late: the zeroing of a chunk created there is late too) and under skew D (main late): the serial
    bits.  A word that is not zero when its kernel accumulates into it - or that is zeroed afterwards - scales the fp16
    slices differently."""
    from pose2mesh_release_amd import ops
    main, side = streams
    M, S = main.cuda_stream, side.cuda_stream
    D, d = _anchor_delays()
    k, ks = _amax_sweep(monkeypatch, M, S)[0][slot]
    ref = _serial()
    log = []
    real = _spy_amax(monkeypatch, log)

    def pre_draw():
        _pre_draw(ops.new_amax, real, side, k, ks)
    if skew == "side_late":
        got = _anchor(True, after_forward=lambda: sk.delay(side, D), before_backward=pre_draw)
    else:
        count, arm = _late_main(monkeypatch, main, d)
        got = _anchor(True, after_forward=pre_draw, before_backward=arm)
    chunks, cross = len({id(b) for _, b, _ in log}), _crossings(log, M, S)
    print(f"amax {slot}, {skew}: k = {k} + {ks} on the side stream, {chunks} chunks, chunks created on the side stream and "
          f"drawn from on main: {len(cross)}, spun {sk.spent_ms():.1f} ms")
    assert chunks == 2, "the chunk did not roll over exactly once"
    assert bool(cross) == (slot == "rolled_on_side")
    _assert_equal(got, ref, f"amax {slot} (k = {k} + {ks}), {skew}")


# ---- F: graphed train step with refreshed inputs --------------------------------------------------------------------
def _train_sequence(graphed, d=None, side=None, timing=None, late=None):
    """The 6-step sequence of test_graphed_train_step_is_bitwise_the_eager_loop (MANO, B = 6, FlatAdam, 3 warm-ups,
    capture, replays, the lr change) with x.copy_(batch[i]) before EVERY step, six different batches, on the current
    stream.  graphed + d: every step has a spin of d on the caller's stream before the copy, on the step's private
    stream while it is still used, and on the weight-gradient stream; late(): called before steps 1 and 5 (each is
    preceded by a device synchronisation: the set-up's and the capture's).  No host synchronisation between the steps."""
    import helpers
    from pose2mesh_release_amd import meshnet, optim, train
    cur = torch.cuda.current_stream()
    gL, _, _ = helpers.golden_graphs("mano")
    B, J = 6, int(gL[-1].shape[0])
    batches = [helpers.meshnet_input(B, J, seed=40 + i).cuda() for i in range(6)]
    x = torch.zeros_like(batches[0])
    w = torch.randn(B, gL[0].shape[0], 3, generator=torch.Generator().manual_seed(1)).cuda()
    net = meshnet.get_model(5, 3, gL, mano=True)
    net.load_state_dict(helpers.numpy_state(net.state_dict(), 3))
    net = net.cuda().train()
    opt = optim.FlatAdam(net.parameters(), lr=1e-3)
    net.accumulate_grads_in_place(True)

    def loss_fn():
        return (net(x) * w).sum() * 1e-3

    torch.cuda.synchronize()
    losses, host, evs = [], [], [torch.cuda.Event(enable_timing=True) for _ in range(7)]
    step = train.GraphedTrainStep(net, opt, loss_fn, warmup=3) if graphed else None
    for i in range(6):
        t0 = time.perf_counter()
        evs[i].record()
        if i == 4:
            opt.param_groups[0]["lr"] = 1e-4
        if late is not None and i in (0, 4):
            late()
        if graphed:
            if d is not None:
                sk.delay(cur, d)
            x.copy_(batches[i])
            if d is not None:
                if step.graph is None:
                    sk.delay(step.stream, d)
                sk.delay(side, d)
            losses.append(step().clone())
        else:
            x.copy_(batches[i])
            opt.zero_grad()
            loss = loss_fn()
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        host.append((time.perf_counter() - t0) * 1e3)
    evs[6].record()
    torch.cuda.synchronize()
    if graphed:
        assert step.graph is not None and step.calls == 6
    if timing is not None:            # the median of the last three steps
        ts = [dict(host_ms=host[i], device_ms=evs[i].elapsed_time(evs[i + 1]),
                   t_step_ms=max(host[i], evs[i].elapsed_time(evs[i + 1]))) for i in (3, 4, 5)]
        timing.update(_median(ts))
    return {"losses": torch.stack(losses), "flat_param": opt.flat_param.clone(),
            **{f"moment::{k}": b.clone() for k, b in opt._bufs.items()},
            **{f"state::{k}": v.clone() for k, v in net.state_dict().items() if "running" in k or "tracked" in k}}


def _train_reference():
    if "train" not in _cache:
        t = {}
        ref = _train_sequence(False, timing=t)
        print(f"train step: host {t['host_ms']:.3f} ms, device {t['device_ms']:.3f} ms (median of the last three eager steps)")
        _cache["train"] = (ref, _delays("train_step", t["t_step_ms"]))
    return _cache["train"]


@pytest.mark.parametrize("caller", ["default_stream", "own_stream"])
def test_graphed_train_step_with_refreshed_inputs_under_skew(streams, caller):
    """The eager unskewed loop against the graphed run with every stream of the hand-off delayed: losses, flat_param, the
    moments and the running statistics, bit for bit.  own_stream: the caller works inside torch.cuda.stream(s), with s
    biting against the default stream, and the default stream is D late - nothing of the step may sit on it."""
    main, side = streams
    ref, (D, d) = _train_reference()
    assert len({float(v) for v in ref["losses"]}) == 6          # six different batches: a stale input would show
    if caller == "default_stream":
        got = _train_sequence(True, d=d, side=side)
    else:
        s = sk.distinct_stream(main)
        assert sk.bites(main, s) and sk.bites(s, main), sk.last_bite
        print(f"bites(default, s {s.cuda_stream:#x}) and bites(s, default): True")
        with torch.cuda.stream(s):
            got = _train_sequence(True, d=d, side=side, late=lambda: sk.delay(main, D))
    print(f"graphed train step, {caller}: d = {d:.2f} ms, spun {sk.spent_ms():.1f} ms in this test")
    _assert_equal(got, ref, f"graphed train step under skew ({caller})")


# ---- G: graphed inference --------------------------------------------------------------------------------------------
def _infer_sequence(D=None, default=None, timing=None):
    """Three calls with three inputs on the CURRENT stream; between call 2 and call 3 one interior weight is edited in
    place, which forces the re-capture path and its warm-up stream.  D: the default stream is D late during the calls."""
    import helpers
    import numpy as np
    from pose2mesh_release_amd import infer, pose2mesh_net, synth
    gL, _, rev = helpers.golden_graphs("mano")
    J, nv, B = int(gL[-1].shape[0]), 778, 3
    net = pose2mesh_net.get_model(J, gL, mano=True)
    net.load_state_dict(helpers.numpy_state(net.state_dict(), 2))
    net = net.cuda().eval()
    xs = [synth.pose2d_batch(B, J, seed=s).cuda() for s in (7, 8, 9)]
    interior = dict(net.named_parameters())["pose2mesh.cl.7.weight"]
    step = infer.GraphedInference(net, np.asarray(rev), nv, synth.synthetic_regressor(J, nv), B, scale=1000.0)
    assert step.graph is not None and step.captures == 1
    torch.cuda.synchronize()
    out = {}
    for i, x in enumerate(xs):
        if i == 2:
            with torch.no_grad():
                interior.mul_(1.25)
        if D is not None and i in (0, 2):
            sk.delay(default, D)
        mesh, joints, pose3d = step(x)
        out.update({f"mesh{i}": mesh.clone(), f"joints{i}": joints.clone(), f"pose3d{i}": pose3d.clone()})
    torch.cuda.synchronize()
    assert step.captures == 2, step.captures
    if timing is not None:            # three more calls, plain replays: the median
        ts = []
        for _ in range(3):
            e0, e1, t0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), time.perf_counter()
            e0.record()
            step(xs[0])
            e1.record()
            host_ms = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            ts.append(dict(host_ms=host_ms, device_ms=e0.elapsed_time(e1), t_step_ms=max(host_ms, e0.elapsed_time(e1))))
        assert step.captures == 2
        timing.update(_median(ts))
    return out


def test_graphed_inference_on_the_callers_stream_under_skew(streams):
    """Caller inside torch.cuda.stream(s), default stream D late: input copy, replay, and the re-capture after an in-place
    weight edit (warm-up on yet another stream) give the mesh, joints and pose3d of a fresh unskewed GraphedInference."""
    main, side = streams
    t = {}
    ref = _infer_sequence(timing=t)
    print(f"inference call: host {t['host_ms']:.3f} ms, device {t['device_ms']:.3f} ms (a replay)")
    D, _ = _delays("inference_call", t["t_step_ms"])
    assert not torch.equal(ref["mesh0"], ref["mesh1"]) and not torch.equal(ref["mesh1"], ref["mesh2"])
    s = sk.distinct_stream(main)
    assert sk.bites(main, s) and sk.bites(s, main), sk.last_bite
    print(f"bites(default, s {s.cuda_stream:#x}) and bites(s, default): True")
    with torch.cuda.stream(s):
        got = _infer_sequence(D=D, default=main)
    _assert_equal(got, ref, "graphed inference under skew")


# ---- H: the control is a test too ------------------------------------------------------------------------------------
def test_the_control_bites_and_the_caps_hold(streams):
    main, side = streams
    assert sk.bites(main, side) and sk.last_bite == (0.0, 1024.0)
    assert sk.bites(side, main) and sk.last_bite == (0.0, 1024.0)
    assert not sk.bites(main, main)                          # one stream cannot run ahead of itself
    torch.cuda.synchronize()
    spent = sk.spent_ms()
    with pytest.raises(sk.SkewCapError):
        sk.delay(main, sk.CAP_CALL_MS + 1.0)
    with pytest.raises(sk.SkewCapError):
        sk.delay(main, 0.0)
    assert sk.spent_ms() == spent and main.query()              # raised on the host, nothing was enqueued
    sk._spent_ms = sk.CAP_TEST_MS - 5.0                         # (booked, not spun) the per-test sum: 5 ms are left
    with pytest.raises(sk.SkewCapError):
        sk.delay(main, 10.0)
    assert sk.spent_ms() == sk.CAP_TEST_MS - 5.0 and main.query()
    sk.delay(main, 5.0)
    assert sk.spent_ms() == sk.CAP_TEST_MS
    torch.cuda.synchronize()
    cpm = sk.calibrate()
    assert cpm > 0 and cpm == sk.calibrate()
