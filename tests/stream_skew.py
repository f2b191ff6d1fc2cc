"""Helper (not a pytest file): skew GPU streams against each other ON PURPOSE, with bounded spins, so that a missing
wait between two streams shows as wrong bits instead of hiding behind "the producer happened to finish first".

  calibrate()             spin cycles per millisecond of torch.cuda._sleep (a bounded spin kernel, not a hang)
  delay(stream, ms)       one spin of `ms` on `stream`; capped per call and per test (reset_budget), checked on the host
                          BEFORE anything is enqueued
  bites(a, b, ms)         the control, torch ops on live memory only: does a delay on b really let a run ahead of it?
                          (streams come from a pool and the process has a handful of hardware queues: two stream objects
                          can share a queue, the delay then stalls both and a skew test would pass vacuously)
  distinct_stream(other)  a new stream for which bites holds in both directions against `other`
  StreamSpy               pass-through recorder of wait_stream / wait_event / Event.record and of named ops functions

Nothing here touches a queue or runtime setting, and nothing reads memory that is not live."""
import math
import threading

import torch

CAP_CALL_MS = 250.0          # one delay() call
CAP_TEST_MS = 3000.0         # all delay() calls between two reset_budget() calls (one test)
CONTROL_MS = 10.0            # the delay bites() injects

_cycles_per_ms = None
_spent_ms = 0.0
last_bite = None             # (sum of the snapshot, sum of the tensor) of the most recent bites() call


class SkewCapError(RuntimeError):
    """A delay beyond the caps was asked for; nothing was enqueued."""


def reset_budget():
    global _spent_ms
    _spent_ms = 0.0


def spent_ms():
    return _spent_ms


def calibrate(force=False):
    """Cycles of torch.cuda._sleep per millisecond, from HIP events around a spin (run twice, the second timing counts;
    the spin is lengthened until it lasts 2 ms so that the event resolution does not matter).  Synchronises the host:
    call it before any skew is in flight.  Cached per process."""
    global _cycles_per_ms
    if _cycles_per_ms is not None and not force:
        return _cycles_per_ms
    n, seen, ms = 2_000_000, [], float("nan")
    for _ in range(6):
        for _rep in range(2):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            torch.cuda._sleep(n)
            e.record()
            e.synchronize()
            ms = s.elapsed_time(e)
        seen.append((n, ms))
        if not (math.isfinite(ms) and ms > 0.0) or ms >= 2.0:
            break
        n *= 8
    cpm = n / ms if (math.isfinite(ms) and ms > 0.0) else float("nan")
    assert math.isfinite(cpm) and cpm > 0.0, f"torch.cuda._sleep could not be calibrated: (cycles, ms) = {seen}"
    _cycles_per_ms = cpm
    return cpm


def delay(stream, ms):
    """Enqueue one bounded spin of `ms` milliseconds on `stream`."""
    global _spent_ms
    ms = float(ms)
    if not (0.0 < ms <= CAP_CALL_MS):
        raise SkewCapError(f"delay of {ms:.3f} ms: one call may spin for at most {CAP_CALL_MS:.0f} ms")
    if _spent_ms + ms > CAP_TEST_MS:
        raise SkewCapError(f"delay of {ms:.3f} ms after {_spent_ms:.3f} ms: one test may spin for at most "
                           f"{CAP_TEST_MS:.0f} ms in all")
    cycles = max(1, int(ms * calibrate()))
    _spent_ms += ms
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


def bites(a, b, ms=CONTROL_MS):
    """True when a delay on b lets a run ahead of it: b spins, then adds 1 to a tensor that a snapshots meanwhile with
    no wait in between.  The snapshot is all zeros (a did not wait for b) and the tensor ends as all ones."""
    global last_bite
    with torch.cuda.stream(a):
        t = torch.zeros(1024, device=a.device)
    delay(b, ms)
    with torch.cuda.stream(b):
        t.add_(1)
    with torch.cuda.stream(a):
        snap = t.clone()
    a.synchronize()
    b.synchronize()
    last_bite = (float(snap.sum()), float(t.sum()))
    return last_bite == (0.0, 1024.0)


def distinct_stream(other, tries=8):
    """A torch.cuda.Stream against which `other` can really be skewed, in both directions."""
    seen = []
    for _ in range(tries):
        s = torch.cuda.Stream(device=other.device)
        ab = bites(other, s)
        ev_ab = last_bite
        ba = bites(s, other)
        seen.append((hex(s.cuda_stream), ab, ev_ab, ba, last_bite))
        if ab and ba:
            return s
    raise AssertionError(f"no stream out of {tries} can be skewed against {hex(other.cuda_stream)}: "
                         f"(stream, bites(other, s), sums, bites(s, other), sums) = {seen}")


class StreamSpy:
    """Records, in call order, into .events:
        ("wait_stream", waiting stream handle, awaited stream handle)
        ("wait_event", waiting stream handle, id of the event)
        ("record", stream handle, id of the event)
        (name, current stream handle, detail)        for every function `name` of `module` listed in `names`
    Only the outermost ordering call is recorded (torch's wait_stream is itself a record + wait_event); a function is
    recorded when it is entered.  detail(name, args, kwargs) -> anything; default None.  at_ordering(kind, a, b) -> anything:
    called at every recorded ordering call, BEFORE it is passed on; what it returns is appended to .probes as (index of
    the event, value) - e.g. which tensors are still alive at a join.  Every call is passed through unchanged."""

    ORDERING = ("wait_stream", "wait_event", "record")

    def __init__(self, monkeypatch, module=None, names=(), detail=None, at_ordering=None):
        self.events, self.probes = [], []
        self._tls = threading.local()          # the backward runs on autograd's thread
        spy = self

        def outermost(kind, handles, call):
            depth = getattr(spy._tls, "depth", 0)
            if depth == 0:
                spy.events.append((kind,) + handles())
                if at_ordering is not None:
                    spy.probes.append((len(spy.events) - 1, at_ordering(*spy.events[-1])))
            spy._tls.depth = depth + 1
            try:
                return call()
            finally:
                spy._tls.depth = depth

        real_ws, real_we = torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event
        real_rec = torch.cuda.Event.record

        def wait_stream(st, other):
            return outermost("wait_stream", lambda: (st.cuda_stream, other.cuda_stream), lambda: real_ws(st, other))

        def wait_event(st, event):
            return outermost("wait_event", lambda: (st.cuda_stream, id(event)), lambda: real_we(st, event))

        def record(ev, stream=None):
            return outermost("record", lambda: ((torch.cuda.current_stream() if stream is None else stream).cuda_stream, id(ev)),
                             lambda: real_rec(ev) if stream is None else real_rec(ev, stream))

        monkeypatch.setattr(torch.cuda.Stream, "wait_stream", wait_stream)
        monkeypatch.setattr(torch.cuda.Stream, "wait_event", wait_event)
        monkeypatch.setattr(torch.cuda.Event, "record", record)
        for name in names:
            monkeypatch.setattr(module, name, self._wrap(name, getattr(module, name), detail))

    def _wrap(self, name, real, detail):
        def wrapped(*args, **kwargs):
            self.events.append((name, torch.cuda.current_stream().cuda_stream,
                                detail(name, args, kwargs) if detail is not None else None))
            return real(*args, **kwargs)
        wrapped.__name__ = name
        return wrapped

    def clear(self):
        del self.events[:]
        del self.probes[:]

    def launches(self):
        return [e for e in self.events if e[0] not in self.ORDERING]
