"""Helper of tests/test_gpu_stream_order.py (no tests here): the checks of the stream sentence of the conventions
block of include/videoprism_hip.h -- a call is asynchronous on `stream`, never allocates, never synchronises, and
the handle-level calls can be captured into a hipGraph.

A `Case` is one call (or a fixed chain of calls) with every device buffer it touches owned by the test:

  inputs    {name: device buffer the call reads}
  x, x_alt  {name: staging tensor of the same shape and dtype}: the inputs X the case is judged on, and different
            inputs X' of the same shape
  outputs   the caller-owned output tensors (empty where the call allocates and returns its own)
  scratch   scratch() -> the workspaces the call uses
  call      call(stream) -> tuple of output tensors (None where absent): makes the call on the torch stream `stream`
            and returns as soon as the entry point does

Contract 1, `check_deferred` (deferred inputs), on a non-blocking side stream `side`:
  1. expected: deliver X, call, synchronise, keep the outputs
  2. the same on X': whatever the call leaves in a handle or a workspace is now wrong for X.  This second, warmed
     call is the one whose host wall time is measured
  3. poison: every input, output and workspace byte becomes 0xFF (NaN in fp32 and bf16, -1 in int32 / int64, 255 in
     uint8: by contract no entry point reads out of bounds on such inputs), then a device synchronise
  4. on `side`: a delay, then device-to-device copies of X into the inputs, then an event `gate`
  5. the call on `side`; the moment it returns, `gate` must not have happened yet
  6. side.synchronize(); every output must equal step 1's bit for bit
Step 5 fails if the call waited for the stream in any way (a synchronise, a blocking copy, a host read of device
data, a free) and also if the delay was too short to tell: a short delay fails, it never passes.  Step 6 fails if
any launch, memset or copy went to another stream: it ran during the delay, on poison or ahead of its producer, and
nothing rewrites what it wrote.  The expected outputs of steps 1 and 2 must be finite: two NaN results are equal bit
for bit, and a library that is wrong in the ordinary call too must not pass that way.

Contract 2, `check_capture` (capture and replay), after contract 1 has warmed the call (the first call on a device
sets kernel attributes): the call is captured with torch.cuda.graph(g, stream=side) -- default global error mode, one
capture stream, one linear chain, no environment variable involved -- with X in the inputs; then the inputs become
X', outputs and workspaces are poisoned, the graph is replayed once on `side`, and every output must equal step 2's.
A call that allocates, frees, synchronises or launches on the legacy stream while capturing makes the capture
refuse: that arrives here as a Python exception, reported with the library's vp_last_error() text.  A value read on
the host at capture time and baked into a launch shows as a mismatch after the replay.  On this runtime (ROCm 7.0) a
refused capture does not end cleanly: hipStreamEndCapture reports hipErrorStreamCaptureInvalidated and the next
blocking copy of the process (a .to(device) of a host tensor) still fails with hipErrorStreamCaptureUnsupported.  A
refusal is a failing suite anyway, but the permanent control for it cannot share a process with other tests: running
this file as a program is that control (`python tests/stream_order.py` prints the failures of a stand-in that
synchronises the device), and the test starts it as a child.

The delay is torch.cuda._sleep, calibrated once per process in cycles per millisecond between two events (and
checked for linearity; were it unusable on this runtime, a chain of 2048 x 2048 fp32 torch.mm calls calibrated the
same way takes its place).  Its length per case is DELAY_MULTIPLE = 50 times the measured host time of the warmed
ordinary call, but at least DELAY_FLOOR_MS = 50 ms (the handful of copies and the event that are enqueued between
the delay and the call cost host time too, and the host thread may lose its CPU for a while on a shared machine) and at most DELAY_CEIL_MS = 500 ms: the entry points enqueue in well
under a millisecond each, so a case's delay is tens of milliseconds.

`side` is torch.cuda.Stream(): hipStreamNonBlocking, so the legacy default stream does not order itself against it.
tests/test_gpu_stream_order.py::test_harness_sees_a_launch_on_another_stream depends on exactly that and proves it
on every run.
"""

import functools
import time

import torch

import workspace_guard as wg
from videoprism import _native as nat

POISON = 0xFF
DELAY_MULTIPLE = 50
DELAY_FLOOR_MS = 50.0
DELAY_CEIL_MS = 500.0


class Case:
    def __init__(self, label, inputs, x, x_alt, outputs, scratch, call, capture=False):
        assert set(inputs) == set(x) == set(x_alt), label
        for n, buf in inputs.items():
            for src in (x[n], x_alt[n]):
                assert buf.is_contiguous() and src.shape == buf.shape and src.dtype == buf.dtype, (label, n)
                assert src.data_ptr() != buf.data_ptr() or buf.numel() == 0, (label, n)
        assert all(t.is_contiguous() for t in outputs), label
        self.label, self.inputs, self.x, self.x_alt = label, inputs, x, x_alt
        self.outputs, self.scratch, self.call, self.capture = list(outputs), scratch, call, capture


def staged(x, alt=None):
    """(buffer, X, X') for one input: X is `x`, X' is `alt` or `x` rolled by about half its length (by one element
    where it is tiny), the buffer is fresh memory of the same shape."""
    x = x.contiguous()
    if alt is None:
        alt = x.reshape(-1).roll(max(1, x.numel() // 2 - 1)).reshape(x.shape).contiguous()
    return torch.empty_like(x), x, alt.contiguous()


def case_from(label, named, outputs, scratch, call, capture=False):
    """A Case from {name: staged(...)} triples."""
    return Case(label, {n: t[0] for n, t in named.items()}, {n: t[1] for n, t in named.items()},
                {n: t[2] for n, t in named.items()}, outputs, scratch, call, capture)


def stream_ptr(stream):
    return nat._stream(stream)


# ---------------------------------------------------------------------------------------------------------------
# the delay
# ---------------------------------------------------------------------------------------------------------------
def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class Delay:
    """enqueue(ms) puts about `ms` milliseconds of device time on the current stream."""

    def __init__(self, kind, per_ms, note):
        self.kind, self.per_ms, self.note = kind, per_ms, note
        self._m = torch.ones(2048, 2048, device="cuda") if kind == "mm" else None

    def enqueue(self, ms):
        if self.kind == "sleep":
            torch.cuda._sleep(int(ms * self.per_ms))
        else:
            for _ in range(max(1, int(ms * self.per_ms + 1))):
                torch.mm(self._m, self._m)


@functools.lru_cache(maxsize=None)
def delay_source():
    """The calibrated delay of this process: torch.cuda._sleep if 5 ms asked for come out as 2.5 .. 10 ms, else the
    torch.mm chain."""
    try:
        torch.cuda._sleep(1000)  # loads the kernel
        first = _timed(lambda: torch.cuda._sleep(1_000_000))
        per_ms = 1_000_000 / max(first, 1e-3)
        second = _timed(lambda: torch.cuda._sleep(int(5 * per_ms)))
        if 2.5 <= second <= 10.0:
            return Delay("sleep", 5 * per_ms / second,
                         f"torch.cuda._sleep: {5 * per_ms / second:.0f} cycles per ms (1e6 cycles took {first:.3f} ms, "
                         f"5 ms asked for took {second:.3f} ms)")
        why = f"torch.cuda._sleep is not linear here ({first:.3f} ms for 1e6 cycles, then {second:.3f} ms for 5 ms)"
    except (AttributeError, RuntimeError) as e:
        why = f"torch.cuda._sleep is unusable here ({e})"
    d = Delay("mm", 1.0, "")
    d.enqueue(1)
    each = _timed(lambda: d.enqueue(19)) / 20
    d.per_ms = 1.0 / each
    d.note = f"{why}; a chain of 2048^3 fp32 torch.mm calls instead, {each:.3f} ms each"
    return d


def delay_ms(host_seconds):
    return min(DELAY_CEIL_MS, max(DELAY_FLOOR_MS, DELAY_MULTIPLE * host_seconds * 1e3))


# ---------------------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------------------
def _deliver(case, which, side):
    with torch.cuda.stream(side):
        for n, buf in case.inputs.items():
            buf.copy_(which[n], non_blocking=True)


def _poison(tensors):
    for t in tensors:
        if t is not None and t.numel():
            assert t.is_contiguous()
            wg.as_bytes(t).fill_(POISON)


def _ordinary(case, which, side):
    """Deliver, synchronise, call, synchronise -> (copies of the outputs, host seconds the call took)."""
    _deliver(case, which, side)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = case.call(side)
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return tuple(None if t is None else t.clone() for t in outs), host


def _differences(what, got, want):
    assert len(got) == len(want), (len(got), len(want))
    out = []
    for i, (a, b) in enumerate(zip(got, want)):
        d = wg.first_difference(a, b)
        if d:
            out.append(f"{what}: output {i}: {d}")
    return out


def _vacuous(what, outs):
    """Two NaN results are equal bit for bit: an expected output that is not finite would compare nothing."""
    return [f"values: {what}: output {i} of the ordinary call holds non-finite values"
            for i, t in enumerate(outs) if t is not None and not wg.all_finite(t)]


def check_deferred(case, side):
    """Contract 1 -> (failures, expected outputs for X, expected outputs for X', text for the record).  A failure
    starts with 'gate:' (step 5) or 'values:' (step 6, or an ordinary call whose own outputs are not finite)."""
    delay = delay_source()
    want, _ = _ordinary(case, case.x, side)
    want_alt, host = _ordinary(case, case.x_alt, side)
    vacuous = _vacuous("on X", want) + _vacuous("on X'", want_alt)
    _poison(list(case.inputs.values()) + case.outputs + list(case.scratch()))
    torch.cuda.synchronize()
    ms = delay_ms(host)
    gate = torch.cuda.Event()
    with torch.cuda.stream(side):
        delay.enqueue(ms)
    _deliver(case, case.x, side)
    gate.record(side)
    outs = case.call(side)
    passed = gate.query()
    side.synchronize()
    torch.cuda.synchronize()
    failures = vacuous
    if passed:
        failures.append(f"gate: the inputs had already been delivered when the call returned: it waited for the "
                        f"stream, or {ms:.1f} ms of delay were too short to tell (the ordinary call took "
                        f"{host * 1e3:.3f} ms on the host)")
    failures += _differences("values: deferred inputs against an ordinary call", outs, want)
    return failures, want, want_alt, f"host {host * 1e3:.3f} ms, delay {ms:.1f} ms"


def _chain(e):
    """The text of an exception and of those it replaced (a failed capture raises again when it is ended)."""
    parts = []
    while e is not None and len(parts) < 3:
        parts.append(f"{type(e).__name__}: {' '.join(str(e).split())[:300]}")
        e = e.__context__
    return " <- ".join(parts)


def check_capture(case, side, want_alt):
    """Contract 2 -> failures, each starting with 'capture:' (refused) or 'values:' (replayed to other bits)."""
    _deliver(case, case.x, side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=side):
            outs = case.call(side)
    except Exception as e:  # noqa: BLE001  (a refused capture is whatever torch or the wrapper raises)
        last = nat.load().vp_last_error().decode("utf-8", "replace")
        del graph
        torch.cuda.synchronize()
        return [f"capture: refused: {_chain(e)}; vp_last_error: {last!r}"]
    _deliver(case, case.x_alt, side)
    with torch.cuda.stream(side):
        _poison(case.outputs + list(case.scratch()))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        graph.replay()
    side.synchronize()
    torch.cuda.synchronize()
    failures = _differences("values: replay on new inputs against an ordinary call", outs, want_alt)
    del graph
    return failures


def torch_stand_in(device, what, body, capture=False):
    """A stand-in "entry point" made of torch ops: body(stream, x, tmp, out) computes out = 2 (x + 1) through tmp."""
    x = torch.randn(1024, generator=torch.Generator().manual_seed(20)).to(device)
    named = dict(x=staged(x))
    tmp, out = torch.empty_like(x), torch.empty_like(x)

    def call(stream):
        body(stream, named["x"][0], tmp, out)
        return (out,)

    return case_from(f"stand-in, {what}", named, [out], lambda: [tmp], call, capture)


def check_case(case, side):
    """Contract 1 and, for a case marked `capture`, contract 2; prints the case's record -> all failures."""
    failures, _, want_alt, note = check_deferred(case, side)
    if case.capture:
        failures += check_capture(case, side, want_alt)
    print(f"{case.label}: {note}, deferred inputs{' + capture and replay' if case.capture else ''}: "
          f"{'no difference' if not failures else f'{len(failures)} failures'}")
    for f in failures:
        print(f"    {f}")
    return failures


if __name__ == "__main__":  # the control for a refused capture, in a process of its own (see the docstring)
    import json
    import os
    import sys

    def _syncs_the_device(stream, x, tmp, out):
        with torch.cuda.stream(stream):
            torch.add(x, 1.0, out=tmp)
            torch.mul(tmp, 2.0, out=out)
        torch.cuda.synchronize()  # legal, if slow, on a stream; refused while the stream is capturing

    _dev = torch.device("cuda:0")
    _found = check_case(torch_stand_in(_dev, "device synchronise before returning", _syncs_the_device, capture=True),
                        torch.cuda.Stream(_dev))
    print("FAILURES " + json.dumps(_found))
    sys.stdout.flush()
    os._exit(0)  # no teardown in a process whose capture was refused
