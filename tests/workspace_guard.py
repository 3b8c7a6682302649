"""Helper of tests/test_gpu_workspace.py (no tests here): a workspace of exactly the advertised size between two
guard bands, the fills it is poisoned with, and the checks of the workspace contract (include/videoprism_hip.h,
conventions) that every entry point taking a workspace must hold:

  1. sufficient         called with exactly `need` bytes, nothing outside [ws, ws + need) is written
  2. refused when short with need - 1 bytes: VP_EINVAL before the first launch, outputs untouched, the message names
                        the same `need`
  3. contents ignored   every output is bit for bit the same whatever the workspace held on entry
  4. meaningful run     every output value is finite (two NaN tensors are equal too)

One device buffer of GUARD + need + GUARD uint8; the workspace is the middle slice, so it is 256-byte aligned and its
numel() is exactly `need`.  The whole buffer is filled with one byte value before each run; after the run and a
synchronize both guards must still hold that byte everywhere.

The entry points are reached the way callers reach them: the handle-based ones through the Python engines, whose
cached workspace `engine._ws[key]` is seeded with the slice, the stateless ops through their `ws=` argument.  All of
them hand (ws, ws_bytes, stream) to `_native.call` as the last three arguments; `watch` sits on that function, asserts
that the slice is what arrives at the C call, and keeps the argument list, which `check_refusal` replays one byte
short.  A helper built with shrink=1 advertises need - 1 bytes for the same slice: the negative control, under which
every case must take the refusal path instead of running.
"""

import contextlib
import ctypes

import torch

from videoprism import _native as nat

GUARD = 1 << 20  # bytes on each side of the workspace; a multiple of 256
assert GUARD % 256 == 0

# zeros; NaN in bf16 and fp32, -1 as an integer; 3.39e38 in both float types (finite, overflows in any sum); and the
# leftovers of a differently shaped call of the same entry point (what the grow-only engines start on)
FILLS = (0x00, 0xFF, 0x7F, "stale")
STALE_BYTE = 0x5A      # under the stale call, and in the guards around it
OUTPUT_BYTE = 0xA5     # outputs before a refused call, and the bands behind caller-owned outputs


def workspace_need(query, handle, *dims):
    """What `query`(handle, *dims, &bytes) reports (handle None: a stateless query)."""
    n = ctypes.c_size_t()
    head = () if handle is None else (handle,)
    nat.call(query, *head, *dims, ctypes.byref(n))
    return n.value


def as_bytes(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


def first_difference(a, b):
    """None if a and b hold the same bits, else a description of the first differing element."""
    if a is None or b is None:
        return None if a is b else "one of the two is absent"
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape / dtype {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    if a.numel() == 0:
        return None
    ne = (as_bytes(a) != as_bytes(b)).reshape(a.numel(), a.element_size()).any(1)
    if not bool(ne.any()):
        return None
    i = int(ne.nonzero()[0])
    return (f"{int(ne.sum())} of {a.numel()} elements differ, the first at flat index {i}: "
            f"{a.reshape(-1)[i].item()!r} vs {b.reshape(-1)[i].item()!r}")


def all_finite(t):
    return bool(torch.isfinite(t.float()).all()) if t.dtype.is_floating_point else True


def banded(shape, dtype, device, band_rows=64):
    """A contiguous tensor of `shape` (rows of shape[-1] values) with a band of band_rows more rows behind its last
    row in the same allocation, all of it prefilled with OUTPUT_BYTE -> (tensor, band)."""
    rows = 1
    for d in shape[:-1]:
        rows *= d
    full = torch.empty((rows + band_rows, shape[-1]), dtype=dtype, device=device)
    as_bytes(full).fill_(OUTPUT_BYTE)
    return full[:rows].view(shape), full[rows:]


def band_intact(band):
    return bool((as_bytes(band) == OUTPUT_BYTE).all())


class GuardedWorkspace:
    def __init__(self, need, device, shrink=0):
        self.need = need
        self.buf = torch.empty(GUARD + need + GUARD, dtype=torch.uint8, device=device)
        self.ws = self.buf[GUARD:GUARD + need]
        assert self.ws.numel() == need and self.ws.data_ptr() % 256 == 0
        self.ws_bytes = need - shrink  # what the C call is told; need itself unless this is the negative control
        self.byte = None
        self.calls = []                # (entry point, arguments) of the watched calls, in order

    def fill(self, byte):
        self.buf.fill_(byte)
        self.byte = byte

    def stale_slice(self, nbytes):
        """The workspace of the differently shaped call that leaves the stale contents: from the same first byte."""
        assert nbytes <= self.need + GUARD, (nbytes, self.need)
        return self.buf[GUARD:GUARD + nbytes]

    def restore_guards(self):
        """After the stale call (which may have been larger than `need`): the guards hold the fill byte again, the
        workspace keeps what that call left."""
        self.buf[:GUARD].fill_(self.byte)
        self.buf[GUARD + self.need:].fill_(self.byte)

    def damaged_guard(self):
        """None, or which guard no longer holds the fill byte and where."""
        torch.cuda.synchronize(self.buf.device)
        for name, g in (("front", self.buf[:GUARD]), ("rear", self.buf[GUARD + self.need:])):
            bad = g != self.byte
            if bool(bad.any()):
                i = int(bad.nonzero()[0])
                return f"{name} guard: {int(bad.sum())} bytes changed, the first at offset {i} of the guard"
        return None

    @contextlib.contextmanager
    def watch(self, entries):
        """While open, every `_native.call` of one of `entries` must carry this helper's slice; it is recorded and
        goes on with ws_bytes as this helper advertises it."""
        orig = nat.call

        def call(name, *args):
            if name in entries:
                ws, ws_bytes = args[-3], args[-2]
                assert ws.value == self.ws.data_ptr(), f"{name}: the workspace handed to the C call is not the slice"
                assert ws_bytes == self.need, f"{name}: ws_bytes {ws_bytes}, need {self.need}"
                args = args[:-2] + (self.ws_bytes, args[-1])
                self.calls.append((name, args))
            return orig(name, *args)

        nat.call = call
        try:
            yield self
        finally:
            nat.call = orig


def check_refusal(gw, outputs, pointers="all"):
    """Contract 2 on the calls `gw` has recorded: each, replayed with need - 1 bytes, returns VP_EINVAL with a
    message that names `need`, and the outputs (prefilled) are untouched.  The refusal comes before anything is read
    or launched, so the replay's input pointers (some of them temporaries of the wrapper) are never followed.
    pointers: 'all' outputs must be among the calls' pointer arguments, or 'any' (the rest travel inside a struct)."""
    lib = nat.load()
    outs = [t for t in outputs if t is not None]
    assert all(t.is_contiguous() for t in outs)
    seen = {a.value for _, args in gw.calls for a in args if isinstance(a, ctypes.c_void_p)}
    hits = [t.data_ptr() in seen for t in outs if t.numel()]
    assert (all if pointers == "all" else any)(hits), "the outputs checked are not the ones the call was given"
    for t in outs:
        as_bytes(t).fill_(OUTPUT_BYTE)
    torch.cuda.synchronize()
    assert gw.calls
    for name, args in gw.calls:
        rc = getattr(lib, name)(*args[:-2], gw.need - 1, args[-1])
        msg = lib.vp_last_error().decode()
        assert rc == nat.VP_EINVAL, (name, rc, msg)
        assert "too small" in msg and f"need {gw.need}" in msg, (name, msg, gw.need)
    torch.cuda.synchronize()
    for i, t in enumerate(outs):
        assert bool((as_bytes(t) == OUTPUT_BYTE).all()), f"output {i} was written by a refused call"


class Case:
    """One call of one entry point (or, for the probe, a forward and its backwards) at one shape.

      label     what is printed
      entries   the C entry points the call reaches through `_native.call`
      need      what the entry point's *_workspace_bytes reports for these arguments
      run       run(ws) -> tuple of output tensors (None where absent): the call, in workspace `ws`
      stale     stale(take): a differently shaped call of the same entry point in take(its own need)
      ordinary  ordinary() -> the same outputs from an ordinary call (a larger workspace than `need`)
      oracle    oracle(outputs) or None: the fp64 check of the fp32 cases (asserts; returns text to print)
      bands     bands(outputs) -> None or a message: the prefilled bands behind caller-owned outputs"""

    def __init__(self, label, entries, need, run, stale, ordinary, oracle=None, bands=None, finite=all_finite,
                 pointers="all"):
        self.label, self.entries, self.need = label, tuple(entries), need
        self.run, self.stale, self.ordinary, self.oracle, self.bands = run, stale, ordinary, oracle, bands
        self.finite, self.pointers = finite, pointers


def check_case(case, device):
    """Contracts 1-4, the output bands and the equality with an ordinary run, for one case; prints its record."""
    gw = GuardedWorkspace(case.need, device)
    first, failures = None, []
    for fill in FILLS:
        if fill == "stale":
            gw.fill(STALE_BYTE)
            case.stale(gw.stale_slice)
            torch.cuda.synchronize()
            gw.restore_guards()
        else:
            gw.fill(fill)
        gw.calls.clear()
        with gw.watch(case.entries):
            outs = case.run(gw.ws)
        raw = outs  # the tensors the recorded calls wrote
        name = fill if isinstance(fill, str) else f"0x{fill:02X}"
        damage = gw.damaged_guard()
        if damage:
            failures.append(f"fill {name}: {damage}")
        if fill != "stale" and not bool((gw.ws != fill).any()):
            failures.append(f"fill {name}: the call left the workspace as it was: nothing was tested")
        if case.bands is not None:
            msg = case.bands(outs)
            if msg:
                failures.append(f"fill {name}: {msg}")
        for i, t in enumerate(outs):
            if t is not None and not case.finite(t):
                failures.append(f"fill {name}: output {i} holds non-finite values")
        outs = tuple(None if t is None else t.clone() for t in outs)
        if first is None:
            first = outs
        else:
            assert len(outs) == len(first)
            for i, (a, b) in enumerate(zip(first, outs)):
                d = first_difference(a, b)
                if d:
                    failures.append(f"fill {name} against 0x00: output {i}: {d}")
    plain = case.ordinary()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(first, plain)):
        d = first_difference(a, b)
        if d:
            failures.append(f"exact workspace against an ordinary run: output {i}: {d}")
    note = case.oracle(first) if case.oracle is not None and not failures else ""
    print(f"{case.label}: need {case.need}, fills 0x00 0xFF 0x7F stale, "
          f"{'first difference: ' + failures[0] if failures else 'no difference'}{'; ' + note if note else ''}")
    assert not failures, (case.label, failures)
    check_refusal(gw, raw, case.pointers)


def check_short_slice(case, device):
    """The negative control: with the helper's slice one byte short the case takes the refusal path: the wrapper
    raises the library's VP_EINVAL, naming `need`, and nothing runs."""
    gw = GuardedWorkspace(case.need, device, shrink=1)
    gw.fill(0x00)
    try:
        with gw.watch(case.entries):
            case.run(gw.ws)
    except ValueError as e:
        assert "too small" in str(e) and f"need {case.need}" in str(e), (case.label, str(e))
    else:
        raise AssertionError(f"{case.label}: ran in need - 1 bytes")
    assert len(gw.calls) == 1, (case.label, [n for n, _ in gw.calls])  # the first watched call refused, no second
    assert gw.damaged_guard() is None and bool((gw.ws == 0).all()), f"{case.label}: a refused call wrote"
