"""The stream and workspace contracts (include/videoprism_hip.h, conventions) for the fp8 gallery's entry points, with
the harnesses of tests/stream_order.py and tests/workspace_guard.py and cases shaped like the bf16 gallery's in
tests/test_gpu_stream_order.py and tests/test_gpu_workspace.py: Q = 5, D = 128, k = 10, N = 5000 (several row ranges).

  stream     vp_op_topk_f8, vp_op_topk_groups_f8, vp_op_quantize_rows_f8: deferred inputs, then capture and replay
  workspace  vp_op_topk_f8, vp_op_topk_groups_f8 at N = 7 (fewer rows than k) and N = 5000: exactly the advertised
             bytes are enough, contents ignored, one byte fewer refused, nothing outside written

The file is named to be collected after tests/test_gpu_stream_order.py: its side stream is one more stream of the
process, and that file's control test_harness_sees_a_launch_on_another_stream depends on its own side stream not
sharing a hardware queue with the legacy stream, which a stream created ahead of it can change (seen once: with this
file collected first, that control found the legacy-stream launch ordered behind the side stream).

Poison (every byte 0xFF) is NaN codes, NaN scales and label -1: garbage scores, no fault; the scan's addresses do not
depend on data."""

import ctypes

import numpy as np
import pytest
import torch

import grouped_retrieval_restatement as gr
import retrieval_f8_restatement as f8
import retrieval_restatement as rr
import stream_order as so
import workspace_guard as wg
from videoprism import _native as nat

pytestmark = pytest.mark.gpu

Q, D, K, ID_BASE = 5, 128, 10, 100
p = nat._ptr


@pytest.fixture(scope="module")
def side(cuda):
    return torch.cuda.Stream(cuda)


def _gallery(N, device, seed=0):
    """(queries fp32, codes uint8, scales fp32) on the device; codes and scales from the restatement, so that these
    tests do not lean on the quantiser kernel."""
    q = f8.unit_rows(Q, D, 1000 + seed)
    codes, scales = f8.quantize(f8.unit_rows(N, D, N + seed)) if N else (torch.empty((0, D), dtype=torch.uint8),
                                                                          torch.empty((0,)))
    return q.to(device), codes.view(torch.uint8).to(device), scales.to(device)


def _ws_need(grouped, Qn=Q, k=K):
    return (nat.op_topk_groups_workspace_bytes if grouped else nat.op_topk_workspace_bytes)(Qn, k)


def _out_dtypes(grouped):
    return (torch.float32, torch.int64, torch.int64) if grouped else (torch.float32, torch.int64)


def _call(entry, grouped, q, codes, scales, labels, k, outs, ws, stream):
    Qn, N = q.shape[0], codes.shape[0]
    with torch.cuda.device(q.device):  # no handle: the op launches on the current device
        if grouped:
            nat.call(entry, p(q), Qn, p(codes), p(scales), N, D, D, p(labels), k, ID_BASE, *(p(t) for t in outs),
                     p(ws), ws.numel(), stream)
        else:
            nat.call(entry, p(q), Qn, p(codes), p(scales), N, D, D, k, ID_BASE, *(p(t) for t in outs), p(ws),
                     ws.numel(), stream)


# ---- the stream contract ----
def _search_stream_case(grouped, device):
    N = 5000
    entry = "vp_op_topk_groups_f8" if grouped else "vp_op_topk_f8"
    q, codes, scales = _gallery(N, device)
    named = dict(queries=so.staged(q), codes=so.staged(codes), scales=so.staged(scales))
    if grouped:
        named["labels"] = so.staged(torch.arange(N, device=device) // 3)
    ws = torch.empty(_ws_need(grouped), dtype=torch.uint8, device=device)
    outs = [torch.empty((Q, K), dtype=dt, device=device) for dt in _out_dtypes(grouped)]

    def call(stream):
        _call(entry, grouped, named["queries"][0], named["codes"][0], named["scales"][0],
              named["labels"][0] if grouped else None, K, outs, ws, so.stream_ptr(stream))
        return tuple(outs)

    return so.case_from(f"{entry} Q=5 D=128 k=10 N=5000", named, outs, lambda: [ws], call, capture=True)


def _quantize_stream_case(device):
    N = 5000
    named = dict(x=so.staged(f8.unit_rows(N, D, 77).to(device)))
    outs = [torch.empty((N, D), dtype=torch.uint8, device=device), torch.empty((N,), device=device)]

    def call(stream):
        with torch.cuda.device(device):
            nat.call("vp_op_quantize_rows_f8", p(named["x"][0]), nat.VP_F32, N, D, D, p(outs[0]), D, p(outs[1]),
                     so.stream_ptr(stream))
        return tuple(outs)

    return so.case_from("vp_op_quantize_rows_f8 N=5000 D=128 f32", named, outs, lambda: [], call, capture=True)


STREAM_CASES = {"topk_f8": lambda d: _search_stream_case(False, d), "topk_groups_f8": lambda d: _search_stream_case(True, d),
                "quantize_rows_f8": _quantize_stream_case}


@pytest.mark.parametrize("label", list(STREAM_CASES))
def test_stream_contract(cuda, side, label):
    failures = so.check_case(STREAM_CASES[label](cuda), side)
    assert not failures, (label, failures)


# ---- the workspace contract ----
def _topk_finite(t):
    """Scores: never NaN or +inf (-inf is the padding tail's, checked against the restatement); ids: anything."""
    return not t.dtype.is_floating_point or not bool((torch.isnan(t) | (t == float("inf"))).any())


def _workspace_case(grouped, N, device):
    entry = "vp_op_topk_groups_f8" if grouped else "vp_op_topk_f8"
    label = f"{entry} Q=5 D=128 k=10 N={N}"
    q, codes, scales = _gallery(N, device)
    labels = torch.arange(N, device=device) // 3
    qs, cs, ss = _gallery(900, device, seed=1)
    qs = torch.cat([qs, qs[:2] * 0.5])  # the stale call: 7 queries, k = 33, 900 rows
    need = _ws_need(grouped)
    band = {}

    def call(ws, q, codes, scales, labels, k, keep_bands):
        outs, bs = zip(*(wg.banded((q.shape[0], k), dt, device, 8) for dt in _out_dtypes(grouped)))
        if keep_bands:
            band["b"] = bs
        _call(entry, grouped, q, codes, scales, labels, k, outs, ws,
              ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
        return outs

    def run(ws):
        return call(ws, q, codes, scales, labels, K, True)

    def stale(take):
        call(take(_ws_need(grouped, 7, 33)), qs, cs, ss, torch.arange(900, device=device) % 50, 33, False)

    def ordinary():
        return call(torch.empty(need + wg.GUARD, dtype=torch.uint8, device=device), q, codes, scales, labels, K, False)

    def bands(outs):
        return None if all(wg.band_intact(b) for b in band["b"]) else "a band behind scores / ids was written"

    def oracle(outs):
        s64 = f8.dequantize(codes.cpu(), scales.cpu()).numpy() @ q.double().cpu().numpy().T  # of the stored gallery
        want = gr.group_topk(s64, labels.cpu().numpy(), K, ID_BASE) if grouped else rr.topk(s64, K, ID_BASE)
        got = [t.cpu().numpy() for t in outs]
        tail = np.isneginf(want[0])
        assert np.array_equal(np.isneginf(got[0]), tail)
        for g_, w_ in zip(got[1:], want[1:]):
            assert np.array_equal(g_[tail], w_[tail]) and (g_[tail] == -1).all()
        e = float(np.abs(got[0][~tail] - want[0][~tail]).max())
        rows = got[-1][~tail] - ID_BASE
        cols = np.broadcast_to(np.arange(Q)[:, None], tail.shape)[~tail]
        e_own = float(np.abs(s64[rows, cols] - got[0][~tail]).max())
        assert e <= 2e-5 and e_own <= 2e-5, (e, e_own)
        return f"oracle max-abs {e:.2e}, against the score of its own id {e_own:.2e} (bar 2e-05)"

    return wg.Case(label, (entry,), need, run, stale, ordinary, oracle, bands, finite=_topk_finite)


@pytest.mark.parametrize("N", [7, 5000])
@pytest.mark.parametrize("grouped", [False, True], ids=["topk_f8", "topk_groups_f8"])
def test_workspace_contract(cuda, grouped, N):
    wg.check_case(_workspace_case(grouped, N, cuda), cuda)


def test_short_slice_takes_the_refusal_path(cuda):
    for grouped in (False, True):
        wg.check_short_slice(_workspace_case(grouped, 5000, cuda), cuda)
