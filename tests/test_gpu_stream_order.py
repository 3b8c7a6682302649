"""The stream contract of include/videoprism_hip.h on the MI355X: every entry point below is asynchronous on the
caller's `stream`, never allocates and never synchronises, and the handle-level ones (with the probe and the
gallery search) can be captured into a hipGraph.  tests/stream_order.py holds the harness; values are compared
bit for bit with an ordinary call of the same entry point on the same inputs (whose parity with the fp64 oracle is
held by the tests named at the top of tests/test_gpu_workspace.py).

  Contract 1, deferred inputs (every case).  On a non-blocking side stream: the expected outputs from an ordinary call
    on X; the same call on other inputs X' (leftover state is now wrong for X); every input, output and workspace
    byte poisoned with 0xFF; then, on the side stream, a delay, the copies that deliver X, and an event `gate`; then
    the call.  When it returns `gate` must not have happened (no synchronisation, no blocking copy, no host read;
    a delay too short to tell fails as well), and after the stream has drained every output must hold the expected
    bits (a launch, memset or copy on any other stream ran during the delay, on poison).
  Contract 2, capture and replay (cases marked +graph).  The warmed call is captured with torch.cuda.graph on the
    side stream in the default global error mode, the inputs become X', outputs and workspaces are poisoned, one
    replay must give the bits of an ordinary call on X'.  A refused capture is reported with vp_last_error().
  Contract 3, the engines' stream= argument.  Contract 1 on Engine.forward, Engine.forward_windows,
    ClipEngine.encode_video, ClipEngine.encode_text and ClassifierEngine.forward with torch's current stream left at
    the default and the side stream passed as stream= only; the inputs need the engine's own torch-side preparation
    (a strided video, float64 paddings, int64 ids and frame_index), which therefore has to run on `stream` too.

Poison: 0xFF is NaN in fp32 and bf16, -1 in int32 and int64, 255 in uint8; frame_idx and text ids are clamped, a
negative label blanks a row, ids < 0 are padding in a merge: a kernel that runs early computes garbage, no fault.
Delay: torch.cuda._sleep, calibrated once; 50 x the measured host time of the warmed ordinary call, 50 ms at least.

Cases (models and geometries of tests/test_gpu_workspace.py: one layer per stack, bf16 and fp32 handles; all with
one padded frame and every optional output requested):
  vp_forward                      72, 288, 252 in both dtypes; 288 bf16 with uint8 frames             +graph
  vp_forward_spatial              72, 288                                                             +graph
  vp_forward_temporal             windows WINDOWS of 4 frame states, 72 (T = 3) and 252 (T = 2)       +graph
  vp_clip_encode_video, _windows  72, 252                                                             +graph
  vp_clip_encode_text             Q = 2, L = 16, second row half padded                               +graph
  vp_classifier_forward, _windows 72                                                                  +graph
  vp_op_probe_forward, _backward  probe_case's shape, both calls in one chain, both token dtypes      +graph
  vp_op_topk, vp_op_topk_groups   Q = 5, D = 128, k = 10, N = 5000 (several row ranges), both dtypes  +graph
  vp_op_topk_merge, _groups_merge 3 lists of Q = 5, k = 10                                            +graph
  vp_op_preprocess_frames, _yuv   2 source frames 64 x 48 to 3 frames of S = 36 through frame_idx (NV12)
  vp_op_gemm                      bf16 (256, 256, 128) epilogues 0 and 5; fp32 (128, 128, 16) epilogue 2; the
                                  small-M kernel (vp_dev_gemm_kernel which = 1) at (64, 64, 256)
  vp_op_attention                 heads = 2, one shape per kernel: bf16 S = 256, 8, 40, 320; S = 320 with key_pad;
                                  S = 40 cap 80; fp32 S = 16; S = 128 cap 50; S = 320 cap 0
  vp_op_attention_masked          bf16 S = 40 and fp32 S = 20, causal with key_pad
  vp_op_layernorm                 48 rows: D = 768 with perm 1 and `add`; D = 1408
  vp_op_patchify                  72 x 72 (band kernel) and 18 x 306 (P*W*C*4 > 65536: element gather), P = 18
  vp_op_pool_l2 (2, 48, 768), vp_op_similarity (2, 3, 768)
and stand-in "entry points" made of torch ops: a well-behaved one, and three that each break one rule (a launch on
the legacy stream, a stream synchronise, a device synchronise), which the harness must report: a value mismatch, the
`gate` failure and a refused capture.  The last runs in a child process (tests/stream_order.py says why).
vp_allgather is not here (tests/test_gpu_boundary.py has its stream test; a collective is no place for a delay).
"""

import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import probe_restatement as pr
import stream_order as so
import test_gpu_workspace as tw
import workspace_guard as wg
from videoprism import _native as nat
from videoprism import encoders

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

D = tw.D
p = nat._ptr


@pytest.fixture(scope="module")
def side(cuda):
    return torch.cuda.Stream(cuda)


def _empty(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _rand(seed, shape, device, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(device)


def _name(bf16):
    return "bf16" if bf16 else "f32"


# ---------------------------------------------------------------------------------------------------------------
# handle-level entry points
# ---------------------------------------------------------------------------------------------------------------
def _results(kind, eng, rows, T, N, bf16, device):
    """(output tensors, the C arguments between frame_paddings and the workspace) of one model kind, every optional
    output requested."""
    feats = [_empty((rows, T * N, D), tw._dt(bf16), device) for _ in range(2)]
    if kind == "enc":
        return feats, lambda: (p(feats[0]), eng.fprop_code, p(feats[1]))
    if kind == "lvt":
        outs = [_empty((rows, D), torch.float32, device), _empty((rows, T, D), torch.float32, device)] + feats
        return outs, lambda: (1, *(p(t) for t in outs), eng.fprop_code)
    outs = [_empty((rows, tw.NUM_CLASSES), torch.float32, device), _empty((rows, D), torch.float32, device)] + feats
    return outs, lambda: (*(p(t) for t in outs), eng.fprop_code)


def clips_case(kind, geom, bf16, u8=False):
    def build(device):
        _, _, eng = tw._model(kind, bf16)
        size, T, B = tw.GEOMS[geom]
        eng._prepare_tables(size, size, T)
        host = tw._video(B, T, size)
        x = tw._dev((host * 255).astype(np.uint8), device) if u8 else tw._dev(host, device, bf16)
        named = dict(video=so.staged(x), pads=so.staged(tw._dev(tw._pads(B, T, True), device)))
        query, entry = tw.CLIP_QUERY[kind]
        ws = _empty(wg.workspace_need(query, eng.handle(), B, T, size, size), torch.uint8, device)
        outs, tail = _results(kind, eng, B, T, tw._tokens(size), bf16, device)
        v, fp = named["video"][0], named["pads"][0]

        def call(stream):
            nat.call(entry, eng.handle(), p(v), nat._prec(v), B, T, size, size, p(fp), *tail(), p(ws), ws.numel(),
                     so.stream_ptr(stream))
            return tuple(outs)

        return so.case_from(label, named, outs, lambda: [ws], call, capture=True)

    label = f"{tw.CLIP_QUERY[kind][1]} {geom} {_name(bf16)}{' u8' if u8 else ''}"
    return label, build


def windows_case(kind, geom, bf16):
    def build(device):
        _, _, eng = tw._model(kind, bf16)
        size, T, _ = tw.GEOMS[geom]
        eng._prepare_tables(size, size, T)
        states = tw._states(kind, bf16, size, True, device).states.clone()
        F = states.shape[0]
        idx = np.array(tw.WINDOWS[T], np.int32)
        Wn = idx.shape[0]
        named = dict(states=so.staged(states), idx=so.staged(tw._dev(idx, device)),
                     pads=so.staged(tw._dev(tw._frame_pads(True)[idx], device)))
        query, entry = tw.WIN_QUERY[kind]
        ws = _empty(wg.workspace_need(query, eng.handle(), Wn, T, size, size), torch.uint8, device)
        outs, tail = _results(kind, eng, Wn, T, tw._tokens(size), bf16, device)
        st, ix, fp = (named[n][0] for n in ("states", "idx", "pads"))

        def call(stream):
            nat.call(entry, eng.handle(), p(st), F, p(ix), Wn, T, size, size, p(fp), *tail(), p(ws), ws.numel(),
                     so.stream_ptr(stream))
            return tuple(outs)

        return so.case_from(label, named, outs, lambda: [ws], call, capture=True)

    label = f"{tw.WIN_QUERY[kind][1]} {geom} {_name(bf16)}"
    return label, build


def spatial_case(geom, bf16):
    def build(device):
        _, _, eng = tw._model("enc", bf16)
        size, T, B = tw.GEOMS[geom]
        F = B * T
        eng._prepare_tables(size, size, 1)
        named = dict(frames=so.staged(tw._dev(tw._video(B, T, size).reshape(F, size, size, 3), device, bf16)),
                     pads=so.staged(tw._dev(tw._pads(B, T, True).reshape(F), device)))
        vh = eng.video_handle()
        ws = _empty(wg.workspace_need("vp_spatial_workspace_bytes", vh, F, size, size), torch.uint8, device)
        states = _empty((F, tw._tokens(size), D), tw._dt(bf16), device)
        fr, fp = named["frames"][0], named["pads"][0]

        def call(stream):
            nat.call("vp_forward_spatial", vh, p(fr), nat._prec(fr), F, size, size, p(fp), p(states), p(ws),
                     ws.numel(), so.stream_ptr(stream))
            return (states,)

        return so.case_from(label, named, [states], lambda: [ws], call, capture=True)

    label = f"vp_forward_spatial {geom} {_name(bf16)}"
    return label, build


def _text_inputs(device, ids_dtype=torch.int32, pad_dtype=torch.float32):
    Q, L = 2, 16
    rng = np.random.default_rng(6)
    ids = torch.from_numpy(rng.integers(0, tw.LVT["vocabulary_size"], (Q, L))).to(ids_dtype).to(device)
    pads = torch.zeros(Q, L, dtype=pad_dtype)
    pads[1, L // 2:] = 1.0
    return Q, L, ids, pads.to(device)


def text_case(bf16):
    def build(device):
        _, _, eng = tw._model("lvt", bf16)
        Q, L, ids, pads = _text_inputs(device)
        named = dict(ids=so.staged(ids), pads=so.staged(pads))
        ws = _empty(wg.workspace_need("vp_clip_text_workspace_bytes", eng.handle(), Q, L), torch.uint8, device)
        out = _empty((Q, D), torch.float32, device)
        i, pd = named["ids"][0], named["pads"][0]

        def call(stream):
            nat.call("vp_clip_encode_text", eng.handle(), p(i), p(pd), Q, L, 1, p(out), p(ws), ws.numel(),
                     so.stream_ptr(stream))
            return (out,)

        return so.case_from(label, named, [out], lambda: [ws], call, capture=True)

    label = f"vp_clip_encode_text Q=2 L=16 {_name(bf16)}"
    return label, build


# ---------------------------------------------------------------------------------------------------------------
# the probe and the gallery search
# ---------------------------------------------------------------------------------------------------------------
def probe_case(bf16):
    def build(device):
        Dm, H, C, B, S = 256, 4, 5, 2, 40
        dims = (Dm, H, C)
        head = pr.synthetic_head(Dm, H, C, 77)
        named = {m: so.staged(head[path].float().contiguous().to(device)) for m, path in nat.PROBE_LEAVES}
        named["tokens"] = so.staged(_rand(78, (B, S, Dm), device, tw._dt(bf16)))
        named["dlogits"] = so.staged(_rand(79, (B, C), device))
        tensors = {m: named[m][0] for m, _ in nat.PROBE_LEAVES}
        x, dl = named["tokens"][0], named["dlogits"][0]
        ws = _empty(nat.op_probe_workspace_bytes(*dims, B, S), torch.uint8, device)
        logits, emb = _empty((B, C), torch.float32, device), _empty((B, Dm), torch.float32, device)
        grads = {m: torch.empty_like(t) for m, t in tensors.items()}
        outs = [logits, emb] + [grads[m] for m, _ in nat.PROBE_LEAVES]

        def call(stream):
            nat.op_probe_forward(dims, tensors, x, logits, emb, ws, stream=stream)
            nat.op_probe_backward(dims, tensors, x, dl, grads, ws, stream=stream)
            return tuple(outs)

        return so.case_from(label, named, outs, lambda: [ws], call, capture=True)

    label = f"vp_op_probe_forward+backward D=256 H=4 C=5 B=2 S=40 {_name(bf16)} tokens"
    return label, build


def topk_case(grouped, bf16):
    def build(device):
        Q, Dm, k, N, id_base = 5, 128, 10, 5000, 100
        rng = np.random.default_rng(N + 1)
        named = dict(queries=so.staged(tw._dev(tw._unit_rows(rng, Q, Dm), device)),
                     gallery=so.staged(tw._dev(tw._unit_rows(rng, N, Dm), device).to(tw._dt(bf16))))
        if grouped:
            named["labels"] = so.staged(torch.arange(N, device=device) // 3)
        q, gal = named["queries"][0], named["gallery"][0]
        need = (nat.op_topk_groups_workspace_bytes if grouped else nat.op_topk_workspace_bytes)(Q, k)
        ws = _empty(need, torch.uint8, device)
        outs = [_empty((Q, k), dt, device)
                for dt in ((torch.float32, torch.int64, torch.int64) if grouped else (torch.float32, torch.int64))]

        def call(stream):
            with torch.cuda.device(device):  # no handle: the op launches on the current device
                if grouped:
                    nat.call(entry, p(q), Q, p(gal), nat._prec(gal), N, Dm, Dm, p(named["labels"][0]), k, id_base,
                             *(p(t) for t in outs), p(ws), ws.numel(), so.stream_ptr(stream))
                else:
                    nat.call(entry, p(q), Q, p(gal), nat._prec(gal), N, Dm, Dm, k, id_base, *(p(t) for t in outs),
                             p(ws), ws.numel(), so.stream_ptr(stream))
            return tuple(outs)

        return so.case_from(label, named, outs, lambda: [ws], call, capture=True)

    entry = "vp_op_topk_groups" if grouped else "vp_op_topk"
    label = f"{entry} Q=5 D=128 k=10 N=5000 {_name(bf16)} gallery"
    return label, build


def merge_case(grouped):
    def build(device):
        parts, Q, k = 3, 5, 10

        def lists(seed):  # sorted as a search writes them, every id and group once
            g = torch.Generator().manual_seed(seed)
            sc = torch.rand(parts, Q, k, generator=g).sort(dim=2, descending=True).values
            ids = torch.stack([torch.randperm(1000, generator=g)[:parts * k].reshape(parts, k) for _ in range(Q)], 1)
            return sc.to(device), (ids % 37).contiguous().to(device), ids.contiguous().to(device)

        (s0, g0, i0), (s1, g1, i1) = lists(3), lists(4)
        named = dict(scores=so.staged(s0, s1), ids=so.staged(i0, i1))
        if grouped:
            named["groups"] = so.staged(g0, g1)
        outs = [_empty((Q, k), dt, device)
                for dt in ((torch.float32, torch.int64, torch.int64) if grouped else (torch.float32, torch.int64))]

        def call(stream):
            with torch.cuda.device(device):
                if grouped:
                    nat.call(entry, p(named["scores"][0]), p(named["groups"][0]), p(named["ids"][0]), parts, Q, k, k,
                             *(p(t) for t in outs), so.stream_ptr(stream))
                else:
                    nat.call(entry, p(named["scores"][0]), p(named["ids"][0]), parts, Q, k, k, *(p(t) for t in outs),
                             so.stream_ptr(stream))
            return tuple(outs)

        return so.case_from(label, named, outs, lambda: [], call, capture=True)

    entry = "vp_op_topk_groups_merge" if grouped else "vp_op_topk_merge"
    label = f"{entry} parts=3 Q=5 k=10"
    return label, build


# ---------------------------------------------------------------------------------------------------------------
# op-level entry points (contract 1)
# ---------------------------------------------------------------------------------------------------------------
def preprocess_case(yuv):
    def build(device):
        N, H, W, S = 2, 48, 64, 36
        g = torch.Generator().manual_seed(11)
        byte = lambda *shape: torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(device)  # noqa: E731
        idx = torch.tensor([1, 0, 1], dtype=torch.int32, device=device)
        named = dict(idx=so.staged(idx, 1 - idx))
        F = idx.numel()
        dst = _empty((F, S, S, 3), torch.uint8, device)
        if yuv:
            named.update(y=so.staged(byte(N, H, W)), uv=so.staged(byte(N, H // 2, W // 2, 2)))
            src, *_ = nat.yuv_frames((named["y"][0], named["uv"][0]), nat.VP_YUV_NV12)

            def call(stream):
                with torch.cuda.device(device):
                    nat.call("vp_op_preprocess_yuv", ctypes.byref(src), N, H, W, p(named["idx"][0]), F,
                             nat.VP_RESIZE_CENTER_CROP, S, p(dst), so.stream_ptr(stream))
                return (dst,)
        else:
            named.update(frames=so.staged(byte(N, H, W, 3)))

            def call(stream):
                with torch.cuda.device(device):
                    nat.call("vp_op_preprocess_frames", p(named["frames"][0]), N, H, W, 3 * W, 3 * W * H,
                             p(named["idx"][0]), F, nat.VP_RESIZE_CENTER_CROP, 0, S, p(dst), so.stream_ptr(stream))
                return (dst,)

        return so.case_from(label, named, [dst], lambda: [], call)

    label = f"{'vp_op_preprocess_yuv NV12' if yuv else 'vp_op_preprocess_frames'} 2 x 64x48 -> 3 x 36x36 frame_idx"
    return label, build


def gemm_case(bf16, M, N, K, epi, small=False):
    def build(device):
        dt = tw._dt(bf16)
        named = dict(a=so.staged(_rand(1, (M, K), device, dt, 0.5)), w=so.staged(_rand(2, (N, K), device, dt, 0.5)),
                     bias=so.staged(_rand(3, (N,), device)))
        resid = rowpad = None
        if epi in (nat.EPI_RESID, nat.EPI_RESID_BF16):
            named["resid"] = so.staged(_rand(4, (M, N), device, dt if epi == nat.EPI_RESID_BF16 else torch.float32))
            named["rowpad"] = so.staged((torch.arange(M) % 5 == 0).float().to(device))
            resid, rowpad = named["resid"][0], named["rowpad"][0]
        out = _empty((M, N), dt if epi in (nat.EPI_STORE, nat.EPI_RESID_BF16) else torch.float32, device)
        a, w, b = (named[n][0] for n in ("a", "w", "bias"))

        def call(stream):
            if small:
                nat.call("vp_dev_gemm_kernel", 1, epi, p(a), p(w), M, N, K, p(out), p(b), None, None, 0, None,
                         so.stream_ptr(stream))
            else:
                nat.call("vp_op_gemm", nat._prec(a), epi, p(a), K, p(w), K, M, N, K, p(out), N, p(b), p(resid), N,
                         None, 0, p(rowpad), so.stream_ptr(stream))
            return (out,)

        return so.case_from(label, named, [out], lambda: [], call)

    label = f"{'vp_dev_gemm_kernel small-M' if small else 'vp_op_gemm'} {_name(bf16)} ({M}, {N}, {K}) epilogue {epi}"
    return label, build


def attention_case(bf16, S, cap, key_pad=False, causal=None):
    """vp_op_attention (causal None) or vp_op_attention_masked (causal 0 / 1): 2 sequences, 2 heads."""
    def build(device):
        num_seq, heads = 2, 2
        named = dict(qkv=so.staged(_rand(S, (num_seq * S, 3 * heads * 64), device, tw._dt(bf16), 0.5)))
        kp = None
        if key_pad:
            pad = torch.zeros(num_seq, S)
            pad[:, S - 3:] = 1.0
            named["key_pad"] = so.staged(pad.reshape(-1).to(device))
            kp = named["key_pad"][0]
        qkv = named["qkv"][0]
        o = _empty((num_seq * S, heads * 64), tw._dt(bf16), device)

        def call(stream):
            if causal is None:
                nat.call("vp_op_attention", nat._prec(qkv), p(qkv), p(o), num_seq, S, heads, float(cap), p(kp),
                         so.stream_ptr(stream))
            else:
                nat.call("vp_op_attention_masked", nat._prec(qkv), p(qkv), p(o), num_seq, S, heads, float(cap), p(kp),
                         causal, so.stream_ptr(stream))
            return (o,)

        return so.case_from(label, named, [o], lambda: [], call)

    label = f"{'vp_op_attention' if causal is None else 'vp_op_attention_masked'} {_name(bf16)} S={S} cap={cap}" \
            f"{' key_pad' if key_pad else ''}{' causal' if causal else ''}"
    return label, build


def layernorm_case(Dm, perm, bf16):
    def build(device):
        T, Nsp = 3, 16
        rows = T * Nsp
        named = dict(x=so.staged(_rand(5, (rows, Dm), device, tw._dt(bf16))),
                     gamma=so.staged(1 + _rand(6, (Dm,), device, scale=0.1)),
                     beta=so.staged(_rand(7, (Dm,), device, scale=0.1)))
        add = None
        if perm:
            named["add"] = so.staged(_rand(8, (T, Dm), device))
            add = named["add"][0]
        x, ga, be = (named[n][0] for n in ("x", "gamma", "beta"))
        out = _empty((rows, Dm), tw._dt(bf16), device)

        def call(stream):
            nat.call("vp_op_layernorm", p(x), nat._prec(x), rows, Dm, p(ga), p(be), p(out), nat._prec(out), perm, T,
                     Nsp, p(add), so.stream_ptr(stream))
            return (out,)

        return so.case_from(label, named, [out], lambda: [], call)

    label = f"vp_op_layernorm {_name(bf16)} rows=48 D={Dm} perm={perm}{' add' if perm else ''}"
    return label, build


def patchify_case(H, W):
    def build(device):
        P, kpad = 18, 976  # P*P*3 = 972
        named = dict(video=so.staged(_rand(9, (1, H, W, 3), device)))
        v = named["video"][0]
        out = _empty(((H // P) * (W // P), kpad), torch.float32, device)

        def call(stream):
            nat.call("vp_op_patchify", p(v), nat.VP_F32, p(out), nat.VP_F32, 1, H, W, 3, P, kpad, so.stream_ptr(stream))
            return (out,)

        return so.case_from(label, named, [out], lambda: [], call)

    label = f"vp_op_patchify f32 {H}x{W} P=18 ({'band' if 18 * W * 3 * 4 <= 65536 else 'element gather'})"
    return label, build


def pool_case():
    def build(device):
        B, L = 2, 48
        named = dict(emb=so.staged(_rand(10, (B, L, D), device)))
        e = named["emb"][0]
        out = _empty((B, D), torch.float32, device)

        def call(stream):
            nat.call("vp_op_pool_l2", p(e), nat.VP_F32, B, L, D, p(out), so.stream_ptr(stream))
            return (out,)

        return so.case_from("vp_op_pool_l2 (2, 48, 768)", named, [out], lambda: [], call)

    return "vp_op_pool_l2 (2, 48, 768)", build


def similarity_case():
    def build(device):
        B, Q = 2, 3
        named = dict(video=so.staged(_rand(12, (B, D), device)), text=so.staged(_rand(13, (Q, D), device)))
        v, t = named["video"][0], named["text"][0]
        out = _empty((B, Q), torch.float32, device)

        def call(stream):
            nat.call("vp_op_similarity", p(v), p(t), B, Q, D, p(out), so.stream_ptr(stream))
            return (out,)

        return so.case_from("vp_op_similarity (2, 3, 768)", named, [out], lambda: [], call)

    return "vp_op_similarity (2, 3, 768)", build


# ---------------------------------------------------------------------------------------------------------------
# contract 3: the engines' stream= argument, torch's current stream left at the default
# ---------------------------------------------------------------------------------------------------------------
def engine_case(which, bf16):
    def build(device):
        kind = {"forward": "enc", "forward_windows": "enc", "encode_video": "lvt", "encode_text": "lvt",
                "classifier_forward": "cls"}[which]
        _, _, eng = tw._model(kind, bf16)
        size, T, B = tw.GEOMS["72"]
        scratch = lambda: [t for t in eng._ws.values() if t is not None]  # noqa: E731
        if which == "encode_text":
            _, _, ids, pads = _text_inputs(device, torch.int64, torch.float64)
            named = dict(ids=so.staged(ids), pads=so.staged(pads))

            def call(stream):
                return (eng.encode_text(named["ids"][0], named["pads"][0], stream=stream),)
        elif which == "forward_windows":
            fs = tw._states(kind, bf16, size, True, device)
            idx = torch.tensor(tw.WINDOWS[T], dtype=torch.int64, device=device)
            named = dict(states=so.staged(fs.states.clone()), pads=so.staged(fs.paddings.double()), idx=so.staged(idx))

            def call(stream):
                st = encoders.FrameStates(named["states"][0], named["pads"][0], (size, size))
                return eng.forward_windows(st, named["idx"][0], want_spatial=True, stream=stream)
        else:  # clips: the video as a strided view (three of four stored channels), float64 paddings
            v4 = torch.zeros(B, T, size, size, 4)
            v4[..., :3] = torch.from_numpy(tw._video(B, T, size))
            named = dict(video=so.staged(v4.to(device)), pads=so.staged(tw._dev(tw._pads(B, T, True), device).double()))

            def call(stream):
                v, fp = named["video"][0][..., :3], named["pads"][0]
                if which == "forward":
                    return eng.forward(v, fp, want_spatial=True, stream=stream)
                if which == "encode_video":
                    return eng.encode_video(v, fp, True, want_frames=True, want_spatial=True, want_spatiotemporal=True,
                                            stream=stream)
                return eng.forward(v, fp, want_embeddings=True, want_spatial=True, want_spatiotemporal=True,
                                   stream=stream)

        return so.case_from(label, named, [], scratch, call)

    label = f"engine {which} stream= {_name(bf16)}"
    return label, build


def _all_cases():
    cases = []
    for bf16 in (True, False):
        for geom in ("72", "288", "252"):
            cases.append(clips_case("enc", geom, bf16))
        for geom in ("72", "288"):
            cases.append(spatial_case(geom, bf16))
        for geom in ("72", "252"):
            cases += [windows_case("enc", geom, bf16), clips_case("lvt", geom, bf16), windows_case("lvt", geom, bf16)]
        cases += [text_case(bf16), clips_case("cls", "72", bf16), windows_case("cls", "72", bf16), probe_case(bf16),
                  topk_case(False, bf16), topk_case(True, bf16)]
        for which in ("forward", "forward_windows", "encode_video", "encode_text", "classifier_forward"):
            cases.append(engine_case(which, bf16))
    cases += [clips_case("enc", "288", True, u8=True), merge_case(False), merge_case(True),
              preprocess_case(False), preprocess_case(True),
              gemm_case(True, 256, 256, 128, nat.EPI_STORE), gemm_case(True, 256, 256, 128, nat.EPI_RESID_BF16),
              gemm_case(False, 128, 128, 16, nat.EPI_RESID), gemm_case(True, 64, 64, 256, nat.EPI_STORE, small=True)]
    cases += [attention_case(True, S, 50.0) for S in (256, 8, 40, 320)]
    cases += [attention_case(True, 320, 50.0, key_pad=True), attention_case(True, 40, 80.0),
              attention_case(False, 16, 50.0), attention_case(False, 128, 50.0), attention_case(False, 320, 0.0),
              attention_case(True, 40, 50.0, key_pad=True, causal=1),
              attention_case(False, 20, 50.0, key_pad=True, causal=1),
              layernorm_case(768, nat.PERM_BTN_TO_BNT, True), layernorm_case(1408, nat.PERM_NONE, False),
              patchify_case(72, 72), patchify_case(18, 306), pool_case(), similarity_case()]
    return cases


CASES = dict(_all_cases())
assert len(CASES) == 2 * (3 + 2 + 6 + 6 + 5) + 9 + 4 + 5 + 2 + 2 + 2 + 2


@pytest.mark.parametrize("label", list(CASES), ids=[c.replace(" ", "-") for c in CASES])
def test_stream_contract(cuda, side, label):
    failures = so.check_case(CASES[label](cuda), side)
    assert not failures, (label, failures)


# ---------------------------------------------------------------------------------------------------------------
# the harness must be able to see: stand-in entry points made of torch ops, each breaking one rule
# ---------------------------------------------------------------------------------------------------------------
_stand_in = so.torch_stand_in


def _kinds(failures):
    return sorted({f.split(":")[0] for f in failures})


def test_harness_passes_a_well_behaved_call(cuda, side):
    def body(stream, x, tmp, out):
        with torch.cuda.stream(stream):
            torch.add(x, 1.0, out=tmp)
            torch.mul(tmp, 2.0, out=out)

    print(f"delay: {so.delay_source().note}")
    assert so.check_case(_stand_in(cuda, "well behaved", body, capture=True), side) == []


def test_harness_sees_a_launch_on_another_stream(cuda, side):
    """Part of the work on the legacy default stream: it runs during the delay, on poison.  This also shows that
    `side` is not ordered against the legacy stream on this runtime (were it, the values would come out right)."""
    def body(stream, x, tmp, out):
        with torch.cuda.stream(torch.cuda.default_stream(cuda)):
            torch.add(x, 1.0, out=tmp)
        with torch.cuda.stream(stream):
            torch.mul(tmp, 2.0, out=out)

    failures = so.check_case(_stand_in(cuda, "one launch on the legacy stream", body), side)
    assert _kinds(failures) == ["values"], failures


def test_harness_sees_a_synchronising_call(cuda, side):
    def body(stream, x, tmp, out):
        with torch.cuda.stream(stream):
            torch.add(x, 1.0, out=tmp)
            torch.mul(tmp, 2.0, out=out)
        stream.synchronize()

    failures = so.check_case(_stand_in(cuda, "stream synchronise before returning", body), side)
    assert _kinds(failures) == ["gate"], failures


def test_harness_sees_a_refused_capture(cuda):
    """A device synchronise inside the call: legal (if slow) on a stream, refused while the stream is capturing.  The
    stand-in runs in a child process (tests/stream_order.py as a program): on this runtime a refused capture leaves
    the process unable to make blocking copies, which must not reach the tests that follow."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(q for q in sys.path if q))
    child = subprocess.run([sys.executable, so.__file__], capture_output=True, text=True, env=env, timeout=100)
    print(child.stdout)
    found = [line for line in child.stdout.splitlines() if line.startswith("FAILURES ")]
    assert child.returncode == 0 and found, (child.returncode, child.stdout[-1000:], child.stderr[-2000:])
    failures = json.loads(found[-1][len("FAILURES "):])
    assert _kinds(failures) == ["capture", "gate"], failures
    assert any("refused" in f for f in failures), failures
