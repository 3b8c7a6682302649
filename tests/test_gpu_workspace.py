"""The workspace contract of include/videoprism_hip.h on the MI355X, for the eleven entry points that take a
workspace: with `need` the value the entry point's *_workspace_bytes returns for the same arguments,

  1. called with exactly `need` bytes the call writes nothing outside [ws, ws + need)        (guard bands)
  2. with need - 1 bytes it returns VP_EINVAL before the first launch: outputs untouched, the message names `need`
  3. every output is bit for bit the same whatever the workspace held on entry               (fills, see below)
  4. every output value is finite, and the fp32 cases meet the fp64 oracle at the bar of the entry point's own test

plus: a prefilled band behind each caller-owned output stays intact, and the outputs equal, bitwise, those of an
ordinary call of the same engine in a larger workspace.  tests/workspace_guard.py holds the helper and the checks.

Each case runs once per fill and compares all outputs bitwise against the first:
  0x00   zeros
  0xFF   NaN in bf16 and fp32, -1 as an integer
  0x7F   3.39e38 in both float types: finite, overflows in any sum
  stale  the leftovers of a differently shaped call of the same entry point, run in the same buffer just before

Entry point                      oracle bar of the fp32 cases (max-abs unless said), and where it comes from
  vp_forward                     1e-5 embeddings and spatial_features   test_gpu_encoder (fp32 parity)
  vp_forward_spatial             1e-5 on spatial_ln(states) against the oracle's spatial_features   test_gpu_encoder
  vp_forward_temporal            1e-5 on the gathered clips             test_gpu_windows.test_windows_against_oracle_f32
  vp_clip_encode_video           2e-5 video and frame embeddings        test_gpu_clip.test_clip_reduced_depth
  vp_clip_encode_video_windows   2e-5 on the gathered clips             test_gpu_clip.test_clip_reduced_depth
  vp_clip_encode_text            2e-5                                   test_gpu_clip.test_clip_reduced_depth
  vp_classifier_forward          2e-5 logits and global embeddings      test_gpu_classifier.test_classifier_reduced_depth
  vp_classifier_forward_windows  2e-5 on the gathered clips             test_gpu_classifier.test_classifier_reduced_depth
  vp_op_probe_forward/_backward  2e-5 ||g - g64|| / ||g64|| per leaf and for the logits   test_gpu_probe.BAR
  vp_op_topk                     2e-5 on the scores of the stored gallery   test_gpu_retrieval.BAR
  vp_op_topk_groups              2e-5 likewise                          test_gpu_retrieval_groups.BAR

Models: Base widths with 1 spatial + 1 temporal layer; LvT-Base reduced as in tests/test_gpu_threads.py (vocabulary
100, one layer per stack); the classifier on the same encoder; a bf16 and an fp32 handle of each.  Geometries, the
smallest at which padding, packing and the second path through each carve-up exist:
  288 x 288, T = 2, B = 1   N = 256, M = 512: tile-aligned; bf16 takes the fused patch embedding (once with uint8
                            frames: video_to_bf16 stages in `big`)
  72 x 72,   T = 3, B = 1   N = 16, M = 48 -> 256 / 128 GEMM rows: almost all rows are padding; S = 16 spatial and
                            S = 3 temporal kernels; vp_forward_spatial takes its copy path
  252 x 252, T = 2, B = 3   N = 196, M = 1176 -> 1280: sequence-packed attention with a partly filled last
                            workgroup; for LvT the auxiliary encoder's padded `feat` rows
each with and without frame paddings (one padded frame) and with and without the optional outputs.  The top-k
outputs are finite where an id is returned; their padding tail is (-inf, -1) by contract and is checked as such.
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

import grouped_retrieval_restatement as gr
import probe_restatement as pr
import retrieval_restatement as rr
import workspace_guard as wg
from oracle import videoprism_oracle as orc
from videoprism import _native as nat
from videoprism import encoders, models, params

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ENC = dict(models.CONFIGS["videoprism_v1_base"], num_spatial_layers=1, num_temporal_layers=1)
LVT = dict(models.CONFIGS["videoprism_lvt_v1_base"], vocabulary_size=100, num_spatial_layers=1,
           num_temporal_layers=1, num_auxiliary_layers=1, num_unimodal_layers=1)
NUM_CLASSES = 40
P, D = ENC["patch_size"], ENC["model_dim"]

GEOMS = {"288": (288, 2, 1), "72": (72, 3, 1), "252": (252, 2, 3)}          # size, T, B
# the differently shaped call before it: another patch grid, no larger in GEMM rows in either dtype (144 x 144: N = 64)
STALE_OF = {"288": (72, 3, 1), "72": (144, 1, 1), "252": (288, 2, 1)}
WINDOWS = {2: [[0, 1], [1, 2], [3, 3]], 3: [[0, 1, 2], [1, 2, 3], [3, 3, 0]]}  # overlapping, one repeated frame
NFRAMES = 4


def _dt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


@functools.lru_cache(maxsize=None)
def _model(kind, bf16):
    """(model, variables, engine on the current device) of one kind and dtype, built once."""
    fd = torch.bfloat16 if bf16 else None
    if kind == "enc":
        m = models.get_model(None, model_fn=lambda: encoders.FactorizedEncoder(**ENC), fprop_dtype=fd)
        var = params.synthetic_params(ENC, seed=31)
    elif kind == "lvt":
        m = models.get_model(None, model_fn=lambda: encoders.FactorizedVideoCLIP(**LVT), fprop_dtype=fd)
        var = params.synthetic_params(LVT, 32, specs=params.clip_leaf_specs(LVT))
    else:
        m = models.get_model(None, model_fn=lambda: encoders.FactorizedVideoClassifier(encoder_params=ENC,
                                                                                      num_classes=NUM_CLASSES),
                             fprop_dtype=fd)
        var = params.synthetic_params(ENC, 33, specs=m.param_specs())
    return m, var, m.engine(var, torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def _video(B, T, size):
    return np.random.default_rng(1000 * size + 10 * T + B).random((B, T, size, size, 3), dtype=np.float32)


def _pads(B, T, padded):
    if not padded:
        return None
    p = np.zeros((B, T), np.float32)
    p[B - 1, T - 1] = 1.0
    return p


def _dev(a, device, bf16=False):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t.to(torch.bfloat16) if bf16 and t.dtype == torch.float32 else t


def _tokens(size):
    return (size // P) ** 2


def _maxabs(got, ref):
    return float(np.abs(got.double().cpu().numpy() - ref).max())


def _oversized(need, device):
    return torch.empty(need + wg.GUARD, dtype=torch.uint8, device=device)


# ---------------------------------------------------------------------------------------------------------------
# fp64 references, computed once and shared
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_clips(kind, geom, padded, windows):
    """The oracle on the case's clips (windows: the clips gathered from the NFRAMES frames) -> dict of outputs."""
    size, T, B = GEOMS[geom]
    _, var, _ = _model(kind, False)
    if windows:
        idx = np.array(WINDOWS[T])
        video = _video(1, NFRAMES, size)[0][idx]
        pads = _frame_pads(padded)[idx] if padded else None
    else:
        video, pads = _video(B, T, size), _pads(B, T, padded)
    if kind == "enc":
        emb, out = orc.factorized_encoder(var["params"], video, ENC, mode="f64", frame_paddings=pads,
                                          return_intermediate=True)
        return dict(emb=emb, spatial=out["spatial_features"])
    if kind == "lvt":
        v, _, out = orc.video_clip(var["params"], LVT, video, None, None, "f64",
                                   return_intermediate=("frame_embeddings",), frame_paddings=pads)
        return dict(video=v, frames=out["frame_embeddings"])
    logits, out = orc.video_classifier(var["params"], ENC, video, return_intermediate=("global_embeddings",),
                                       frame_paddings=pads)
    return dict(logits=logits, emb=out["global_embeddings"])


def _frame_pads(padded):
    if not padded:
        return None
    p = np.zeros(NFRAMES, np.float32)
    p[NFRAMES - 1] = 1.0
    return p


def _oracle_outputs(kind, geom, padded, windows):
    """The oracle check of a video case's outputs, in the order the engine returns them."""
    def check(outs):
        ref = _ref_clips(kind, geom, padded, windows)
        if kind == "enc":
            e = [_maxabs(outs[0], ref["emb"])] + ([_maxabs(outs[1], ref["spatial"])] if outs[1] is not None else [])
            bar = 1e-5
        elif kind == "lvt":
            e = [_maxabs(outs[0], ref["video"])] + ([_maxabs(outs[1], ref["frames"])] if outs[1] is not None else [])
            bar = 2e-5
        else:
            e = [_maxabs(outs[0], ref["logits"])] + ([_maxabs(outs[1], ref["emb"])] if outs[1] is not None else [])
            bar = 2e-5
        assert max(e) <= bar, (e, bar)
        return "oracle max-abs " + " ".join(f"{x:.2e}" for x in e) + f" (bar {bar:g})"
    return check


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
CLIP_QUERY = {"enc": ("vp_workspace_bytes", "vp_forward"),
              "lvt": ("vp_clip_video_workspace_bytes", "vp_clip_encode_video"),
              "cls": ("vp_classifier_workspace_bytes", "vp_classifier_forward")}
WIN_QUERY = {"enc": ("vp_temporal_workspace_bytes", "vp_forward_temporal"),
             "lvt": ("vp_clip_video_windows_workspace_bytes", "vp_clip_encode_video_windows"),
             "cls": ("vp_classifier_windows_workspace_bytes", "vp_classifier_forward_windows")}


def _clip_call(kind, eng, x, fp, extras, out=None):
    if kind == "enc":
        return eng.forward(x, fp, want_spatial=extras, out=out)
    if kind == "lvt":
        return eng.encode_video(x, fp, True, want_frames=extras, want_spatial=extras, want_spatiotemporal=extras)
    return eng.forward(x, fp, want_embeddings=extras, want_spatial=extras, want_spatiotemporal=extras)


def _windows_call(kind, eng, fs, idx, extras):
    if kind == "enc":
        return eng.forward_windows(fs, idx, want_spatial=extras)
    if kind == "lvt":
        return eng.encode_video_windows(fs, idx, True, want_frames=extras, want_spatial=extras,
                                        want_spatiotemporal=extras)
    return eng.forward_windows(fs, idx, want_embeddings=extras, want_spatial=extras, want_spatiotemporal=extras)


def clips_case(kind, geom, bf16, padded, extras, u8=False):
    """vp_forward / vp_clip_encode_video / vp_classifier_forward over the geometry's clips."""
    def build(device):
        _, _, eng = _model(kind, bf16)
        size, T, B = GEOMS[geom]
        query, entry = CLIP_QUERY[kind]
        host = _video(B, T, size)
        x = _dev((host * 255).astype(np.uint8), device) if u8 else _dev(host, device, bf16)
        fp = _dev(_pads(B, T, padded), device)
        need = wg.workspace_need(query, eng.handle(), B, T, size, size)
        ss, st, sb = STALE_OF[geom]
        xs, fps = _dev(_video(sb, st, ss), device, bf16), _dev(_pads(sb, st, True), device)
        band = {}

        def run(ws):
            eng._ws["video"] = ws
            out = None
            if kind == "enc":  # the one wrapper that takes the caller's output tensor
                out, band["out"] = wg.banded((B, T * _tokens(size), D), _dt(bf16), device)
            outs = _clip_call(kind, eng, x, fp, extras, out)
            assert eng._ws["video"] is ws
            return outs

        def stale(take):
            eng._ws["video"] = take(wg.workspace_need(query, eng.handle(), sb, st, ss, ss))
            _clip_call(kind, eng, xs, fps, True)

        def ordinary():
            eng._ws["video"] = _oversized(need, device)
            return _clip_call(kind, eng, x, fp, extras)

        def bands(outs):
            return None if not band or wg.band_intact(band["out"]) else "the band behind `out` was written"

        oracle = None if bf16 or u8 else _oracle_outputs(kind, geom, padded, False)
        return wg.Case(label, (entry,), need, run, stale, ordinary, oracle, bands)

    label = f"{CLIP_QUERY[kind][1]} {geom} {'bf16' if bf16 else 'f32'}{' u8' if u8 else ''}" \
            f"{' pads' if padded else ''}{' +outputs' if extras else ''}"
    return label, build


@functools.lru_cache(maxsize=None)
def _states(kind, bf16, size, padded, device):
    """Frame states of NFRAMES frames from an ordinary encode_frames call (its own, engine-allocated workspace)."""
    _, _, eng = _model(kind, bf16)
    eng._ws.pop("spatial", None)
    frames = _dev(_video(1, NFRAMES, size)[0], device, bf16)
    return eng.encode_frames(frames, _dev(_frame_pads(padded), device))


def windows_case(kind, geom, bf16, padded, extras):
    """vp_forward_temporal / vp_clip_encode_video_windows / vp_classifier_forward_windows over windows of states."""
    def build(device):
        _, _, eng = _model(kind, bf16)
        size, T, _ = GEOMS[geom]
        query, entry = WIN_QUERY[kind]
        fs = _states(kind, bf16, size, padded, device)
        idx = torch.tensor(WINDOWS[T], device=device)
        Wn = idx.shape[0]
        assert size == 288 or (Wn * T * _tokens(size)) % 256  # no multiple of the row tile where one can be avoided
        need = wg.workspace_need(query, eng.handle(), Wn, T, size, size)
        ss, st, _ = STALE_OF[geom]
        fss = _states(kind, bf16, ss, True, device)
        idxs = torch.tensor([[3] * st], device=device)

        def run(ws):
            eng._ws["video"] = ws
            outs = _windows_call(kind, eng, fs, idx, extras)
            assert eng._ws["video"] is ws
            return outs

        def stale(take):
            eng._ws["video"] = take(wg.workspace_need(query, eng.handle(), 1, st, ss, ss))
            _windows_call(kind, eng, fss, idxs, True)

        def ordinary():
            eng._ws["video"] = _oversized(need, device)
            return _windows_call(kind, eng, fs, idx, extras)

        oracle = None if bf16 else _oracle_outputs(kind, geom, padded, True)
        return wg.Case(label, (entry,), need, run, stale, ordinary, oracle)

    label = f"{WIN_QUERY[kind][1]} {geom} {'bf16' if bf16 else 'f32'}{' pads' if padded else ''}" \
            f"{' +outputs' if extras else ''}"
    return label, build


def spatial_case(geom, bf16, padded):
    """vp_forward_spatial over the geometry's B * T frames."""
    def build(device):
        _, var, eng = _model("enc", bf16)
        size, T, B = GEOMS[geom]
        F = B * T
        frames = _dev(_video(B, T, size).reshape(F, size, size, 3), device, bf16)
        fp = _dev(None if not padded else _pads(B, T, True).reshape(F), device)
        vh = eng.video_handle()
        need = wg.workspace_need("vp_spatial_workspace_bytes", vh, F, size, size)
        ss, st, sb = STALE_OF[geom]
        fr_s = _dev(_video(sb, st, ss).reshape(sb * st, ss, ss, 3), device, bf16)
        fp_s = _dev(_pads(sb, st, True).reshape(sb * st), device)

        def run(ws):
            eng._ws["spatial"] = ws
            fs = eng.encode_frames(frames, fp)
            assert eng._ws["spatial"] is ws
            return (fs.states,)

        def stale(take):
            eng._ws["spatial"] = take(wg.workspace_need("vp_spatial_workspace_bytes", vh, sb * st, ss, ss))
            eng.encode_frames(fr_s, fp_s)

        def ordinary():
            eng._ws["spatial"] = _oversized(need, device)
            return (eng.encode_frames(frames, fp).states,)

        def oracle(outs):
            sp = var["params"]["spatial_ln"]
            ln = orc.layer_norm(outs[0].double().cpu().numpy(), sp["scale"], sp["bias"], orc.Numerics("f64"))
            ref = _ref_clips("enc", geom, padded, False)["spatial"].reshape(ln.shape)
            e = float(np.abs(ln - ref).max())
            assert e <= 1e-5, e
            return f"oracle max-abs {e:.2e} on spatial_ln(states) (bar 1e-05)"

        return wg.Case(label, ("vp_forward_spatial",), need, run, stale, ordinary, None if bf16 else oracle)

    label = f"vp_forward_spatial {geom} {'bf16' if bf16 else 'f32'}{' pads' if padded else ''}"
    return label, build


def text_case(bf16):
    """vp_clip_encode_text: Q = 3, L = 16, one half-padded and one fully padded row."""
    def build(device):
        _, var, eng = _model("lvt", bf16)
        Q, L = 3, 16
        rng = np.random.default_rng(5)
        ids = rng.integers(0, LVT["vocabulary_size"], (Q, L)).astype(np.int32)
        pads = np.zeros((Q, L), np.float32)
        pads[1, L // 2:] = 1.0
        pads[2, :] = 1.0
        ids_d, pads_d = _dev(ids, device), _dev(pads, device)
        need = wg.workspace_need("vp_clip_text_workspace_bytes", eng.handle(), Q, L)
        ids_s = _dev(rng.integers(0, LVT["vocabulary_size"], (5, 9)).astype(np.int32), device)
        pads_s = torch.ones(5, 9, device=device)

        def run(ws):
            eng._ws["text"] = ws
            out = eng.encode_text(ids_d, pads_d)
            assert eng._ws["text"] is ws
            return (out,)

        def stale(take):
            eng._ws["text"] = take(wg.workspace_need("vp_clip_text_workspace_bytes", eng.handle(), 5, 9))
            eng.encode_text(ids_s, pads_s)

        def ordinary():
            eng._ws["text"] = _oversized(need, device)
            return (eng.encode_text(ids_d, pads_d),)

        def oracle(outs):
            _, t, _ = orc.video_clip(var["params"], LVT, None, ids, pads, "f64")
            e = _maxabs(outs[0], t)
            assert e <= 2e-5, e
            return f"oracle max-abs {e:.2e} (bar 2e-05)"

        return wg.Case(label, ("vp_clip_encode_text",), need, run, stale, ordinary, None if bf16 else oracle)

    label = f"vp_clip_encode_text Q=3 L=16 {'bf16' if bf16 else 'f32'}"
    return label, build


def probe_case(bf16):
    """vp_op_probe_forward + two vp_op_probe_backward on one workspace: D = 256, H = 4, C = 5, B = 2, S = 40.  The
    fill goes in before the forward only; the backward reads what the forward left."""
    def build(device):
        Dm, H, C, B, S = 256, 4, 5, 2, 40
        dims = (Dm, H, C)
        g = torch.Generator().manual_seed(77)
        p = pr.synthetic_head(Dm, H, C, 77)
        tensors = {m: p[path].float().contiguous().to(device) for m, path in nat.PROBE_LEAVES}
        x64 = torch.randn(B, S, Dm, generator=g).to(torch.bfloat16).double()  # bf16-representable in either dtype
        x = x64.to(_dt(bf16)).to(device)
        dl64 = torch.randn(B, C, generator=g).float().double()
        dlogits = dl64.float().to(device)
        need = nat.op_probe_workspace_bytes(*dims, B, S)
        xs = torch.randn(3, 17, Dm, generator=g).to(_dt(bf16)).to(device)
        dls = torch.randn(3, C, generator=g).to(device)

        def call(ws, x, dlogits, backwards):
            logits = torch.empty(x.shape[0], C, device=device)
            emb = torch.empty(x.shape[0], Dm, device=device)
            nat.op_probe_forward(dims, tensors, x, logits, emb, ws)
            grads = []
            for _ in range(backwards):
                gr_ = {m: torch.empty_like(t) for m, t in tensors.items()}
                nat.op_probe_backward(dims, tensors, x, dlogits, gr_, ws)
                grads.append(gr_)
            return logits, emb, grads

        def outputs(logits, emb, grads):
            return (logits, emb) + tuple(gr_[m] for gr_ in grads for m, _ in nat.PROBE_LEAVES)

        def run(ws):
            logits, emb, grads = call(ws, x, dlogits, 2)
            for m, _ in nat.PROBE_LEAVES:  # two backward calls on the same workspace give the same bits
                d = wg.first_difference(grads[0][m], grads[1][m])
                assert d is None, f"second backward on the same workspace: {m}: {d}"
            return outputs(logits, emb, grads)

        def stale(take):
            call(take(nat.op_probe_workspace_bytes(*dims, 3, 17)), xs, dls, 1)

        def ordinary():
            return outputs(*call(_oversized(need, device), x, dlogits, 2))

        def oracle(outs):
            ref_logits, st = pr.forward(x64, p)
            ref = pr.backward(p, st, dl64)
            rel = lambda a, b: ((a.double().cpu() - b).norm() / b.norm()).item()  # noqa: E731
            errs = {"logits": rel(outs[0], ref_logits)}
            for i, (m, path) in enumerate(nat.PROBE_LEAVES):
                if m == "key_b":
                    assert not outs[2 + i].any(), "the key bias's gradient is exactly zero"
                else:
                    errs[m] = rel(outs[2 + i], ref[path])
            assert max(errs.values()) <= 2e-5, errs
            return f"oracle largest relative error {max(errs.values()):.2e} (bar 2e-05)"

        return wg.Case(label, ("vp_op_probe_forward", "vp_op_probe_backward"), need, run, stale, ordinary,
                       None if bf16 else oracle, pointers="any")

    label = f"vp_op_probe_forward+backward D=256 H=4 C=5 B=2 S=40 {'bf16' if bf16 else 'f32'} tokens"
    return label, build


def _unit_rows(rng, n, d):
    a = rng.standard_normal((n, d))
    return (a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-30)).astype(np.float32)


def _topk_finite(t):
    """Scores: never NaN or +inf (-inf is the padding tail's, checked against the restatement); ids: anything."""
    return not t.dtype.is_floating_point or not bool((torch.isnan(t) | (t == float("inf"))).any())


def topk_case(grouped, N, bf16):
    """vp_op_topk / vp_op_topk_groups, Q = 5, D = 128, k = 10: N = 0, N = 7 (fewer rows than k) and N = 5000 (several
    row ranges, fewer than the workspace's fixed bound of parts: part of the lists is never written)."""
    def build(device):
        Q, Dm, k, id_base = 5, 128, 10, 100
        rng = np.random.default_rng(N + 1)
        q = _dev(_unit_rows(rng, Q, Dm), device)
        gal = _dev(_unit_rows(rng, N, Dm), device).to(_dt(bf16))
        labels = torch.arange(N, device=device) // 3
        entry = "vp_op_topk_groups" if grouped else "vp_op_topk"
        need = (nat.op_topk_groups_workspace_bytes if grouped else nat.op_topk_workspace_bytes)(Q, k)
        qs = _dev(_unit_rows(rng, 7, Dm), device)
        gs = _dev(_unit_rows(rng, 900, Dm), device).to(_dt(bf16))
        band = {}

        def call(ws, q, gal, labels, k, keep_bands):
            Qn, Nn = q.shape[0], gal.shape[0]
            outs, bs = zip(*(wg.banded((Qn, k), dt, device, 8) for dt in
                             ((torch.float32, torch.int64, torch.int64) if grouped else (torch.float32, torch.int64))))
            if keep_bands:
                band["b"] = bs
            p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
            stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            with torch.cuda.device(device):
                if grouped:
                    nat.call(entry, p(q), Qn, p(gal), nat._prec(gal), Nn, Dm, Dm, p(labels), k, id_base, p(outs[0]),
                             p(outs[1]), p(outs[2]), p(ws), ws.numel(), stream)
                else:
                    nat.call(entry, p(q), Qn, p(gal), nat._prec(gal), Nn, Dm, Dm, k, id_base, p(outs[0]), p(outs[1]),
                             p(ws), ws.numel(), stream)
            return outs

        def run(ws):
            return call(ws, q, gal, labels, k, True)

        def stale(take):
            st_need = (nat.op_topk_groups_workspace_bytes if grouped else nat.op_topk_workspace_bytes)(7, 33)
            call(take(st_need), qs, gs, torch.arange(900, device=device) % 50, 33, False)

        def ordinary():
            return call(_oversized(need, device), q, gal, labels, k, False)

        def bands(outs):
            return None if all(wg.band_intact(b) for b in band["b"]) else "a band behind scores / ids was written"

        def oracle(outs):
            s64 = gal.double().cpu().numpy() @ q.double().cpu().numpy().T  # [N, Q], of the stored gallery
            if grouped:
                want = gr.group_topk(s64, labels.cpu().numpy(), k, id_base)
            else:
                want = rr.topk(s64, k, id_base)
            got = [t.cpu().numpy() for t in outs]
            tail = np.isneginf(want[0])
            assert np.array_equal(np.isneginf(got[0]), tail)
            for g_, w_ in zip(got[1:], want[1:]):
                assert np.array_equal(g_[tail], w_[tail]) and (g_[tail] == -1).all()
            e = float(np.abs(got[0][~tail] - want[0][~tail]).max()) if (~tail).any() else 0.0
            rows = got[-1][~tail] - id_base
            cols = np.broadcast_to(np.arange(Q)[:, None], tail.shape)[~tail]
            e_own = float(np.abs(s64[rows, cols] - got[0][~tail]).max()) if (~tail).any() else 0.0
            assert e <= 2e-5 and e_own <= 2e-5, (e, e_own)
            return f"oracle max-abs {e:.2e}, against the score of its own id {e_own:.2e} (bar 2e-05)"

        return wg.Case(label, (entry,), need, run, stale, ordinary, oracle, bands, finite=_topk_finite)

    label = f"{'vp_op_topk_groups' if grouped else 'vp_op_topk'} Q=5 D=128 k=10 N={N} " \
            f"{'bf16' if bf16 else 'f32'} gallery"
    return label, build


def _all_cases():
    cases = []
    for bf16 in (True, False):
        for geom in GEOMS:
            for padded in (False, True):
                for kind in ("enc", "lvt", "cls"):
                    for extras in (False, True):
                        cases.append(clips_case(kind, geom, bf16, padded, extras))
                        if geom != "288":  # windows: Wn * T * N not a multiple of the row tile
                            cases.append(windows_case(kind, geom, bf16, padded, extras))
                cases.append(spatial_case(geom, bf16, padded))
        for kind in ("enc", "lvt", "cls"):
            cases.append(clips_case(kind, "288", bf16, False, True, u8=True))
        cases.append(text_case(bf16))
        cases.append(probe_case(bf16))
        for grouped in (False, True):
            for N in (0, 7, 5000):
                cases.append(topk_case(grouped, N, bf16))
    return cases


CASES = dict(_all_cases())
assert len(CASES) == 2 * (3 * 2 * 3 * 2 + 2 * 2 * 3 * 2 + 3 * 2 + 3 + 1 + 1 + 6)


@pytest.mark.parametrize("label", list(CASES), ids=[c.replace(" ", "-") for c in CASES])
def test_workspace_contract(cuda, label):
    wg.check_case(CASES[label](cuda), cuda)


def test_short_slice_takes_the_refusal_path(cuda):
    """The negative control: a helper whose slice is advertised one byte short makes every case refuse (VP_EINVAL
    naming `need`, raised by the wrapper) before anything is launched or written."""
    for label, build in CASES.items():
        wg.check_short_slice(build(cuda), cuda)
    print(f"{len(CASES)} cases refused in need - 1 bytes")


def test_forward_spatial_states_out_band(cuda):
    """The raw C-ABI at 72 x 72: M = 48 rows of states in Mp = 256 / 128 GEMM rows.  vp_forward_spatial computes in
    the workspace and copies M rows out: the one place a padded-row store could leave the caller's buffer.  A band
    behind states_out stays intact under every fill, and the states are the engine's."""
    size, T, B = GEOMS["72"]
    F, N = B * T, _tokens(size)
    for bf16 in (True, False):
        _, _, eng = _model("enc", bf16)
        frames = _dev(_video(B, T, size).reshape(F, 1, size, size, 3), cuda, bf16)
        video, in_dt, fp, *_ = eng._check_video(frames, _dev(_pads(B, T, True).reshape(F, 1), cuda))
        vh = eng.video_handle()
        need = wg.workspace_need("vp_spatial_workspace_bytes", vh, F, size, size)
        gw = wg.GuardedWorkspace(need, cuda)
        eng._ws.pop("spatial", None)
        want = eng.encode_frames(frames[:, 0], fp.reshape(F)).states
        for fill in (0x00, 0xFF, 0x7F):
            gw.fill(fill)
            states, band = wg.banded((F, N, D), _dt(bf16), cuda)
            nat.call("vp_forward_spatial", vh, ctypes.c_void_p(video.data_ptr()), in_dt, F, size, size,
                     ctypes.c_void_p(fp.data_ptr()), ctypes.c_void_p(states.data_ptr()),
                     ctypes.c_void_p(gw.ws.data_ptr()), gw.ws.numel(),
                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert gw.damaged_guard() is None
            assert wg.band_intact(band), f"fill 0x{fill:02X}: the band behind states_out was written"
            assert wg.first_difference(states, want) is None and wg.all_finite(states)
        print(f"vp_forward_spatial 72 {'bf16' if bf16 else 'f32'} raw: need {need}, fills 0x00 0xFF 0x7F, "
              f"band behind states_out intact")
