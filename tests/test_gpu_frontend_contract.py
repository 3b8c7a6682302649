"""The contract of the Python front end (videoprism/encoders.py) on the MI355X: what `apply`, `encode_frames` and
`apply_windows` of the three models accept, and in what container, dtype, shape and on which device they answer.
The behaviour of the front end as it stood before its input and launch paths were merged is the reference; every
case is one line of a table and a forward of a few milliseconds.

Models: Base widths with 1 spatial + 1 temporal layer (`enc`); the LvT Base config with 1 + 1 vision, 1 auxiliary
and 1 text layer and a vocabulary of 1000 (`lvt`); the classifier on the same encoder with 5 classes (`cls`); each
in fp32 and bf16 on synthetic parameters.  Shapes: B = 2 clips of T = 2 frames of 72 x 72 (a 4 x 4 patch grid);
text Q = 2, L = 16 with the second row half padded; windows over F = 4 states with
frame_index = [[0, 1], [2, 3], [3, 2]], frame 3 padded.

Case families (one parametrised table, CASES):
  frames   the six input kinds of the frames (numpy fp32 / uint8, CPU fp32 tensor, CUDA fp32 / bf16 / uint8), with
           frame paddings of the same kind, through `apply` (5-D) and `encode_frames` (4-D): container, dtype,
           shape, device of every returned value (FrameStates: states, paddings None or [F] fp32, frame_size), and
           numpy fp32 == CPU fp32 == CUDA fp32, CUDA fp32 == its .to(bfloat16) for a bf16 model,
           numpy uint8 == CUDA uint8, all bit for bit
  keys     the exact key set of `outputs` for return_intermediate in {False, True, [each name], a pair of names},
           through `apply` and `apply_windows`
  index    frame_index as list / numpy int64 / CPU tensor / CUDA int32 tensor: all equal, and equal to
           `apply(frames[idx], frame_paddings=pads[idx])`
  text     LvT text ids as numpy / CUDA tensor; video-only, text-only and both-at-once calls give the same
           embeddings, through `apply` and `apply_windows`
  refuse   the refusals and their exception types
  empty    B = 0, F = 0, Wn = 0, Q = 0: zero-size results of the right shapes and dtypes, nothing launched (the
           call does not even ask for a workspace)

What the reference does that one might not expect, pinned here as it is:
  * Results are numpy arrays exactly when `inputs` (for `apply_windows`: `frame_index`) and, for the LvT model,
    `text_token_ids` are no torch tensors.  `frame_paddings` and `text_paddings` do not count: numpy frames with
    CUDA paddings give numpy results.
  * A CPU tensor counts as a tensor: it is moved to the current device and the results are CUDA tensors.
  * An fp32 model takes CUDA bf16 frames as they are and answers in fp32.
  * Names in return_intermediate that a model does not know are ignored.
  * `FactorizedEncoder.apply_windows` and `FactorizedVideoClassifier.apply_windows` take no **kwargs, so
    method="x" is a TypeError there and a NotImplementedError everywhere else.
  * A CUDA input's device wins over the current device.  Only one device is visible to a test here, so that rule is
    exercised on cuda:0 alone, where it coincides with the current device.
"""

import functools

import numpy as np
import pytest
import torch

from videoprism import encoders, models, params

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ENC = dict(models.CONFIGS["videoprism_v1_base"], num_spatial_layers=1, num_temporal_layers=1)
LVT = dict(models.CONFIGS["videoprism_lvt_v1_base"], num_spatial_layers=1, num_temporal_layers=1,
           num_auxiliary_layers=1, num_unimodal_layers=1, vocabulary_size=1000)
NUM_CLASSES = 5
B, T, SIZE, F, Q, L = 2, 2, 72, 4, 2, 16
N, D = (SIZE // ENC["patch_size"]) ** 2, ENC["model_dim"]
INDEX = [[0, 1], [2, 3], [3, 2]]
WN = len(INDEX)

KINDS = ("enc", "lvt", "cls")
NAMES = {"enc": ("spatial_features",),
         "lvt": ("spatial_features", "spatiotemporal_features", "frame_embeddings"),
         "cls": ("spatial_features", "spatiotemporal_features", "global_embeddings")}
PAIR = ("spatial_features", "spatiotemporal_features")  # the encoder knows only the first
FRAME_KINDS = ("np_f32", "np_u8", "cpu_f32", "cuda_f32", "cuda_bf16", "cuda_u8")
INDEX_KINDS = ("list", "np_i64", "cpu", "cuda_i32")


def _fdt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


@functools.lru_cache(maxsize=None)
def _model(kind, bf16):
    fd = torch.bfloat16 if bf16 else None
    if kind == "enc":
        m = models.get_model(None, model_fn=lambda: encoders.FactorizedEncoder(**ENC), fprop_dtype=fd)
        var = params.synthetic_params(ENC, seed=41)
    elif kind == "lvt":
        m = models.get_model(None, model_fn=lambda: encoders.FactorizedVideoCLIP(**LVT), fprop_dtype=fd)
        var = params.synthetic_params(LVT, 42, specs=params.clip_leaf_specs(LVT))
    else:
        m = models.get_model(None, model_fn=lambda: encoders.FactorizedVideoClassifier(
            encoder_params=ENC, num_classes=NUM_CLASSES), fprop_dtype=fd)
        var = params.synthetic_params(ENC, 43, specs=m.param_specs())
    return m, var


# ---------------------------------------------------------------------------------------------------------------
# inputs, made once
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_frames():
    """[F, SIZE, SIZE, 3] fp32 in [0, 1); the clips are its two halves."""
    return np.random.default_rng(7).random((F, SIZE, SIZE, 3), dtype=np.float32)


def _frame_pads():
    p = np.zeros(F, np.float32)
    p[F - 1] = 1.0
    return p


def _text():
    ids = np.random.default_rng(8).integers(0, LVT["vocabulary_size"], (Q, L)).astype(np.int32)
    pads = np.zeros((Q, L), np.float32)
    pads[1, L // 2:] = 1.0
    return ids, pads


def _frames_as(host, kind, cuda):
    """`host` (fp32 numpy) as one of FRAME_KINDS."""
    if kind.endswith("u8"):
        host = (host * 255).astype(np.uint8)
    if kind.startswith("np"):
        return host
    t = torch.from_numpy(host)
    if kind.startswith("cuda"):
        t = t.to(cuda)
    return t.to(torch.bfloat16) if kind == "cuda_bf16" else t


def _pads_as(host, kind, cuda):
    """Frame paddings in the container of the frames' kind."""
    if kind.startswith("np"):
        return host
    t = torch.from_numpy(host)
    return t.to(cuda) if kind.startswith("cuda") else t


def _index_as(kind, cuda):
    return {"list": INDEX, "np_i64": np.array(INDEX, np.int64), "cpu": torch.tensor(INDEX),
            "cuda_i32": torch.tensor(INDEX, dtype=torch.int32, device=cuda)}[kind]


# ---------------------------------------------------------------------------------------------------------------
# what a call returns, flattened to {name: value}, and the checks on it
# ---------------------------------------------------------------------------------------------------------------
def _named(kind, result):
    """apply / apply_windows results as one dict: the primary values under their own names, then `outputs`."""
    *primary, outputs = result
    assert type(outputs) is dict
    names = {"enc": ("embeddings",), "lvt": ("video_embeddings", "text_embeddings"), "cls": ("logits",)}[kind]
    assert len(primary) == len(names)
    got = {n: v for n, v in zip(names, primary) if v is not None}
    assert not set(got) & set(outputs)
    got.update(outputs)
    return got


def _shapes(kind, rows, queries=Q):
    """The shape of every value a model can return for `rows` clips (or windows)."""
    return {"embeddings": (rows, T * N, D), "video_embeddings": (rows, D), "text_embeddings": (queries, D),
            "logits": (rows, NUM_CLASSES), "spatial_features": (rows, T * N, D),
            "spatiotemporal_features": (rows, T * N, D), "frame_embeddings": (rows, T, D),
            "global_embeddings": (rows, D)}


def _check_values(got, want_names, shapes, as_numpy, bf16, cuda, what):
    assert set(got) == set(want_names), (what, sorted(got), sorted(want_names))
    for name, v in got.items():
        if as_numpy:
            assert type(v) is np.ndarray and v.dtype == np.float32, (what, name, type(v), getattr(v, "dtype", None))
        else:
            assert isinstance(v, torch.Tensor) and v.dtype == _fdt(bf16) and v.device == cuda, \
                (what, name, type(v), getattr(v, "dtype", None), getattr(v, "device", None))
        assert tuple(v.shape) == shapes[name], (what, name, tuple(v.shape), shapes[name])


def _bits(v):
    a = v if isinstance(v, np.ndarray) else v.float().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for name in a:
        x, y = _bits(a[name]), _bits(b[name])
        assert x.shape == y.shape and np.array_equal(x, y), \
            f"{what}: {name} differs in {int((x != y).sum()) if x.shape == y.shape else 'shape'} elements"


def _primary(kind, text=False):
    return {"enc": ["embeddings"], "lvt": ["video_embeddings"] + (["text_embeddings"] if text else []),
            "cls": ["logits"]}[kind]


def _equal_groups(bf16):
    groups = [("np_f32", "cpu_f32", "cuda_f32"), ("np_u8", "cuda_u8")]
    if bf16:
        groups.append(("cuda_f32", "cuda_bf16"))
    return groups


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
def frames_apply_case(kind, bf16):
    def run(cuda):
        m, var = _model(kind, bf16)
        host = _host_frames().reshape(B, T, SIZE, SIZE, 3)
        pads = _frame_pads().reshape(B, T)
        want = _primary(kind) + list(NAMES[kind])
        got = {}
        for fk in FRAME_KINDS:
            res = m.apply(var, _frames_as(host, fk, cuda), return_intermediate=True,
                          frame_paddings=_pads_as(pads, fk, cuda))
            got[fk] = _named(kind, res)
            _check_values(got[fk], want, _shapes(kind, B), fk.startswith("np"), bf16, cuda, fk)
        for group in _equal_groups(bf16):
            for other in group[1:]:
                _same(got[group[0]], got[other], f"{group[0]} vs {other}")
        # the paddings' container does not decide the results' container
        mixed = _named(kind, m.apply(var, host, return_intermediate=True, frame_paddings=_pads_as(pads, "cuda", cuda)))
        _check_values(mixed, want, _shapes(kind, B), True, bf16, cuda, "numpy frames, CUDA paddings")
        _same(got["np_f32"], mixed, "numpy frames, CUDA paddings")
        # __call__ is apply
        _same(got["cuda_f32"], _named(kind, m(var, _frames_as(host, "cuda_f32", cuda), return_intermediate=True,
                                              frame_paddings=_pads_as(pads, "cuda", cuda))), "__call__")
    return f"frames apply {kind} {'bf16' if bf16 else 'f32'}", run


def _check_states(fs, padded, bf16, cuda, what, num_frames=F):
    assert type(fs) is encoders.FrameStates, what
    assert fs.states.dtype == _fdt(bf16) and fs.states.device == cuda, (what, fs.states.dtype, fs.states.device)
    assert tuple(fs.states.shape) == (num_frames, N, D) and len(fs) == num_frames, (what, tuple(fs.states.shape))
    assert fs.frame_size == (SIZE, SIZE), (what, fs.frame_size)
    if padded:
        p = fs.paddings
        assert isinstance(p, torch.Tensor) and p.dtype == torch.float32 and p.device == cuda, what
        assert tuple(p.shape) == (num_frames,), (what, tuple(p.shape))
    else:
        assert fs.paddings is None, what


def _states_dict(fs):
    d = {"states": fs.states}
    if fs.paddings is not None:
        d["paddings"] = fs.paddings
    return d


def frames_encode_case(kind, bf16):
    def run(cuda):
        m, var = _model(kind, bf16)
        host, pads = _host_frames(), _frame_pads()
        got = {}
        for fk in FRAME_KINDS:
            fs = m.encode_frames(var, _frames_as(host, fk, cuda), _pads_as(pads, fk, cuda))
            _check_states(fs, True, bf16, cuda, fk)
            assert np.array_equal(fs.paddings.cpu().numpy(), pads), fk
            got[fk] = _states_dict(fs)
        for group in _equal_groups(bf16):
            for other in group[1:]:
                _same(got[group[0]], got[other], f"{group[0]} vs {other}")
        plain = m.encode_frames(var, host)
        _check_states(plain, False, bf16, cuda, "no paddings")
    return f"frames encode_frames {kind} {'bf16' if bf16 else 'f32'}", run


def _windows_inputs(kind, bf16, cuda):
    m, var = _model(kind, bf16)
    frames = torch.from_numpy(_host_frames()).to(cuda)
    pads = torch.from_numpy(_frame_pads()).to(cuda)
    return m, var, frames, pads, m.encode_frames(var, frames, pads)


def keys_case(kind, bf16, windows):
    def run(cuda):
        m, var, frames, pads, fs = _windows_inputs(kind, bf16, cuda)
        idx = _index_as("cuda_i32", cuda)
        rows = WN if windows else B
        for ri in [False, True] + [[n] for n in NAMES[kind]] + [PAIR, frozenset(PAIR)]:
            if windows:
                res = m.apply_windows(var, fs, idx, return_intermediate=ri)
            else:
                res = m.apply(var, frames.reshape(B, T, SIZE, SIZE, 3), return_intermediate=ri)
            asked = NAMES[kind] if ri is True else () if ri is False else [n for n in NAMES[kind] if n in ri]
            _check_values(_named(kind, res), _primary(kind) + list(asked), _shapes(kind, rows), False, bf16, cuda,
                          f"return_intermediate={ri!r}")
    return f"keys {'apply_windows' if windows else 'apply'} {kind} {'bf16' if bf16 else 'f32'}", run


def index_case(kind, bf16):
    def run(cuda):
        m, var, frames, pads, fs = _windows_inputs(kind, bf16, cuda)
        want = _primary(kind) + list(NAMES[kind])
        got = {}
        for ik in INDEX_KINDS:
            got[ik] = _named(kind, m.apply_windows(var, fs, _index_as(ik, cuda), return_intermediate=True))
            _check_values(got[ik], want, _shapes(kind, WN), ik in ("list", "np_i64"), bf16, cuda, ik)
        for ik in INDEX_KINDS[1:]:
            _same(got["list"], got[ik], f"frame_index list vs {ik}")
        gather = torch.tensor(INDEX, device=cuda)
        clips = _named(kind, m.apply(var, frames[gather], return_intermediate=True, frame_paddings=pads[gather]))
        _same(clips, got["cuda_i32"], "apply on the gathered clips vs apply_windows")
        assert float(pads[gather].sum()) == 2.0  # the padded frame is in two windows
    return f"index {kind} {'bf16' if bf16 else 'f32'}", run


def text_case(bf16):
    def run(cuda):
        kind = "lvt"
        m, var, frames, pads, fs = _windows_inputs(kind, bf16, cuda)
        ids, tpads = _text()
        ids_d, tpads_d = torch.from_numpy(ids).to(cuda), torch.from_numpy(tpads).to(cuda)
        clips_h = _host_frames().reshape(B, T, SIZE, SIZE, 3)
        clips_d = frames.reshape(B, T, SIZE, SIZE, 3)
        idx_h, idx_d = np.array(INDEX, np.int32), _index_as("cuda_i32", cuda)
        both = ["video_embeddings", "text_embeddings"]

        # apply: text only (numpy, CUDA), video only, both at once
        t_np = _named(kind, m.apply(var, None, ids, tpads))
        _check_values(t_np, ["text_embeddings"], _shapes(kind, B), True, bf16, cuda, "text only, numpy")
        t_cu = _named(kind, m.apply(var, None, ids_d, tpads_d))
        _check_values(t_cu, ["text_embeddings"], _shapes(kind, B), False, bf16, cuda, "text only, CUDA")
        _same(t_np, t_cu, "numpy ids vs CUDA ids")
        mixed_pads = _named(kind, m.apply(var, None, ids, tpads_d))  # the paddings' container does not count
        _check_values(mixed_pads, ["text_embeddings"], _shapes(kind, B), True, bf16, cuda, "numpy ids, CUDA paddings")
        _same(t_np, mixed_pads, "numpy ids, CUDA paddings")
        v_np = _named(kind, m.apply(var, clips_h))
        _check_values(v_np, ["video_embeddings"], _shapes(kind, B), True, bf16, cuda, "video only, numpy")
        vt_np = _named(kind, m.apply(var, clips_h, ids, tpads))
        _check_values(vt_np, both, _shapes(kind, B), True, bf16, cuda, "both, numpy")
        _same(vt_np, {**v_np, **t_np}, "both at once vs video only + text only")
        for x, i, what in ((clips_h, ids_d, "numpy frames, CUDA ids"), (clips_d, ids, "CUDA frames, numpy ids"),
                           (clips_d, ids_d, "CUDA frames, CUDA ids")):
            vt = _named(kind, m.apply(var, x, i, tpads_d))
            _check_values(vt, both, _shapes(kind, B), False, bf16, cuda, what)  # one tensor among them: tensors out
            _same(vt_np, vt, what)

        # apply_windows: the same over the windows
        w_np = _named(kind, m.apply_windows(var, fs, idx_h))
        _check_values(w_np, ["video_embeddings"], _shapes(kind, WN), True, bf16, cuda, "windows only, numpy")
        tw_np = _named(kind, m.apply_windows(var, text_token_ids=ids, text_paddings=tpads))
        _check_values(tw_np, ["text_embeddings"], _shapes(kind, WN), True, bf16, cuda, "windows: text only, numpy")
        _same(tw_np, t_np, "apply_windows text only vs apply text only")
        tw_cu = _named(kind, m.apply_windows(var, None, None, ids_d, tpads_d))
        _check_values(tw_cu, ["text_embeddings"], _shapes(kind, WN), False, bf16, cuda, "windows: text only, CUDA")
        _same(tw_cu, t_np, "apply_windows CUDA ids vs apply numpy ids")
        wt_np = _named(kind, m.apply_windows(var, fs, idx_h, ids, tpads))
        _check_values(wt_np, both, _shapes(kind, WN), True, bf16, cuda, "windows: both, numpy")
        _same(wt_np, {**w_np, **t_np}, "windows: both at once vs video only + text only")
        for i, t, what in ((idx_h, ids_d, "numpy index, CUDA ids"), (idx_d, ids, "CUDA index, numpy ids"),
                           (idx_d, ids_d, "CUDA index, CUDA ids")):
            wt = _named(kind, m.apply_windows(var, fs, i, t, tpads))
            _check_values(wt, both, _shapes(kind, WN), False, bf16, cuda, what)
            _same(wt_np, wt, what)
    return f"text lvt {'bf16' if bf16 else 'f32'}", run


def refuse_case(kind, bf16):
    def run(cuda):
        m, var, frames, pads, fs = _windows_inputs(kind, bf16, cuda)
        clips = frames.reshape(B, T, SIZE, SIZE, 3)
        idx = _index_as("cuda_i32", cuda)
        for x in (frames, frames.cpu().numpy()):  # a 4-D `inputs`, a 5-D `frames`
            with pytest.raises(ValueError, match=r"\[B, T, H, W, 3\]"):
                m.apply(var, x)
        for x in (clips, clips.cpu().numpy()):
            with pytest.raises(ValueError, match=r"\[F, H, W, 3\]"):
                m.encode_frames(var, x)
        tall = np.zeros((B, T, SIZE, SIZE - 18, 3), np.float32)  # H != W
        for x in (tall, torch.from_numpy(tall).to(cuda)):
            with pytest.raises(AssertionError):
                m.apply(var, x)
            with pytest.raises(AssertionError):
                m.encode_frames(var, x[0])
        for bad in (np.zeros((B, T + 1), np.float32), torch.zeros(B * T, device=cuda)):
            with pytest.raises(AssertionError, match="frame_paddings"):
                m.apply(var, clips, frame_paddings=bad)
        for bad in (np.zeros(F + 1, np.float32), torch.zeros(F - 1, device=cuda)):
            with pytest.raises(AssertionError, match="frame_paddings"):
                m.encode_frames(var, frames, bad)
        with pytest.raises(NotImplementedError, match="method="):
            m.apply(var, clips, method="x")
        with pytest.raises(NotImplementedError if kind == "lvt" else TypeError, match="method"):
            m.apply_windows(var, fs, idx, method="x")
        m.apply(var, clips, method=None)  # the default spelled out is no refusal
        if kind == "lvt":
            ids, tpads = _text()
            with pytest.raises(AssertionError, match="paddings"):
                m.apply(var, None, ids)
            with pytest.raises(AssertionError, match="paddings"):
                m.apply_windows(var, text_token_ids=torch.from_numpy(ids).to(cuda))
            with pytest.raises(AssertionError, match="frame_index"):
                m.apply_windows(var, fs)
            with pytest.raises(NotImplementedError, match="method="):
                m.apply_windows(var, text_token_ids=ids, text_paddings=tpads, method="x")
    return f"refuse {kind} {'bf16' if bf16 else 'f32'}", run


def empty_case(kind, bf16):
    def run(cuda):
        m, var, frames, pads, fs = _windows_inputs(kind, bf16, cuda)
        eng = m.engine(var, cuda.index)
        saved = dict(eng._ws)
        eng._ws.clear()  # a call that launches asks for its workspace first
        try:
            none = np.zeros((0, T, SIZE, SIZE, 3), np.float32)
            for x, as_numpy in ((none, True), (torch.from_numpy(none).to(cuda), False)):
                got = _named(kind, m.apply(var, x, return_intermediate=True))
                _check_values(got, _primary(kind) + list(NAMES[kind]), _shapes(kind, 0), as_numpy, bf16, cuda,
                              f"B = 0, numpy {as_numpy}")
            for x, p in ((none[:, 0], None), (torch.from_numpy(none[:, 0]).to(cuda), torch.zeros(0, device=cuda))):
                _check_states(m.encode_frames(var, x, p), p is not None, bf16, cuda, "F = 0", num_frames=0)
            for idx, as_numpy in ((np.zeros((0, T), np.int32), True),
                                  (torch.zeros((0, T), dtype=torch.int32, device=cuda), False)):
                got = _named(kind, m.apply_windows(var, fs, idx, return_intermediate=True))
                _check_values(got, _primary(kind) + list(NAMES[kind]), _shapes(kind, 0), as_numpy, bf16, cuda,
                              f"Wn = 0, numpy {as_numpy}")
            if kind == "lvt":
                ids, tpads = np.zeros((0, L), np.int32), np.zeros((0, L), np.float32)
                for i, p, as_numpy in ((ids, tpads, True),
                                       (torch.from_numpy(ids).to(cuda), torch.from_numpy(tpads).to(cuda), False)):
                    for res in (m.apply(var, None, i, p), m.apply_windows(var, text_token_ids=i, text_paddings=p)):
                        _check_values(_named(kind, res), ["text_embeddings"], _shapes(kind, 0, queries=0), as_numpy,
                                      bf16, cuda, f"Q = 0, numpy {as_numpy}")
            assert not eng._ws, f"an empty batch asked for a workspace: {sorted(eng._ws)}"
        finally:
            eng._ws.update(saved)
    return f"empty {kind} {'bf16' if bf16 else 'f32'}", run


def _all_cases():
    cases = []
    for bf16 in (False, True):
        for kind in KINDS:
            cases += [frames_apply_case(kind, bf16), frames_encode_case(kind, bf16), keys_case(kind, bf16, False),
                      keys_case(kind, bf16, True), index_case(kind, bf16), refuse_case(kind, bf16),
                      empty_case(kind, bf16)]
        cases.append(text_case(bf16))
    return cases


CASES = dict(_all_cases())
assert len(CASES) == 2 * (3 * 7 + 1)


@pytest.mark.parametrize("label", list(CASES), ids=[c.replace(" ", "-") for c in CASES])
def test_frontend_contract(cuda, label):
    CASES[label](cuda)
