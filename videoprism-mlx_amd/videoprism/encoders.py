"""FactorizedEncoder host object backed by libvideoprism_hip.so.

Mirrors the reference module `encoders.FactorizedEncoder` (encoders.py:391-580) as used
through Flax: attributes = the CONFIGS keys, `init(rng, inputs, train=False)` returns
{'params': tree} and `apply(variables, inputs, train=False, return_intermediate=False,
frame_paddings=None)` returns `(embeddings [B, T*N, D], outputs)`.  All arithmetic runs
in the HIP kernels behind the C-ABI; this file only moves parameters and buffers.
"""

from __future__ import annotations

import contextlib
import ctypes
import dataclasses
import weakref
from collections.abc import Collection
from typing import Any

import numpy as np

from . import _native
from . import params as params_lib


def _contains(collection, key: str) -> bool:
    """encoders.py:36-47."""
    return collection if isinstance(collection, bool) else key in collection


def _torch():
    import torch
    return torch


def _is_bf16_dtype(dt) -> bool:
    if dt is None:
        return False
    name = getattr(dt, "name", None) or getattr(dt, "__name__", None) or str(dt)
    return "bfloat16" in str(name) or "bfloat16" in str(dt)


def _check_device(t, device: int, what: str) -> None:
    """Tensors handed to the C-ABI must live on the handle's device (raw pointers + its stream)."""
    if not t.is_cuda or t.device.index != device:
        raise ValueError(f"{what} must be on cuda:{device} (the engine's device), got {t.device}")


def _profile_class_names() -> list:
    lib = _native.load()
    names = []
    for i in range(lib.vp_profile_class_count()):
        name = ctypes.c_char_p()
        _native.call("vp_profile_class_name", i, ctypes.byref(name))
        names.append(name.value.decode())
    return names


def _vp_config(cfg: dict, fprop_code: int):
    return _native.vp_config(
        patch_size=cfg["patch_size"], pos_emb_t=cfg["pos_emb_shape"][0],
        pos_emb_h=cfg["pos_emb_shape"][1], pos_emb_w=cfg["pos_emb_shape"][2],
        model_dim=cfg["model_dim"], num_spatial_layers=cfg["num_spatial_layers"],
        num_temporal_layers=cfg["num_temporal_layers"], num_heads=cfg["num_heads"],
        mlp_dim=cfg["mlp_dim"], atten_logit_cap=float(cfg.get("atten_logit_cap", 0.0)),
        fprop_dtype=fprop_code)


class FrameStates:
    """Per-frame spatial states of one frame size: what `encode_frames` computes once per frame and
    `apply_windows` reads any number of windows from.

      states      CUDA tensor [F, N, D] in the model's fprop dtype: the spatial residual stream after the last
                  spatial layer, before spatial_ln (not the reference's post-LN 'spatial_features')
      paddings    CUDA fp32 tensor [F] (1 = padded frame) or None
      frame_size  (H, W) of the frames

    A state depends on its frame's pixels and padding only, so states may be sliced (`fs[a:b]`) and concatenated
    (`FrameStates.cat([...])`) freely: a stream appends the new frames' states and drops the old ones."""

    def __init__(self, states, paddings, frame_size):
        if states.dim() != 3:
            raise ValueError(f"states must be [F, N, D], got {tuple(states.shape)}")
        if paddings is not None and tuple(paddings.shape) != (states.shape[0],):
            raise ValueError(f"paddings must be [{states.shape[0]}], got {tuple(paddings.shape)}")
        self.states = states
        self.paddings = paddings
        self.frame_size = (int(frame_size[0]), int(frame_size[1]))

    def __len__(self) -> int:
        return self.states.shape[0]

    def __getitem__(self, key) -> "FrameStates":
        if not isinstance(key, slice):
            raise TypeError("FrameStates takes slices only (fs[a:b]); windows pick single frames by frame_index")
        return FrameStates(self.states[key], None if self.paddings is None else self.paddings[key], self.frame_size)

    @staticmethod
    def cat(parts) -> "FrameStates":
        """The states of `parts` (FrameStates of one model and frame size) one after the other; frames of a part
        without paddings count as unpadded when another part has them."""
        parts = list(parts)
        if not parts:
            raise ValueError("FrameStates.cat needs at least one part")
        torch = _torch()
        first = parts[0]
        for q in parts[1:]:
            if q.frame_size != first.frame_size or q.states.shape[1:] != first.states.shape[1:] or \
                    q.states.dtype != first.states.dtype or q.states.device != first.states.device:
                raise ValueError("FrameStates.cat: parts differ in frame size, widths, dtype or device")
        full = [q for q in parts if len(q)]
        if len(full) == 1:  # nothing to join: no copy
            return full[0]
        pads = None
        if any(q.paddings is not None for q in parts):
            pads = torch.cat([q.paddings if q.paddings is not None else
                              torch.zeros(len(q), dtype=torch.float32, device=q.states.device) for q in parts])
        return FrameStates(torch.cat([q.states for q in parts]), pads, first.frame_size)


def _pick_device(*arrays) -> int:
    """The device a call runs on: that of a CUDA tensor among its array arguments (the last one given), otherwise
    the current device.  Everything else is moved there."""
    torch = _torch()
    device = torch.cuda.current_device()
    for t in arrays:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            device = t.device.index
    return device


def _wants_numpy(*arrays) -> bool:
    """Results are numpy arrays unless one of these arguments came as a torch tensor."""
    torch = _torch()
    return not any(isinstance(t, torch.Tensor) for t in arrays)


def _frames_on_device(frames, rank: int, bf16: bool, device: int):
    """Clips [B, T, H, W, 3] (rank 5) or frames [F, H, W, 3] (rank 4), numpy or torch, as a CUDA tensor on
    cuda:`device`.  numpy uint8 travels as bytes (4x less H2D than fp32) and is normalised /255 on device exactly
    as video_utils.py:94; any other numpy dtype goes as fp32; fp32 becomes bf16 for a bf16 model (colab usage:
    inputs cast to the fprop dtype by the caller)."""
    torch = _torch()
    if isinstance(frames, torch.Tensor):
        x = frames
    else:
        arr = np.asarray(frames)
        x = torch.from_numpy(np.ascontiguousarray(arr if arr.dtype == np.uint8 else
                                                  arr.astype(np.float32, copy=False)))
    x = x.to(f"cuda:{device}")
    if x.dim() != rank:
        raise ValueError(f"inputs must be [B, T, H, W, 3], got {tuple(x.shape)}" if rank == 5 else
                         f"frames must be [F, H, W, 3], got {tuple(x.shape)}")
    assert x.shape[-3] == x.shape[-2]  # encoders.py:435
    if bf16 and x.dtype == torch.float32:
        x = x.to(torch.bfloat16)
    return x


class _CheckedIndex:
    """A frame_index [Wn, T] that `_frame_index` has already validated against `num_frames` states."""

    def __init__(self, tensor, num_frames: int):
        self.tensor = tensor
        self.num_frames = num_frames


def _frame_index(frame_index, num_frames: int):
    """frame_index [Wn, T] as a torch integer tensor.  A host index (numpy, list, CPU tensor) is range-checked
    against the `num_frames` states (IndexError) and comes back as a CPU int32 tensor; a CUDA tensor comes back as it
    is, unchecked, since reading it would synchronise: the kernel clamps it to the states.  A _CheckedIndex for the
    same number of states is not checked again."""
    torch = _torch()
    if isinstance(frame_index, _CheckedIndex) and frame_index.num_frames == num_frames:
        return frame_index.tensor
    if isinstance(frame_index, torch.Tensor) and frame_index.is_cuda:
        if frame_index.dtype.is_floating_point or frame_index.dtype == torch.bool:
            raise TypeError("frame_index must be an integer tensor")
        idx = frame_index
    else:
        host = frame_index.numpy() if isinstance(frame_index, torch.Tensor) else np.asarray(frame_index)
        if host.dtype.kind not in "iu":
            raise TypeError("frame_index must hold integers")
        if host.size and (int(host.min()) < 0 or int(host.max()) >= num_frames):
            raise IndexError(f"frame_index out of range for {num_frames} frames: "
                             f"[{int(host.min())}, {int(host.max())}]")
        idx = torch.from_numpy(np.ascontiguousarray(host.astype(np.int32)))
    if idx.dim() != 2 or idx.shape[1] < 1:
        raise ValueError(f"frame_index must be [Wn, T] with T >= 1, got {tuple(idx.shape)}")
    if idx.shape[0] > 0 and num_frames == 0:
        raise IndexError("frame_index points into states that hold no frames")
    return idx


def _states_device(states) -> int:
    """The device index of the FrameStates handed to apply_windows."""
    if not isinstance(states, FrameStates):
        raise TypeError("states must be the FrameStates that encode_frames returns")
    if not states.states.is_cuda:
        raise ValueError(f"states must be on a cuda device, got {states.states.device}")
    return states.states.device.index


def _as_paddings(p):
    torch = _torch()
    if p is None or isinstance(p, torch.Tensor):
        return p
    return torch.from_numpy(np.asarray(p, dtype=np.float32))


def _encode_text(eng, ids, paddings, normalize: bool):
    """Text ids and paddings [Q, L] (numpy or torch) on the engine's device -> eng.encode_text."""
    torch = _torch()
    assert paddings is not None, "Text paddings are required."
    if not isinstance(ids, torch.Tensor):
        ids = torch.from_numpy(np.asarray(ids, dtype=np.int32))
    dev = f"cuda:{eng.device}"
    return eng.encode_text(ids.to(dev), _as_paddings(paddings).to(dev), normalize)


def _pack(primary, named, fprop_dtype, as_numpy: bool):
    """What `apply` returns: the `primary` results (None stays None), then `outputs` built from the (name, buffer
    or None) pairs whose buffer exists; every value cast to the fprop dtype (encoders.py:50-67 casts the normalised
    fp32 vector back), and an fp32 numpy array if `as_numpy`."""
    def cvt(t):
        if t is None:
            return None
        t = t.to(fprop_dtype)
        return t.float().cpu().numpy() if as_numpy else t
    return (*(cvt(t) for t in primary), {k: cvt(v) for k, v in named if v is not None})


def _c_args(args) -> list:
    """C-ABI arguments: a tensor stands for its address."""
    torch = _torch()
    return [_native._ptr(a) if isinstance(a, torch.Tensor) else a for a in args]


@dataclasses.dataclass
class _Source:
    """What a video forward reads, as `_check_video` (clips) or `_check_windows` (windows of frame states) found it
    fit for the C-ABI.  Every engine has one entry point and one workspace query per kind of source: the entry
    point takes (handle, *lead, B, T, H, W, fp, ...), the query (handle, B, T, H, W)."""

    windows: bool  # which of the engine's two entry points and workspace queries
    lead: tuple    # clips: (video, its dtype code); windows: (states [F, N, D], F, frame_index int32 [Wn, T])
    B: int         # clips, or windows (Wn)
    T: int
    H: int
    W: int
    N: int         # tokens per frame
    fp: Any        # frame paddings [B, T] fp32 on the device, or None
    device: Any    # where the results are allocated

    def __iter__(self):
        """Unpacks as the C arguments in call order: for clips (video, dtype code, fp, B, T, H, W, N)."""
        return iter((*self.lead, self.fp, self.B, self.T, self.H, self.W, self.N))


class _EngineBase:
    """One native handle (packed weights on one device) plus its grow-only workspaces.  A subclass
    names its C entry points (`_PREFIX`_create / _set_param / _finalize / _destroy) and gives the
    arguments of its create call ahead of (device, &handle), and its video entry points and their
    workspace queries as (over clips, over windows of frame states).  Every public call takes `stream=`:
    with it, all device work of the call is ordered on that stream (`_ordered_on`)."""

    _PREFIX = ""
    _ENTRY = _QUERY = ("", "")

    def __init__(self, cfg: dict, flat_params: dict, device: int, bf16: bool):
        self.cfg = dict(cfg)
        self.device = device
        self.bf16 = bf16
        lib = _native.load()
        fn = lambda name: getattr(lib, f"{self._PREFIX}_{name}")  # noqa: E731
        h = ctypes.c_void_p()
        _native.check(fn("create")(*self._create_args(), device, ctypes.byref(h)))
        try:
            for name, arr in flat_params.items():
                a = np.ascontiguousarray(arr, dtype=np.float32)
                shape = (ctypes.c_int64 * a.ndim)(*a.shape)
                _native.check(fn("set_param")(h, name.encode(), a.ctypes.data_as(ctypes.c_void_p),
                                              shape, a.ndim))
            _native.check(fn("finalize")(h))
        except Exception:
            fn("destroy")(h)
            raise
        self._h = h
        # bound to the library's function and the handle value, not to this object or the module's
        # globals: it still runs (once) when the interpreter is shutting down
        weakref.finalize(self, fn("destroy"), h)
        self._ws = {}
        self._grids = set()

    def _create_args(self) -> tuple:
        raise NotImplementedError

    @property
    def fprop_dtype(self):
        """The model's fprop dtype as a torch dtype."""
        return _torch().bfloat16 if self.bf16 else _torch().float32

    @property
    def fprop_code(self) -> int:
        """The model's fprop dtype as the C-ABI's VP_* code."""
        return _native.VP_BF16 if self.bf16 else _native.VP_F32

    def handle(self):
        """The native handle itself (vp_handle / vp_clip / vp_classifier), for the _native.dev_* entries."""
        return self._h

    def video_handle(self):
        """The vp_handle of the encoder (its profiler and positional tables live there)."""
        v = ctypes.c_void_p()
        _native.call(f"{self._PREFIX}_video_handle", self._h, ctypes.byref(v))
        return v

    # -- live per-kernel timing (HIP events on the launch stream, vp_profile_*) ---------
    def profile_enable(self, capacity: int) -> None:
        """HIP events around every launch of the handle (for an LvT engine: both towers)."""
        _native.call("vp_profile_enable", self.video_handle(), int(capacity))

    def profile_only(self, names=None) -> None:
        """Restrict events to the named kernel classes (None: all)."""
        mask = 0xFFFFFFFF
        if names is not None:
            mask = sum(1 << i for i, name in enumerate(_profile_class_names()) if name in names)
        _native.call("vp_profile_set_mask", self.video_handle(), mask)

    def profile_read(self) -> dict:
        """{kernel class: {ms, flops, bytes, launches}} since the previous read (vp_profile_read)."""
        names = _profile_class_names()
        n = len(names)
        ms = (ctypes.c_double * n)()
        fl = (ctypes.c_double * n)()
        by = (ctypes.c_double * n)()
        la = (ctypes.c_int64 * n)()
        _native.call("vp_profile_read", self.video_handle(), n, ms, fl, by, la)
        return {names[i]: dict(ms=ms[i], flops=fl[i], bytes=by[i], launches=la[i])
                for i in range(n) if la[i]}

    def kernel_name(self, cls_name: str) -> str:
        """Short symbol of the kernel behind profiler class `cls_name` (last launch)."""
        return _native.profile_kernel_name(self.video_handle(), cls_name)

    def _workspace(self, key: str, query: str, *dims, handle=None):
        """The cached workspace `key`, regrown if `query`(handle, *dims, &bytes) asks for more."""
        n = ctypes.c_size_t()
        _native.call(query, self._h if handle is None else handle, *dims, ctypes.byref(n))
        ws = self._ws.get(key)
        if ws is None or ws.numel() < n.value:
            ws = self._ws[key] = None  # the old one is freed before the new one is allocated
            ws = _torch().empty(max(n.value, 256), dtype=_torch().uint8, device=f"cuda:{self.device}")
            self._ws[key] = ws
        return ws

    def _stream(self, stream):
        s = stream if stream is not None else _torch().cuda.current_stream(self.device)
        return ctypes.c_void_p(s.cuda_stream)

    def _ordered_on(self, stream):
        """The context every public call of an engine runs in.  With `stream=` given, all device work of the call is
        ordered on that stream: the engine's own torch operations (casts, .contiguous(), the gather of the windows'
        paddings), the allocation of the results and of a regrown workspace, and the native launches.  The inputs
        only have to be ready on `stream`, whatever torch's current stream is, and the returned tensors belong to
        `stream`: a consumer on another stream waits for it (and calls Tensor.record_stream) as for any tensor made
        on a side stream.  With stream=None nothing is entered: the call runs on torch's current stream."""
        return contextlib.nullcontext() if stream is None else _torch().cuda.stream(stream)

    def _check_video(self, video, frame_paddings) -> _Source:
        """The clips `video` [B, T, H, W, 3] and their frame paddings [B, T] or None as a _Source, with the
        positional tables for this frame size and clip length prepared."""
        torch = _torch()
        if video.dim() != 5:
            raise ValueError(f"inputs must be [B, T, H, W, 3], got {tuple(video.shape)}")
        B, T, H, W, C = video.shape
        if C != 3:
            raise ValueError("inputs must have 3 channels")
        N = self._tokens_per_frame(H, W)
        _check_device(video, self.device, "video")
        video = video.contiguous()
        if video.dtype not in (torch.bfloat16, torch.float32, torch.uint8):
            video = video.float()
        fp = None
        if frame_paddings is not None:
            fp = frame_paddings.to(device=video.device, dtype=torch.float32).contiguous()
            if tuple(fp.shape) != (B, T):
                raise AssertionError(f"frame_paddings.shape == {(B, T)} failed (encoders.py:442)")
        self._prepare_tables(H, W, T)
        # uint8 frames are normalised /255 on device
        return _Source(False, (video, _native._prec(video)), B, T, H, W, N, fp, video.device)

    def _tokens_per_frame(self, H: int, W: int) -> int:
        P = self.cfg["patch_size"]
        if H % P or W % P:
            raise ValueError(f"Image height ({H}) and width ({W}) should be multiples of patch_size ({P}).")
        return (H // P) * (W // P)

    def _prepare_tables(self, H: int, W: int, T: int) -> None:
        """First sight of a frame size / clip length: the interpolated spatial (encoders.py:497-512) and temporal
        (:543-553) positional tables, cached on the device by the library (the forward itself never allocates)."""
        if (H, W) not in self._grids:
            _native.call("vp_prepare_geometry", self.video_handle(), H, W)
            self._grids.add((H, W))
        if T not in self._grids:
            _native.call("vp_prepare_frames", self.video_handle(), T)
            self._grids.add(T)

    # -- sliding windows: per-frame states once, then windows of them -------------------
    def encode_frames(self, frames, frame_paddings=None, stream=None) -> FrameStates:
        """frames: CUDA tensor [F, H, W, 3] (fp32, bf16 or uint8) on this engine's device; frame_paddings [F] or
        None.  The spatial half of the encoder, once per frame (vp_forward_spatial)."""
        if frames.dim() != 4:
            raise ValueError(f"frames must be [F, H, W, 3], got {tuple(frames.shape)}")
        with self._ordered_on(stream):
            src = self._check_video(frames.unsqueeze(1),
                                    None if frame_paddings is None else frame_paddings.reshape(-1, 1))
            F = src.B
            states = _torch().empty((F, src.N, self.cfg["model_dim"]), dtype=self.fprop_dtype, device=src.device)
            fp = None if src.fp is None else src.fp.reshape(F)
            if F > 0:
                vh = self.video_handle()
                ws = self._workspace("spatial", "vp_spatial_workspace_bytes", F, src.H, src.W, handle=vh)
                _native.call("vp_forward_spatial", vh, *_c_args(src.lead), F, src.H, src.W,
                             *_c_args((fp, states, ws)), ws.numel(), self._stream(stream))
        return FrameStates(states, fp, (src.H, src.W))

    def _check_windows(self, fs: FrameStates, frame_index) -> _Source:
        """Windows `frame_index` [Wn, T] of the frame states `fs` as a _Source (the index as device int32, the
        windows' frame paddings gathered), with the positional tables prepared.  A host frame_index is range-checked
        (IndexError); a CUDA tensor is not, since that would synchronise: the kernel clamps it."""
        torch = _torch()
        if not isinstance(fs, FrameStates):
            raise TypeError("states must be the FrameStates that encode_frames returns")
        st = fs.states
        _check_device(st, self.device, "states")
        H, W = fs.frame_size
        N, D = self._tokens_per_frame(H, W), self.cfg["model_dim"]
        if st.dim() != 3 or tuple(st.shape[1:]) != (N, D):
            raise ValueError(f"states must be [F, {N}, {D}] for this model and frame size, got {tuple(st.shape)}")
        if st.dtype != self.fprop_dtype:
            raise ValueError(f"states must be {self.fprop_dtype} (this model's fprop dtype), got {st.dtype}")
        F = st.shape[0]
        idx = _frame_index(frame_index, F)
        if idx.is_cuda:
            _check_device(idx, self.device, "frame_index")
        Wn, T = idx.shape
        idx = idx.to(device=st.device, dtype=torch.int32).contiguous()
        fp = None
        if fs.paddings is not None and Wn > 0:
            _check_device(fs.paddings, self.device, "states.paddings")
            fp = fs.paddings.to(torch.float32)[idx.clamp(0, F - 1).long()].contiguous()
        self._prepare_tables(H, W, T)  # the frame size too: states carried over from another engine of the model
        return _Source(True, (st.contiguous(), F, idx), Wn, T, H, W, N, fp, st.device)

    def _launch(self, src: _Source, *results, stream=None) -> None:
        """This engine's entry point for `src` (_ENTRY, with its workspace query _QUERY: clips, windows):
        (handle, *src.lead, B, T, H, W, frame paddings, *results, workspace, its size, stream)."""
        dims = (src.B, src.T, src.H, src.W)
        ws = self._workspace("video", self._QUERY[src.windows], *dims)
        _native.call(self._ENTRY[src.windows], self._h, *_c_args(src.lead), *dims, *_c_args((src.fp, *results, ws)),
                     ws.numel(), self._stream(stream))

    def _features(self, want: bool, src: _Source):
        """A [B, T*N, D] buffer in the fprop dtype for spatial / spatio-temporal features, if wanted."""
        return _torch().empty((src.B, src.T * src.N, self.cfg["model_dim"]), dtype=self.fprop_dtype,
                              device=src.device) if want else None


class Engine(_EngineBase):
    """One vp_handle (packed weights on one device) plus a reusable workspace."""

    _PREFIX = "vp"
    _ENTRY = ("vp_forward", "vp_forward_temporal")
    _QUERY = ("vp_workspace_bytes", "vp_temporal_workspace_bytes")

    def _create_args(self):
        return (ctypes.byref(_vp_config(self.cfg, self.fprop_code)),)

    def video_handle(self):
        return self._h

    def workspace(self, B, T, H, W):
        return self._workspace("video", self._QUERY[0], B, T, H, W)

    def _run(self, src: _Source, out_dtype=None, want_spatial=False, out=None, stream=None):
        """-> (embeddings [B, T*N, D], spatial features or None) of the clips or windows `src`."""
        torch = _torch()
        shape = (src.B, src.T * src.N, self.cfg["model_dim"])
        if out is None:
            out = torch.empty(shape, dtype=out_dtype or self.fprop_dtype, device=src.device)
        else:  # the kernels write B*T*N*D elements through the raw pointer
            _check_device(out, self.device, "out")
            if tuple(out.shape) != shape or out.dtype not in (torch.bfloat16, torch.float32) \
                    or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous bf16/fp32 tensor of shape {shape}, "
                                 f"got {tuple(out.shape)} {out.dtype} contiguous={out.is_contiguous()}")
        sp = torch.empty_like(out) if want_spatial else None
        if src.B:  # otherwise an empty batch: the reference's zero-size result, nothing to launch
            self._launch(src, out, _native._prec(out), sp, stream=stream)
        return out, sp

    def forward(self, video, frame_paddings=None, out_dtype=None, want_spatial=False,
                out=None, stream=None):
        """video: CUDA tensor [B,T,H,W,3] (fp32, bf16 or uint8) on this engine's device.  stream: see
        _EngineBase._ordered_on (all device work of the call, the results' allocation included, is on it)."""
        with self._ordered_on(stream):
            return self._run(self._check_video(video, frame_paddings), out_dtype, want_spatial, out, stream)

    def forward_windows(self, fs: FrameStates, frame_index, out_dtype=None, want_spatial=False, stream=None):
        """The temporal half over windows of frame states (vp_forward_temporal): frame_index int [Wn, T] ->
        embeddings [Wn, T*N, D], bitwise `forward` on the gathered clips."""
        with self._ordered_on(stream):
            return self._run(self._check_windows(fs, frame_index), out_dtype, want_spatial, None, stream)


def _cached_engine(model, variables, device: int, norm_policy: str, make, policies=("pre",)):
    """The engine of `model` (one of the dataclasses below) for this parameter tree, device and
    dtype: built by make(flat leaves) on first use, kept in model._engines while the tree lives.
    policies: the norm policies this kind of model runs."""
    p = variables["params"] if isinstance(variables, dict) and "params" in variables else variables
    key = (id(p), device, model.is_bf16)
    ent = model._engines.get(key)
    if ent is not None and ent[0] is p:
        return ent[1]
    if norm_policy not in policies:
        raise NotImplementedError(f"norm_policy={norm_policy!r} is not implemented here (implemented: "
                                  f"{', '.join(repr(p) for p in policies)}; 'primer_hybrid' in the LvT text tower only)")
    flat = params_lib.canonical_params(variables)
    params_lib.validate(flat, model.param_specs())
    eng = make(flat)
    model._engines[key] = (p, eng)
    return eng


class _VideoModel:
    """What the three model dataclasses below share: the engine cache, the Flax-style `init`, `encode_frames`, the
    `method=` refusal and the two ways a video reaches an engine (clips, windows of frame states).  A model adds
    config(), param_specs(), engine(variables, device) and its `apply` / `apply_windows`, two entries into one
    `_forward` over an engine and its _Source."""

    def __post_init__(self):
        self._engines: dict = {}

    @property
    def is_bf16(self) -> bool:
        return _is_bf16_dtype(self.fprop_dtype)

    def init(self, rng=0, inputs=None, train: bool = False, **kwargs) -> dict:
        """Returns {'params': tree} for the seed that `rng` holds."""
        del inputs, train, kwargs
        return self._init(rng if isinstance(rng, int) else int(np.asarray(rng).ravel()[-1]))

    def _init(self, seed: int) -> dict:
        return params_lib.synthetic_params(self.config(), seed, specs=self.param_specs())

    @staticmethod
    def _refuse_method(entry: str, kwargs: dict) -> None:
        if kwargs.get("method") not in (None,):
            raise NotImplementedError(f"{entry}(method=...) is not supported")

    def encode_frames(self, variables, frames, frame_paddings=None) -> FrameStates:
        """The spatial half (encoders.py:459-478 and what feeds it) of `frames` [F, H, W, 3] (numpy or CUDA
        tensor; fp32, bf16 or uint8), frame_paddings [F] or None, once per frame -> FrameStates for
        `apply_windows`.  Overlapping windows of one long video share these states."""
        device = _pick_device(frames)
        x = _frames_on_device(frames, 4, self.is_bf16, device)
        return self.engine(variables, device).encode_frames(x, _as_paddings(frame_paddings))

    def _clips(self, variables, inputs, frame_paddings, device: int):
        """-> (the engine on `device`, its _Source for the clips `inputs` [B, T, H, W, 3])."""
        x = _frames_on_device(inputs, 5, self.is_bf16, device)
        eng = self.engine(variables, device)
        return eng, eng._check_video(x, _as_paddings(frame_paddings))

    def _windows(self, variables, states: FrameStates, frame_index):
        """-> (the engine on the states' device, its _Source for the windows `frame_index` of `states`).  A host
        index is range-checked before an engine is built, and only here."""
        index = _CheckedIndex(_frame_index(frame_index, len(states)), len(states))
        eng = self.engine(variables, _states_device(states))
        return eng, eng._check_windows(states, index)


@dataclasses.dataclass
class FactorizedEncoder(_VideoModel):
    """encoders.py:391-408 attributes; `fprop_dtype` as set by models.get_model."""

    patch_size: int = 18
    pos_emb_shape: tuple = (16, 16, 16)
    model_dim: int = 768
    num_spatial_layers: int = 12
    num_temporal_layers: int = 4
    num_heads: int = 12
    mlp_dim: int = 3072
    atten_logit_cap: float = 0.0
    norm_policy: str = "pre"
    scan: bool = False
    fprop_dtype: Any = None
    dtype: Any = None

    # -- config view ---------------------------------------------------------------
    def config(self) -> dict:
        return dict(patch_size=self.patch_size, pos_emb_shape=tuple(self.pos_emb_shape),
                    model_dim=self.model_dim, num_spatial_layers=self.num_spatial_layers,
                    num_temporal_layers=self.num_temporal_layers, num_heads=self.num_heads,
                    mlp_dim=self.mlp_dim, atten_logit_cap=self.atten_logit_cap)

    def param_specs(self) -> dict:
        return params_lib.encoder_leaf_specs(self.config(), scan=True)

    def _init(self, seed: int) -> dict:
        """Flax's initialiser distributions."""
        return params_lib.flax_default_init(self.config(), seed)

    def engine(self, variables, device: int) -> Engine:
        return _cached_engine(self, variables, device, self.norm_policy,
                              lambda flat: Engine(self.config(), flat, device, self.is_bf16))

    # -- Flax-style API ------------------------------------------------------------
    def apply(self, variables, inputs, train: bool = False,
              return_intermediate: bool | Collection[str] = False, frame_paddings=None,
              **kwargs):
        """encoders.py:411-456.  `train` has no effect at inference (dropouts are 0)."""
        del train
        self._refuse_method("apply", kwargs)
        return self._forward(*self._clips(variables, inputs, frame_paddings, _pick_device(inputs)),
                             return_intermediate, _wants_numpy(inputs))

    __call__ = apply

    def apply_windows(self, variables, states: FrameStates, frame_index, train: bool = False,
                      return_intermediate: bool | Collection[str] = False):
        """`apply` over windows of frame states -> (embeddings [Wn, T*N, D], outputs): window w is the frames
        states[frame_index[w, t]], t = 0..T-1 (video_utils.sliding_windows builds the usual index), with the
        frames' paddings.  Bit for bit `apply(frames[frame_index], frame_paddings=paddings[frame_index])`.
        A host frame_index (numpy, list, CPU tensor) is range-checked (IndexError); a CUDA tensor is not (that
        would synchronise) and is clamped to the states by the kernel.  Results are numpy arrays unless
        frame_index is a torch tensor.  For a short last window, keep one padded frame among the states and
        point the missing slots at it."""
        del train
        return self._forward(*self._windows(variables, states, frame_index), return_intermediate,
                             _wants_numpy(frame_index))

    def _forward(self, eng: Engine, src: _Source, return_intermediate, as_numpy: bool):
        emb, sp = eng._run(src, want_spatial=_contains(return_intermediate, "spatial_features"))
        return _pack((emb,), (("spatial_features", sp),), eng.fprop_dtype, as_numpy)


class ClipEngine(_EngineBase):
    """One vp_clip handle (packed LvT weights on one device) plus reusable workspaces."""

    _PREFIX = "vp_clip"
    _ENTRY = ("vp_clip_encode_video", "vp_clip_encode_video_windows")
    _QUERY = ("vp_clip_video_workspace_bytes", "vp_clip_video_windows_workspace_bytes")

    def _create_args(self):
        cfg = self.cfg
        c = _native.vp_clip_config(
            video=_vp_config(cfg, self.fprop_code), num_auxiliary_layers=cfg.get("num_auxiliary_layers", 0),
            vocabulary_size=cfg["vocabulary_size"],
            num_unimodal_layers=cfg["num_unimodal_layers"],
            enable_causal_atten=1 if cfg.get("enable_causal_atten", True) else 0,
            norm_policy=_native.NORM_POLICIES[cfg.get("norm_policy", "pre")])
        return (ctypes.byref(c),)

    def _run(self, src: _Source, normalize=True, want_frames=False, want_spatial=False,
             want_spatiotemporal=False, stream=None):
        """-> (video embeddings [B, D] fp32, frame embeddings [B, T, D] fp32 or None, spatial and spatio-temporal
        features or None) of the clips or windows `src`."""
        torch = _torch()
        D = self.cfg["model_dim"]
        vemb = torch.empty((src.B, D), dtype=torch.float32, device=src.device)
        femb = torch.empty((src.B, src.T, D), dtype=torch.float32, device=src.device) if want_frames else None
        sp = self._features(want_spatial, src)
        st = self._features(want_spatiotemporal, src)
        if src.B:  # otherwise an empty batch: zero-size embeddings, nothing to launch
            self._launch(src, 1 if normalize else 0, vemb, femb, sp, st, self.fprop_code, stream=stream)
        return vemb, femb, sp, st

    def encode_video(self, video, frame_paddings=None, normalize=True, want_frames=False,
                     want_spatial=False, want_spatiotemporal=False, stream=None):
        with self._ordered_on(stream):
            return self._run(self._check_video(video, frame_paddings), normalize, want_frames, want_spatial,
                             want_spatiotemporal, stream)

    def encode_video_windows(self, fs: FrameStates, frame_index, normalize=True, want_frames=False,
                             want_spatial=False, want_spatiotemporal=False, stream=None):
        """encode_video over windows of the vision tower's frame states (vp_clip_encode_video_windows)."""
        with self._ordered_on(stream):
            return self._run(self._check_windows(fs, frame_index), normalize, want_frames, want_spatial,
                             want_spatiotemporal, stream)

    def encode_text(self, ids, paddings, normalize=True, stream=None):
        torch = _torch()
        Q, L = ids.shape
        _check_device(ids, self.device, "text_token_ids")
        with self._ordered_on(stream):
            ids = ids.to(dtype=torch.int32).contiguous()
            pad = paddings.to(device=ids.device, dtype=torch.float32).contiguous()
            if tuple(pad.shape) != (Q, L):
                raise ValueError(f"text_paddings must be [{Q}, {L}], got {tuple(pad.shape)}")
            out = torch.empty((Q, self.cfg["model_dim"]), dtype=torch.float32, device=ids.device)
            if Q == 0 and L >= 1:  # no queries: a zero-size result, nothing to launch
                return out
            ws = self._workspace("text", "vp_clip_text_workspace_bytes", Q, L)
            _native.call("vp_clip_encode_text", self._h, *_c_args((ids, pad)), Q, L, 1 if normalize else 0,
                         *_c_args((out, ws)), ws.numel(), self._stream(stream))
        return out


@dataclasses.dataclass
class FactorizedVideoCLIP(_VideoModel):
    """encoders.py:762-910 attributes (the LvT video-text model); `fprop_dtype` as set by
    models.get_model."""

    patch_size: int = 18
    pos_emb_shape: tuple = (16, 16, 16)
    num_spatial_layers: int = 12
    num_temporal_layers: int = 4
    mlp_dim: int = 3072
    num_auxiliary_layers: int = 0
    vocabulary_size: int = 128
    enable_causal_atten: bool = True
    num_unimodal_layers: int = 12
    norm_policy: str = "pre"
    model_dim: int = 768
    num_heads: int = 12
    atten_logit_cap: float = 0.0
    scan: bool = False
    fprop_dtype: Any = None
    dtype: Any = None

    def config(self) -> dict:
        return dict(patch_size=self.patch_size, pos_emb_shape=tuple(self.pos_emb_shape),
                    num_spatial_layers=self.num_spatial_layers,
                    num_temporal_layers=self.num_temporal_layers, mlp_dim=self.mlp_dim,
                    num_auxiliary_layers=self.num_auxiliary_layers,
                    vocabulary_size=self.vocabulary_size,
                    enable_causal_atten=self.enable_causal_atten,
                    num_unimodal_layers=self.num_unimodal_layers, model_dim=self.model_dim,
                    num_heads=self.num_heads, atten_logit_cap=self.atten_logit_cap,
                    norm_policy=self.norm_policy)  # the text tower's (encoders.py:899)

    def param_specs(self) -> dict:
        return params_lib.clip_leaf_specs(self.config(), scan=True)

    def engine(self, variables, device: int) -> ClipEngine:
        return _cached_engine(self, variables, device, self.norm_policy,
                              lambda flat: ClipEngine(self.config(), flat, device, self.is_bf16),
                              policies=("pre", "primer_hybrid"))

    def apply(self, variables, inputs=None, text_token_ids=None, text_paddings=None,
              train: bool = False, normalize: bool = True,
              return_intermediate: bool | Collection[str] = False, frame_paddings=None, **kwargs):
        """encoders.py:788-910 -> (video_embeddings [B, D] | None, text_embeddings [B, D] | None,
        outputs).  Embeddings are returned in the fprop dtype (encoders.py:50-67 casts the
        normalised fp32 vector back)."""
        del train
        self._refuse_method("apply", kwargs)
        device = _pick_device(inputs, text_token_ids)
        if inputs is not None:
            eng, src = self._clips(variables, inputs, frame_paddings, device)
        else:
            eng, src = self.engine(variables, device), None
        return self._forward(eng, src, text_token_ids, text_paddings, normalize, return_intermediate,
                             _wants_numpy(inputs, text_token_ids))

    __call__ = apply

    def apply_windows(self, variables, states: FrameStates = None, frame_index=None, text_token_ids=None,
                      text_paddings=None, train: bool = False, normalize: bool = True,
                      return_intermediate: bool | Collection[str] = False, **kwargs):
        """`apply` with the video side over windows of frame states (FactorizedEncoder.apply_windows) ->
        (video_embeddings [Wn, D] | None, text_embeddings | None, outputs); `states` (with frame_index) or the
        text inputs may be None as in `apply`.  Results are numpy arrays unless frame_index or text_token_ids is a
        torch tensor."""
        del train
        self._refuse_method("apply_windows", kwargs)
        if states is not None:
            assert frame_index is not None, "frame_index is required with states."
            eng, src = self._windows(variables, states, frame_index)
        else:
            eng, src = self.engine(variables, _pick_device(text_token_ids)), None
        return self._forward(eng, src, text_token_ids, text_paddings, normalize, return_intermediate,
                             _wants_numpy(frame_index, text_token_ids))

    def _forward(self, eng: ClipEngine, src: _Source | None, text_token_ids, text_paddings, normalize: bool,
                 return_intermediate, as_numpy: bool):
        """The video side over `src` and the text side over the ids, either of which may be None."""
        vemb = femb = sp = st = temb = None
        if src is not None:
            vemb, femb, sp, st = eng._run(
                src, normalize, want_frames=_contains(return_intermediate, "frame_embeddings"),
                want_spatial=_contains(return_intermediate, "spatial_features"),
                want_spatiotemporal=_contains(return_intermediate, "spatiotemporal_features"))
        if text_token_ids is not None:
            temb = _encode_text(eng, text_token_ids, text_paddings, normalize)
        return _pack((vemb, temb), (("spatial_features", sp), ("spatiotemporal_features", st),
                                    ("frame_embeddings", femb)), eng.fprop_dtype, as_numpy)


class ClassifierEngine(_EngineBase):
    """One vp_classifier handle (FactorizedVideoClassifier weights on one device)."""

    _PREFIX = "vp_classifier"
    _ENTRY = ("vp_classifier_forward", "vp_classifier_forward_windows")
    _QUERY = ("vp_classifier_workspace_bytes", "vp_classifier_windows_workspace_bytes")

    def __init__(self, cfg: dict, num_classes: int, flat_params: dict, device: int, bf16: bool):
        self.num_classes = num_classes
        super().__init__(cfg, flat_params, device, bf16)

    def _create_args(self):
        return (ctypes.byref(_vp_config(self.cfg, self.fprop_code)), self.num_classes)

    def _run(self, src: _Source, want_embeddings=False, want_spatial=False, want_spatiotemporal=False,
             stream=None):
        """-> (logits [B, num_classes] fp32, global embeddings [B, D] fp32 or None, spatial and spatio-temporal
        features or None) of the clips or windows `src`."""
        torch = _torch()
        logits = torch.empty((src.B, self.num_classes), dtype=torch.float32, device=src.device)
        emb = torch.empty((src.B, self.cfg["model_dim"]), dtype=torch.float32, device=src.device) \
            if want_embeddings else None
        sp = self._features(want_spatial, src)
        st = self._features(want_spatiotemporal, src)
        if src.B:  # otherwise an empty batch: zero-size logits, nothing to launch
            self._launch(src, logits, emb, sp, st, self.fprop_code, stream=stream)
        return logits, emb, sp, st

    def forward(self, video, frame_paddings=None, want_embeddings=False, want_spatial=False,
                want_spatiotemporal=False, stream=None):
        with self._ordered_on(stream):
            return self._run(self._check_video(video, frame_paddings), want_embeddings, want_spatial,
                             want_spatiotemporal, stream)

    def forward_windows(self, fs: FrameStates, frame_index, want_embeddings=False, want_spatial=False,
                        want_spatiotemporal=False, stream=None):
        """forward over windows of the encoder's frame states (vp_classifier_forward_windows)."""
        with self._ordered_on(stream):
            return self._run(self._check_windows(fs, frame_index), want_embeddings, want_spatial,
                             want_spatiotemporal, stream)


@dataclasses.dataclass
class FactorizedVideoClassifier(_VideoModel):
    """encoders.py:583-653: `encoder_params` (a FactorizedEncoder config) and `num_classes`."""

    encoder_params: dict = dataclasses.field(default_factory=dict)
    num_classes: int = 0
    fprop_dtype: Any = None
    dtype: Any = None

    def config(self) -> dict:
        c = {k: v for k, v in self.encoder_params.items() if k not in ("scan", "norm_policy")}
        c["pos_emb_shape"] = tuple(c["pos_emb_shape"])
        return c

    def param_specs(self) -> dict:
        return params_lib.classifier_leaf_specs(self.config(), self.num_classes, scan=True)

    def engine(self, variables, device: int) -> ClassifierEngine:
        return _cached_engine(
            self, variables, device, self.encoder_params.get("norm_policy", "pre"),
            lambda flat: ClassifierEngine(self.config(), self.num_classes, flat, device, self.is_bf16))

    def apply(self, variables, inputs, train: bool = False,
              return_intermediate: bool | Collection[str] = False, frame_paddings=None, **kwargs):
        """encoders.py:594-653 -> (logits [B, num_classes], outputs)."""
        del train
        self._refuse_method("apply", kwargs)
        return self._forward(*self._clips(variables, inputs, frame_paddings, _pick_device(inputs)),
                             return_intermediate, _wants_numpy(inputs))

    __call__ = apply

    def apply_windows(self, variables, states: FrameStates, frame_index, train: bool = False,
                      return_intermediate: bool | Collection[str] = False):
        """`apply` over windows of frame states (FactorizedEncoder.apply_windows) -> (logits [Wn, num_classes],
        outputs)."""
        del train
        return self._forward(*self._windows(variables, states, frame_index), return_intermediate,
                             _wants_numpy(frame_index))

    def _forward(self, eng: ClassifierEngine, src: _Source, return_intermediate, as_numpy: bool):
        logits, emb, sp, st = eng._run(
            src, want_embeddings=_contains(return_intermediate, "global_embeddings"),
            want_spatial=_contains(return_intermediate, "spatial_features"),
            want_spatiotemporal=_contains(return_intermediate, "spatiotemporal_features"))
        return _pack((logits,), (("spatial_features", sp), ("spatiotemporal_features", st),
                                 ("global_embeddings", emb)), eng.fprop_dtype, as_numpy)
