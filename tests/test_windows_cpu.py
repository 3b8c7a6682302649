"""Sliding windows over per-frame spatial states, the parts that need no GPU: the window index arithmetic of
video_utils.sliding_windows, the new C-ABI symbols (exported, bound, ABI version unchanged), their argument checks
ahead of any device call, and the host frame_index range check of apply_windows."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from videoprism import _native, encoders, models, models_mlx, video_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "videoprism_hip.h")

NEW_SYMBOLS = ("vp_spatial_workspace_bytes", "vp_forward_spatial", "vp_temporal_workspace_bytes",
               "vp_forward_temporal", "vp_clip_video_windows_workspace_bytes", "vp_clip_encode_video_windows",
               "vp_classifier_windows_workspace_bytes", "vp_classifier_forward_windows")


def test_sliding_windows_counts_and_contents():
    w = video_utils.sliding_windows(20, 16, 1)
    assert w.dtype == np.int32 and w.shape == (5, 16)
    np.testing.assert_array_equal(w[0], np.arange(16))
    np.testing.assert_array_equal(w[4], np.arange(4, 20))
    # stride: windows start every `stride` frames, and only full windows count
    w = video_utils.sliding_windows(527, 16, 4)
    assert w.shape == ((527 - 16) // 4 + 1, 16)
    np.testing.assert_array_equal(w[:, 0], np.arange(w.shape[0]) * 4)
    assert w.max() == 4 * (w.shape[0] - 1) + 15 <= 526
    assert video_utils.sliding_windows(527, 16, 16).shape == (32, 16)
    # dilation: the frame step inside a window; a window reaches over (T - 1) * dilation + 1 frames
    w = video_utils.sliding_windows(20, 8, 1, dilation=2)
    assert w.shape == (20 - 15 + 1, 8)
    np.testing.assert_array_equal(w[1], 1 + 2 * np.arange(8))
    w = video_utils.sliding_windows(20, 8, 3, dilation=2)
    np.testing.assert_array_equal(w[:, 0], [0, 3])
    # exactly one window, and one frame short of it
    assert video_utils.sliding_windows(16, 16).shape == (1, 16)
    assert video_utils.sliding_windows(15, 16).shape == (0, 16)
    assert video_utils.sliding_windows(0, 4).shape == (0, 4)
    assert video_utils.sliding_windows(15, 8, dilation=2).shape == (1, 8)
    assert video_utils.sliding_windows(14, 8, dilation=2).shape == (0, 8)
    assert video_utils.sliding_windows(5, 1, 2).tolist() == [[0], [2], [4]]
    for bad in (dict(num_frames=0), dict(stride=0), dict(dilation=0)):
        with pytest.raises(ValueError):
            video_utils.sliding_windows(10, **bad)


def test_window_symbols_exported_and_bound():
    lib = _native.load()
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in _native.exported_symbols(), sym
        assert getattr(lib, sym).argtypes is not None, sym
    # the op-level frame gather (alone, and with the LayerNorm after it) is bound but stays out of the public header
    for sym in ("vp_dev_gather_frames", "vp_dev_layernorm_gather"):
        assert sym in _native.exported_symbols(), sym
        assert getattr(lib, sym).argtypes is not None, sym
        assert sym not in header, sym
    assert lib.vp_abi_version() == 8


def test_null_arguments_are_refused_before_any_device_call():
    lib = _native.load()
    n = ctypes.c_size_t()
    one = ctypes.c_void_p(256)  # a non-null pointer that a refused call never follows
    E = _native.VP_EINVAL
    assert lib.vp_spatial_workspace_bytes(None, 1, 288, 288, ctypes.byref(n)) == E
    assert lib.vp_temporal_workspace_bytes(None, 1, 16, 288, 288, ctypes.byref(n)) == E
    assert lib.vp_clip_video_windows_workspace_bytes(None, 1, 16, 288, 288, ctypes.byref(n)) == E
    assert lib.vp_classifier_windows_workspace_bytes(None, 1, 16, 288, 288, ctypes.byref(n)) == E
    assert lib.vp_forward_spatial(None, one, 0, 1, 288, 288, None, one, one, 0, None) == E
    assert lib.vp_forward_temporal(None, one, 16, one, 1, 16, 288, 288, None, one, 0, None, one, 0, None) == E
    assert lib.vp_clip_encode_video_windows(None, one, 1, one, 1, 16, 288, 288, None, 1, one, None, None, None, 0,
                                            one, 0, None) == E
    assert lib.vp_classifier_forward_windows(None, one, 1, one, 1, 16, 288, 288, None, one, None, None, None, 0, one,
                                             0, None) == E
    assert b"null" in lib.vp_last_error()
    assert lib.vp_dev_gather_frames(None, 1, None, 1, 16, None, None) == E
    assert lib.vp_dev_layernorm_gather(None, 0, 1, None, 4, 768, None, None, None, 0, 0, 1, 4, None, None, None,
                                       None) == E
    # vp_forward_temporal needs its index
    assert lib.vp_forward_temporal(one, one, 16, None, 1, 16, 288, 288, None, one, 0, None, one, 0, None) == E


def _cpu_states(F=4, dtype=torch.float32):
    return encoders.FrameStates(torch.zeros(F, 256, 768, dtype=dtype), None, (288, 288))


@pytest.mark.parametrize("bad", [[[0, 4]], [[-1, 0]], np.array([[3, 2], [1, 17]], np.int64),
                                 torch.tensor([[0, 1, 2, 4]])])
def test_host_frame_index_out_of_range(bad):
    """A host frame_index is range-checked before a model engine is built or anything is launched."""
    cfg = dict(models.CONFIGS["videoprism_v1_base"])
    enc = encoders.FactorizedEncoder(**cfg)
    with pytest.raises(IndexError, match="out of range for 4 frames"):
        enc.apply_windows(None, _cpu_states(), bad)
    vc = encoders.FactorizedVideoClassifier(encoder_params=cfg, num_classes=3)
    with pytest.raises(IndexError):
        vc.apply_windows(None, _cpu_states(), bad)
    clip = encoders.FactorizedVideoCLIP(**models.CONFIGS["videoprism_lvt_v1_base"])
    with pytest.raises(IndexError):
        clip.apply_windows(None, _cpu_states(), bad)


def test_frame_index_shape_and_type():
    enc = encoders.FactorizedEncoder(**models.CONFIGS["videoprism_v1_base"])
    with pytest.raises(ValueError, match=r"\[Wn, T\]"):
        enc.apply_windows(None, _cpu_states(), [0, 1, 2])
    with pytest.raises(TypeError, match="integers"):
        enc.apply_windows(None, _cpu_states(), np.zeros((1, 2), np.float32))
    with pytest.raises(IndexError, match="for 0 frames"):
        enc.apply_windows(None, _cpu_states(F=0), [[0, 0]])


def test_frame_states_slice_and_cat():
    st = torch.arange(5 * 2 * 3, dtype=torch.float32).reshape(5, 2, 3)
    pads = torch.tensor([0.0, 0.0, 1.0, 0.0, 0.0])
    fs = encoders.FrameStates(st, pads, (36, 18))
    assert len(fs) == 5 and fs.frame_size == (36, 18)
    a, b = fs[:2], fs[2:]
    assert len(a) == 2 and len(b) == 3 and b.paddings.tolist() == [1.0, 0.0, 0.0]
    back = encoders.FrameStates.cat([a, b])
    assert torch.equal(back.states, st) and torch.equal(back.paddings, pads) and back.frame_size == (36, 18)
    # a stream: drop the oldest frame, append a new one without paddings
    new = encoders.FrameStates(torch.ones(1, 2, 3), None, (36, 18))
    rolled = encoders.FrameStates.cat([fs[1:], new])
    assert len(rolled) == 5 and rolled.paddings.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0]
    assert encoders.FrameStates.cat([new, new]).paddings is None
    with pytest.raises(TypeError):
        fs[1]
    with pytest.raises(ValueError):
        encoders.FrameStates.cat([fs, encoders.FrameStates(torch.ones(1, 2, 3), None, (18, 18))])
    with pytest.raises(ValueError):
        encoders.FrameStates(st, torch.zeros(4), (36, 18))


def test_models_mlx_wrappers_delegate():
    for cls in (models_mlx.VideoEncoder, models_mlx.VideoCLIP):
        assert callable(getattr(cls, "encode_frames")) and callable(getattr(cls, "apply_windows"))
    m = models_mlx.VideoEncoder(models_mlx.get_model_config("videoprism_public_v1_base"), None)
    with pytest.raises(IndexError):
        m.apply_windows(_cpu_states(), [[0, 9]])
