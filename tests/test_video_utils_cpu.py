"""video_utils without a GPU: the crop geometry, the properties of the fixed-point restatement the HIP
kernel is compared with (tests/preprocess_restatement.py), the argument checks of
vp_op_preprocess_frames (made before any GPU call) and load_video's ImportError."""

import ctypes
import sys

import numpy as np
import pytest
import torch

import preprocess_restatement as pr
from videoprism import _native, video_utils


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("h, w, s, want", [
    (240, 426, 288, (288, 511, 0, 111)),   # int() truncation: 426 * 1.2 = 511.19..
    (20, 31, 36, (36, 55, 0, 9)),
    (360, 640, 288, (288, 512, 0, 112)),
    (720, 1280, 288, (288, 512, 0, 112)),
    (1080, 1920, 288, (288, 512, 0, 112)),
    (53, 37, 36, (51, 36, 7, 0)),
    (45, 80, 36, (36, 64, 0, 14)),
    (36, 36, 36, (36, 36, 0, 0)),
])
def test_center_crop_geometry(h, w, s, want):
    assert video_utils.center_crop_geometry(h, w, s) == want
    assert pr.center_crop_geometry(h, w, s) == want


@pytest.mark.parametrize("src, dst", [((37, 53), (36, 51)), ((20, 20), (36, 36)), ((19, 61), (36, 115))])
def test_restatement_within_one_level_of_float64_bilinear(src, dst):
    img = _img(*src, seed=src[0])
    got = pr.resize_u8(img, dst[0], dst[1]).astype(np.float64)
    x = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
    ref = torch.nn.functional.interpolate(x, size=dst, mode="bilinear", align_corners=False, antialias=False)
    ref = ref[0].permute(1, 2, 0).numpy()
    err = np.abs(got - ref).max()
    print(f"{src} -> {dst}: max |restatement - float64 bilinear| = {err:.4f}")
    assert err < 1.0


def test_restatement_identity_at_equal_size():
    img = _img(36, 36, 1)
    assert np.array_equal(pr.resize_u8(img, 36, 36), img)
    assert np.array_equal(pr.preprocess(img, 36, "resize"), img)
    assert np.array_equal(pr.preprocess(img, 36, "center_crop"), img)


def test_restatement_exact_halving_is_the_rounded_2x2_mean():
    img = _img(72, 72, 2).astype(np.int32)
    want = (img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2] + 2) >> 2
    assert np.array_equal(pr.resize_u8(img.astype(np.uint8), 36, 36), want.astype(np.uint8))


def test_restatement_window_is_a_slice_of_the_full_resize():
    img = _img(20, 31, 3)
    full = pr.resize_u8(img, 36, 55)
    assert np.array_equal(pr.preprocess(img, 36), full[:, 9:45])
    frames = np.stack([_img(53, 37, 4), _img(53, 37, 5)])
    assert np.array_equal(pr.preprocess(frames, 36)[1], pr.resize_u8(frames[1], 51, 36)[7:43])


def test_preprocess_frames_argument_checks_touch_no_gpu():
    lib = _native.load()
    fn = lib.vp_op_preprocess_frames
    p = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused first
    E = _native.VP_EINVAL

    def call(src=p, N=4, H=20, W=30, rs=90, fs=1800, idx=None, F=4, mode=0, swap=0, S=16, dst=p):
        return fn(src, N, H, W, rs, fs, idx, F, mode, swap, S, dst, None)

    assert call(src=None) == E and call(dst=None) == E
    for k in ("N", "H", "W", "F", "S"):
        assert call(**{k: 0}) == E, k
        assert call(**{k: -1}) == E, k
    assert call(rs=89) == E
    assert b"row_stride" in lib.vp_last_error()
    assert call(fs=1799) == E
    assert b"frame_stride" in lib.vp_last_error()
    assert call(mode=2) == E and call(mode=-1) == E
    assert call(F=5) == E
    assert b"Video has only 4 frames, but 5 requested" in lib.vp_last_error()
    with pytest.raises(ValueError):
        _native.check(call(F=5))


def test_preprocess_frames_host_checks():
    x = np.zeros((4, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="Unknown resize_mode: pad"):
        video_utils.preprocess_frames(x, resize_mode="pad")
    with pytest.raises(ValueError, match="channel_order"):
        video_utils.preprocess_frames(x, channel_order="gbr")


def test_load_video_without_cv2_raises_the_reference_import_error(monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)  # `import cv2` now raises ImportError
    with pytest.raises(ImportError, match="OpenCV is required for video loading. "
                                          "Install it with: pip install opencv-python"):
        video_utils.load_video("clip.mp4")
    with pytest.raises(ImportError, match="OpenCV is required"):
        video_utils.load_video_batch(["clip.mp4"])


def test_exported_from_the_package():
    import videoprism
    assert videoprism.video_utils is video_utils
    assert videoprism.load_video is video_utils.load_video
    assert videoprism.preprocess_frames is video_utils.preprocess_frames
