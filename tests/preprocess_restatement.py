"""NumPy restatement of the reference's frame preprocessing (video_utils.py:76-87, 97-127): what
cv2.resize(frame, (new_w, new_h)) -- INTER_LINEAR on uint8, 11-bit fixed point -- and the centre crop
compute before the loader's / 255.  This file pins the arithmetic the HIP kernel
(csrc/preprocess.hip) is compared with bitwise; OpenCV itself is not needed to run it.

Per axis (dst = output size, src = input size):
    inv = float(dst) / float(src); scale = 1.0 / inv                 (double; not src / dst)
    f = float32((d + 0.5) * scale - 0.5)          (double product, double difference, one rounding)
    s = floor(f); f -= s;  s < 0 -> (0, 0.0);  s >= src - 1 -> (src - 1, 0.0);  s1 = min(s + 1, src - 1)
    a1 = rint(f * 2048), a0 = rint((1 - f) * 2048)                    (float32, round half to even)
Per value, in int32:
    h(row) = px[row][sx] * ax0 + px[row][sx1] * ax1
    out = (((by0 * (h(sy) >> 4)) >> 16) + ((by1 * (h(sy1) >> 4)) >> 16) + 2) >> 2
"""

import numpy as np


def axis_table(dst: int, src: int):
    """(s0, s1, a0, a1) int32 arrays of length dst."""
    inv = float(dst) / float(src)
    scale = 1.0 / inv
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    fl = np.floor(f)
    s = fl.astype(np.int64)
    f = (f - fl).astype(np.float32)
    lo = s < 0
    s[lo] = 0
    f[lo] = 0.0
    hi = s >= src - 1
    s[hi] = src - 1
    f[hi] = 0.0
    s1 = np.minimum(s + 1, src - 1)
    a1 = np.rint(f * np.float32(2048.0)).astype(np.int32)
    a0 = np.rint((np.float32(1.0) - f) * np.float32(2048.0)).astype(np.int32)
    return s.astype(np.int32), s1.astype(np.int32), a0, a1


def center_crop_geometry(h: int, w: int, target_size: int):
    """(new_h, new_w, y0, x0) of video_utils.py:109-124 (Python doubles, int() truncation)."""
    if h < w:
        new_h = target_size
        new_w = int(w * (target_size / h))
    else:
        new_w = target_size
        new_h = int(h * (target_size / w))
    return new_h, new_w, (new_h - target_size) // 2, (new_w - target_size) // 2


def resize_u8(img: np.ndarray, new_h: int, new_w: int, y0: int = 0, x0: int = 0, out_h=None, out_w=None):
    """The [y0:y0+out_h, x0:x0+out_w] window of cv2.resize(img, (new_w, new_h)); img uint8 [..., H, W, C]."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    H, W = img.shape[-3], img.shape[-2]
    out_h = new_h - y0 if out_h is None else out_h
    out_w = new_w - x0 if out_w is None else out_w
    sy0, sy1, by0, by1 = (t[y0:y0 + out_h] for t in axis_table(new_h, H))
    sx0, sx1, ax0, ax1 = (t[x0:x0 + out_w] for t in axis_table(new_w, W))
    px = img.astype(np.int32)
    ax0 = ax0[:, None]
    ax1 = ax1[:, None]
    h = px[..., :, sx0, :] * ax0 + px[..., :, sx1, :] * ax1      # [..., H, out_w, C]
    h0 = h[..., sy0, :, :] >> 4
    h1 = h[..., sy1, :, :] >> 4
    by0 = by0[:, None, None]
    by1 = by1[:, None, None]
    out = (((by0 * h0) >> 16) + ((by1 * h1) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def preprocess(frames: np.ndarray, target_size: int = 288, resize_mode: str = "center_crop"):
    """uint8 [..., H, W, 3] -> uint8 [..., S, S, 3], as the reference's loader before its / 255."""
    S = target_size
    H, W = frames.shape[-3], frames.shape[-2]
    if resize_mode == "center_crop":
        new_h, new_w, y0, x0 = center_crop_geometry(H, W, S)
        return resize_u8(frames, new_h, new_w, y0, x0, S, S)
    if resize_mode == "resize":
        return resize_u8(frames, S, S)
    raise ValueError(f"Unknown resize_mode: {resize_mode}")
