"""Video loading and frame preprocessing (the reference's videoprism/video_utils.py).

`load_video` / `load_video_batch` keep the reference's signatures and return values.  OpenCV only
decodes: the BGR->RGB swap, the short-side resize (cv2.resize's INTER_LINEAR on uint8) and the centre
crop run in one HIP kernel (csrc/preprocess.hip, vp_op_preprocess_frames) on the raw uint8 frames.
`preprocess_frames` is that step on its own: decoded frames of any resolution in, uint8
`[.., T, S, S, 3]` on the device out, ready for `model.apply` (which normalises uint8 by / 255 on the
device).  There is no CPU resize path, and copying the raw frames to the device is the caller's job
(NumPy and CPU-tensor inputs are copied for convenience; there is no GPU decode).
`preprocess_yuv_frames` is the same step in front of a decoder's 4:2:0 planes (NV12, I420, P010): the
kernel converts each tap to RGB on the way and reads the planes in place, so a GPU decoder's surfaces need no
conversion pass and no host round trip.  The decoder itself stays the caller's.
"""

from __future__ import annotations

import numpy as np

from . import _native

_MODES = {"center_crop": _native.VP_RESIZE_CENTER_CROP, "resize": _native.VP_RESIZE_STRETCH}


def center_crop_geometry(h: int, w: int, target_size: int):
    """(new_h, new_w, y0, x0) of the reference's _center_crop_resize (video_utils.py:109-124): the size
    the frame is resized to (shortest side = target_size, the other truncated by int()) and the origin
    of the target_size x target_size window in it."""
    if h < w:
        new_h = target_size
        new_w = int(w * (target_size / h))
    else:
        new_w = target_size
        new_h = int(h * (target_size / w))
    return new_h, new_w, (new_h - target_size) // 2, (new_w - target_size) // 2


def sliding_windows(num_frames_total: int, num_frames: int = 16, stride: int = 1, dilation: int = 1) -> np.ndarray:
    """Frame indices of every full window over a video of `num_frames_total` frames, int32 [Wn, num_frames]:
    window w holds frames w*stride + t*dilation, t = 0..num_frames-1 (`dilation` is the frame step inside a
    window).  A video too short for one window gives [0, num_frames].  The `frame_index` of `apply_windows`."""
    if num_frames_total < 0 or num_frames < 1 or stride < 1 or dilation < 1:
        raise ValueError("sliding_windows needs num_frames_total >= 0 and num_frames, stride, dilation >= 1")
    span = (num_frames - 1) * dilation + 1  # frames a window reaches over
    count = (num_frames_total - span) // stride + 1 if num_frames_total >= span else 0
    starts = np.arange(count, dtype=np.int64) * stride
    return (starts[:, None] + np.arange(num_frames, dtype=np.int64)[None, :] * dilation).astype(np.int32)


def _mode(resize_mode):
    if resize_mode not in _MODES:
        raise ValueError(f"Unknown resize_mode: {resize_mode}")
    return _MODES[resize_mode]


def preprocess_frames(frames, num_frames=None, target_size: int = 288, resize_mode: str = "center_crop",
                      frame_indices=None, channel_order: str = "rgb", device=None):
    """Resizes and crops raw uint8 frames on the GPU, as the reference's loader does before its / 255.

    Args:
      frames: uint8 [N, H, W, 3] or [B, N, H, W, 3], NumPy or torch (CPU or device; device views with
        padded rows or frames are read in place).
      num_frames: if given (and frame_indices is None), samples the frames
        np.linspace(0, N - 1, num_frames, dtype=int) of each video, as load_video does.
      target_size: output height and width S.
      resize_mode: "center_crop" (shortest side to S, then centre crop) or "resize" (stretch to S x S).
      frame_indices: frame indices into each video instead of the uniform sample: a host sequence
        (validated) or an integer device tensor (out-of-range entries are clamped).
      channel_order: "rgb", or "bgr" to swap R and B on the way (OpenCV's decoded frames).
      device: the device for host inputs (default: the current one).

    Returns:
      uint8 device tensor [T, S, S, 3] or [B, T, S, S, 3] in RGB order.
    """
    import torch
    mode = _mode(resize_mode)
    if channel_order not in ("rgb", "bgr"):
        raise ValueError(f"Unknown channel_order: {channel_order}")
    if isinstance(frames, torch.Tensor):
        x = frames
        if not x.is_cuda:
            x = x.to(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    else:
        x = torch.from_numpy(np.ascontiguousarray(frames))
        x = x.to(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    if x.dtype != torch.uint8 or x.dim() not in (4, 5) or x.shape[-1] != 3:
        raise ValueError(f"frames must be uint8 [N, H, W, 3] or [B, N, H, W, 3], got {x.dtype} {tuple(x.shape)}")
    batched = x.dim() == 5
    b = x.shape[0] if batched else 1
    n, h, w = x.shape[-4], x.shape[-3], x.shape[-2]
    if x.stride(-1) != 1 or (w > 1 and x.stride(-2) != 3):
        x = x.contiguous()
    if batched:
        x = x.reshape(b * n, h, w, 3)  # a view whenever the batch stride allows it

    idx, t = _device_indices(_host_indices(n, num_frames, frame_indices), b if batched else None, n, x.device)
    out = _native.op_preprocess_frames(x, idx, mode=mode, swap_rb=channel_order == "bgr", size=target_size)
    return out.view(b, t, target_size, target_size, 3) if batched else out


def _host_indices(n, num_frames, frame_indices):
    """The frames to take of a video of n: None (all), a validated host array (the uniform sample, or
    frame_indices given on the host) or frame_indices as given on the device.  No device use."""
    import torch
    if frame_indices is None and num_frames is not None:
        if n < num_frames:
            raise ValueError(f"Video has only {n} frames, but {num_frames} requested")
        return np.linspace(0, n - 1, num_frames, dtype=int)
    if isinstance(frame_indices, torch.Tensor) and frame_indices.is_cuda:
        return frame_indices
    if frame_indices is None:
        return None
    idx = np.asarray(frame_indices)
    if idx.ndim != 1 or idx.size < 1 or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("frame_indices must be a non-empty 1-D sequence of integers")
    if idx.min() < 0 or idx.max() >= n:
        raise ValueError(f"frame_indices must lie in [0, {n - 1}] for a video of {n} frames")
    return idx


def _device_indices(idx, b, n, device):
    """_host_indices' result as the kernel's int32 index vector on `device` (device indices clamped), for b
    videos of n frames flattened to one (b None: a single video), and the number of frames per video."""
    import torch
    if idx is None:
        return None, n
    if isinstance(idx, torch.Tensor):
        idx = idx.to(device).reshape(-1).clamp(0, n - 1)
    else:
        idx = torch.from_numpy(idx.astype(np.int64)).to(device)
    t = idx.shape[0]
    if b is not None:  # one launch for the whole batch: frame b*N + idx
        idx = (torch.arange(b, device=device)[:, None] * n + idx[None, :]).reshape(-1)
    return idx.to(torch.int32).contiguous(), t


_YUV_FORMATS = {"nv12": _native.VP_YUV_NV12, "i420": _native.VP_YUV_I420, "p010": _native.VP_YUV_P010}
_YUV_MATRICES = {"bt601": _native.VP_YUV_BT601, "bt709": _native.VP_YUV_BT709}
_YUV_RANGES = {"limited": _native.VP_YUV_LIMITED, "full": _native.VP_YUV_FULL}


def yuv_matrix(matrix: str, height: int, width: int) -> str:
    """"bt601" or "bt709" as given; "auto" is the usual player convention for streams that carry no tag:
    BT.709 for HD (width >= 1280 or height > 576), BT.601 below."""
    if matrix == "auto":
        return "bt709" if width >= 1280 or height > 576 else "bt601"
    if matrix not in _YUV_MATRICES:
        raise ValueError(f"Unknown matrix: {matrix}")
    return matrix


def preprocess_yuv_frames(planes, height=None, width=None, pixel_format: str = "nv12", matrix: str = "auto",
                          color_range: str = "limited", num_frames=None, target_size: int = 288,
                          resize_mode: str = "center_crop", frame_indices=None, device=None):
    """preprocess_frames in front of a video decoder's 4:2:0 output: converts to RGB, resizes and crops in
    one kernel that reads the decoder's planes where they lie.  The result is, bit for bit, preprocess_frames
    of the full-resolution RGB frames, which are never stored.  No decoder is shipped or required: the
    planes are whatever produced them (VA-API or rocDecode surfaces through DLPack, PyAV arrays, ...).

    Args:
      planes: a tuple of NumPy arrays or torch tensors, with an optional leading batch dimension:
        "nv12": (y [N, H, W] uint8, uv [N, ceil(H/2), ceil(W/2), 2] uint8), U and V interleaved;
        "i420": (y, u [N, ceil(H/2), ceil(W/2)], v), uint8;
        "p010": as "nv12" in 16-bit words (torch.int16 or uint16, np.uint16), the 10-bit sample in the
          high bits (word >> 6).
        Device tensors are read in place through their strides -- for a decoder surface with a pitch and
        an aligned height, y = surf[:, :H, :W] and
        uv = surf[:, Ha:Ha + (H + 1) // 2, :2 * ((W + 1) // 2)].unflatten(-1, (-1, 2)) -- as long as the
        samples (the U,V pairs) are contiguous; anything else is made contiguous first.  Host inputs are
        copied to the device for convenience.
      height, width: the frame size (default: the Y plane's); the planes' shapes must match it.
      pixel_format: "nv12", "i420" or "p010".
      matrix: "bt601", "bt709" or "auto": BT.709 when width >= 1280 or height > 576, else BT.601, the usual
        player convention for streams that carry no tag.
      color_range: "limited" (16..235 / 16..240, scaled for 10 bits) or "full".
      num_frames, target_size, resize_mode, frame_indices, device: as in preprocess_frames.

    Chroma is not interpolated: luma pixel (y, x) takes chroma sample (y >> 1, x >> 1).  Odd heights and
    widths are legal.  The conversion is the project's own 16.16 fixed point (tests/yuv_restatement.py),
    within 0.52 of a level of the real-valued BT.601 / BT.709 formula; it is not OpenCV's table.

    Returns:
      uint8 device tensor [T, S, S, 3] or [B, T, S, S, 3] in RGB order.
    """
    import torch
    mode = _mode(resize_mode)
    if pixel_format not in _YUV_FORMATS:
        raise ValueError(f"Unknown pixel_format: {pixel_format}")
    if color_range not in _YUV_RANGES:
        raise ValueError(f"Unknown color_range: {color_range}")
    if matrix != "auto" and matrix not in _YUV_MATRICES:
        raise ValueError(f"Unknown matrix: {matrix}")
    nplanes = 3 if pixel_format == "i420" else 2
    if not isinstance(planes, (tuple, list)) or len(planes) != nplanes:
        raise ValueError(f"{pixel_format} takes a tuple of {nplanes} planes")
    p010 = pixel_format == "p010"
    ts = []
    for p in planes:
        if not isinstance(p, torch.Tensor):
            p = np.ascontiguousarray(p)
            if p.dtype == np.uint16:  # the kernel reads the words' bits; int16 is the dtype every torch op takes
                p = p.view(np.int16)
            elif p.dtype != np.uint8:  # refused below; torch.from_numpy need not know the dtype
                raise ValueError(f"{pixel_format} planes must be {'16-bit words' if p010 else 'uint8'}, got {p.dtype}")
            p = torch.from_numpy(p)
        elif p.dtype == getattr(torch, "uint16", None):
            p = p.view(torch.int16)
        if p.dtype != (torch.int16 if p010 else torch.uint8):
            raise ValueError(f"{pixel_format} planes must be {'16-bit words' if p010 else 'uint8'}, got {p.dtype}")
        ts.append(p)
    y = ts[0]
    if y.dim() not in (3, 4):
        raise ValueError(f"the Y plane must be [N, H, W] or [B, N, H, W], got {tuple(y.shape)}")
    batched = y.dim() == 4
    lead = tuple(y.shape[:-2])
    h = int(y.shape[-2]) if height is None else int(height)
    w = int(width) if width is not None else int(y.shape[-1])
    if h < 1 or w < 1 or tuple(y.shape[-2:]) != (h, w):
        raise ValueError(f"the Y plane must be [.., {h}, {w}], got {tuple(y.shape)}")
    chroma = lead + ((h + 1) // 2, (w + 1) // 2) + (() if nplanes == 3 else (2,))
    for name, p in zip(("UV",) if nplanes == 2 else ("U", "V"), ts[1:]):
        if tuple(p.shape) != chroma:
            raise ValueError(f"the {name} plane of {tuple(y.shape)} {pixel_format} frames must be {chroma}, "
                             f"got {tuple(p.shape)}")
    mat = yuv_matrix(matrix, h, w)
    b = lead[0] if batched else 1
    n = lead[-1]
    idx = _host_indices(n, num_frames, frame_indices)

    # everything above ran on the host; from here on the device is used
    if not all(p.is_cuda for p in ts):
        dev = next((p.device for p in ts if p.is_cuda), None) or (
            device if device is not None else f"cuda:{torch.cuda.current_device()}")
        ts = [p.to(dev) for p in ts]
    for i, p in enumerate(ts):
        inner = (2, 1) if (nplanes == 2 and i == 1) else (1,)
        if any(s != k for s, k, e in zip(p.stride()[-len(inner):], inner, p.shape[-len(inner):]) if e > 1):
            p = p.contiguous()
        if batched:
            p = p.reshape((b * n,) + tuple(p.shape[2:]))  # a view whenever the batch stride allows it
        ts[i] = p
    idx, t = _device_indices(idx, b if batched else None, n, ts[0].device)
    out = _native.op_preprocess_yuv(tuple(ts), _YUV_FORMATS[pixel_format], _YUV_MATRICES[mat],
                                    _YUV_RANGES[color_range], idx, mode=mode, size=target_size)
    return out.view(b, t, target_size, target_size, 3) if batched else out


def load_video(
    video_path: str,
    num_frames: int = 16,
    target_size: int = 288,
    resize_mode: str = "center_crop",
) -> np.ndarray:
    """The reference's load_video: num_frames frames sampled uniformly from the file, resized and cropped
    to target_size ("center_crop": short side to target_size, then the centre window; "resize": stretched),
    returned as float32 RGB in [0, 1], shape [num_frames, target_size, target_size, 3].

    cv2 decodes (ImportError without it, ValueError for an unreadable file or too few frames); the resize
    runs on the current GPU through preprocess_frames."""
    try:
        import cv2
    except ImportError as e:
        raise ImportError(
            "OpenCV is required for video loading. "
            "Install it with: pip install opencv-python"
        ) from e

    cap = cv2.VideoCapture(video_path)
    if not cap.isOpened():
        raise ValueError(f"Could not open video file: {video_path}")
    total_frames = int(cap.get(cv2.CAP_PROP_FRAME_COUNT))
    if total_frames < num_frames:
        raise ValueError(f"Video has only {total_frames} frames, but {num_frames} requested")
    _mode(resize_mode)

    # decode only the sampled frames (BGR, native resolution); everything after runs on the GPU
    frames = []
    for frame_idx in np.linspace(0, total_frames - 1, num_frames, dtype=int):
        cap.set(cv2.CAP_PROP_POS_FRAMES, frame_idx)
        ret, frame = cap.read()
        if not ret:
            raise ValueError(f"Could not read frame {frame_idx} from {video_path}")
        frames.append(frame)
    cap.release()

    out = preprocess_frames(np.stack(frames, axis=0), target_size=target_size, resize_mode=resize_mode,
                            channel_order="bgr")
    return out.cpu().numpy().astype(np.float32) / 255.0


def load_video_batch(
    video_paths: list[str],
    num_frames: int = 16,
    target_size: int = 288,
    resize_mode: str = "center_crop",
) -> np.ndarray:
    """load_video over several files, stacked: float32 [len(video_paths), num_frames, S, S, 3]."""
    videos = [load_video(path, num_frames, target_size, resize_mode) for path in video_paths]
    return np.stack(videos, axis=0)
