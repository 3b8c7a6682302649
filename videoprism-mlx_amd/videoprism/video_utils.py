"""Video loading and frame preprocessing (the reference's videoprism/video_utils.py).

`load_video` / `load_video_batch` keep the reference's signatures and return values.  OpenCV only
decodes: the BGR->RGB swap, the short-side resize (cv2.resize's INTER_LINEAR on uint8) and the centre
crop run in one HIP kernel (csrc/preprocess.hip, vp_op_preprocess_frames) on the raw uint8 frames.
`preprocess_frames` is that step on its own: decoded frames of any resolution in, uint8
`[.., T, S, S, 3]` on the device out, ready for `model.apply` (which normalises uint8 by / 255 on the
device).  There is no CPU resize path, and copying the raw frames to the device is the caller's job
(NumPy and CPU-tensor inputs are copied for convenience; there is no GPU decode).
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

    idx = None
    if frame_indices is None and num_frames is not None:
        if n < num_frames:
            raise ValueError(f"Video has only {n} frames, but {num_frames} requested")
        idx = np.linspace(0, n - 1, num_frames, dtype=int)
    elif isinstance(frame_indices, torch.Tensor) and frame_indices.is_cuda:
        idx = frame_indices.to(x.device).reshape(-1).clamp(0, n - 1)
    elif frame_indices is not None:
        idx = np.asarray(frame_indices)
        if idx.ndim != 1 or idx.size < 1 or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError("frame_indices must be a non-empty 1-D sequence of integers")
        if idx.min() < 0 or idx.max() >= n:
            raise ValueError(f"frame_indices must lie in [0, {n - 1}] for a video of {n} frames")
    if idx is not None:
        if not isinstance(idx, torch.Tensor):
            idx = torch.from_numpy(idx.astype(np.int64)).to(x.device)
        t = idx.shape[0]
        if batched:  # one launch for the whole batch: frame b*N + idx
            idx = (torch.arange(b, device=x.device)[:, None] * n + idx[None, :]).reshape(-1)
        idx = idx.to(torch.int32).contiguous()
    else:
        t = n
    out = _native.op_preprocess_frames(x, idx, mode=mode, swap_rb=channel_order == "bgr", size=target_size)
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
