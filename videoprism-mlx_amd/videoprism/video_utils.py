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


# ---- views: a source box, the size it is resized to, the window kept from that resize, and a mirror ----
# One view is nine int32: box_y, box_x, box_h, box_w, new_h, new_w, win_y, win_x, flags.  Its picture of a frame is
#   cv2.resize(frame[box_y:box_y+box_h, box_x:box_x+box_w], (new_w, new_h))[win_y:win_y+S, win_x:win_x+S],
# mirrored along x where flags & 1 (vp_op_preprocess_views in include/videoprism_hip.h).
_POSITIONS = ("start", "center", "end")


def _per_view(value, count, name):
    """`value` (one for all, or one per view) as a list of `count`."""
    if isinstance(value, (str, bool, np.bool_)) or np.ndim(value) == 0:
        return [value] * count
    value = list(value)
    if len(value) == 1:
        return value * count
    if len(value) != count:
        raise ValueError(f"{name} must be one value or one per view ({count}), got {len(value)}")
    return value


def view_table(h: int, w: int, boxes=None, target_size: int = 288, resize_mode: str = "center_crop",
               position="center", flip=False) -> np.ndarray:
    """The view table int32 [V, 9] of `preprocess_frames(views=...)` for frames of h x w.  No device use.

    Args:
      boxes: (y, x, h, w) rows, the part of the frame each view is cut from; None is the whole frame.
      target_size: S, the side of the output.
      resize_mode: how a box becomes the resize: "center_crop" gives it `center_crop_geometry` of the box (short
        side to S), "resize" stretches it to S x S.
      position: where the S x S window lies in the resize, along both axes: "start" (0), "center" ((new - S) // 2,
        the origin of `center_crop_geometry`) or "end" (new - S); one for all views or one per view.
      flip: mirror the picture along x; a bool or one per view.

    The number of views is the number of boxes, or of positions or flips where those are per view.  The whole frame
    with the defaults is exactly what preprocess_frames computes without views."""
    _mode(resize_mode)
    s = int(target_size)
    if h < 1 or w < 1 or s < 1:
        raise ValueError("view_table needs h, w and target_size of at least 1")
    count = max([1] + [len(v) for v in (boxes, position, flip)
                       if v is not None and not isinstance(v, (str, bool, np.bool_)) and np.ndim(v) > 0])
    if boxes is None:
        boxes = np.array([[0, 0, h, w]], dtype=np.int64)
    boxes = np.asarray(boxes)
    if boxes.ndim != 2 or boxes.shape[1] != 4 or not np.issubdtype(boxes.dtype, np.integer):
        raise ValueError("boxes must be integer rows (y, x, h, w)")
    boxes = _per_view(boxes.tolist(), count, "boxes")
    table = np.zeros((count, 9), dtype=np.int64)
    for v, (box, pos, fl) in enumerate(zip(boxes, _per_view(position, count, "position"), _per_view(flip, count, "flip"))):
        by, bx, bh, bw = box
        if bh < 1 or bw < 1:  # (the rest of the box is _check_views')
            raise ValueError(f"view {v}: box_h and box_w must be at least 1, got {bh} x {bw}")
        if pos not in _POSITIONS:
            raise ValueError(f"view {v}: unknown position {pos!r} (one of {_POSITIONS})")
        new_h, new_w = center_crop_geometry(bh, bw, s)[:2] if resize_mode == "center_crop" else (s, s)
        win_y, win_x = ((0, 0) if pos == "start" else ((new_h - s) // 2, (new_w - s) // 2) if pos == "center"
                        else (new_h - s, new_w - s))
        table[v] = (by, bx, bh, bw, new_h, new_w, win_y, win_x, 1 if fl else 0)
    _check_views(table, h, w, s)
    return table.astype(np.int32)


def multi_view(num_frames_total: int, h: int, w: int, num_frames: int = 16, temporal_views: int = 4,
               spatial_views: int = 3, dilation: int = 1, target_size: int = 288):
    """The usual multi-view evaluation of a video classifier: `temporal_views` clips spread evenly over the video,
    each seen through `spatial_views` windows spread evenly over the short-side-resized frame (3: left, centre, right
    of a landscape frame).  Returns (frame_indices int32 [V, num_frames], views int32 [V, 9]) for
    `preprocess_frames(views=..., frame_indices=...)`, V = temporal_views * spatial_views, temporal-major: view
    t * spatial_views + s is clip t through window s.  No device use.

    Clip t starts at np.linspace(0, n - span, temporal_views, dtype=int)[t], span = (num_frames - 1) * dilation + 1,
    and steps by `dilation`.  Window s lies at np.linspace(0, slack, spatial_views, dtype=int)[s] along each axis
    (slack = new - S), and at the centre for a single window."""
    if num_frames < 1 or temporal_views < 1 or spatial_views < 1 or dilation < 1:
        raise ValueError("multi_view needs num_frames, temporal_views, spatial_views and dilation of at least 1")
    s = int(target_size)
    span = (num_frames - 1) * dilation + 1
    if num_frames_total < span:
        raise ValueError(f"Video has only {num_frames_total} frames, but a clip spans {span}")
    starts = np.linspace(0, num_frames_total - span, temporal_views, dtype=int)
    clips = starts[:, None] + np.arange(num_frames, dtype=int)[None, :] * dilation
    new_h, new_w, y0, x0 = center_crop_geometry(h, w, s)
    if spatial_views == 1:
        ys, xs = np.array([y0]), np.array([x0])
    else:
        ys = np.linspace(0, new_h - s, spatial_views, dtype=int)
        xs = np.linspace(0, new_w - s, spatial_views, dtype=int)
    windows = np.array([[0, 0, h, w, new_h, new_w, y, x, 0] for y, x in zip(ys, xs)], dtype=np.int64)
    _check_views(windows, h, w, s)
    return (np.repeat(clips, spatial_views, axis=0).astype(np.int32),
            np.tile(windows, (temporal_views, 1)).astype(np.int32))


def random_resized_crop(h: int, w: int, n: int, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), rng=None) -> np.ndarray:
    """n random boxes (y, x, h, w), int32 [n, 4], in a frame of h x w, by the algorithm of torchvision's
    RandomResizedCrop.get_params: up to ten tries of an area drawn uniformly from `scale` (as a fraction of the
    frame's) and an aspect ratio w / h drawn log-uniformly from `ratio`, placed uniformly; if none fits, the central
    box of the whole frame clamped to `ratio`.  Draws come from `rng` (a numpy.random.Generator, or a seed for one).
    Feed the boxes to view_table(h, w, boxes=..., resize_mode="resize").  No device use."""
    if h < 1 or w < 1 or n < 0:
        raise ValueError("random_resized_crop needs h, w >= 1 and n >= 0")
    if not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]):
        raise ValueError("scale and ratio must be (min, max) with 0 < min <= max")
    rng = np.random.default_rng(rng)
    log_ratio = np.log(np.asarray(ratio, dtype=np.float64))
    out = np.zeros((n, 4), dtype=np.int32)
    for k in range(n):
        for _ in range(10):
            target_area = h * w * rng.uniform(scale[0], scale[1])
            aspect = np.exp(rng.uniform(log_ratio[0], log_ratio[1]))
            cw = int(round(np.sqrt(target_area * aspect)))
            ch = int(round(np.sqrt(target_area / aspect)))
            if 0 < cw <= w and 0 < ch <= h:
                out[k] = (rng.integers(0, h - ch + 1), rng.integers(0, w - cw + 1), ch, cw)
                break
        else:
            in_ratio = w / h
            if in_ratio < ratio[0]:
                cw, ch = w, min(h, max(1, int(round(w / ratio[0]))))
            elif in_ratio > ratio[1]:
                ch, cw = h, min(w, max(1, int(round(h * ratio[1]))))
            else:
                cw, ch = w, h
            out[k] = ((h - ch) // 2, (w - cw) // 2, ch, cw)
    return out


def _check_views(table, h, w, s):
    """Raises ValueError naming the first view of a host table [.., 9] that the kernel would have to clamp."""
    table = np.asarray(table)
    per_video = table.shape[-2]
    for v, (by, bx, bh, bw, nh, nw, wy, wx, flags) in enumerate(table.reshape(-1, 9).tolist()):
        name = f"view {v}" if table.ndim == 2 else f"view {v % per_video} of video {v // per_video}"
        if bh < 1 or bw < 1:
            raise ValueError(f"{name}: box_h and box_w must be at least 1, got {bh} x {bw}")
        if by < 0 or bx < 0 or by + bh > h or bx + bw > w:
            raise ValueError(f"{name}: box (y, x, h, w) = {(by, bx, bh, bw)} does not lie inside the {h} x {w} frame")
        if not (s <= nh < 1 << 24 and s <= nw < 1 << 24):
            raise ValueError(f"{name}: new_h and new_w must lie in [{s}, 2^24), got {nh} x {nw}")
        if wy < 0 or wx < 0 or wy + s > nh or wx + s > nw:
            raise ValueError(f"{name}: the {s} x {s} window at {(wy, wx)} does not lie inside the {nh} x {nw} resize")
        if flags not in (0, 1):
            raise ValueError(f"{name}: flags must be 0 or 1 (mirror), got {flags}")


def _host_views(views, frame_indices, num_frames, resize_mode, b, n, h, w, s):
    """The host half of a call with views (no device use): the table and the frame indices, each either a validated
    NumPy array or the CUDA tensor given (shape-checked only: reading it would synchronise; the kernel clamps
    it), and V.  b is None for a single video."""
    import torch
    if resize_mode != "center_crop":
        raise ValueError("views carry the geometry: resize_mode cannot be given with them "
                         "(view_table(..., resize_mode=...) builds the table)")
    dims = (2,) if b is None else (2, 3)
    if isinstance(views, torch.Tensor) and views.is_cuda:
        if views.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"views must be integers, got {views.dtype}")
        shape = tuple(views.shape)
    else:
        views = np.asarray(views.cpu() if isinstance(views, torch.Tensor) else views)
        if not np.issubdtype(views.dtype, np.integer):
            raise ValueError(f"views must be integers, got {views.dtype}")
        shape = views.shape
    if len(shape) not in dims or shape[-1] != 9 or shape[-2] < 1 or (len(shape) == 3 and shape[0] != b):
        raise ValueError(f"views must be int32 [V, 9]{'' if b is None else f' or [{b}, V, 9]'}, got {tuple(shape)}")
    if isinstance(views, np.ndarray):
        _check_views(views, h, w, s)
    nv = shape[-2]

    idx = frame_indices
    if idx is None:
        if num_frames is not None:
            idx = _host_indices(n, num_frames, None)
    elif isinstance(idx, torch.Tensor) and idx.is_cuda:
        if idx.dtype.is_floating_point or idx.dtype == torch.bool:
            raise ValueError(f"frame_indices must be integers, got {idx.dtype}")
    else:
        idx = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx)
        if idx.size < 1 or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError("frame_indices must be a non-empty array of integers")
        if idx.min() < 0 or idx.max() >= n:
            raise ValueError(f"frame_indices must lie in [0, {n - 1}] for a video of {n} frames")
    if idx is not None:
        ishape = tuple(idx.shape)
        ok = len(ishape) in ((1, 2) if b is None else (1, 2, 3)) and ishape[-1] >= 1
        if ok and len(ishape) >= 2 and ishape[-2] != nv:
            ok = False
        if ok and len(ishape) == 3 and ishape[0] != b:
            ok = False
        if not ok:
            raise ValueError(f"frame_indices must be [T], [{nv}, T]{'' if b is None else f' or [{b}, {nv}, T]'} "
                             f"with views, got {ishape}")
    return views, idx, nv


def _device_views(views, idx, nv, b, n, device):
    """_host_views' result as the kernel's arguments on `device`: the table int32 [B*V, 9], the frame indices int32
    [B*V, T] into the b videos of n frames flattened to one (None: every frame of a single video), and T."""
    import torch
    nb = 1 if b is None else b
    tab = views if isinstance(views, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(views, dtype=np.int32))
    tab = tab.to(device=device, dtype=torch.int32)
    if tab.dim() == 2:
        tab = tab[None].expand(nb, nv, 9)
    tab = tab.reshape(nb * nv, 9).contiguous()
    if idx is None and b is None:
        return tab, None, n
    if idx is None:
        idx = torch.arange(n, device=device)
    elif isinstance(idx, torch.Tensor):
        idx = idx.to(device).long().clamp(0, n - 1)
    else:
        idx = torch.from_numpy(idx.astype(np.int64)).to(device)
    t = idx.shape[-1]
    idx = idx.expand(nb, nv, t) if idx.dim() == 3 else idx.expand(nv, t)[None].expand(nb, nv, t)
    if b is not None:  # one launch for the whole batch: frame b*N + idx
        idx = idx + torch.arange(nb, device=device)[:, None, None] * n
    return tab, idx.reshape(nb * nv, t).to(torch.int32).contiguous(), t


def preprocess_frames(frames, num_frames=None, target_size: int = 288, resize_mode: str = "center_crop",
                      frame_indices=None, channel_order: str = "rgb", device=None, views=None):
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
      views: a view table int32 [V, 9] (`view_table`, `multi_view`), or [B, V, 9] for batched frames ([V, 9] is then
        shared by all videos): every video gives V clips in one launch, each cut from its own source box, resize
        window and mirror.  resize_mode must then be left alone (the table carries the geometry), and
        frame_indices may be [T] (shared), [V, T] or [B, V, T].  A host table is validated (ValueError naming the
        view); a device table is not read on the host and the kernel clamps it, as it does device frame_indices.

    Returns:
      uint8 device tensor [T, S, S, 3] or [B, T, S, S, 3] in RGB order; with views [V, T, S, S, 3] or
      [B, V, T, S, S, 3].
    """
    import torch
    mode = _mode(resize_mode)
    if channel_order not in ("rgb", "bgr"):
        raise ValueError(f"Unknown channel_order: {channel_order}")
    plan = None
    if views is not None:  # the table's checks need the frames' shape only: before any device use
        shape = tuple(frames.shape) if isinstance(frames, torch.Tensor) else np.shape(frames)
        if len(shape) not in (4, 5) or shape[-1] != 3:
            raise ValueError(f"frames must be uint8 [N, H, W, 3] or [B, N, H, W, 3], got {tuple(shape)}")
        plan = _host_views(views, frame_indices, num_frames, resize_mode, shape[0] if len(shape) == 5 else None,
                           shape[-4], shape[-3], shape[-2], target_size)
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

    if plan is not None:
        tab, idx, t = _device_views(*plan, b if batched else None, n, x.device)
        out = _native.op_preprocess_views(x, tab, idx, swap_rb=channel_order == "bgr", size=target_size)
        return out.view(*((b,) if batched else ()), plan[2], t, target_size, target_size, 3)
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
                          resize_mode: str = "center_crop", frame_indices=None, device=None, views=None):
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
      num_frames, target_size, resize_mode, frame_indices, device, views: as in preprocess_frames.  A view's box
        is in luma pixels of the full-resolution frame and may start at an odd one.

    Chroma is not interpolated: luma pixel (y, x) takes chroma sample (y >> 1, x >> 1).  Odd heights and
    widths are legal.  The conversion is the project's own 16.16 fixed point (tests/yuv_restatement.py),
    within 0.52 of a level of the real-valued BT.601 / BT.709 formula; it is not OpenCV's table.

    Returns:
      uint8 device tensor [T, S, S, 3] or [B, T, S, S, 3] in RGB order; with views [V, T, S, S, 3] or
      [B, V, T, S, S, 3].
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
    plan = None
    if views is not None:
        plan = _host_views(views, frame_indices, num_frames, resize_mode, b if batched else None, n, h, w, target_size)
    else:
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
    if plan is not None:
        tab, idx, t = _device_views(*plan, b if batched else None, n, ts[0].device)
        out = _native.op_preprocess_yuv_views(tuple(ts), tab, _YUV_FORMATS[pixel_format], _YUV_MATRICES[mat],
                                              _YUV_RANGES[color_range], idx, size=target_size)
        return out.view(*((b,) if batched else ()), plan[2], t, target_size, target_size, 3)
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
