"""Views in the frame ingest (csrc/preprocess.hip through vp_op_preprocess_views / vp_op_preprocess_yuv_views and
videoprism.video_utils.preprocess_frames / preprocess_yuv_frames with views=): each output clip is cut from its own
source box, resize, window and mirror, in one launch.  Every comparison is bitwise against

    preprocess_restatement.resize_u8(img[box], new_h, new_w, win_y, win_x, S, S), then the mirror,

for YUV chained after yuv_restatement.yuv_to_rgb.  The RGB source is 5 frames of 37 x 53 (both sides odd), random
uint8 with a block of extremes, held as an interior view of a larger buffer filled with a sentinel (0x00, then 0xFF):
a tap that left the frame would change the bits, and one that left its box reads other random pixels."""

import functools

import numpy as np
import pytest
import torch

import preprocess_restatement as pr
import yuv_restatement as yr
from videoprism import _native as nat
from videoprism import video_utils

pytestmark = pytest.mark.gpu

N, H, W = 5, 37, 53
CROP, STRETCH = nat.VP_RESIZE_CENTER_CROP, nat.VP_RESIZE_STRETCH
FMT = {"nv12": nat.VP_YUV_NV12, "i420": nat.VP_YUV_I420, "p010": nat.VP_YUV_P010}
MATRIX = {"bt601": nat.VP_YUV_BT601, "bt709": nat.VP_YUV_BT709}
RANGE = {"limited": nat.VP_YUV_LIMITED, "full": nat.VP_YUV_FULL}
# per-view frames: a repeat (views 2, 4), descending runs (views 1, 5, 7)
IDX = np.array([[0, 1, 2], [4, 3, 2], [1, 1, 3], [2, 0, 4], [4, 4, 4], [3, 2, 1], [0, 2, 4], [4, 1, 0]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _frames(n=N, h=H, w=W, seed=7):
    """Host frames uint8 [n, h, w, 3] (read-only): random, one 4 x 4 block of 0 and 255 per frame."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    for i in range(n):
        by, bx = (3 * i + 1) % (h - 4), (5 * i + 2) % (w - 4)
        x[i, by:by + 4, bx:bx + 4] = 255 * rng.integers(0, 2, (4, 4, 3), dtype=np.uint8)
    x.setflags(write=False)
    return x


def _table(s):
    """The eight views of the module's 37 x 53 frames at output size s, int32 [8, 9]."""
    whole = video_utils.view_table(H, W, target_size=s, position=["center", "start", "end"])        # views 1-3
    odd = video_utils.view_table(H, W, boxes=[(5, 7, 21, 30)], target_size=s, resize_mode="resize")  # 4: odd origin
    corner = video_utils.view_table(H, W, boxes=[(36, 52, 1, 1)], target_size=s, resize_mode="resize")  # 5: all clamp
    tall = video_utils.view_table(H, W, boxes=[(3, 1, 30, 9)], target_size=s)          # 6: downscales y, y window
    flipped = video_utils.view_table(H, W, target_size=s, flip=True)                   # 7
    # 8: a 9 x 40 box resized to (2 s + 2) x (5 s + 5) (y upscaled: 18 rows at s = 8), the end window, mirrored
    wide = np.array([[1, 3, 9, 40, 2 * s + 2, 5 * s + 5, s + 2, 4 * s + 5, 1]], dtype=np.int32)
    t = np.concatenate([whole, odd, corner, tall, flipped, wide])
    assert t.shape == (8, 9) and t.dtype == np.int32 and t[5, 4] > s and t[5, 6] > 0
    return t


def _picture(frames, row, s):
    """The restatement of one view: frames uint8 [.., H, W, 3] -> uint8 [.., s, s, 3]."""
    by, bx, bh, bw, nh, nw, wy, wx, flags = (int(v) for v in row)
    out = pr.resize_u8(frames[..., by:by + bh, bx:bx + bw, :], nh, nw, wy, wx, s, s)
    return out[..., ::-1, :] if flags & 1 else out


def _want(frames, table, idx, s):
    """[V, T, s, s, 3]: view v of frames idx[v]."""
    return np.stack([_picture(frames[idx[v]], table[v], s) for v in range(len(table))])


def _interior(host, cuda, fill, lead=()):
    """`host` [n, h, w, 3] on the device as the interior of a buffer [n, h + 6, w + 8, 3] filled with `fill`: padded
    rows and frames, the videos of a batch (`lead` = (b, n)) evenly spaced."""
    n, h, w, _ = host.shape
    buf = torch.full((n, h + 6, w + 8, 3), fill, dtype=torch.uint8, device=cuda)
    x = buf[:, 3:3 + h, 4:4 + w]
    x.copy_(torch.from_numpy(host.copy()).to(cuda))
    assert not x.is_contiguous()
    return x.unflatten(0, lead) if lead else x


def _same(got, want):
    torch.cuda.synchronize()
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want)


def _dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)  # a writable copy of what may be a shared read-only array


# S = 8: whole groups, dword stores.  S = 7: 49 pixels a frame, so groups run over row ends, the last group holds one
# pixel, and frames of 147 bytes put every other one on the byte-store path
@pytest.mark.parametrize("s", [8, 7])
def test_eight_views_in_one_launch(cuda, s):
    frames, table = _frames(), _table(s)
    want = _want(frames, table, IDX, s)
    for fill in (0x00, 0xFF):
        x = _interior(frames, cuda, fill)
        got = nat.op_preprocess_views(x, _dev(table, cuda), _dev(IDX, cuda), size=s)
        _same(got.view(8, 3, s, s, 3), want)
        _same(video_utils.preprocess_frames(x, target_size=s, views=table, frame_indices=IDX), want)
    # NumPy frames in; frame_idx None: all N frames for every view
    got = video_utils.preprocess_frames(np.array(frames), target_size=s, views=table)
    _same(got, _want(frames, table, np.tile(np.arange(N), (8, 1)), s))
    got = video_utils.preprocess_frames(np.array(frames[..., ::-1]), target_size=s, views=table, channel_order="bgr",
                                        num_frames=2)
    _same(got, _want(frames, table, np.tile([0, 4], (8, 1)), s))


@pytest.mark.parametrize("s", [8, 7])
def test_whole_frame_views_equal_the_plain_kernel(cuda, s):
    """GPU against GPU: the whole frame with the geometry of either resize mode is op_preprocess_frames' output."""
    frames = _frames()
    table = np.concatenate([video_utils.view_table(H, W, target_size=s),
                            video_utils.view_table(H, W, target_size=s, resize_mode="resize")])
    idx = np.stack([IDX[1], IDX[1]])
    x = _interior(frames, cuda, 0x5A)
    for swap in (False, True):
        got = nat.op_preprocess_views(x, _dev(table, cuda), _dev(idx, cuda), swap_rb=swap, size=s).view(2, 3, s, s, 3)
        torch.cuda.synchronize()
        for v, mode in enumerate((CROP, STRETCH)):
            plain = nat.op_preprocess_frames(x, _dev(idx[v], cuda), mode=mode, swap_rb=swap, size=s)
            torch.cuda.synchronize()
            assert torch.equal(got[v], plain), (swap, mode)
        src = frames[..., ::-1] if swap else frames
        _same(got, _want(src, table, idx, s))


@pytest.mark.parametrize("s", [7, 8, 36])
def test_flip_is_the_unflipped_view_reversed(cuda, s):
    plain = _table(s)
    plain[:, 8] = 0
    mirrored = plain.copy()
    mirrored[:, 8] = 1
    x = _dev(_frames(), cuda)
    a = video_utils.preprocess_frames(x, target_size=s, views=plain, frame_indices=IDX)
    b = video_utils.preprocess_frames(x, target_size=s, views=mirrored, frame_indices=IDX)
    torch.cuda.synchronize()
    assert torch.equal(b, a.flip(-2))
    _same(a, _want(_frames(), plain, IDX, s))
    _same(b, _want(_frames(), mirrored, IDX, s))


def test_batched_tables_indices_and_strided_sources(cuda, monkeypatch):
    s, b, n = 8, 2, 3
    frames = _frames(6, H, W, 9).reshape(b, n, H, W, 3)
    t8 = _table(s)
    tables = np.stack([t8[[0, 3, 7]], t8[[5, 6, 2]]])                     # [B, V, 9], another set per video
    idx = np.array([[[0, 1], [2, 2], [2, 0]], [[1, 0], [0, 2], [1, 1]]])  # [B, V, T]
    x = _interior(frames.reshape(b * n, H, W, 3), cuda, 0xFF, lead=(b, n))
    seen = []
    real = nat.op_preprocess_views
    monkeypatch.setattr(nat, "op_preprocess_views", lambda src, *a, **k: (seen.append(src.data_ptr()), real(src, *a, **k))[1])

    def want(tab, ind):
        return np.stack([_want(frames[i], tab[i], ind[i], s) for i in range(b)])

    _same(video_utils.preprocess_frames(x, target_size=s, views=tables, frame_indices=idx), want(tables, idx))
    # device tables and indices of the same shapes
    _same(video_utils.preprocess_frames(x, target_size=s, views=_dev(tables, cuda), frame_indices=_dev(idx, cuda)),
          want(tables, idx))
    # broadcasts: a [V, 9] table for all videos, [V, T] and [T] indices, none at all
    shared = np.broadcast_to(tables[0], (b, 3, 9))
    _same(video_utils.preprocess_frames(x, target_size=s, views=tables[0], frame_indices=idx), want(shared, idx))
    _same(video_utils.preprocess_frames(x, target_size=s, views=tables, frame_indices=idx[1]),
          want(tables, np.broadcast_to(idx[1], (b, 3, 2))))
    _same(video_utils.preprocess_frames(x, target_size=s, views=tables, frame_indices=[2, 0]),
          want(tables, np.broadcast_to([2, 0], (b, 3, 2))))
    _same(video_utils.preprocess_frames(x, target_size=s, views=tables[1]),
          want(np.broadcast_to(tables[1], (b, 3, 9)), np.broadcast_to(np.arange(n), (b, 3, n))))
    assert seen == [x.data_ptr()] * 6  # padded rows and frames were read where they lie
    # one video of the batch alone
    _same(video_utils.preprocess_frames(x[1], target_size=s, views=tables[1], frame_indices=idx[1]), want(tables, idx)[1])


def _clamped(row, s):
    """The clamps of vp_op_preprocess_views, restated."""
    by, bx = min(max(row[0], 0), H - 1), min(max(row[1], 0), W - 1)
    bh, bw = min(max(row[2], 1), H - by), min(max(row[3], 1), W - bx)
    nh, nw = min(max(row[4], s), (1 << 24) - 1), min(max(row[5], s), (1 << 24) - 1)
    return [by, bx, bh, bw, nh, nw, min(max(row[6], 0), nh - s), min(max(row[7], 0), nw - s), row[8] & 1]


def test_device_table_is_clamped_host_table_is_refused(cuda):
    s = 8
    bad = np.array([[30, 40, 20, 20, 12, 12, 2, 3, 0],        # the box reaches past the frame on both axes
                    [-4, -5, 21, 30, 9, 11, 0, 1, 1],         # a negative origin
                    [5, 7, 21, 30, 9, 0, 1, 0, 0],            # new_w = 0
                    [0, 0, H, W, 10, 14, -3, 10 ** 6, 0],     # the window far outside the resize
                    [2 ** 31 - 1, -2 ** 31, -2 ** 31, 2 ** 31 - 1, 9, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 1],
                    [3, 4, 0, -7, 8, 8, 0, 0, 0]], dtype=np.int64).astype(np.int32)
    good = np.array([_clamped(r, s) for r in bad.tolist()], dtype=np.int32)
    assert good[0].tolist() == [30, 40, 7, 13, 12, 12, 2, 3, 0] and good[1].tolist() == [0, 0, 21, 30, 9, 11, 0, 1, 1]
    assert good[2, 5] == s and good[3, 6:8].tolist() == [0, 14 - s]
    assert good[4].tolist() == [H - 1, 0, 1, W, 9, s, 9 - s, 0, 1]
    assert good[5].tolist() == [3, 4, 1, 1, 8, 8, 0, 0, 0]
    idx = IDX[:6]
    x = _interior(_frames(), cuda, 0xFF)
    got = video_utils.preprocess_frames(x, target_size=s, views=_dev(bad, cuda), frame_indices=idx)
    _same(got, _want(_frames(), good, idx, s))
    clean = video_utils.preprocess_frames(x, target_size=s, views=good, frame_indices=idx)  # valid: passes the host check
    torch.cuda.synchronize()
    assert torch.equal(got, clean)
    for v in range(6):
        with pytest.raises(ValueError, match="view 0"):
            video_utils.preprocess_frames(x, target_size=s, views=bad[v:v + 1], frame_indices=idx[v:v + 1])


# ---- YUV ----
@functools.lru_cache(maxsize=None)
def _planes(fmt, seed=13):
    """Host planes of N frames of H x W (read-only): random over the full sample range, a block of extremes."""
    rng = np.random.default_rng(seed)
    top = 1023 if fmt == "p010" else 255
    ch, cw = (H + 1) // 2, (W + 1) // 2
    y = rng.integers(0, top + 1, (N, H, W))
    u, v = rng.integers(0, top + 1, (2, N, ch, cw))
    for i in range(N):
        by, bx = 2 * ((3 * i + 1) % 16), 2 * ((5 * i + 2) % 24)
        y[i, by:by + 4, bx:bx + 4] = top * rng.integers(0, 2, (4, 4))
        u[i, by // 2:by // 2 + 2, bx // 2:bx // 2 + 2] = [[0, top], [top, 0]]
        v[i, by // 2:by // 2 + 2, bx // 2:bx // 2 + 2] = [[0, top], [0, top]]
    if fmt == "p010":  # the low 6 bits are noise the kernel must ignore
        y, u, v = ((p.astype(np.uint16) << 6) | rng.integers(0, 64, p.shape).astype(np.uint16) for p in (y, u, v))
    else:
        y, u, v = (p.astype(np.uint8) for p in (y, u, v))
    out = (y, u, v) if fmt == "i420" else (y, np.stack([u, v], -1))
    for p in out:
        p.setflags(write=False)
    return out


def _upload(planes, cuda, shift):
    """The planes on the device, each `shift` elements into an allocation of its own (shift 1: an NV12 pair starts at
    an odd byte, a P010 pair 2 bytes off a multiple of 4: one load a sample in place of one a pair)."""
    out = []
    for p in planes:
        t = torch.from_numpy(p.copy().view(np.int16) if p.dtype == np.uint16 else p.copy())
        buf = torch.empty(t.numel() + shift, dtype=t.dtype, device=cuda)
        d = buf[shift:].view(t.shape)
        d.copy_(t.to(cuda))
        assert d.data_ptr() == buf.data_ptr() + shift * t.element_size()
        out.append(d)
    return tuple(out)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("matrix, rng", [("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full")])
@pytest.mark.parametrize("fmt", ["nv12", "i420", "p010"])
def test_yuv_views(cuda, fmt, matrix, rng, shift):
    s = 8
    table = _table(s)[[0, 3, 4, 7]]  # the whole frame; an odd origin; the last luma pixel; a mirrored upscale
    idx = IDX[[0, 3, 4, 7]]
    rgb = yr.yuv_to_rgb(_planes(fmt), fmt, matrix, rng)
    want = _want(rgb, table, idx, s)
    planes = _upload(_planes(fmt), cuda, shift)
    if fmt != "i420":  # which of the two instantiations runs: the pairs' common alignment
        pair = (planes[1].data_ptr() | planes[1].stride(1) * planes[1].element_size()) % (4 if fmt == "p010" else 2) == 0
        assert pair == (shift == 0)
    got = nat.op_preprocess_yuv_views(planes, _dev(table, cuda), FMT[fmt], MATRIX[matrix], RANGE[rng], _dev(idx, cuda),
                                      size=s)
    _same(got.view(4, 3, s, s, 3), want)
    _same(video_utils.preprocess_yuv_frames(planes, pixel_format=fmt, matrix=matrix, color_range=rng, target_size=s,
                                            views=table, frame_indices=idx), want)
    on_rgb = nat.op_preprocess_views(_dev(rgb, cuda), _dev(table, cuda), _dev(idx, cuda), size=s)
    torch.cuda.synchronize()
    assert torch.equal(got, on_rgb)


def test_yuv_batched_and_device_table(cuda):
    s, fmt = 7, "nv12"
    planes = _planes(fmt)
    rgb = yr.yuv_to_rgb(planes, fmt, "bt601", "limited")[:4].reshape(2, 2, H, W, 3)
    batch = tuple(p[:4].reshape((2, 2) + p.shape[1:]).copy() for p in planes)
    t8 = _table(s)
    tables = np.stack([t8[[7, 3]], t8[[4, 0]]])
    idx = np.array([[[1, 0], [0, 0]], [[1, 1], [0, 1]]])
    want = np.stack([_want(rgb[i], tables[i], idx[i], s) for i in range(2)])
    _same(video_utils.preprocess_yuv_frames(batch, matrix="bt601", target_size=s, views=tables, frame_indices=idx), want)
    bad = tables.copy()
    bad[0, 0, 2:4] = 10 ** 6  # view 8's box runs out of the frame: clamped to the frame's edge
    good = bad.copy()
    good[0, 0, 2:4] = (H - 1, W - 3)
    dev = tuple(_dev(p, cuda) for p in batch)
    got = video_utils.preprocess_yuv_frames(dev, matrix="bt601", target_size=s, views=_dev(bad, cuda),
                                            frame_indices=_dev(idx, cuda))
    _same(got, np.stack([_want(rgb[i], good[i], idx[i], s) for i in range(2)]))
    with pytest.raises(ValueError, match="view 0 of video 0: box"):
        video_utils.preprocess_yuv_frames(dev, matrix="bt601", target_size=s, views=bad, frame_indices=idx)


# ---- end to end ----
def test_multi_view_evaluation_clips(cuda):
    n, h, w, s = 20, 40, 64, 16
    video = _frames(n, h, w, 21)
    idx, views = video_utils.multi_view(n, h, w, num_frames=4, temporal_views=2, spatial_views=3, target_size=s)
    assert idx.shape == (6, 4) and views.shape == (6, 9)
    assert idx[0].tolist() == [0, 1, 2, 3] and idx[5].tolist() == [16, 17, 18, 19]
    assert views[:, 7].tolist() == [0, 4, 9] * 2 and (views[:, 4:6] == [16, 25]).all()
    got = video_utils.preprocess_frames(np.array(video), target_size=s, views=views, frame_indices=idx)
    assert tuple(got.shape) == (6, 4, s, s, 3)
    _same(got, _want(video, views, idx, s))
    # the centre window of clip 0 is what preprocess_frames gives without views
    plain = video_utils.preprocess_frames(np.array(video), target_size=s, frame_indices=idx[1])
    torch.cuda.synchronize()
    assert torch.equal(got[1], plain)
