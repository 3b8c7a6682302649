"""Views in the frame ingest, without a GPU: the two entry points are exported and bound, the host helpers of
videoprism.video_utils (view_table, multi_view, random_resized_crop) build what they document, a host table is
validated before any device use, and vp_op_preprocess_views / vp_op_preprocess_yuv_views refuse bad arguments before
any device call."""

import ctypes

import numpy as np
import pytest

import preprocess_restatement as pr
from videoprism import _native, video_utils

S24 = 1 << 24


def test_symbols_exported_and_abi_version_unchanged():
    lib = _native.load()
    for s in ("vp_op_preprocess_views", "vp_op_preprocess_yuv_views"):
        assert hasattr(lib, s), s
        assert s in _native.exported_symbols(), s
        assert getattr(lib, s).argtypes is not None
    assert lib.vp_abi_version() == 8
    assert callable(_native.op_preprocess_views) and callable(_native.op_preprocess_yuv_views)


# ---- view_table ----
# the frame sizes tests/test_gpu_preprocess.py and tests/test_gpu_preprocess_yuv.py run, and the benchmark's
@pytest.mark.parametrize("h, w, s", [(37, 53, 36), (45, 80, 36), (53, 37, 36), (20, 31, 36), (240, 426, 288),
                                     (720, 1280, 288), (1080, 1920, 288), (64, 48, 36), (72, 72, 36), (25, 33, 37)])
def test_whole_frame_centre_view_is_center_crop_geometry(h, w, s):
    new_h, new_w, y0, x0 = video_utils.center_crop_geometry(h, w, s)
    assert (new_h, new_w, y0, x0) == pr.center_crop_geometry(h, w, s)
    t = video_utils.view_table(h, w, target_size=s)
    assert t.dtype == np.int32 and t.shape == (1, 9)
    assert t[0].tolist() == [0, 0, h, w, new_h, new_w, y0, x0, 0]
    assert video_utils.view_table(h, w, target_size=s, resize_mode="resize")[0].tolist() == [0, 0, h, w, s, s, 0, 0, 0]


def test_view_table_positions_boxes_and_flips():
    h, w, s = 45, 80, 36
    new_h, new_w, y0, x0 = pr.center_crop_geometry(h, w, s)  # 36 x 64
    assert (new_h, new_w) == (36, 64)
    t = video_utils.view_table(h, w, target_size=s, position=["start", "center", "end"])
    assert t.shape == (3, 9)
    assert t[:, 6:8].tolist() == [[0, 0], [0, (64 - 36) // 2], [0, 64 - 36]]
    assert (t[:, :6] == [0, 0, h, w, 36, 64]).all() and (t[:, 8] == 0).all()
    # portrait: the slack is along y
    t = video_utils.view_table(80, 45, target_size=s, position=["start", "center", "end"])
    assert t[:, 4:8].tolist() == [[64, 36, 0, 0], [64, 36, 14, 0], [64, 36, 28, 0]]
    # boxes: the geometry is the box's, not the frame's
    boxes = [(3, 1, 30, 9), (5, 7, 21, 30)]
    t = video_utils.view_table(h, w, boxes=boxes, target_size=8, position="end", flip=[False, True])
    for row, (by, bx, bh, bw), fl in zip(t.tolist(), boxes, (0, 1)):
        nh, nw, _, _ = pr.center_crop_geometry(bh, bw, 8)
        assert row == [by, bx, bh, bw, nh, nw, nh - 8, nw - 8, fl]
    t = video_utils.view_table(h, w, boxes=np.array(boxes), target_size=8, resize_mode="resize", flip=True)
    assert t.tolist() == [[3, 1, 30, 9, 8, 8, 0, 0, 1], [5, 7, 21, 30, 8, 8, 0, 0, 1]]
    # one box, several flips
    t = video_utils.view_table(h, w, boxes=[(0, 0, 45, 45)], target_size=8, flip=np.array([False, True]))
    assert t.shape == (2, 9) and t[:, 8].tolist() == [0, 1] and (t[0, :8] == t[1, :8]).all()


def test_view_table_refuses():
    f = video_utils.view_table
    with pytest.raises(ValueError, match="view 1: box"):
        f(20, 30, boxes=[(0, 0, 20, 30), (1, 0, 20, 30)])
    with pytest.raises(ValueError, match="view 0: box"):
        f(20, 30, boxes=[(0, -1, 20, 30)])
    with pytest.raises(ValueError, match="view 0: box_h and box_w"):
        f(20, 30, boxes=[(0, 0, 0, 30)])
    with pytest.raises(ValueError, match="position"):
        f(20, 30, position="middle")
    with pytest.raises(ValueError, match="Unknown resize_mode"):
        f(20, 30, resize_mode="pad")
    with pytest.raises(ValueError, match="one per view"):
        f(20, 30, boxes=[(0, 0, 20, 30)] * 3, flip=[True, False])
    with pytest.raises(ValueError, match="integer rows"):
        f(20, 30, boxes=[(0.5, 0, 20, 30)])


# ---- multi_view ----
def test_multi_view_indices_windows_and_order():
    idx, views = video_utils.multi_view(100, 45, 80, num_frames=4, temporal_views=4, spatial_views=3, dilation=2,
                                        target_size=36)
    assert idx.dtype == np.int32 and idx.shape == (12, 4) and views.dtype == np.int32 and views.shape == (12, 9)
    span = 3 * 2 + 1
    starts = np.linspace(0, 100 - span, 4, dtype=int)
    assert starts.tolist() == [0, 31, 62, 93]
    xs = np.linspace(0, 64 - 36, 3, dtype=int)
    assert xs.tolist() == [0, 14, 28]
    for v in range(12):  # temporal-major
        t, s = divmod(v, 3)
        assert idx[v].tolist() == [starts[t] + 2 * k for k in range(4)]
        assert views[v].tolist() == [0, 0, 45, 80, 36, 64, 0, xs[s], 0]
    assert idx.max() == 99
    # a single window is the centre one, i.e. the view preprocess_frames computes without a table
    idx, views = video_utils.multi_view(16, 240, 426, temporal_views=2, spatial_views=1)
    assert idx.tolist() == [list(range(16))] * 2
    assert (views == video_utils.view_table(240, 426)).all() and views[0, 7] == 111
    # two windows: the two ends; a square frame has no slack
    _, views = video_utils.multi_view(16, 53, 37, spatial_views=2, temporal_views=1, target_size=36)
    assert views[:, 4:8].tolist() == [[51, 36, 0, 0], [51, 36, 15, 0]]
    _, views = video_utils.multi_view(16, 72, 72, temporal_views=1, target_size=36)
    assert (views[:, 6:8] == 0).all()


def test_multi_view_short_video():
    with pytest.raises(ValueError, match="Video has only 30 frames, but a clip spans 31"):
        video_utils.multi_view(30, 45, 80, num_frames=16, dilation=2)
    idx, _ = video_utils.multi_view(31, 45, 80, num_frames=16, dilation=2, target_size=36)
    assert (idx == np.arange(0, 31, 2)).all()  # every clip is the whole video
    with pytest.raises(ValueError):
        video_utils.multi_view(100, 45, 80, temporal_views=0)


# ---- random_resized_crop ----
def test_random_resized_crop_boxes_within_the_ranges():
    # scale <= 0.5 on a square frame: sqrt(0.5 * 4 / 3) < 1, so every first try fits
    h = w = 100
    scale, ratio = (0.08, 0.5), (3 / 4, 4 / 3)
    boxes = video_utils.random_resized_crop(h, w, 500, scale=scale, ratio=ratio, rng=np.random.default_rng(5))
    assert boxes.dtype == np.int32 and boxes.shape == (500, 4)
    y, x, bh, bw = boxes.T.astype(np.float64)
    assert (y >= 0).all() and (x >= 0).all() and (bh >= 1).all() and (bw >= 1).all()
    assert (y + bh <= h).all() and (x + bw <= w).all()
    # each side was rounded to an integer: half a pixel a side around the drawn area and ratio
    lo_area = (np.sqrt(scale[0] * h * w * ratio[0]) - 0.5) * (np.sqrt(scale[0] * h * w / ratio[0]) - 0.5)
    hi_area = (np.sqrt(scale[1] * h * w * ratio[0]) + 0.5) * (np.sqrt(scale[1] * h * w / ratio[0]) + 0.5)
    assert (bh * bw >= lo_area).all() and (bh * bw <= hi_area).all()
    assert ((bw + 0.5) / (bh - 0.5) >= ratio[0]).all() and ((bw - 0.5) / (bh + 0.5) <= ratio[1]).all()
    assert len({tuple(b) for b in boxes.tolist()}) > 400  # they are spread
    # the default ranges on a video frame: inside the frame whatever path a box took
    boxes = video_utils.random_resized_crop(720, 1280, 200, rng=3)
    assert (boxes[:, :2] >= 0).all() and (boxes[:, 2:] >= 1).all()
    assert (boxes[:, 0] + boxes[:, 2] <= 720).all() and (boxes[:, 1] + boxes[:, 3] <= 1280).all()
    assert video_utils.view_table(720, 1280, boxes=boxes, resize_mode="resize").shape == (200, 9)


def test_random_resized_crop_fallback():
    # the whole area of a 10 x 1000 strip at a ratio of at most 4/3 is at least 86 high: no try fits
    assert video_utils.random_resized_crop(10, 1000, 3, scale=(1.0, 1.0), rng=0).tolist() == [[0, 493, 10, 13]] * 3
    assert video_utils.random_resized_crop(1000, 10, 2, scale=(1.0, 1.0), rng=0).tolist() == [[493, 0, 13, 10]] * 2
    # inside the ratio range but never fitting (an area twice the frame's): the whole frame
    assert video_utils.random_resized_crop(30, 40, 1, scale=(2.0, 2.0), rng=0).tolist() == [[0, 0, 30, 40]]


def test_random_resized_crop_is_reproducible():
    a = video_utils.random_resized_crop(720, 1280, 50, rng=np.random.default_rng(11))
    b = video_utils.random_resized_crop(720, 1280, 50, rng=np.random.default_rng(11))
    c = video_utils.random_resized_crop(720, 1280, 50, rng=np.random.default_rng(12))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(a, video_utils.random_resized_crop(720, 1280, 50, rng=11))
    g = np.random.default_rng(11)  # one generator carries on
    first, second = video_utils.random_resized_crop(720, 1280, 25, rng=g), video_utils.random_resized_crop(720, 1280, 25, rng=g)
    assert np.array_equal(np.concatenate([first, second]), a)
    with pytest.raises(ValueError):
        video_utils.random_resized_crop(720, 1280, 1, scale=(0.5, 0.1))


# ---- host-table validation: before any device use ----
GOOD = [0, 0, 20, 30, 16, 24, 0, 4, 0]  # the whole 20 x 30 frame, centre-crop geometry of S = 16


def _bad(**kw):
    names = ["box_y", "box_x", "box_h", "box_w", "new_h", "new_w", "win_y", "win_x", "flags"]
    row = list(GOOD)
    for k, v in kw.items():
        row[names.index(k)] = v
    return row


BAD_ROWS = [
    (_bad(box_y=-1), "box"), (_bad(box_x=1), "box"), (_bad(box_h=21), "box"), (_bad(box_y=19, box_h=2), "box"),
    (_bad(box_h=0), "box_h and box_w"), (_bad(box_w=-3), "box_h and box_w"),
    (_bad(new_h=15), "new_h and new_w"), (_bad(new_w=S24), "new_h and new_w"), (_bad(new_w=0), "new_h and new_w"),
    (_bad(win_y=1), "window"), (_bad(win_x=9), "window"), (_bad(win_x=-1), "window"), (_bad(win_x=10 ** 6), "window"),
    (_bad(flags=2), "flags"), (_bad(flags=-1), "flags"),
]


@pytest.fixture
def no_device(monkeypatch):
    import torch
    # any device use would end here: the checks run before it
    monkeypatch.setattr(torch.Tensor, "to", lambda *a, **k: pytest.fail("device use before the argument checks"))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: pytest.fail("device use before the argument checks"))


@pytest.mark.parametrize("row, what", BAD_ROWS, ids=[f"{i}-{w.split()[0]}" for i, (_, w) in enumerate(BAD_ROWS)])
def test_host_table_is_validated_before_any_device_use(no_device, row, what):
    frames = np.zeros((2, 20, 30, 3), np.uint8)
    planes = (np.zeros((2, 20, 30), np.uint8), np.zeros((2, 10, 15, 2), np.uint8))
    table = [GOOD, row, GOOD]
    for call in (lambda v: video_utils.preprocess_frames(frames, target_size=16, views=v),
                 lambda v: video_utils.preprocess_yuv_frames(planes, target_size=16, views=v)):
        with pytest.raises(ValueError, match=f"view 1: .*{what}"):
            call(table)
        with pytest.raises(ValueError, match=f"view 1: .*{what}"):
            call(np.array(table, dtype=np.int32))
    with pytest.raises(ValueError, match=f"view 1 of video 1: .*{what}"):
        video_utils.preprocess_frames(frames[None].repeat(2, 0), target_size=16, views=[[GOOD] * 3, table])


def test_views_argument_checks_before_any_device_use(no_device):
    frames = np.zeros((2, 20, 30, 3), np.uint8)
    planes = (np.zeros((2, 20, 30), np.uint8), np.zeros((2, 10, 15, 2), np.uint8))
    f = lambda **kw: video_utils.preprocess_frames(frames, target_size=16, **kw)  # noqa: E731
    y = lambda **kw: video_utils.preprocess_yuv_frames(planes, target_size=16, **kw)  # noqa: E731
    for g in (f, y):
        with pytest.raises(ValueError, match="views carry the geometry"):
            g(views=[GOOD], resize_mode="resize")
        with pytest.raises(ValueError, match=r"views must be int32 \[V, 9\]"):
            g(views=[GOOD[:8]])
        with pytest.raises(ValueError, match=r"views must be int32 \[V, 9\]"):
            g(views=[[GOOD]])  # [B, V, 9] needs batched frames
        with pytest.raises(ValueError, match=r"views must be int32 \[V, 9\]"):
            g(views=np.zeros((0, 9), np.int32))
        with pytest.raises(ValueError, match="views must be integers"):
            g(views=np.array([GOOD], dtype=np.float32))
        with pytest.raises(ValueError, match=r"frame_indices must lie in \[0, 1\]"):
            g(views=[GOOD], frame_indices=[0, 2])
        with pytest.raises(ValueError, match=r"frame_indices must be \[T\], \[2, T\]"):
            g(views=[GOOD, GOOD], frame_indices=[[0, 1]] * 3)
        with pytest.raises(ValueError, match=r"frame_indices must be \[T\], \[1, T\]"):
            g(views=[GOOD], frame_indices=[[[0, 1]]])  # [B, V, T] needs batched frames
        with pytest.raises(ValueError, match="Video has only 2 frames, but 3 requested"):
            g(views=[GOOD], num_frames=3)
    with pytest.raises(ValueError, match=r"views must be int32 \[V, 9\] or \[2, V, 9\]"):
        video_utils.preprocess_frames(frames[None].repeat(2, 0), target_size=16, views=[[GOOD]] * 3)
    with pytest.raises(ValueError, match="frames must be uint8"):
        video_utils.preprocess_frames(frames[0], target_size=16, views=[GOOD])


# ---- the C entry points refuse before any device call ----
def test_preprocess_views_argument_checks_touch_no_gpu():
    lib = _native.load()
    E = _native.VP_EINVAL
    P = 0x1000  # never dereferenced: every call below is refused first
    ptr = ctypes.c_void_p

    def rgb(src=ptr(P), N=4, H=20, W=30, rs=90, fs=1800, idx=None, views=ptr(P), V=2, T=4, S=16, dst=ptr(P)):
        return lib.vp_op_preprocess_views(src, N, H, W, rs, fs, idx, views, V, T, 0, S, dst, None)

    def yuv(src="default", planes=(P, P + 0x10000, None), rs=(30, 30, 0), fs=(600, 300, 0), fmt=0, N=4, H=20, W=30,
            idx=None, views=ptr(P), V=2, T=4, S=16, dst=ptr(P)):
        if src == "default":
            s = _native.vp_yuv_frames(format=fmt, matrix=0, range=0)
            for i in range(3):
                s.plane[i], s.row_stride[i], s.frame_stride[i] = planes[i], rs[i], fs[i]
            src = ctypes.byref(s)
        return lib.vp_op_preprocess_yuv_views(src, N, H, W, idx, views, V, T, S, dst, None)

    for call in (rgb, yuv):
        assert call(src=None) == E and call(dst=None) == E and call(views=None) == E
        for k in ("N", "H", "W", "V", "T", "S"):
            assert call(**{k: 0}) == E, k
            assert call(**{k: -1}) == E, k
        assert call(T=5) == E and b"Video has only 4 frames, but 5 requested" in lib.vp_last_error()
        assert call(H=S24) == E and call(W=S24) == E and call(S=16385) == E
        assert call(V=1 << 16, T=1 << 15, idx=ptr(P)) == E and b"V * T" in lib.vp_last_error()
        assert call(V=1 << 31, idx=ptr(P)) == E and call(T=1 << 31, idx=ptr(P)) == E
        # 81 blocks a frame at S = 288: 2^26 frames are more than one launch takes
        assert call(V=1 << 13, T=1 << 13, S=288, idx=ptr(P)) == E and b"too many output pixels" in lib.vp_last_error()
    assert rgb(rs=89) == E and b"row_stride" in lib.vp_last_error()
    assert rgb(fs=1799) == E and b"frame_stride" in lib.vp_last_error()
    assert yuv(rs=(29, 30, 0)) == E and b"row_stride[0]" in lib.vp_last_error()
    assert yuv(fs=(600, 299, 0)) == E and b"frame_stride[1]" in lib.vp_last_error()
    assert yuv(planes=(P, None, None)) == E and b"chroma" in lib.vp_last_error()
    assert yuv(fmt=3) == E and b"Unknown pixel format" in lib.vp_last_error()
    assert yuv(fmt=2, planes=(P + 1, P + 0x10000, None), rs=(60, 60, 0), fs=(1200, 600, 0)) == E
    assert b"multiples of 2" in lib.vp_last_error()
