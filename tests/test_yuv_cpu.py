"""YUV ingest without a GPU: the pinned coefficient tables (library and restatement), the distance of the
integer conversion from the real-valued formula, chroma replication, P010's sample position, the
argument checks of vp_op_preprocess_yuv (made before any device call) and preprocess_yuv_frames' host checks."""

import ctypes
import itertools

import numpy as np
import pytest

import yuv_restatement as yr
from videoprism import _native, video_utils

# (bit depth, matrix, range) -> rows R, G, B x (cy, cu, cv)
TABLES = {
    (8, "bt601", "limited"): ((76309, 0, 104597), (76309, -25675, -53279), (76309, 132201, 0)),
    (8, "bt601", "full"): ((65536, 0, 91881), (65536, -22553, -46802), (65536, 116130, 0)),
    (8, "bt709", "limited"): ((76309, 0, 117489), (76309, -13975, -34925), (76309, 138438, 0)),
    (8, "bt709", "full"): ((65536, 0, 103206), (65536, -12276, -30679), (65536, 121609, 0)),
    (10, "bt601", "limited"): ((19077, 0, 26149), (19077, -6419, -13320), (19077, 33050, 0)),
    (10, "bt601", "full"): ((16336, 0, 22903), (16336, -5622, -11666), (16336, 28947, 0)),
    (10, "bt709", "limited"): ((19077, 0, 29372), (19077, -3494, -8731), (19077, 34610, 0)),
    (10, "bt709", "full"): ((16336, 0, 25726), (16336, -3060, -7647), (16336, 30313, 0)),
}
MATRIX = {"bt601": _native.VP_YUV_BT601, "bt709": _native.VP_YUV_BT709}
RANGE = {"limited": _native.VP_YUV_LIMITED, "full": _native.VP_YUV_FULL}
# 0.5 for the final rounding + (1023 + 512 + 512) * 2^-17 for the coefficients' rounding
BOUND = 0.516


@pytest.mark.parametrize("key", list(TABLES), ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}")
def test_coefficient_tables(key):
    depth, matrix, rng = key
    want = [list(row) for row in TABLES[key]]
    yoff = (16 << (depth - 8)) if rng == "limited" else 0
    coff = 128 << (depth - 8)
    out = (ctypes.c_int32 * 11)()
    assert _native.load().vp_dev_yuv_coefficients(MATRIX[matrix], RANGE[rng], depth, out) == _native.VP_OK
    assert list(out) == sum(want, []) + [yoff, coff]
    assert _native.yuv_coefficients(MATRIX[matrix], RANGE[rng], depth) == (want, yoff, coff)
    c, y0, c0 = yr.coefficients(matrix, rng, depth)
    assert c.dtype == np.int32 and c.tolist() == want and (y0, c0) == (yoff, coff)


def test_coefficients_refuse_unknown_arguments():
    fn = _native.load().vp_dev_yuv_coefficients
    out = (ctypes.c_int32 * 11)()
    E = _native.VP_EINVAL
    assert fn(2, 0, 8, out) == E and fn(-1, 0, 8, out) == E
    assert fn(0, 2, 8, out) == E and fn(0, 0, 9, out) == E and fn(0, 0, 12, out) == E
    assert fn(0, 0, 8, None) == E


def _triples(depth, seed, count=1 << 20):
    top = (1 << depth) - 1
    corners = np.array(list(itertools.product([0, 1, 1 << (depth - 1), top - 1, top], repeat=3)), dtype=np.int64)
    assert corners.shape == (125, 3)
    rand = np.random.default_rng(seed).integers(0, top + 1, (count, 3), dtype=np.int64)
    return np.concatenate([corners, rand])


@pytest.mark.parametrize("key", list(TABLES), ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}")
def test_integer_form_within_bound_of_real_formula_and_inside_int32(key):
    depth, matrix, rng = key
    t = _triples(depth, seed=depth * 7 + len(matrix) + len(rng))
    y, u, v = t[:, 0], t[:, 1], t[:, 2]
    got = yr.convert(y, u, v, matrix, rng, depth)
    assert got.dtype == np.uint8 and got.shape == (len(t), 3)
    err = np.abs(got.astype(np.float64) - yr.convert_real(y, u, v, matrix, rng, depth)).max()
    acc = yr.accumulate(y, u, v, matrix, rng, depth)
    print(f"{key}: max |integer - real| = {err:.4f}, accumulators in [{acc.min()}, {acc.max()}]")
    assert err <= BOUND
    assert acc.min() >= -2 ** 31 and acc.max() < 2 ** 31
    # int32 arithmetic and the wide one agree, so nothing wrapped on the way
    assert np.array_equal(got, np.clip(acc >> 16, 0, 255).astype(np.uint8))
    # the extreme sums over the whole sample cube are at its corners (the form is linear): they fit too
    top = (1 << depth) - 1
    cube = np.array(list(itertools.product([0, top], repeat=3)), dtype=np.int64)
    ext = yr.accumulate(cube[:, 0], cube[:, 1], cube[:, 2], matrix, rng, depth)
    assert np.abs(ext).max() < 3.7e7


def _planes(fmt, h, w, y, u, v):
    """Planes of `fmt` from sample arrays y [h, w] and u, v [ch, cw] (10-bit samples for p010)."""
    if fmt == "i420":
        return y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)
    uv = np.stack([u, v], -1)
    if fmt == "nv12":
        return y.astype(np.uint8), uv.astype(np.uint8)
    return (y.astype(np.uint16) << 6), (uv.astype(np.uint16) << 6)


@pytest.mark.parametrize("fmt", ["nv12", "i420", "p010"])
def test_chroma_replication_on_an_odd_frame(fmt):
    h, w, ch, cw = 5, 7, 3, 4
    top = 1023 if fmt == "p010" else 255
    scale = 4 if fmt == "p010" else 1
    y = np.full((h, w), 128 * scale)
    u = (10 + 13 * np.arange(ch * cw).reshape(ch, cw)) * scale     # a distinct value per chroma sample
    v = (top - 7 * scale * np.arange(ch * cw)).reshape(ch, cw)
    assert len(set(u.ravel())) == len(set(v.ravel())) == ch * cw and u.max() <= top and v.min() >= 0
    rgb = yr.yuv_to_rgb(_planes(fmt, h, w, y, u, v), fmt, "bt601", "full")
    assert rgb.shape == (h, w, 3)
    depth = yr.BIT_DEPTH[fmt]
    for yy in range(h):
        for xx in range(w):
            want = yr.convert(y[yy, xx], u[yy >> 1, xx >> 1], v[yy >> 1, xx >> 1], "bt601", "full", depth)
            assert np.array_equal(rgb[yy, xx], want), (yy, xx)
    # the replicated planes themselves
    assert np.array_equal(yr.replicate_chroma(u, h, w)[4, 6], u[2, 3])
    assert np.array_equal(yr.replicate_chroma(u, h, w)[:, 1::2][:, :3], yr.replicate_chroma(u, h, w)[:, 0:6:2])


def test_p010_reads_the_high_ten_bits():
    rng = np.random.default_rng(3)
    h, w = 6, 8
    y = rng.integers(0, 1024, (h, w))
    u, v = rng.integers(0, 1024, (2, 3, 4))
    clean = _planes("p010", h, w, y, u, v)
    dirty = tuple(p | rng.integers(0, 64, p.shape).astype(np.uint16) for p in clean)
    assert any((d & 63).any() for d in dirty)
    for got in (yr.samples(dirty, "p010"), yr.samples(tuple(d.view(np.int16) for d in dirty), "p010")):
        assert np.array_equal(got[0], y) and np.array_equal(got[1], u) and np.array_equal(got[2], v)
    want = yr.yuv_to_rgb(clean, "p010", "bt709", "limited")
    assert np.array_equal(yr.yuv_to_rgb(dirty, "p010", "bt709", "limited"), want)
    assert np.array_equal(want, yr.convert(y, yr.replicate_chroma(u, h, w), yr.replicate_chroma(v, h, w),
                                           "bt709", "limited", 10))


def test_symbols_exported_and_abi_version_unchanged():
    lib = _native.load()
    for s in ("vp_op_preprocess_yuv", "vp_dev_yuv_coefficients"):
        assert hasattr(lib, s), s
        assert s in _native.exported_symbols(), s
        assert getattr(lib, s).argtypes is not None
    assert lib.vp_abi_version() == 8
    assert callable(_native.op_preprocess_yuv)


def test_preprocess_yuv_argument_checks_touch_no_gpu():
    lib = _native.load()
    fn = lib.vp_op_preprocess_yuv
    E = _native.VP_EINVAL
    P = 0x1000  # never dereferenced: every call below is refused first

    def call(src="default", fmt=0, matrix=0, rng=0, planes=(P, P + 0x10000, None), rs=(30, 30, 0),
             fs=(600, 300, 0), N=4, H=20, W=30, idx=None, F=4, mode=0, S=16, dst=ctypes.c_void_p(P)):
        if src == "default":
            s = _native.vp_yuv_frames(format=fmt, matrix=matrix, range=rng)
            for i in range(3):
                s.plane[i], s.row_stride[i], s.frame_stride[i] = planes[i], rs[i], fs[i]
            src = ctypes.byref(s)
        return fn(src, N, H, W, idx, F, mode, S, dst, None)

    i420 = dict(fmt=1, planes=(P, P + 0x10000, P + 0x20000), rs=(30, 15, 15), fs=(600, 150, 150))
    p010 = dict(fmt=2, rs=(60, 60, 0), fs=(1200, 600, 0))
    # null src, Y plane, dst
    assert call(src=None) == E
    assert call(planes=(None, P, None)) == E
    assert call(dst=None) == E
    # a missing chroma plane
    assert call(planes=(P, None, None)) == E and b"chroma" in lib.vp_last_error()
    assert call(**dict(i420, planes=(P, P, None))) == E and b"chroma" in lib.vp_last_error()
    assert call(**dict(p010, planes=(P, None, None))) == E
    # a row stride shorter than the row (odd W = 31: 16 pairs = 32 bytes of chroma)
    assert call(rs=(29, 30, 0)) == E and b"row_stride[0]" in lib.vp_last_error()
    assert call(rs=(30, 29, 0)) == E and b"row_stride[1]" in lib.vp_last_error()
    assert call(W=31, rs=(31, 31, 0), fs=(620, 310, 0)) == E and b"row_stride[1]" in lib.vp_last_error()
    assert call(**dict(i420, rs=(30, 15, 14))) == E and b"row_stride[2]" in lib.vp_last_error()
    assert call(**dict(p010, rs=(58, 60, 0))) == E and call(**dict(p010, rs=(60, 58, 0))) == E
    assert call(fs=(599, 300, 0)) == E and b"frame_stride[0]" in lib.vp_last_error()
    assert call(fs=(600, 299, 0)) == E and b"frame_stride[1]" in lib.vp_last_error()
    # P010: strides and bases are multiples of 2
    assert call(**dict(p010, rs=(61, 60, 0), fs=(1220, 600, 0))) == E and b"multiples of 2" in lib.vp_last_error()
    assert call(**dict(p010, rs=(60, 61, 0), fs=(1200, 610, 0))) == E
    assert call(**dict(p010, fs=(1201, 600, 0))) == E and call(**dict(p010, fs=(1200, 601, 0))) == E
    assert call(**dict(p010, planes=(P + 1, P + 0x10000, None))) == E
    assert call(**dict(p010, planes=(P, P + 0x10001, None))) == E
    # H, W, S (and N, F) below 1
    for k in ("N", "H", "W", "F", "S"):
        assert call(**{k: 0}) == E, k
        assert call(**{k: -1}) == E, k
    # unknown enums
    assert call(fmt=3) == E and call(fmt=-1) == E
    assert call(matrix=2) == E and call(matrix=-1) == E
    assert call(rng=2) == E and call(rng=-1) == E
    assert call(mode=2) == E and call(mode=-1) == E
    # as vp_op_preprocess_frames: more frames than the video has, and a geometry preprocess_geometry refuses
    assert call(F=5) == E and b"Video has only 4 frames, but 5 requested" in lib.vp_last_error()
    rgb = lib.vp_op_preprocess_frames(ctypes.c_void_p(P), 1, 1, 1 << 23, 3 << 23, 3 << 23, None, 1, 0, 0, 16,
                                      ctypes.c_void_p(P), None)
    rgb_msg = lib.vp_last_error()
    assert rgb == E
    assert call(N=1, F=1, H=1, W=1 << 23, rs=(1 << 23, 1 << 23, 0), fs=(1 << 23, 1 << 23, 0)) == rgb
    assert lib.vp_last_error() == rgb_msg
    with pytest.raises(ValueError):
        _native.check(call(fmt=3))


def _nv12(n=2, h=8, w=10, lead=()):
    return (np.zeros(lead + (n, h, w), np.uint8), np.zeros(lead + (n, (h + 1) // 2, (w + 1) // 2, 2), np.uint8))


def test_preprocess_yuv_frames_host_checks(monkeypatch):
    import torch
    # any device use would end here: the checks below run before it
    monkeypatch.setattr(torch.Tensor, "to", lambda *a, **k: pytest.fail("device use before the argument checks"))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: pytest.fail("device use before the argument checks"))
    f = video_utils.preprocess_yuv_frames
    y, uv = _nv12()
    with pytest.raises(ValueError, match="Unknown pixel_format: yuyv"):
        f((y, uv), pixel_format="yuyv")
    with pytest.raises(ValueError, match="Unknown matrix: bt2020"):
        f((y, uv), matrix="bt2020")
    with pytest.raises(ValueError, match="Unknown color_range: tv"):
        f((y, uv), color_range="tv")
    with pytest.raises(ValueError, match="Unknown resize_mode: pad"):
        f((y, uv), resize_mode="pad")
    # number of planes
    with pytest.raises(ValueError, match="2 planes"):
        f((y, uv, uv))
    with pytest.raises(ValueError, match="3 planes"):
        f((y, uv), pixel_format="i420")
    # dtypes
    with pytest.raises(ValueError, match="uint8"):
        f((y.astype(np.uint16), uv.astype(np.uint16)))
    with pytest.raises(ValueError, match="16-bit"):
        f((y, uv), pixel_format="p010")
    with pytest.raises(ValueError, match="uint8"):
        f((y.astype(np.float32), uv))
    with pytest.raises(ValueError, match="uint8"):
        f((torch.zeros(2, 8, 10, dtype=torch.float32), torch.from_numpy(uv)))
    # plane shapes against height / width
    with pytest.raises(ValueError, match="Y plane"):
        f((y, uv), height=9)
    with pytest.raises(ValueError, match="Y plane"):
        f((y, uv), width=12)
    with pytest.raises(ValueError, match="Y plane"):
        f((y[0, 0], uv))
    with pytest.raises(ValueError, match="UV plane"):
        f((y, uv[:, :3]))
    with pytest.raises(ValueError, match="UV plane"):
        f((y, uv[..., 0]))
    with pytest.raises(ValueError, match="UV plane"):
        f((np.zeros((2, 9, 11), np.uint8), np.zeros((2, 4, 5, 2), np.uint8)))  # odd sizes round up: 5 x 6
    with pytest.raises(ValueError, match="V plane"):
        f((y, uv[..., 0], uv[:, :, :4, 1]), pixel_format="i420")
    yb, uvb = _nv12(lead=(3,))
    with pytest.raises(ValueError, match="UV plane"):
        f((yb, uvb[0]))
    # sampling, as preprocess_frames
    with pytest.raises(ValueError, match="Video has only 2 frames, but 3 requested"):
        f((y, uv), num_frames=3)
    with pytest.raises(ValueError, match=r"frame_indices must lie in \[0, 1\]"):
        f((y, uv), frame_indices=[0, 2])
    with pytest.raises(ValueError, match="non-empty 1-D"):
        f((y, uv), frame_indices=[])


@pytest.mark.parametrize("h, w, want", [(720, 1280, "bt709"), (576, 1024, "bt601"), (576, 720, "bt601"),
                                        (480, 720, "bt601"), (1080, 1920, "bt709"), (577, 720, "bt709")])
def test_auto_matrix(h, w, want):
    assert video_utils.yuv_matrix("auto", h, w) == want
    assert video_utils.yuv_matrix("bt601", h, w) == "bt601" and video_utils.yuv_matrix("bt709", h, w) == "bt709"
    with pytest.raises(ValueError):
        video_utils.yuv_matrix("bt2020", h, w)


def test_exported_from_the_package():
    import videoprism
    assert videoprism.preprocess_yuv_frames is video_utils.preprocess_yuv_frames
