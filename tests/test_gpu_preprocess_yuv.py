"""Frame preprocessing from a decoder's 4:2:0 planes (csrc/preprocess.hip through vp_op_preprocess_yuv and
videoprism.video_utils.preprocess_yuv_frames): NV12, I420 and P010 converted to RGB, resized and cropped in
one kernel.  Every comparison is bitwise against the two NumPy restatements chained,
preprocess_restatement.preprocess(yuv_restatement.yuv_to_rgb(planes)).  Every sample is uniform over the
whole 8- or 10-bit range (outside the nominal limited range too), so both clip branches run, and every
frame carries one 4 x 4 block of extremes."""

import functools

import numpy as np
import pytest
import torch

import preprocess_restatement as pr
import yuv_restatement as yr
from videoprism import _native as nat
from videoprism import encoders, models, params, video_utils

pytestmark = pytest.mark.gpu

CROP, STRETCH = nat.VP_RESIZE_CENTER_CROP, nat.VP_RESIZE_STRETCH
MODE = {"center_crop": CROP, "resize": STRETCH}
FMT = {"nv12": nat.VP_YUV_NV12, "i420": nat.VP_YUV_I420, "p010": nat.VP_YUV_P010}
MATRIX = {"bt601": nat.VP_YUV_BT601, "bt709": nat.VP_YUV_BT709}
RANGE = {"limited": nat.VP_YUV_LIMITED, "full": nat.VP_YUV_FULL}


@functools.lru_cache(maxsize=None)
def _planes(fmt, n, h, w, seed):
    """Host planes of `fmt` (read-only): random over the full sample range, one block of extremes per frame."""
    rng = np.random.default_rng(seed)
    top = 1023 if fmt == "p010" else 255
    ch, cw = (h + 1) // 2, (w + 1) // 2
    y = rng.integers(0, top + 1, (n, h, w))
    u, v = rng.integers(0, top + 1, (2, n, ch, cw))
    for i in range(n):  # a 4 x 4 luma block (2 x 2 chroma) of 0 and top, at another even place in every frame
        by, bx = 2 * ((3 * i + 1) % max(1, (h - 4) // 2)), 2 * ((5 * i + 2) % max(1, (w - 4) // 2))
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


@functools.lru_cache(maxsize=None)
def _rgb(fmt, n, h, w, seed, matrix, rng):
    out = yr.yuv_to_rgb(_planes(fmt, n, h, w, seed), fmt, matrix, rng)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(fmt, n, h, w, seed, matrix, rng, size, mode):
    out = pr.preprocess(_rgb(fmt, n, h, w, seed, matrix, rng), size, mode)
    out.setflags(write=False)
    return out


def _upload(planes, dev):
    return tuple(torch.from_numpy(p.copy().view(np.int16) if p.dtype == np.uint16 else p.copy()).to(dev)
                 for p in planes)


def _host(planes, lead=None):
    """Writable NumPy copies of the shared planes, the N frames reshaped to `lead` if given."""
    return tuple(p.reshape(lead + p.shape[1:]).copy() if lead else p.copy() for p in planes)


def _same(got, want):
    torch.cuda.synchronize()
    want = torch.from_numpy(np.array(want))  # a writable copy of the shared reference
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want)


def _run(dev, fmt, n, h, w, seed, matrix, rng, size, mode, **kw):
    x = _upload(_planes(fmt, n, h, w, seed), dev)
    return nat.op_preprocess_yuv(x, FMT[fmt], MATRIX[matrix], RANGE[rng], mode=MODE[mode], size=size, **kw)


# (37, 53): both sides odd, a partial last chroma row and column; (20, 20): upscale; (72, 72): exact 2:1
@pytest.mark.parametrize("h, w", [(37, 53), (20, 20), (72, 72), (19, 61)])
def test_nv12_stretch_to_36(cuda, h, w):
    case = ("nv12", 2, h, w, h * 100 + w, "bt601", "limited", 36, "resize")
    _same(_run(cuda, *case), _want(*case))


# landscape; portrait (y0 = 7); truncated new_w = 55
@pytest.mark.parametrize("h, w", [(45, 80), (53, 37), (20, 31)])
def test_nv12_center_crop_to_36(cuda, h, w):
    case = ("nv12", 2, h, w, h + w, "bt601", "limited", 36, "center_crop")
    _same(_run(cuda, *case), _want(*case))


def test_nv12_center_crop_to_288(cuda):
    """240 x 426: new_w = 511, so x0 = 111 is odd."""
    planes = _planes("nv12", 1, 240, 426, 426)
    assert video_utils.center_crop_geometry(240, 426, 288)[3] == 111
    got = video_utils.preprocess_yuv_frames(_upload(planes, cuda))  # every default: nv12, auto -> bt601, limited
    _same(got, _want("nv12", 1, 240, 426, 426, "bt601", "limited", 288, "center_crop"))


@pytest.mark.parametrize("h, w, mode", [(37, 53, "resize"), (45, 80, "center_crop")])
@pytest.mark.parametrize("fmt", ["i420", "p010"])
def test_i420_and_p010(cuda, fmt, h, w, mode):
    case = (fmt, 2, h, w, h + 3 * w, "bt601", "limited", 36, mode)
    _same(_run(cuda, *case), _want(*case))
    got = video_utils.preprocess_yuv_frames(_host(_planes(fmt, 2, h, w, h + 3 * w)), pixel_format=fmt, matrix="bt601",
                                            target_size=36, resize_mode=mode)  # NumPy in (np.uint16 for p010)
    _same(got, _want(*case))


@pytest.mark.parametrize("fmt, matrix, rng", [("nv12", "bt601", "limited"), ("nv12", "bt601", "full"),
                                              ("nv12", "bt709", "limited"), ("nv12", "bt709", "full"),
                                              ("p010", "bt709", "limited"), ("p010", "bt709", "full")])
def test_matrix_and_range(cuda, fmt, matrix, rng):
    case = (fmt, 2, 37, 53, 11, matrix, rng, 36, "resize")
    _same(_run(cuda, *case), _want(*case))
    rgb = _rgb(fmt, 2, 37, 53, 11, matrix, rng)
    assert (rgb == 0).any() and (rgb == 255).any()  # both clip branches ran


def test_equals_the_rgb_kernel_on_the_converted_frame(cuda):
    case = ("nv12", 2, 45, 80, 21, "bt709", "full")
    rgb = torch.from_numpy(_rgb(*case).copy()).to(cuda)
    for size, mode in ((36, "center_crop"), (18, "resize")):
        got = _run(cuda, *case, size, mode)
        torch.cuda.synchronize()
        assert torch.equal(got, video_utils.preprocess_frames(rgb, target_size=size, resize_mode=mode))


# pitch (W + 11) samples: (37, 53) -> 64, the interleaved pairs are aligned (one load a pair); (45, 80) -> 91,
# they are not (a load a sample).  yoff: the Y plane starts that many bytes into its rows (odd base).
@pytest.mark.parametrize("fmt, h, w, yoff", [("nv12", 37, 53, 0), ("nv12", 45, 80, 0), ("nv12", 37, 53, 1),
                                             ("nv12", 45, 80, 3), ("i420", 37, 53, 0), ("i420", 45, 80, 1),
                                             ("p010", 37, 53, 0), ("p010", 45, 80, 0)])
def test_decoder_surfaces_read_in_place(cuda, fmt, h, w, yoff):
    """One allocation per clip: Y rows at a pitch of W + 11, 3 unused rows, then the chroma rows; the planes are
    strided views of it.  Whatever fills the rest of the surface, the result is the contiguous planes' result:
    a tap that left its plane would change it."""
    n, size = 2, 36
    planes = _planes(fmt, n, h, w, 31 + h)
    want = _want(fmt, n, h, w, 31 + h, "bt601", "limited", size, "center_crop")
    ch, cw = (h + 1) // 2, (w + 1) // 2
    pitch, rows = w + 11, h + 3 + (2 * ch if fmt == "i420" else ch)
    dtype = torch.int16 if fmt == "p010" else torch.uint8
    host = _upload(planes, "cpu")
    for fill in (0x00, 0xFF):
        surf = torch.full((n, rows, pitch), fill if dtype == torch.uint8 else -(fill & 1), dtype=dtype, device=cuda)
        y = surf[:, :h, yoff:yoff + w]
        if fmt == "i420":
            views = (y, surf[:, h + 3:h + 3 + ch, :cw], surf[:, h + 3 + ch:h + 3 + 2 * ch, :cw])
        else:
            views = (y, surf[:, h + 3:h + 3 + ch, :2 * cw].unflatten(-1, (-1, 2)))
        for view, p in zip(views, host):
            assert view.data_ptr() >= surf.data_ptr() and not view.is_contiguous()
            view.copy_(p.to(cuda))
        if yoff:
            assert y.data_ptr() % 2 == 1
        got = nat.op_preprocess_yuv(views, FMT[fmt], mode=CROP, size=size)  # refuses what it cannot read in place
        _same(got, want)
        _same(video_utils.preprocess_yuv_frames(views, pixel_format=fmt, matrix="bt601", target_size=size), want)


# S = 36 at a 4-byte aligned dst (dword stores) and at an odd one (byte stores); S = 37: frames of
# 4107 bytes, so every other frame is unaligned, and 1369 pixels leave a last group of one
@pytest.mark.parametrize("size, offset", [(36, 64), (36, 61), (37, 64)])
def test_writes_stay_inside_dst(cuda, size, offset):
    case = ("nv12", 3, 25, 33, size + offset, "bt601", "limited", size, "center_crop")
    nbytes = 3 * size * size * 3
    buf = torch.full((offset + nbytes + 67,), 0xA5, dtype=torch.uint8, device=cuda)
    dst = buf[offset:offset + nbytes].view(3, size, size, 3)
    _run(cuda, *case, out=dst)
    _same(dst, _want(*case))
    host = buf.cpu()
    assert bool((host[:offset] == 0xA5).all()) and bool((host[offset + nbytes:] == 0xA5).all())


def test_frame_indices(cuda):
    case = ("nv12", 7, 20, 31, 41, "bt601", "limited", 36, "center_crop")
    ref = _want(*case)
    x = _upload(_planes(*case[:5]), cuda)
    f = functools.partial(video_utils.preprocess_yuv_frames, x, target_size=36)
    _same(f(), ref)
    _same(f(frame_indices=[6, 5, 3, 3, 0, 0]), ref[[6, 5, 3, 3, 0, 0]])  # host: repeats, in reverse
    _same(f(num_frames=3), ref[[0, 3, 6]])
    # device indices are not validated on the host: they are clamped to [0, N-1]
    bad = torch.tensor([9, -2, 3, 7, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=cuda)
    _same(f(frame_indices=bad), ref[[6, 0, 3, 6, 6, 0]])
    _same(nat.op_preprocess_yuv(x, frame_idx=bad, size=36), ref[[6, 0, 3, 6, 6, 0]])
    with pytest.raises(ValueError):
        f(frame_indices=[0, 7])
    with pytest.raises(ValueError, match="Video has only 7 frames, but 8 requested"):
        f(num_frames=8)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_batched_uniform_sample_equals_the_per_video_results(cuda, fmt):
    planes = _planes(fmt, 10, 20, 31, 43)
    ref = _want(fmt, 10, 20, 31, 43, "bt601", "limited", 36, "center_crop").reshape(2, 5, 36, 36, 3)
    batch = _host(planes, lead=(2, 5))
    want = ref[:, np.linspace(0, 4, 3, dtype=int)]
    got = video_utils.preprocess_yuv_frames(batch, pixel_format=fmt, num_frames=3, target_size=36)  # NumPy in
    _same(got, want)
    dev = _upload(batch, cuda)
    _same(video_utils.preprocess_yuv_frames(dev, pixel_format=fmt, num_frames=3, target_size=36), want)
    for b in range(2):
        one = video_utils.preprocess_yuv_frames(tuple(p[b] for p in dev), pixel_format=fmt, num_frames=3,
                                                target_size=36)
        assert torch.equal(one, got[b])
    # a batch whose videos are not evenly spaced in memory is flattened by a copy
    part = tuple(p[:, 1:4] for p in dev)
    _same(video_utils.preprocess_yuv_frames(part, pixel_format=fmt, num_frames=2, target_size=36), ref[:, [1, 3]])


@pytest.mark.parametrize("bf16", [False, True])
def test_apply_on_fused_output_equals_the_rgb_route_bitwise(cuda, bf16):
    cfg = dict(models.CONFIGS["videoprism_v1_base"])
    cfg.update(num_spatial_layers=1, num_temporal_layers=1)
    var = params.synthetic_params(cfg, seed=2)
    m = models.get_model(None, model_fn=lambda: encoders.FactorizedEncoder(**cfg),
                         fprop_dtype=torch.bfloat16 if bf16 else None)
    planes = _planes("nv12", 3, 240, 426, 47)
    fused = video_utils.preprocess_yuv_frames(_host(planes, lead=(1, 3)), num_frames=2)
    assert fused.is_cuda and fused.dtype == torch.uint8 and tuple(fused.shape) == (1, 2, 288, 288, 3)
    rgb = video_utils.preprocess_frames(_rgb("nv12", 3, 240, 426, 47, "bt601", "limited")[None].copy(), num_frames=2)
    assert torch.equal(fused, rgb)
    got, _ = m.apply(var, fused)
    want, _ = m.apply(var, rgb)
    np.testing.assert_array_equal(got.float().cpu().numpy(), want.float().cpu().numpy())
