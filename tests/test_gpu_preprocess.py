"""Frame preprocessing on the GPU (csrc/preprocess.hip through vp_op_preprocess_frames and
videoprism.video_utils): gather by frame index, cv2.resize's fixed-point bilinear on uint8, centre
crop, optional R<->B swap.  Every comparison is bitwise against the NumPy restatement of that
arithmetic (tests/preprocess_restatement.py); a float bilinear differs from it by a level in about
an eighth of the values, so it is no reference here."""

import sys
import types

import numpy as np
import pytest
import torch

import preprocess_restatement as pr
from videoprism import _native as nat
from videoprism import encoders, models, params, video_utils

pytestmark = pytest.mark.gpu

CROP, STRETCH = nat.VP_RESIZE_CENTER_CROP, nat.VP_RESIZE_STRETCH


def _frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _same(got, want):
    torch.cuda.synchronize()
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want)


# (37, 53): odd sizes, 3*W no multiple of 4; (20, 20): upscale; (72, 72): exact 2x; (36, 36): identity
@pytest.mark.parametrize("h, w", [(37, 53), (20, 20), (72, 72), (36, 36), (19, 61)])
def test_stretch_to_36(cuda, h, w):
    v = _frames(2, h, w, h * 100 + w)
    got = nat.op_preprocess_frames(torch.from_numpy(v).to(cuda), mode=STRETCH, size=36)
    _same(got, pr.preprocess(v, 36, "resize"))
    if (h, w) == (36, 36):
        _same(got, v)


@pytest.mark.parametrize("mode, name", [(STRETCH, "resize"), (CROP, "center_crop")])
def test_54_byte_rows(cuda, mode, name):
    """S = 18: rows of 54 bytes, so a thread's 4 pixels run over a row's end."""
    v = _frames(3, 25, 33, 7)
    got = nat.op_preprocess_frames(torch.from_numpy(v).to(cuda), mode=mode, size=18)
    _same(got, pr.preprocess(v, 18, name))


# landscape; portrait (y0 = 7); truncated new_w = 55
@pytest.mark.parametrize("h, w", [(45, 80), (53, 37), (20, 31)])
def test_center_crop_to_36(cuda, h, w):
    v = _frames(2, h, w, h + w)
    got = nat.op_preprocess_frames(torch.from_numpy(v).to(cuda), mode=CROP, size=36)
    _same(got, pr.preprocess(v, 36, "center_crop"))


@pytest.mark.parametrize("h, w", [(240, 426), (360, 640)])  # new_w = 511 (x0 = 111); 512 (x0 = 112)
def test_center_crop_to_288(cuda, h, w):
    v = _frames(1, h, w, w)
    got = video_utils.preprocess_frames(torch.from_numpy(v).to(cuda))
    _same(got, pr.preprocess(v, 288, "center_crop"))


def test_gather(cuda):
    v = _frames(7, 20, 31, 11)
    ref = pr.preprocess(v, 36)
    x = torch.from_numpy(v).to(cuda)
    idx = torch.tensor([6, 0, 3, 3], dtype=torch.int32, device=cuda)
    _same(nat.op_preprocess_frames(x, idx, size=36), ref[[6, 0, 3, 3]])
    _same(nat.op_preprocess_frames(x, None, size=36), ref)
    # device indices are not validated on the host: the kernel clamps them to [0, N-1]
    bad = torch.tensor([9, -2, 3, 7, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=cuda)
    _same(nat.op_preprocess_frames(x, bad, size=36), ref[[6, 0, 3, 6, 6, 0]])
    _same(video_utils.preprocess_frames(x, target_size=36, frame_indices=[5, 1]), ref[[5, 1]])
    _same(video_utils.preprocess_frames(x, target_size=36, frame_indices=bad), ref[[6, 0, 3, 6, 6, 0]])
    with pytest.raises(ValueError):
        video_utils.preprocess_frames(x, target_size=36, frame_indices=[0, 7])
    with pytest.raises(ValueError, match="Video has only 7 frames, but 8 requested"):
        video_utils.preprocess_frames(x, num_frames=8, target_size=36)


def test_batched_uniform_sample_is_one_gather(cuda):
    v = _frames(10, 20, 31, 12).reshape(2, 5, 20, 31, 3)
    ref = pr.preprocess(v, 36)[:, np.linspace(0, 4, 3, dtype=int)]
    _same(video_utils.preprocess_frames(v, num_frames=3, target_size=36), ref)             # NumPy in
    _same(video_utils.preprocess_frames(torch.from_numpy(v), num_frames=3, target_size=36), ref)  # CPU tensor in
    # a batch whose videos are not evenly spaced in memory is flattened by a copy
    big = torch.from_numpy(_frames(20, 20, 31, 13)).to(cuda).view(2, 10, 20, 31, 3)
    part = big[:, 2:7]
    refp = pr.preprocess(part.cpu().numpy(), 36)[:, np.linspace(0, 4, 3, dtype=int)]
    _same(video_utils.preprocess_frames(part, num_frames=3, target_size=36), refp)


def test_swap_rb(cuda):
    v = _frames(2, 45, 80, 14)
    x = torch.from_numpy(v).to(cuda)
    for mode, name in ((CROP, "center_crop"), (STRETCH, "resize")):
        _same(nat.op_preprocess_frames(x, mode=mode, swap_rb=True, size=36), pr.preprocess(v[..., ::-1], 36, name))
    _same(video_utils.preprocess_frames(x, target_size=36, channel_order="bgr"), pr.preprocess(v[..., ::-1], 36))


def test_views_with_padded_rows_and_unaligned_base(cuda):
    big = torch.from_numpy(_frames(3, 40, 56, 15)).to(cuda)
    view = big[:, 2:-1, 1:-2, :]  # [3, 37, 53, 3]: row stride 168 > 3 * 53, frames padded too
    assert view.data_ptr() % 4 != 0 and not view.is_contiguous()
    want = view.cpu().numpy()
    _same(nat.op_preprocess_frames(view, mode=STRETCH, size=36), pr.preprocess(want, 36, "resize"))
    _same(nat.op_preprocess_frames(view, mode=CROP, size=18), pr.preprocess(want, 18))
    _same(nat.op_preprocess_frames(view[1:2], mode=CROP, size=36), pr.preprocess(want[1:2], 36))


# S = 36 at a 4-byte aligned dst (dword stores) and at an odd one (byte stores); S = 37: frames of
# 4107 bytes, so every other frame is unaligned, and 1369 pixels leave a last group of one
@pytest.mark.parametrize("size, offset", [(36, 64), (36, 61), (37, 64), (18, 2)])
def test_writes_stay_inside_dst(cuda, size, offset):
    v = _frames(3, 25, 33, size + offset)
    nbytes = 3 * size * size * 3
    buf = torch.full((offset + nbytes + 67,), 0xA5, dtype=torch.uint8, device=cuda)
    dst = buf[offset:offset + nbytes].view(3, size, size, 3)
    nat.op_preprocess_frames(torch.from_numpy(v).to(cuda), mode=CROP, size=size, out=dst)
    _same(dst, pr.preprocess(v, size))
    host = buf.cpu()
    assert bool((host[:offset] == 0xA5).all()) and bool((host[offset + nbytes:] == 0xA5).all())


def test_source_ending_at_the_end_of_its_allocation(cuda):
    """The last frame's last row ends where the allocation ends (2 * 32 * 64 * 3 bytes = 24 * 512, a whole
    number of the allocator's blocks): the clamped taps of the last row and column read nothing past it."""
    v = _frames(2, 32, 64, 16)
    x = torch.from_numpy(v).to(cuda)
    assert x.numel() % 512 == 0
    _same(nat.op_preprocess_frames(x, mode=STRETCH, size=36), pr.preprocess(v, 36, "resize"))
    _same(nat.op_preprocess_frames(x, mode=CROP, size=36), pr.preprocess(v, 36))
    tail = x[:, 1:, 2:]  # a view that still ends on the allocation's last byte
    _same(nat.op_preprocess_frames(tail, mode=STRETCH, size=36), pr.preprocess(v[:, 1:, 2:], 36, "resize"))


@pytest.mark.parametrize("bf16", [False, True])
def test_apply_on_preprocessed_frames_bitwise(cuda, bf16):
    """Raw 360 x 640 frames -> preprocess_frames -> model.apply equals, bitwise, the reference's route:
    the restated resize on the host, / 255 in float32, then the float forward."""
    cfg = dict(models.CONFIGS["videoprism_v1_base"])
    cfg.update(num_spatial_layers=1, num_temporal_layers=1)
    var = params.synthetic_params(cfg, seed=2)
    m = models.get_model(None, model_fn=lambda: encoders.FactorizedEncoder(**cfg),
                         fprop_dtype=torch.bfloat16 if bf16 else None)
    src = _frames(3, 360, 640, 17).reshape(1, 3, 360, 640, 3)
    frames = video_utils.preprocess_frames(src, num_frames=2)
    assert frames.is_cuda and frames.dtype == torch.uint8 and tuple(frames.shape) == (1, 2, 288, 288, 3)
    got, _ = m.apply(var, frames)
    ref = pr.preprocess(src[:, [0, 2]], 288).astype(np.float32) / np.float32(255)
    want, _ = m.apply(var, ref)
    np.testing.assert_array_equal(got.float().cpu().numpy(), want)


def _stub_cv2(videos):
    """A stand-in for cv2's decoding surface over in-memory BGR arrays {path: [N, H, W, 3]}."""
    cv2 = types.ModuleType("cv2")
    cv2.CAP_PROP_POS_FRAMES, cv2.CAP_PROP_FRAME_COUNT, cv2.COLOR_BGR2RGB = 1, 7, 4

    class VideoCapture:
        def __init__(self, path):
            self.frames, self.pos = videos.get(path), 0

        def isOpened(self):
            return self.frames is not None

        def get(self, prop):
            assert prop == cv2.CAP_PROP_FRAME_COUNT
            return float(len(self.frames))

        def set(self, prop, value):
            assert prop == cv2.CAP_PROP_POS_FRAMES
            self.pos = int(value)
            return True

        def read(self):
            if not 0 <= self.pos < len(self.frames):
                return False, None
            self.pos += 1
            return True, self.frames[self.pos - 1].copy()

        def release(self):
            pass

    cv2.VideoCapture = VideoCapture
    return cv2


def test_load_video_and_batch_over_a_stub_decoder(cuda, monkeypatch):
    vids = {"a.mp4": _frames(9, 45, 80, 18), "b.mp4": _frames(6, 45, 80, 19)}  # BGR, as cv2 decodes
    monkeypatch.setitem(sys.modules, "cv2", _stub_cv2(vids))

    def want(path, t, size, mode):
        rgb = vids[path][..., ::-1]
        idx = np.linspace(0, len(rgb) - 1, t, dtype=int)
        return pr.preprocess(rgb, size, mode)[idx].astype(np.float32) / 255.0

    a = video_utils.load_video("a.mp4", num_frames=4, target_size=36)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (4, 36, 36, 3)
    np.testing.assert_array_equal(a, want("a.mp4", 4, 36, "center_crop"))
    np.testing.assert_array_equal(video_utils.load_video("a.mp4", 3, 18, "resize"), want("a.mp4", 3, 18, "resize"))
    both = video_utils.load_video_batch(["a.mp4", "b.mp4"], num_frames=4, target_size=36)
    assert both.dtype == np.float32 and both.shape == (2, 4, 36, 36, 3)
    np.testing.assert_array_equal(both, np.stack([want(p, 4, 36, "center_crop") for p in ("a.mp4", "b.mp4")]))
    with pytest.raises(ValueError, match="Could not open video file: c.mp4"):
        video_utils.load_video("c.mp4")
    with pytest.raises(ValueError, match="Video has only 6 frames, but 16 requested"):
        video_utils.load_video("b.mp4")
    with pytest.raises(ValueError, match="Unknown resize_mode: pad"):
        video_utils.load_video("a.mp4", 4, 36, "pad")


def test_against_real_opencv(cuda):
    """Parity with an actual OpenCV build, where one is installed: within one level (builds differ in
    their SIMD paths; the contract is the restatement)."""
    cv2 = pytest.importorskip("cv2")
    v = _frames(2, 45, 80, 20)
    got = nat.op_preprocess_frames(torch.from_numpy(v).to(cuda), mode=STRETCH, size=36).cpu().numpy()
    ref = np.stack([cv2.resize(f, (36, 36)) for f in v])
    assert np.abs(got.astype(np.int32) - ref.astype(np.int32)).max() <= 1
    got = nat.op_preprocess_frames(torch.from_numpy(v).to(cuda), mode=CROP, size=36).cpu().numpy()
    ref = np.stack([cv2.resize(f, (64, 36))[:, 14:50] for f in v])
    assert np.abs(got.astype(np.int32) - ref.astype(np.int32)).max() <= 1
