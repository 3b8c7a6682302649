"""The stream contract (include/videoprism_hip.h, conventions) for the two view entry points of the frame ingest,
vp_op_preprocess_views and vp_op_preprocess_yuv_views (NV12), on the harness of tests/stream_order.py: deferred
inputs, then capture and replay.  The case is the plain calls' of tests/test_gpu_stream_order.py -- 2 source frames of
64 x 48 to S = 36 -- as 2 views of 3 frames each: the whole frame, and a mirrored box at an odd origin.

The frames, the frame indices and the view table are all inputs: X' is another table (the views exchanged) and other
indices, so a table or an index read on the host at capture time would show after the replay.  Poison (every byte
0xFF) is frame index -1 and a table of -1, which the kernel clamps: garbage pixels, no fault.

The file is named to be collected after tests/test_gpu_stream_order.py, whose control test depends on its side stream
being the first of the process (tests/test_gpu_stream_order_retrieval_f8.py says why)."""

import ctypes

import pytest
import torch

import stream_order as so
from videoprism import _native as nat
from videoprism import video_utils

pytestmark = pytest.mark.gpu

p = nat._ptr
N, H, W, S, V, T = 2, 48, 64, 36, 2, 3


@pytest.fixture(scope="module")
def side(cuda):
    return torch.cuda.Stream(cuda)


def _case(yuv, device):
    g = torch.Generator().manual_seed(12)
    byte = lambda *shape: torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(device)  # noqa: E731
    idx = torch.tensor([[1, 0, 1], [0, 0, 1]], dtype=torch.int32, device=device)
    table = torch.from_numpy(video_utils.view_table(H, W, boxes=[(0, 0, H, W), (5, 7, 30, 41)], target_size=S,
                                                    flip=[False, True])).to(device)
    named = dict(idx=so.staged(idx, 1 - idx), views=so.staged(table, table.flip(0)))
    dst = torch.empty((V * T, S, S, 3), dtype=torch.uint8, device=device)
    if yuv:
        named.update(y=so.staged(byte(N, H, W)), uv=so.staged(byte(N, H // 2, W // 2, 2)))
        src, *_ = nat.yuv_frames((named["y"][0], named["uv"][0]), nat.VP_YUV_NV12)

        def call(stream):
            with torch.cuda.device(device):
                nat.call("vp_op_preprocess_yuv_views", ctypes.byref(src), N, H, W, p(named["idx"][0]),
                         p(named["views"][0]), V, T, S, p(dst), so.stream_ptr(stream))
            return (dst,)
    else:
        named.update(frames=so.staged(byte(N, H, W, 3)))

        def call(stream):
            with torch.cuda.device(device):
                nat.call("vp_op_preprocess_views", p(named["frames"][0]), N, H, W, 3 * W, 3 * W * H,
                         p(named["idx"][0]), p(named["views"][0]), V, T, 0, S, p(dst), so.stream_ptr(stream))
            return (dst,)

    label = f"{'vp_op_preprocess_yuv_views NV12' if yuv else 'vp_op_preprocess_views'} 2 x 64x48 -> 2 views x 3 x 36x36"
    return so.case_from(label, named, [dst], lambda: [], call, capture=True)


@pytest.mark.parametrize("yuv", [False, True], ids=["preprocess_views", "preprocess_yuv_views"])
def test_stream_contract(cuda, side, yuv):
    failures = so.check_case(_case(yuv, cuda), side)
    assert not failures, (yuv, failures)
