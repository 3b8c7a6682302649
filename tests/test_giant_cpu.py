"""The Giant encoder's widths (model_dim 1408 = 16 heads x 88) without a GPU: what vp_create accepts and still
refuses, which attention kernel 88-wide heads get, and that the head-width entry points are exported and bound.
The dispatch tables are written out by hand, as in test_attention_dispatch_cpu.py."""

import ctypes
import os

import pytest

from test_attention_dispatch_cpu import CAPS, S_VALUES
from videoprism import _native, models
from videoprism._native import ATT_LONG, ATT_OP, ATT_TEXT, ATT_VIDEO, VP_BF16, VP_F32

NEW_SYMBOLS = ("vp_op_attention_dh", "vp_op_attention_masked_dh", "vp_dev_attention_choice_dh")


def _config(name, fprop_dtype, **kw):
    c = dict(models.CONFIGS[name])
    c.update(kw)
    t, h, w = c["pos_emb_shape"]
    return _native.vp_config(patch_size=c["patch_size"], pos_emb_t=t, pos_emb_h=h, pos_emb_w=w,
                             model_dim=c["model_dim"], num_spatial_layers=c["num_spatial_layers"],
                             num_temporal_layers=c["num_temporal_layers"], num_heads=c["num_heads"],
                             mlp_dim=c["mlp_dim"], atten_logit_cap=c["atten_logit_cap"], fprop_dtype=fprop_dtype)


def _create(cfg):
    lib = _native.load()
    h = ctypes.c_void_p()
    rc = lib.vp_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    msg = lib.vp_last_error().decode()
    if rc == _native.VP_OK:
        lib.vp_destroy(h)
    return rc, msg


def test_giant_bf16_is_refused_by_name():
    rc, msg = _create(_config("videoprism_v1_giant", VP_BF16))
    assert rc == _native.VP_ENOTSUP
    assert "dim_per_head" in msg and "float32" in msg


@pytest.mark.parametrize("fprop_dtype", [VP_F32, VP_BF16])
def test_48_wide_heads_stay_refused(fprop_dtype):
    """test_abi_cpu.py's configuration (768 / 16), in both precisions."""
    rc, msg = _create(_config("videoprism_v1_base", fprop_dtype, num_heads=16))
    assert rc == _native.VP_ENOTSUP
    assert "dim_per_head" in msg


def test_bf16_model_dim_stays_a_multiple_of_256():
    """64-wide heads at model_dim 128 x 11 (22 heads): fp32 takes the width, bf16's 256-wide GEMM tiles do not."""
    rc, msg = _create(_config("videoprism_v1_giant", VP_BF16, num_heads=22))
    assert rc == _native.VP_ENOTSUP
    assert "256" in msg
    rc, _ = _create(_config("videoprism_v1_giant", VP_F32, num_heads=22))
    assert rc != _native.VP_ENOTSUP


def test_giant_f32_gets_past_the_configuration_checks():
    """Not VP_ENOTSUP: with a GPU the handle is created, without one the call stops at the device check."""
    rc, msg = _create(_config("videoprism_v1_giant", VP_F32))
    assert rc != _native.VP_ENOTSUP, msg
    assert rc == _native.VP_OK or (rc == _native.VP_EINVAL and "device" in msg), (rc, msg)
    rc, msg = _create(_config("videoprism_v1_giant", VP_F32, model_dim=1408 + 64, num_heads=16))  # 92-wide
    assert rc == _native.VP_ENOTSUP and "dim_per_head" in msg


ALL_MASKED = ("MASKED",) * 9
# K|V of an 88-wide sequence fill the generic fp32 kernel's LDS at S = 224: without a fast cap there is no MFMA
# kernel to take 224 < S <= 256, so those go to the online-softmax kernel with the longer ones
F32_88_NO_FAST_CAP = ("F32",) * 5 + ("MASKED",) * 4

# fp32, 88-wide heads: (kind, cap) -> the kernel at each of S_VALUES
TABLE_88 = {
    (ATT_VIDEO, 0.0): F32_88_NO_FAST_CAP,
    (ATT_VIDEO, 50.0): ("F32",) * 7 + ("F32_MFMA", "F32_MFMA"),   # the 64-wide row
    (ATT_VIDEO, 50.5): F32_88_NO_FAST_CAP,
    (ATT_LONG, 0.0): ALL_MASKED,
    (ATT_LONG, 50.0): ("F32_MFMA",) * 9,                           # the 64-wide row
    (ATT_LONG, 50.5): ALL_MASKED,
}


def test_table_covers_every_case():
    assert S_VALUES == (1, 16, 17, 127, 128, 255, 256, 257, 4096)
    assert set(TABLE_88) == {(k, c) for k in (ATT_VIDEO, ATT_LONG) for c in CAPS}


@pytest.mark.parametrize("key_pad", [False, True])
@pytest.mark.parametrize("kind,cap", sorted(TABLE_88))
def test_choice_88_f32(kind, cap, key_pad):
    got = tuple(_native.dev_attention_choice(kind, VP_F32, S, cap, key_pad, dim_per_head=88) for S in S_VALUES)
    assert got == TABLE_88[(kind, cap)]
    if cap == 50.0:
        assert got == tuple(_native.dev_attention_choice(kind, VP_F32, S, cap, key_pad) for S in S_VALUES)


def test_choice_88_generic_kernel_boundary():
    """224 is the last sequence length whose K|V (8 S 88 bytes) fit the generic kernel's LDS."""
    for cap, want in ((0.0, ("F32", "MASKED")), (50.5, ("F32", "MASKED")), (50.0, ("F32", "F32"))):
        got = tuple(_native.dev_attention_choice(ATT_VIDEO, VP_F32, S, cap, False, dim_per_head=88) for S in (224, 225))
        assert got == want, cap
    # vp_op_attention's own mapping and the text stack at 88
    assert _native.dev_attention_choice(ATT_OP, VP_F32, 300, 50.0, False, dim_per_head=88) == "F32_MFMA"
    assert _native.dev_attention_choice(ATT_OP, VP_F32, 300, 0.0, True, dim_per_head=88) == "MASKED"
    for S in S_VALUES:
        assert _native.dev_attention_choice(ATT_TEXT, VP_F32, S, 50.0, True, dim_per_head=88) == "MASKED"


@pytest.mark.parametrize("kind", [ATT_OP, ATT_VIDEO, ATT_LONG, ATT_TEXT])
def test_choice_88_bf16_is_the_refusal(kind):
    for cap in CAPS:
        for S in S_VALUES:
            with pytest.raises(NotImplementedError):
                _native.dev_attention_choice(kind, VP_BF16, S, cap, False, dim_per_head=88)


def test_other_widths_are_refused_and_64_is_the_old_entry_point():
    lib = _native.load()
    with pytest.raises(NotImplementedError):
        _native.dev_attention_choice(ATT_VIDEO, VP_F32, 256, 50.0, dim_per_head=48)
    for S in S_VALUES:
        for cap in CAPS:
            k = lib.vp_dev_attention_choice(ATT_VIDEO, VP_F32, S, cap, 0)
            assert _native.dev_attention_choice(ATT_VIDEO, VP_F32, S, cap, dim_per_head=64) == _native.ATTN_KERNELS[k]
    # the op entry points refuse before they look at the (null) buffers' device
    buf = ctypes.c_void_p(16)
    assert lib.vp_op_attention_dh(VP_BF16, buf, buf, 1, 16, 2, 88, 50.0, None, None) == _native.VP_ENOTSUP
    assert "dim_per_head" in lib.vp_last_error().decode()
    assert lib.vp_op_attention_masked_dh(VP_BF16, buf, buf, 1, 16, 2, 88, 50.0, None, 1, None) == _native.VP_ENOTSUP
    assert lib.vp_op_attention_dh(VP_F32, buf, buf, 1, 16, 2, 96, 50.0, None, None) == _native.VP_ENOTSUP


def test_new_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_native.library_path())
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _native.exported_symbols(), s
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                           "videoprism_hip.h")) as f:
        header = f.read()
    assert "vp_op_attention_dh(" in header and "vp_op_attention_masked_dh(" in header


def test_giant_stays_out_of_the_checkpoint_table():
    assert not models.has_model("videoprism_public_v1_giant")
    assert models.videoprism_v1_giant().model_dim == 1408
