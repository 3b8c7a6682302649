"""videoprism_lvt_v1_giant and videoprism_vc_v1_giant without a GPU: the 'primer_hybrid' restatements the GPU tests
compare against (tests/primer_restatement.py) checked against the oracle and against each other, the leaf names of
a primer text stack, and what vp_clip_create accepts and refuses at Giant's widths."""

import ctypes

import numpy as np
import pytest

import primer_restatement as pr
from oracle import videoprism_oracle as orc
from videoprism import _native, encoders, models, params
from videoprism._native import VP_BF16, VP_F32

# D = 32, 2 heads, 2 layers, L = 6 with a padded tail (and one row with no padding)
TINY = dict(model_dim=32, num_heads=2, num_unimodal_layers=2, atten_logit_cap=50.0, enable_causal_atten=True,
            vocabulary_size=50)
NEW_SYMBOLS = ("vp_dev_pool_logits_wide", "vp_dev_pool_softmax_wsum_wide", "vp_dev_ln_l2_rows_wide",
               "vp_dev_layernorm_residual")


def _text_tree(cfg, policy, seed):
    """The 'text_encoder' subtree of a clip tree with this text norm policy (synthetic: non-zero scales and biases)."""
    full = dict(cfg, patch_size=2, pos_emb_shape=(1, 1, 1), num_spatial_layers=0, num_temporal_layers=0, mlp_dim=64,
                num_auxiliary_layers=0, norm_policy=policy)
    specs = {k: v for k, v in params.clip_leaf_specs(full).items() if k.startswith("text_encoder/")}
    return params.synthetic_params(full, seed, specs=specs)["params"]["text_encoder"]


def _tiny_text():
    ids = np.random.default_rng(2).integers(0, TINY["vocabulary_size"], (3, 6)).astype(np.int32)
    pads = np.zeros((3, 6), np.float32)
    pads[0, 4:] = 1.0
    pads[2, 1:] = 1.0
    return ids, pads


def test_pre_restatement_is_the_oracle():
    """With policy 'pre' the NumPy restatement repeats orc.text_encoder operation for operation: equal bits, in the
    fp64 and the fp32 graph."""
    tree = _text_tree(TINY, "pre", 5)
    ids, pads = _tiny_text()
    for mode in ("f64", "f32"):
        nm = orc.Numerics(mode)
        got = pr.text_encoder(tree, ids, pads, TINY, nm, "pre")
        np.testing.assert_array_equal(got, orc.text_encoder(tree, ids, pads, TINY, nm))


@pytest.mark.parametrize("policy", pr.POLICIES)
def test_numpy_and_torch_restatements_agree(policy):
    tree = _text_tree(TINY, policy, 6)
    ids, pads = _tiny_text()
    a = pr.text_encoder(tree, ids, pads, TINY, orc.Numerics("f64"), policy)
    b = pr.torch_text_encoder(tree, ids, pads, TINY, policy).numpy()
    assert a.shape == b.shape == (3, 7, 32)
    err = np.abs(a - b).max()
    print(f"{policy}: NumPy vs torch max-abs {err:.3e} (|ref| max {np.abs(a).max():.2f})")
    assert err <= 1e-12


def test_primer_differs_from_pre_and_a_padded_row_gets_beta():
    """The FFN sublayer of a padded row is x + beta_post (LayerNorm of the zeroed row), not x as with 'pre'."""
    tree = _text_tree(TINY, "primer_hybrid", 7)
    nm = orc.Numerics("f64")
    x = np.random.default_rng(3).standard_normal((2, 7, 32))
    pad = np.zeros((2, 7))
    pad[0, 3:6] = 1.0
    ff = orc._layer_slice(tree["unimodal_transformer"]["x_layers"], 1)["ff_layer"]
    out = pr.ffn_sublayer(x, ff, pad, nm, "primer_hybrid")
    beta = np.asarray(ff["post_layer_norm"]["bias"], np.float64)
    assert np.abs(beta).max() > 1e-3
    np.testing.assert_allclose(out[0, 3:6], x[0, 3:6] + beta, rtol=0, atol=1e-15)
    assert np.abs(out[0, :3] - (x[0, :3] + beta)).max() > 1e-2
    # 'pre' on the same kind of input: the padded rows come back as they went in
    pre = _text_tree(TINY, "pre", 7)
    ffp = orc._layer_slice(pre["unimodal_transformer"]["x_layers"], 1)["ff_layer"]
    np.testing.assert_array_equal(pr.ffn_sublayer(x, ffp, pad, nm, "pre")[0, 3:6], x[0, 3:6])


def test_giant_lvt_leaf_specs():
    m = models.videoprism_lvt_v1_giant()
    assert (m.model_dim, m.num_heads, m.num_unimodal_layers, m.norm_policy) == (1408, 16, 16, "primer_hybrid")
    specs = m.param_specs()
    pre = "text_encoder/unimodal_transformer/x_layers/"
    text = {k[len(pre):]: v for k, v in specs.items() if k.startswith(pre)}
    assert len(text) == 20
    assert not any("layer_norm" in k and "pre_layer_norm" not in k and "post_layer_norm" not in k for k in text)
    for ln in ("pre_layer_norm", "post_layer_norm", "ff_layer/pre_layer_norm", "ff_layer/post_layer_norm"):
        for leaf in ("scale", "bias"):
            assert text[f"{ln}/{leaf}"] == (16, 1408), ln
    assert text["self_attention/query/w"] == (16, 1408, 16, 88)
    assert text["ff_layer/ffn_layer1/linear/kernel"] == (16, 1408, 4 * 1408)
    # the vision and auxiliary stacks stay 'pre' (encoders.py:832, :853)
    for stack in ("vision_encoder/spatial_encoder/transformers_stack", "auxiliary_encoder/transformers_stack"):
        assert f"{stack}/x_layers/layer_norm/scale" in specs
        assert f"{stack}/x_layers/pre_layer_norm/scale" not in specs
    assert specs["contrastive_vision_pooler/pooling_attention/key/w"] == (1408, 16, 352)
    assert len(specs) == 92
    vc = models.videoprism_vc_v1_giant(40).param_specs()
    assert len(vc) == 54 and vc["atten_pooler/pooling_attention/key/w"] == (1408, 16, 88)


@pytest.mark.parametrize("name", ["videoprism_lvt_v1_base", "videoprism_lvt_v1_large"])
def test_base_and_large_specs_are_unchanged(name):
    cfg = dict(models.CONFIGS[name], vocabulary_size=32000)
    specs = params.clip_leaf_specs(cfg)
    assert len(specs) == 88
    no_policy = {k: v for k, v in cfg.items() if k != "norm_policy"}
    assert params.clip_leaf_specs(no_policy) == specs
    pre = "text_encoder/unimodal_transformer/x_layers/"
    assert sorted(k[len(pre):] for k in specs if k.startswith(pre)) == sorted(n for n, _ in params._LAYER_LEAVES)


def _clip_config(name, fprop_dtype, norm_policy=None, **kw):
    c = dict(models.CONFIGS[name])
    c.update(kw)
    t, h, w = c["pos_emb_shape"]
    video = _native.vp_config(patch_size=c["patch_size"], pos_emb_t=t, pos_emb_h=h, pos_emb_w=w,
                              model_dim=c["model_dim"], num_spatial_layers=c["num_spatial_layers"],
                              num_temporal_layers=c["num_temporal_layers"], num_heads=c["num_heads"],
                              mlp_dim=c["mlp_dim"], atten_logit_cap=c["atten_logit_cap"], fprop_dtype=fprop_dtype)
    extra = {} if norm_policy is None else {"norm_policy": norm_policy}
    return _native.vp_clip_config(video=video, num_auxiliary_layers=c["num_auxiliary_layers"], vocabulary_size=1000,
                                  num_unimodal_layers=c["num_unimodal_layers"], enable_causal_atten=1, **extra)


def _create(cfg):
    lib = _native.load()
    h = ctypes.c_void_p()
    rc = lib.vp_clip_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    msg = lib.vp_last_error().decode()
    if rc == _native.VP_OK:
        lib.vp_clip_destroy(h)
    return rc, msg


def test_config_struct_defaults_to_pre():
    assert _clip_config("videoprism_lvt_v1_base", VP_F32).norm_policy == 0
    assert _native.NORM_POLICIES == {"pre": 0, "primer_hybrid": 1}
    assert ctypes.sizeof(_native.vp_clip_config) == ctypes.sizeof(_native.vp_config) + 5 * 4


def test_giant_clip_bf16_is_refused_by_name():
    rc, msg = _create(_clip_config("videoprism_lvt_v1_giant", VP_BF16, norm_policy=1))
    assert rc == _native.VP_ENOTSUP
    assert "dim_per_head" in msg


@pytest.mark.parametrize("policy", [2, -1, 7])
def test_unknown_norm_policy_is_refused(policy):
    for name in ("videoprism_lvt_v1_giant", "videoprism_lvt_v1_base"):
        rc, msg = _create(_clip_config(name, VP_F32, norm_policy=policy))
        assert rc == _native.VP_ENOTSUP, (rc, msg)
        assert "norm_policy" in msg


def test_giant_clip_f32_gets_past_the_configuration_checks():
    """Not VP_ENOTSUP: with a GPU the handle is created, without one the call stops at the device check."""
    for policy in (0, 1):
        rc, msg = _create(_clip_config("videoprism_lvt_v1_giant", VP_F32, norm_policy=policy))
        assert rc == _native.VP_OK or (rc == _native.VP_EINVAL and "device" in msg), (rc, msg)


@pytest.mark.parametrize("policy", ["post", "post_skip", "primer"])
def test_other_policies_stay_not_implemented(policy):
    cfg = dict(models.CONFIGS["videoprism_lvt_v1_base"], vocabulary_size=10, norm_policy=policy)
    with pytest.raises(NotImplementedError, match="norm_policy"):
        encoders.FactorizedVideoCLIP(**cfg).engine({"params": {}}, 0)


def test_primer_outside_the_text_tower_stays_not_implemented():
    enc = dict(models.CONFIGS["videoprism_v1_base"], norm_policy="primer_hybrid")
    with pytest.raises(NotImplementedError, match="norm_policy"):
        encoders.FactorizedEncoder(**enc).engine({"params": {}}, 0)
    with pytest.raises(NotImplementedError, match="norm_policy"):
        encoders.FactorizedVideoClassifier(encoder_params=enc, num_classes=3).engine({"params": {}}, 0)


def test_new_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_native.library_path())
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _native.exported_symbols(), s
    assert lib.vp_abi_version() == 8


def test_wide_entry_points_refuse_before_they_touch_a_buffer():
    """The limits of the *_wide entry points and of the old names, checked on the host (the buffers are never read)."""
    lib = _native.load()
    buf = ctypes.c_void_p(256)
    args = lambda D: (buf, VP_F32, 8, 4, D, buf, None, 2, buf, None)  # noqa: E731
    assert lib.vp_dev_pool_logits(*args(1088)) == _native.VP_EINVAL
    assert "at most 1024" in lib.vp_last_error().decode()
    assert lib.vp_dev_pool_logits_wide(*args(1600)) == _native.VP_EINVAL
    assert "at most 1536" in lib.vp_last_error().decode()
    assert lib.vp_dev_pool_logits_wide(*args(1408 + 32)) == _native.VP_EINVAL
    wargs = lambda D: (buf, VP_F32, 2, 4, D, 2, buf, buf, buf, buf, None)  # noqa: E731
    assert lib.vp_dev_pool_softmax_wsum(*wargs(1408)) == _native.VP_EINVAL
    assert "multiple of 256, at most 1024" in lib.vp_last_error().decode()
    assert lib.vp_dev_pool_softmax_wsum_wide(*wargs(1408 + 64)) == _native.VP_EINVAL
    assert "multiple of 128, at most 1536" in lib.vp_last_error().decode()
    assert lib.vp_dev_pool_softmax_wsum_wide(*wargs(1664)) == _native.VP_EINVAL
    largs = lambda D: (buf, VP_F32, D, 2, D, None, None, 1, buf, None)  # noqa: E731
    assert lib.vp_dev_ln_l2_rows(*largs(1025)) == _native.VP_EINVAL
    assert "1 <= D <= 1024" in lib.vp_last_error().decode()
    assert lib.vp_dev_ln_l2_rows_wide(*largs(1537)) == _native.VP_EINVAL
    assert "1 <= D <= 1536" in lib.vp_last_error().decode()
    assert lib.vp_dev_layernorm_residual(buf, VP_F32, 4, 1408 + 64, buf, buf, None, buf, None) == _native.VP_ENOTSUP
    assert "128" in lib.vp_last_error().decode()
