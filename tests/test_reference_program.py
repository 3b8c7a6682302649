"""The oracle against the reference's own program.

tests/golden/ref_*.npz hold what the reference's Flax code (its layers.py, encoders.py, models.py, unmodified)
computed when it was executed in float64 on the NumPy stand-ins of oracle/refshim (recipe:
oracle/make_ref_fixtures.py).  Here the NumPy oracle (Numerics 'f64'), the torch restatement and the model
registry are held against those records.

Bar: |oracle - ref| <= 1e-10 * max(1, |ref|) elementwise -- the bar between the project's two fp64 restatements.
Both sides are float64 and differ in the order of their sums only; the largest difference measured over all cases
is 8.7e-14 (DESIGN.md §2 lists every case), so no case needs more.

Pinned by this: the reference's graph, order of operations, masks, layouts, parameter paths and builder settings.
Not pinned: XLA's arithmetic, bf16 dtype flow (the stand-ins have no bfloat16), the MLX path, a real checkpoint.
"""

import json
import os
import sys

import einops
import numpy as np
import pytest
import scipy.special

from oracle import videoprism_oracle as orc
from oracle import refshim
from videoprism import encoders, models, params
import primer_restatement as primer
from ref_fixtures import BAR, GOLD, MEASURED, Case, fixture  # noqa: F401
import torch_restatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("VIDEOPRISM_REFERENCE", "/root/reference")
NM = orc.Numerics("f64")


def _ln(x, p):
    return orc.layer_norm(x, p["scale"], p["bias"], NM)


def _act(name):
    return orc.gelu if name == "gelu" else orc.relu


# ---------------------------------------------------------------------------------------------------------
# layer level
# ---------------------------------------------------------------------------------------------------------
def test_layer_norm_both_scales():
    c = Case("ref_layers", "ln_plus1")
    c.check("out", _ln(c.inp["x"], c.tree))
    c = Case("ref_layers", "ln_direct")
    p = c.tree                                   # direct_scale: the leaf is the factor itself, not factor - 1
    c.check("out", orc.layer_norm(c.inp["x"], p["scale"].astype(np.float64) - 1.0, p["bias"], NM))


def test_feed_forward():
    for name, act in (("ff_gelu", orc.gelu), ("ff_relu", orc.relu)):
        c = Case("ref_layers", name)
        p = c.tree["linear"]
        c.check("out", act(orc.dense(c.inp["x"].astype(np.float64), p["kernel"], p["bias"], NM)))


def _tff(x, p, pad, policy, act):
    """layers.py:372-430 from the oracle's LayerNorm and Dense, every norm_policy."""
    keep = 1.0 - pad[..., None]
    y = x
    if policy == "primer_hybrid":
        y = _ln(x, p["pre_layer_norm"])
    elif policy == "pre":
        y = _ln(x, p["layer_norm"])
    a = act(orc.dense(y, p["ffn_layer1"]["linear"]["kernel"], p["ffn_layer1"]["linear"]["bias"], NM)) * keep
    o = orc.dense(a, p["ffn_layer2"]["linear"]["kernel"], p["ffn_layer2"]["linear"]["bias"], NM) * keep
    if policy == "primer_hybrid":
        o = _ln(o, p["post_layer_norm"])
    elif policy == "post":
        o = _ln(o, p["layer_norm"])
    o = x + o
    return _ln(o, p["layer_norm"]) if policy == "post_skip" else o


@pytest.mark.parametrize("policy", ["pre", "primer_hybrid", "post", "post_skip"])
@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_transformer_feed_forward(policy, act):
    c = Case("ref_layers", f"tff_{policy}_{act}")
    x, pad = c.inp["x"].astype(np.float64), c.inp["paddings"].astype(np.float64)
    assert pad.any()
    c.check("out", _tff(x, c.tree, pad, policy, _act(act)))
    if policy in primer.POLICIES:                # the restatement the text-tower tests use
        c.check("out", primer.ffn_sublayer(x, c.tree, pad, NM, policy, _act(act)))


def test_attention_projection_layouts():
    c = Case("ref_layers", "proj_q")
    c.check("out", orc.attention_projection_in(c.inp["x"].astype(np.float64), c.tree["w"], c.tree["b"], NM))
    c = Case("ref_layers", "proj_post")
    assert c.tree["w"].shape == (16, 2, 6)       # 'post' keeps [D, N, H]
    c.check("out", orc.attention_projection_out(c.inp["x"].astype(np.float64), c.tree["w"], c.tree["b"], NM))


def test_per_dim_scale():
    c = Case("ref_layers", "per_dim_scale")
    x = c.inp["x"].astype(np.float64)
    c.check("out", x * (1.442695041 / np.sqrt(x.shape[-1])) * orc.softplus(c.tree["per_dim_scale"].astype(np.float64)))


@pytest.mark.parametrize("name", ["masks_pad", "masks_causal_pad", "masks_allpad"])
def test_attention_masks(name):
    """The mask's constant is -0.7 * finfo(dtype).max, so its value follows the float type: the float64 record
    pins which entries are masked, the float32 one ('native' stand-ins) the value the oracle uses."""
    c = Case("ref_layers", name)
    got = orc.attention_masks_for_fprop(c.inp["paddings"].astype(np.float64), c.cfg["causal"])
    wide, native = c.out["out"], c.out["out_native"]
    assert got.shape == wide.shape == native.shape
    assert native.dtype == np.float32
    np.testing.assert_array_equal(got >= 0.5 * got.min(), wide >= 0.5 * wide.min())
    assert np.all(np.abs(got - native.astype(np.float64)) <= 2.0 ** -24 * np.abs(got))
    assert (got < 0).any() and (got == 0).any()


@pytest.mark.parametrize("name", ["dpa_cap50_pad", "dpa_cap0_causal_pad", "dpa_cap50_allpad"])
def test_dot_product_attention(name):
    c = Case("ref_layers", name)
    m = Case("ref_layers", c.cfg["mask"])
    mask = orc.attention_masks_for_fprop(m.inp["paddings"].astype(np.float64), m.cfg["causal"])
    x, p = c.inp["x"].astype(np.float64), c.tree
    q, k, v = (orc.attention_projection_in(x, p[n]["w"], p[n]["b"], NM) for n in ("query", "key", "value"))
    dh = q.shape[-1]
    if c.cfg["per_dim_scale"]:
        q = q * (1.442695041 / np.sqrt(dh)) * orc.softplus(p["per_dim_scale"]["per_dim_scale"].astype(np.float64))
        enc = orc._dot_atten_rows(q, k, v, mask, NM, c.cfg["cap"])
    else:
        enc = orc.dot_atten(q, k, v, mask, NM, c.cfg["cap"], dh)
    c.check("out/0", orc.attention_projection_out(enc, p["post"]["w"], p["post"]["b"], NM))
    probs = c.out["out/1"]                        # [B, N, T, S]
    np.testing.assert_allclose(probs.sum(-1), 1.0, rtol=0, atol=1e-14)
    pad = m.inp["paddings"]
    if name == "dpa_cap50_allpad":               # every key padded: all logits equal, uniform weights
        np.testing.assert_array_equal(probs[1], 1.0 / probs.shape[-1])
        assert np.all(probs[0][..., pad[0] > 0] == 0.0)
    if m.cfg["causal"]:                          # a padded query's row is masked everywhere: uniform as well
        assert np.all(np.triu(probs[0], 1) == 0.0)
        np.testing.assert_array_equal(probs[1][:, pad[1] > 0], 1.0 / probs.shape[-1])


def test_transformer_layer():
    c = Case("ref_layers", "transformer_pre_gelu")
    m = Case("ref_layers", c.cfg["mask"])
    x, pad = c.inp["x"].astype(np.float64), c.inp["paddings"].astype(np.float64)
    mask = orc.attention_masks_for_fprop(m.inp["paddings"].astype(np.float64), m.cfg["causal"])
    c.check("out", orc.transformer_layer_act(x, c.tree, pad, mask, NM, 2, 50.0, orc.gelu))
    c.check("out", primer.transformer_layer(x, c.tree, pad, mask, NM, 2, 50.0, "pre", orc.gelu))
    c = Case("ref_layers", "transformer_primer_relu")
    m = Case("ref_layers", c.cfg["mask"])
    mask = orc.attention_masks_for_fprop(m.inp["paddings"].astype(np.float64), m.cfg["causal"])
    c.check("out", primer.transformer_layer(x, c.tree, pad, mask, NM, 2, 50.0, "primer_hybrid", orc.relu))


def test_atten_token_pooling_with_paddings():
    c = Case("ref_layers", "pooler_pad")
    x, pad = c.inp["x"].astype(np.float64), c.inp["paddings"].astype(np.float64)
    c.check("out", orc.atten_token_pooling(x, c.tree, NM, 2, 32, paddings=pad))
    n = Case("ref_layers", "pooler_nopad")
    n.check("out", orc.atten_token_pooling(x, n.tree, NM, 2, 32))
    assert np.abs(orc.atten_token_pooling(x, c.tree, NM, 2, 32) - c.out["out"]).max() > 1e-3   # the paddings count


def test_l2_normalize_and_patches():
    c = Case("ref_layers", "l2_normalize")
    c.check("out", orc.l2_normalize(c.inp["x"]))
    c = Case("ref_layers", "image_to_patch")
    np.testing.assert_array_equal(orc.image_to_patch(c.inp["x"].astype(np.float64), 4), c.out["out"])


def test_positional_interpolation():
    for name in ("interp_1d_up", "interp_1d_down"):
        c = Case("ref_layers", name)
        c.check("out", orc.interpolate_emb_1d(c.inp["emb"].astype(np.float64), c.cfg["target"]))
    for name in ("interp_2d_down", "interp_2d_up"):
        c = Case("ref_layers", name)
        c.check("out", orc.interpolate_emb_2d(c.inp["emb"].astype(np.float64), tuple(c.cfg["source"]),
                                              tuple(c.cfg["target"])))


def test_positional_embeddings():
    for name in ("sinusoid_even", "sinusoid_odd"):
        c = Case("ref_layers", name)
        c.check("out", orc.sinusoidal_positions(c.cfg["seq_length"], c.cfg["dim"])[None])
    c = Case("ref_layers", "trainable_pos_full")
    np.testing.assert_array_equal(c.out["out"], c.tree["emb_var"][None].astype(np.float64))
    c = Case("ref_layers", "trainable_pos_short")
    np.testing.assert_array_equal(c.out["out"], c.tree["emb_var"][None, :4].astype(np.float64))
    # past max_seq_length the reference slices its table out of range, which lax refuses: it has no such path
    c = Case("ref_layers", "trainable_pos_past_max")
    assert str(c.out["out/raised"]) != "" and "out" not in c.out


# ---------------------------------------------------------------------------------------------------------
# the reference's own tiny models
# ---------------------------------------------------------------------------------------------------------
def test_tiny_encoder_scan_unrolled_paddings():
    c = Case("ref_models_tiny", "enc_tiny")
    np.testing.assert_array_equal(c.out["out_scan/0"], c.out["out_unrolled/0"])
    np.testing.assert_array_equal(c.out["out_scan/1/spatial_features"], c.out["out_unrolled/1/spatial_features"])
    emb, out = orc.factorized_encoder(c.tree, c.video, c.cfg, "f64", return_intermediate=True)
    c.check("out_scan/0", emb)
    c.check("out_scan/1/spatial_features", out["spatial_features"])
    fp = c.inp["frame_paddings"]
    emb_p, out_p = orc.factorized_encoder(c.tree, c.video, c.cfg, "f64", frame_paddings=fp, return_intermediate=True)
    c.check("out_padded/0", emb_p)
    c.check("out_padded/1/spatial_features", out_p["spatial_features"])
    t_emb, t_sp = torch_restatement.factorized_encoder(c.tree, c.video, c.cfg, fp)
    np.testing.assert_allclose(t_emb, c.out["out_padded/0"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(t_sp, c.out["out_padded/1/spatial_features"], rtol=0, atol=1e-10)
    # the program in its own float32 ('native' stand-ins): no parity bar, only that it runs and lands near fp64
    native = c.out["out_padded_native/0"]
    assert native.dtype == np.float32 and np.abs(native - c.out["out_padded/0"]).max() < 1e-4


@pytest.mark.parametrize("T", [2, 4, 6])
def test_tiny_encoder_clip_lengths(T):
    """T below, at and above the temporal table's 4 rows (encoders.py:551-552)."""
    c = Case("ref_models_tiny", "enc_t")
    x = c.inp[f"inputs_t{T}"]
    emb, _ = orc.factorized_encoder(c.tree, x, c.cfg, "f64")
    c.check(f"out_t{T}/0", emb)
    t_emb, _ = torch_restatement.factorized_encoder(c.tree, x, c.cfg)
    np.testing.assert_allclose(t_emb, c.out[f"out_t{T}/0"], rtol=0, atol=1e-10)


def test_tiny_video_clip():
    c = Case("ref_models_tiny", "clip_tiny")
    ids, tp, fp = c.inp["text_token_ids"], c.inp["text_paddings"], c.inp["frame_paddings"]
    v, t, out = orc.video_clip(c.tree, c.cfg, c.video, ids, tp, "f64", return_intermediate=True)
    c.check("out_norm/0", v)
    c.check("out_norm/1", t)
    for k in ("frame_embeddings", "spatial_features", "spatiotemporal_features"):
        c.check(f"out_norm/2/{k}", out[k])
    v, t, out = orc.video_clip(c.tree, c.cfg, c.video, ids, tp, "f64", normalize=False,
                               return_intermediate=("frame_embeddings",))
    c.check("out_raw/0", v)
    c.check("out_raw/1", t)
    c.check("out_raw/2/frame_embeddings", out["frame_embeddings"])
    assert set(k for k in c.out if k.startswith("out_raw/2/")) == {"out_raw/2/frame_embeddings"}
    v, t, out = orc.video_clip(c.tree, c.cfg, c.video, ids, tp, "f64", return_intermediate=("frame_embeddings",),
                               frame_paddings=fp)
    c.check("out_padded/0", v)
    c.check("out_padded/2/frame_embeddings", out["frame_embeddings"])
    tv, tt, tf = torch_restatement.video_clip(c.tree, c.cfg, c.video, ids, tp, fp)
    np.testing.assert_allclose(tv, c.out["out_padded/0"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(tt, c.out["out_padded/1"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(tf, c.out["out_padded/2/frame_embeddings"], rtol=0, atol=1e-10)


def test_tiny_text_encoder_primer_hybrid():
    c = Case("ref_models_tiny", "text_primer")
    cfg = dict(model_dim=c.cfg["model_dim"], num_unimodal_layers=c.cfg["num_layers"], num_heads=c.cfg["num_heads"],
               atten_logit_cap=c.cfg["atten_logit_cap"], enable_causal_atten=c.cfg["enable_causal_atten"])
    ids, tp = c.inp["text_token_ids"], c.inp["text_paddings"]
    c.check("out", primer.text_encoder(c.tree, ids, tp, cfg, NM, "primer_hybrid"))
    t = primer.torch_text_encoder(c.tree, ids, tp, cfg, "primer_hybrid").numpy()
    np.testing.assert_allclose(t, c.out["out"], rtol=0, atol=1e-10)


def test_tiny_classifier():
    c = Case("ref_models_tiny", "classifier_tiny")
    cfg = {k: v for k, v in c.cfg.items() if k != "num_classes"}
    logits, out = orc.video_classifier(c.tree, cfg, c.video, return_intermediate=True)
    c.check("out/0", logits)
    for k in ("spatial_features", "spatiotemporal_features", "global_embeddings"):
        c.check(f"out/1/{k}", out[k])
    logits, _ = orc.video_classifier(c.tree, cfg, c.video, frame_paddings=c.inp["frame_paddings"])
    c.check("out_padded/0", logits)
    np.testing.assert_allclose(torch_restatement.video_classifier(c.tree, cfg, c.video), c.out["out/0"],
                               rtol=0, atol=1e-10)


# ---------------------------------------------------------------------------------------------------------
# the shapes the HIP path runs (the GPU tests read the same files)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("file,name", [("ref_base_encoder", "base_encoder"), ("ref_giant_encoder", "giant_encoder")])
def test_wide_encoder(file, name):
    c = Case(file, name)
    tree, fp = c.seeded_variables()["params"], c.inp["frame_paddings"]
    emb, out = orc.factorized_encoder(tree, c.video, c.cfg, "f64", frame_paddings=fp, return_intermediate=True)
    c.check("out_padded/0", emb)
    c.check("out_padded/1/spatial_features", out["spatial_features"])
    emb, _ = orc.factorized_encoder(tree, c.video, c.cfg, "f64")
    c.check("out/0", emb)
    if name == "base_encoder":
        t_emb, _ = torch_restatement.factorized_encoder(tree, c.video, c.cfg, fp)
        stride = 2
        np.testing.assert_allclose(t_emb[:, ::stride], c.out[f"out_padded/0@rows{stride}"], rtol=0, atol=1e-10)


def test_wide_lvt():
    c = Case("ref_base_lvt", "base_lvt")
    tree = c.seeded_variables(params.clip_leaf_specs(c.cfg))["params"]
    ids, tp = c.inp["text_token_ids"], c.inp["text_paddings"]
    assert sorted((tp == 0).sum(-1)) == [3, 7, 12]
    v, t, out = orc.video_clip(tree, c.cfg, c.video, ids, tp, "f64", return_intermediate=("frame_embeddings",),
                               frame_paddings=c.inp["frame_paddings"])
    c.check("out_padded/0", v)
    c.check("out_padded/1", t)
    c.check("out_padded/2/frame_embeddings", out["frame_embeddings"])
    v, _, _ = orc.video_clip(tree, c.cfg, c.video, None, None, "f64")
    c.check("out/0", v)


def test_wide_classifier():
    c = Case("ref_base_classifier", "base_classifier")
    cfg = {k: v for k, v in c.cfg.items() if k != "num_classes"}
    tree = c.seeded_variables(params.classifier_leaf_specs(cfg, c.cfg["num_classes"]))["params"]
    logits, out = orc.video_classifier(tree, cfg, c.video, return_intermediate=("global_embeddings",),
                                       frame_paddings=c.inp["frame_paddings"])
    c.check("out_padded/0", logits)
    c.check("out_padded/1/global_embeddings", out["global_embeddings"])
    logits, _ = orc.video_classifier(tree, cfg, c.video)
    c.check("out/0", logits)


# ---------------------------------------------------------------------------------------------------------
# sensitivity: the records could not be met by a program that ignores what they are meant to pin
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("file,name,padded,plain", [
    ("ref_models_tiny", "enc_tiny", "out_padded/0", "out_scan/0"),
    ("ref_models_tiny", "clip_tiny", "out_padded/0", "out_norm/0"),
    ("ref_models_tiny", "classifier_tiny", "out_padded/0", "out/0"),
    ("ref_base_encoder", "base_encoder", "out_padded/0@rowsums", "out/0@rowsums"),
    ("ref_giant_encoder", "giant_encoder", "out_padded/0@rowsums", "out/0@rowsums"),
    ("ref_base_lvt", "base_lvt", "out_padded/0", "out/0"),
    ("ref_base_classifier", "base_classifier", "out_padded/0", "out/0")])
def test_paddings_change_the_recorded_outputs(file, name, padded, plain):
    c = Case(file, name)
    assert np.abs(c.out[padded] - c.out[plain]).max() > 1e-3


def _perturbed(tree, path, delta=1e-2):
    """One element of the leaf moved by delta.  (Moving a whole bias by one constant would prove nothing where a
    LayerNorm follows: its mean subtraction removes a uniform shift.)"""
    flat = {k: np.array(v, np.float64) for k, v in params.flatten(tree).items()}
    assert path in flat, path
    flat[path].reshape(-1)[0] += delta
    return params.unflatten(flat)


@pytest.mark.parametrize("path", ["vision_encoder/spatial_ln/scale",
                                  "vision_encoder/spatial_encoder/transformers_stack/x_layers/layer_norm/scale",
                                  "contrastive_vision_pooler/pooling_attention/per_dim_scale/per_dim_scale",
                                  "contrastive_vision_pooler/pooling_attention/post/b",
                                  "text_encoder/unimodal_ln/scale",
                                  "text_encoder/unimodal_transformer/x_layers/ff_layer/ffn_layer2/linear/bias"])
def test_clip_outputs_depend_on_scales_and_biases(path):
    c = Case("ref_models_tiny", "clip_tiny")
    ids, tp = c.inp["text_token_ids"], c.inp["text_paddings"]
    v0, t0, _ = orc.video_clip(c.tree, c.cfg, c.video, ids, tp, "f64", normalize=False)
    v1, t1, _ = orc.video_clip(_perturbed(c.tree, path), c.cfg, c.video, ids, tp, "f64", normalize=False)
    moved = np.abs((t1 - t0) if path.startswith("text_encoder") else (v1 - v0)).max()
    assert moved > 1e-6, (path, moved)


@pytest.mark.parametrize("path", ["encoder/temporal_ln/scale",
                                  "atten_pooler/pooling_attention/per_dim_scale/per_dim_scale",
                                  "encoder/patch_projection/linear/bias", "projection/linear/bias"])
def test_classifier_outputs_depend_on_scales_and_biases(path):
    c = Case("ref_models_tiny", "classifier_tiny")
    cfg = {k: v for k, v in c.cfg.items() if k != "num_classes"}
    l0, _ = orc.video_classifier(c.tree, cfg, c.video)
    l1, _ = orc.video_classifier(_perturbed(c.tree, path), cfg, c.video)
    assert np.abs(l1 - l0).max() > 1e-6, path


# ---------------------------------------------------------------------------------------------------------
# builder settings
# ---------------------------------------------------------------------------------------------------------
def _settings(z, key):
    return json.loads(str(z[f"settings/{key}/settings"]))


def _plain(v):
    return list(v) if isinstance(v, tuple) else v


def test_configs_match_the_reference_field_by_field():
    z = fixture("ref_settings")
    ref = _settings(z, "constant/CONFIGS")
    assert sorted(ref) == sorted(models.CONFIGS)
    for name, cfg in models.CONFIGS.items():
        assert {k: _plain(v) for k, v in cfg.items()} == ref[name], name
    assert models.K400_NUM_CLASSES == _settings(z, "constant/K400_NUM_CLASSES")
    assert models.SSV2_NUM_CLASSES == _settings(z, "constant/SSV2_NUM_CLASSES")
    assert models.TEXT_MAX_LEN == _settings(z, "constant/TEXT_MAX_LEN")
    assert models.TEXT_TOKENIZERS == _settings(z, "constant/TEXT_TOKENIZERS")
    assert {k: list(v) for k, v in models.CHECKPOINTS.items()} == _settings(z, "constant/CHECKPOINTS")


def _module_settings(m):
    out = {}
    for k, v in vars(m).items():
        if k in ("dtype", "fprop_dtype") or k.startswith("_"):
            continue
        if isinstance(v, dict):
            out.update({f"{k}.{kk}": _plain(vv) for kk, vv in v.items()})
        else:
            out[k] = _plain(v)
    return out


def test_builders_match_the_reference_field_by_field():
    z = fixture("ref_settings")
    args = json.loads(str(z["settings/builder_args"]))
    assert len(args) == 9
    for name, a in args.items():
        ours = getattr(models, name)(*a)
        ref = _settings(z, f"builder/{name}")
        assert type(ours) is getattr(encoders, {"v1": "FactorizedEncoder", "lvt": "FactorizedVideoCLIP",
                                                "vc": "FactorizedVideoClassifier"}[name.split("_")[1]])
        assert _module_settings(ours) == ref, name
    assert "vocabulary_size" not in models.CONFIGS["videoprism_lvt_v1_base"]   # our builders copy, never write back


# ---------------------------------------------------------------------------------------------------------
# live: the committed records are what the reference's program gives today
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, "videoprism", "layers.py")),
                    reason="no reference checkout on this machine")
def test_fixtures_are_what_the_reference_program_computes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    try:
        import make_ref_fixtures
    finally:
        sys.path.pop(0)
    written = make_ref_fixtures.generate(REFERENCE, str(tmp_path))
    committed = sorted(f[:-4] for f in os.listdir(GOLD) if f.startswith("ref_") and f.endswith(".npz"))
    assert sorted(written) == committed
    for name in committed:
        old = fixture(name)
        with np.load(os.path.join(str(tmp_path), name + ".npz"), allow_pickle=False) as new:
            assert sorted(new.files) == sorted(old)
            for k in new.files:
                if old[k].dtype.kind in "fiub":
                    assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
                    np.testing.assert_allclose(new[k].astype(np.float64), old[k].astype(np.float64), rtol=0,
                                               atol=1e-12, err_msg=k)
                else:
                    np.testing.assert_array_equal(new[k], old[k], err_msg=k)


# ---------------------------------------------------------------------------------------------------------
# the stand-ins themselves (no reference, no oracle)
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def shim():
    mods = refshim.install("wide")
    try:
        yield mods
    finally:
        refshim.uninstall()


def test_shim_is_not_importable_by_accident():
    """Outside `install` no import finds the stand-ins: nothing in the repository answers to their names."""
    import importlib.util
    for name in ("jax", "flax", "einshape"):
        assert not getattr(sys.modules.get(name), "__refshim__", False), name
        spec = importlib.util.find_spec(name)
        assert spec is None or not str(spec.origin).startswith(ROOT), (name, spec.origin)


@pytest.mark.parametrize("eq,pattern,sizes,shape", [
    ("(bt)nd->(bn)td", "(b t) n d -> (b n) t d", dict(t=3), (6, 4, 5)),
    ("(bt)n->(bn)t", "(b t) n -> (b n) t", dict(t=3), (6, 4)),
    ("(bn)td->b(tn)d", "(b n) t d -> b (t n) d", dict(b=2), (8, 3, 5)),
    ("(bt)nd->b(tn)d", "(b t) n d -> b (t n) d", dict(t=3), (6, 4, 5)),
    ("b(tn)d->(bt)nd", "b (t n) d -> (b t) n d", dict(t=3), (2, 12, 5)),
    ("(bt)d->btd", "(b t) d -> b t d", dict(t=3), (6, 5))])
def test_shim_einshape_against_einops(shim, eq, pattern, sizes, shape):
    x = np.arange(np.prod(shape), dtype=np.float64).reshape(shape)
    got = shim["einshape"].jax_einshape(eq, x, **sizes)
    np.testing.assert_array_equal(np.asarray(got), einops.rearrange(x, pattern, **sizes))


def test_shim_resize_hand_checked(shim):
    resize = shim["jax.image"].resize
    for n_in, n_out in ((8, 16), (16, 4), (5, 7), (7, 3), (16, 3)):
        np.testing.assert_allclose(np.asarray(resize(np.full((n_in, 2), 3.25), (n_out, 2), "bilinear")), 3.25,
                                   rtol=0, atol=1e-15)
    # 2x up-sampling of the ramp 0..7: output o sits at (o + 0.5) / 2 - 0.5, clamped to the ends
    up = np.asarray(resize(np.arange(8.0)[:, None], (16, 1), "bilinear"))[:, 0]
    np.testing.assert_allclose(up, [0.0, 0.25, 0.75, 1.25, 1.75, 2.25, 2.75, 3.25, 3.75, 4.25, 4.75, 5.25, 5.75, 6.25,
                                    6.75, 7.0], rtol=0, atol=1e-15)
    # 4x antialiased down-sampling of the ramp 0..15: centres 1.5, 5.5, 9.5, 13.5, triangle of radius 4.  An interior
    # output weighs taps c-3.5 .. c+3.5 by (1, 3, 5, 7, 7, 5, 3, 1) / 32: symmetric, so it returns c.  The first
    # output loses the taps at -2 and -1; the rest, (5, 7, 7, 5, 3, 1) / 28 on 0..5, give 53 / 28.
    down = np.asarray(resize(np.arange(16.0)[:, None], (4, 1), "bilinear"))[:, 0]
    np.testing.assert_allclose(down, [53.0 / 28.0, 5.5, 9.5, 15.0 - 53.0 / 28.0], rtol=0, atol=1e-14)
    from oracle.refshim import jaxlike
    w = jaxlike.resize_weights(16, 4)
    np.testing.assert_allclose(w[1], np.array([0, 0, 1, 3, 5, 7, 7, 5, 3, 1, 0, 0, 0, 0, 0, 0]) / 32.0, atol=1e-15)
    np.testing.assert_allclose(w[0], np.array([5, 7, 7, 5, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]) / 28.0, atol=1e-15)
    # two dimensions resize one after the other
    img = np.add.outer(np.arange(16.0), 10.0 * np.arange(16.0))[..., None]
    got = np.asarray(resize(img, (4, 4, 1), "bilinear"))[..., 0]
    np.testing.assert_allclose(got, np.add.outer(down, 10.0 * down), rtol=0, atol=1e-12)


def test_shim_activations_against_scipy(shim):
    nn = shim["jax.nn"]
    x = np.linspace(-9.0, 9.0, 181)
    np.testing.assert_allclose(np.asarray(nn.gelu(x, approximate=False)), x * scipy.special.ndtr(x), rtol=1e-13,
                               atol=1e-15)
    np.testing.assert_allclose(np.asarray(nn.softplus(x)), -scipy.special.log_expit(-x), rtol=1e-14, atol=0)
    m = np.random.default_rng(0).normal(0, 4, (3, 5, 7))
    np.testing.assert_allclose(np.asarray(nn.softmax(m, axis=-1)), scipy.special.softmax(m, axis=-1), rtol=1e-14)
    np.testing.assert_array_equal(np.asarray(nn.one_hot(np.array([[0, 2]]), 3)), [[[1, 0, 0], [0, 0, 1]]])
    np.testing.assert_array_equal(np.asarray(nn.relu(np.array([-1.0, 0.0, 2.0]))), [0.0, 0.0, 2.0])


def test_shim_arrays_are_immutable_like_jax(shim):
    jnp = shim["jax.numpy"]
    base = np.ones((2, 3))
    a = jnp.asarray(base)
    view = a[:, None]
    view *= 5.0                                   # rebinding, as on a jax array: neither `a` nor `base` changes
    np.testing.assert_array_equal(np.asarray(a), 1.0)
    np.testing.assert_array_equal(base, 1.0)
    np.testing.assert_array_equal(np.asarray(view), 5.0)
    assert jnp.mean(a, axis=[-1], keepdims=True).shape == (2, 1)
    assert a.astype(jnp.float32).dtype == np.float64 and jnp.zeros([2], dtype=jnp.bfloat16).dtype == np.float64
    with pytest.raises(TypeError):
        shim["jax.lax"].slice_in_dim(a, 0, 3, axis=0)


def test_shim_pytrees(shim):
    """Dict keys in sorted order, None an empty subtree, flatten / unflatten inverse of each other."""
    tree = {"b": [1, (2, None)], "a": {"z": 3, "y": None}}
    leaves, treedef = shim["jax.tree"].flatten(tree)
    assert leaves == [3, 1, 2]
    assert treedef.unflatten(leaves) == {"a": {"y": None, "z": 3}, "b": [1, (2, None)]}
    assert shim["jax.tree_util"].tree_map(lambda v: v * 10, tree) == {"a": {"y": None, "z": 30}, "b": [10, (20, None)]}


def _cell(nn, jnp):
    class Cell(nn.Module):
        width: int = 3

        @nn.compact
        def __call__(self, x):
            w = self.param("w", nn.initializers.lecun_normal(), [self.width, self.width], jnp.float32)
            return jnp.tanh(x @ w + self.param("b", nn.initializers.zeros_init(), [self.width], jnp.float32))

    class Stack(nn.Module):
        scan: bool = True

        @nn.compact
        def __call__(self, x):
            if self.scan:
                cell = Cell(name="cells")
                y, _ = nn.scan(lambda m, c: (m(c), None), variable_axes={"params": 0},
                               split_rngs={"params": True}, length=4)(cell, x)
                return y
            for i in range(4):
                x = Cell(name=f"cells_{i}")(x)
            return x
    return Stack


def test_shim_scan_equals_unrolled_and_numpy(shim):
    nn, jnp = shim["flax.linen"], shim["jax.numpy"]
    Stack = _cell(nn, jnp)
    rng = np.random.default_rng(1)
    w, b, x = rng.normal(size=(4, 3, 3)), rng.normal(size=(4, 3)), rng.normal(size=(2, 3))
    scanned = Stack(scan=True).apply({"params": {"cells": {"w": w, "b": b}}}, jnp.asarray(x))
    unrolled = Stack(scan=False).apply({"params": {f"cells_{i}": {"w": w[i], "b": b[i]} for i in range(4)}},
                                       jnp.asarray(x))
    want = x
    for i in range(4):
        want = np.tanh(want @ w[i] + b[i])
    np.testing.assert_array_equal(np.asarray(scanned), want)
    np.testing.assert_array_equal(np.asarray(unrolled), want)


def test_shim_apply_raises_on_unread_missing_and_misshapen_leaves(shim):
    nn, jnp = shim["flax.linen"], shim["jax.numpy"]
    Stack = _cell(nn, jnp)
    x = jnp.asarray(np.zeros((2, 3)))
    good = {f"cells_{i}": {"w": np.ones((3, 3)), "b": np.ones(3)} for i in range(4)}
    Stack(scan=False).apply({"params": good}, x)
    with pytest.raises(ValueError, match="never read"):
        Stack(scan=False).apply({"params": dict(good, extra={"w": np.ones(1)})}, x)
    with pytest.raises(KeyError, match="cells_3/b"):
        Stack(scan=False).apply({"params": dict(good, cells_3={"w": np.ones((3, 3))})}, x)
    with pytest.raises(ValueError, match="shape"):
        Stack(scan=False).apply({"params": dict(good, cells_0={"w": np.ones((3, 4)), "b": np.ones(3)})}, x)
    with pytest.raises(RuntimeError, match="apply-only"):
        Stack().param("w", None, [1])


def test_report_measured_differences():
    """Prints the largest oracle-minus-reference-program difference of every case checked above (pytest -s)."""
    for k in sorted(MEASURED):
        print(f"{k}: {MEASURED[k]:.2e}")
    assert all(v <= 1e-9 for v in MEASURED.values())
