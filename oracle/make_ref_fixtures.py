"""Records what the reference's own Flax program computes, as fixtures tests/golden/ref_*.npz.

    python oracle/make_ref_fixtures.py [REFERENCE_ROOT] [--out DIR]

REFERENCE_ROOT defaults to $VIDEOPRISM_REFERENCE, then /root/reference.  The reference's layers.py, encoders.py
and models.py are executed unmodified, in a child process (oracle/refshim/child.py), on the NumPy stand-ins for
jax / flax.linen / einshape of oracle/refshim in their 'wide' mode: every float of the program is float64.  Inputs
and parameters are drawn here, from seeded NumPy generators and params.synthetic_params; the fixtures hold those
inputs, the parameters (or their seed and checksums), the configuration and the program's outputs -- data only.

Fixture layout, per case:  <case>/in/<name>, <case>/param/<leaf path> (or <case>/param_seed, param_names,
param_sums, param_heads), <case>/cfg (JSON), <case>/<call id>[/<index or key>] for the outputs.  Token-level
outputs of the wide models are stored as every k-th token row (<key>@rows<k>) plus the sum of every row
(<key>@rowsums) and the mean over the tokens (<key>@tokenmean), which keeps each file below the largest fixture
already committed.
"""

import argparse
import concurrent.futures
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "videoprism-mlx_amd")]

from videoprism import models, params  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CHILD = os.path.join(HERE, "refshim", "child.py")

# encoders_test.py:130,145-156 and :290-324 -- the reference's own tiny models
TINY = dict(patch_size=4, pos_emb_shape=(16, 16, 16), model_dim=8, num_spatial_layers=2, num_temporal_layers=2,
            num_heads=2, mlp_dim=4, atten_logit_cap=50.0)
CLIP_TINY = dict(patch_size=4, pos_emb_shape=(16, 16, 16), num_spatial_layers=2, num_temporal_layers=2, mlp_dim=4,
                 num_auxiliary_layers=1, vocabulary_size=20, enable_causal_atten=True, num_unimodal_layers=2,
                 norm_policy="pre", model_dim=8, num_heads=2, atten_logit_cap=50.0)
TEXT_PRIMER = dict(vocabulary_size=20, num_class_tokens=1, model_dim=8, num_layers=2, mlp_dim=32, num_heads=2,
                   atten_logit_cap=50.0, norm_policy="primer_hybrid", enable_causal_atten=True)

FILES = {
    "ref_layers": None,          # filled by layer_cases()
    "ref_models_tiny": None,
    "ref_base_encoder": ["base_encoder"],
    "ref_base_lvt": ["base_lvt"],
    "ref_base_classifier": ["base_classifier"],
    "ref_giant_encoder": ["giant_encoder"],
    "ref_settings": ["settings"],
}


def enc(v):
    """Python value -> the JSON forms oracle/refshim/child.py resolves."""
    if isinstance(v, tuple):
        return {"$tuple": [enc(x) for x in v]}
    if isinstance(v, (set, frozenset)):
        return {"$set": sorted(enc(x) for x in v)}
    if isinstance(v, dict):
        return {k: enc(x) for k, x in v.items()}
    if isinstance(v, list):
        return [enc(x) for x in v]
    return v


class Job:
    def __init__(self):
        self.arrays, self.calls, self.cfg, self.transient, self.subsample = {}, [], {}, set(), {}

    def arr(self, case, name, a):
        self.arrays[f"{case}/in/{name}"] = np.asarray(a)
        return {"$a": f"{case}/in/{name}"}

    def params(self, case, flat, tag="param", keep=True):
        """Leaves of one case; every one must be spread out (a constant leaf pins nothing about how it is used)."""
        for k, v in flat.items():
            v = np.asarray(v)
            assert v.size == 1 or float(np.std(v)) > 0.0, f"{case}: leaf {k} has no spread"
            assert float(np.abs(v).max()) > 0.0, f"{case}: leaf {k} is zero"
            self.arrays[f"{case}/{tag}/{k}"] = v
            if not keep:
                self.transient.add(f"{case}/{tag}/{k}")
        return f"{case}/{tag}/"

    def seeded_params(self, case, flat, seed):
        """Parameters too large to store: passed to the child, recorded as seed + checksums (as g2_base_dims)."""
        prefix = self.params(case, flat, keep=False)
        names = sorted(flat)
        self.arrays[f"{case}/param_seed"] = np.array(seed)
        self.arrays[f"{case}/param_names"] = np.array(names)
        self.arrays[f"{case}/param_sums"] = np.array([float(np.sum(flat[k], dtype=np.float64)) for k in names])
        self.arrays[f"{case}/param_heads"] = np.stack([np.asarray(flat[k]).ravel()[:4] for k in names])
        return prefix

    def apply(self, call_id, cls, ctor, prefix, *args, **kwargs):
        self.calls.append(dict(id=call_id, kind="apply", cls=cls, ctor=enc(ctor), params=prefix, args=enc(list(args)),
                               kwargs=enc(kwargs)))
        return {"$ref": call_id}

    def fn(self, call_id, fn, *args, expect_error=False, **kwargs):
        self.calls.append(dict(id=call_id, kind="fn", fn=fn, args=enc(list(args)), kwargs=enc(kwargs),
                               expect_error=expect_error))
        return {"$ref": call_id}


def _n(rng, shape, std=1.0, mean=0.0):
    return (rng.standard_normal(shape) * std + mean).astype(np.float32)


GELU, RELU = {"$attr": "layers.gelu"}, {"$attr": "layers.nn.relu"}
D, N, H, F = 16, 2, 8, 24


def layer_leaves(rng, policy):
    """One Transformer layer's leaves (params._LAYER_LEAVES / the primer_hybrid set) at D 16, N 2, H 8, F 24."""
    dims = {"D": D, "N": N, "H": H, "F": F}
    names = params._primer_leaves() if policy == "primer_hybrid" else params._LAYER_LEAVES
    return {k: _n(rng, tuple(dims[s] for s in shp), 0.3) for k, shp in names}


def layer_cases(job):
    rng = np.random.default_rng(2025)
    cases = []

    def case(name, cfg=None):
        cases.append(name)
        job.cfg[name] = cfg or {}
        return name

    x = _n(rng, (2, 5, D), 3.0, 1.0)
    pad = np.zeros((2, 5), np.float32)
    pad[1, 3:] = 1.0
    allpad = np.zeros((2, 5), np.float32)
    allpad[0, 4] = 1.0
    allpad[1, :] = 1.0

    for name, direct in (("ln_plus1", False), ("ln_direct", True)):
        c = case(name, dict(direct_scale=direct))
        p = job.params(c, {"scale": _n(rng, D, 0.3, 1.0 if direct else 0.0), "bias": _n(rng, D, 0.3)})
        job.apply(f"{c}/out", "layers.LayerNorm", dict(direct_scale=direct), p, job.arr(c, "x", x))

    for name, act in (("ff_gelu", GELU), ("ff_relu", None)):
        c = case(name)
        p = job.params(c, {"linear/kernel": _n(rng, (D, F), 0.25), "linear/bias": _n(rng, F, 0.3)})
        ctor = dict(output_dim=F, **({"activation_fn": act} if act else {}))
        job.apply(f"{c}/out", "layers.FeedForward", ctor, p, job.arr(c, "x", x))

    for policy in ("pre", "primer_hybrid", "post", "post_skip"):
        for aname, act in (("gelu", GELU), ("relu", RELU)):
            c = case(f"tff_{policy}_{aname}", dict(norm_policy=policy, activation=aname))
            lns = ("pre_layer_norm", "post_layer_norm") if policy == "primer_hybrid" else ("layer_norm",)
            flat = {"ffn_layer1/linear/kernel": _n(rng, (D, F), 0.25), "ffn_layer1/linear/bias": _n(rng, F, 0.3),
                    "ffn_layer2/linear/kernel": _n(rng, (F, D), 0.2), "ffn_layer2/linear/bias": _n(rng, D, 0.3)}
            for ln in lns:
                flat[f"{ln}/scale"], flat[f"{ln}/bias"] = _n(rng, D, 0.3), _n(rng, D, 0.3)
            p = job.params(c, flat)
            job.apply(f"{c}/out", "layers.TransformerFeedForward",
                      dict(hidden_dim=F, activation_fn=act, norm_policy=policy), p,
                      job.arr(c, "x", x), job.arr(c, "paddings", pad), False)

    # w is [D, N, H] in both directions; H = 6 so that N*H != D and a swapped layout cannot pass
    c = case("proj_q")
    p = job.params(c, {"w": _n(rng, (D, N, 6), 0.25), "b": _n(rng, (N, 6), 0.3)})
    job.apply(f"{c}/out", "layers.AttentionProjection", dict(num_heads=N, dim_per_head=6), p, job.arr(c, "x", x))
    c = case("proj_post")
    p = job.params(c, {"w": _n(rng, (D, N, 6), 0.25), "b": _n(rng, D, 0.3)})
    job.apply(f"{c}/out", "layers.AttentionProjection",
              dict(output_dim=D, num_heads=N, dim_per_head=6, is_output_projection=True), p,
              job.arr(c, "x", _n(rng, (2, 5, N, 6))))

    c = case("per_dim_scale")
    p = job.params(c, {"per_dim_scale": _n(rng, H, 0.5)})
    job.apply(f"{c}/out", "layers.PerDimScale", {}, p, job.arr(c, "x", _n(rng, (2, 5, N, H))))

    masks = {}
    for name, pd, causal in (("masks_pad", pad, False), ("masks_causal_pad", pad, True),
                             ("masks_allpad", allpad, False)):
        c = case(name, dict(causal=causal))
        masks[name] = job.fn(f"{c}/out", "layers.compute_attention_masks_for_fprop", job.arr(c, "x", x),
                             job.arr(c, "paddings", pd), causal_attention=causal)

    for name, cap, pds, mask in (("dpa_cap50_pad", 50.0, False, "masks_pad"),
                                 ("dpa_cap0_causal_pad", 0.0, True, "masks_causal_pad"),
                                 ("dpa_cap50_allpad", 50.0, False, "masks_allpad")):
        c = case(name, dict(cap=cap, per_dim_scale=pds, mask=mask))
        flat = {f"{q}/w": _n(rng, (D, N, H), 0.25) for q in ("query", "key", "value", "post")}
        flat.update({f"{q}/b": _n(rng, (N, H), 0.3) for q in ("query", "key", "value")})
        flat["post/b"] = _n(rng, D, 0.3)
        if pds:
            flat["per_dim_scale/per_dim_scale"] = _n(rng, H, 0.5)
        p = job.params(c, flat)
        xa = job.arr(c, "x", x)
        job.apply(f"{c}/out", "layers.DotProductAttention",
                  dict(hidden_dim=D, num_heads=N, atten_logit_cap=cap, internal_enable_per_dim_scale=pds), p,
                  xa, xa, xa, atten_mask=masks[mask], train=False)

    for name, policy, aname, act, mask in (("transformer_pre_gelu", "pre", "gelu", GELU, "masks_pad"),
                                           ("transformer_primer_relu", "primer_hybrid", "relu", RELU,
                                            "masks_causal_pad")):
        c = case(name, dict(norm_policy=policy, activation=aname, mask=mask))
        p = job.params(c, layer_leaves(rng, policy))
        job.apply(f"{c}/out", "layers.Transformer",
                  dict(hidden_dim=F, num_heads=N, norm_policy=policy, activation_fn=act,
                       internal_enable_per_dim_scale=False, atten_logit_cap=50.0), p,
                  job.arr(c, "x", x), job.arr(c, "paddings", pad), masks[mask], False)

    for name, pd in (("pooler_pad", pad), ("pooler_nopad", None)):
        c = case(name, dict(hidden_dim=32, num_heads=N))
        flat = {"pooling_attention_query": _n(rng, (1, D), 1.0),
                "pooling_attention/per_dim_scale/per_dim_scale": _n(rng, 16, 0.5),
                "pooling_attention/post/w": _n(rng, (D, N, 16), 0.2), "pooling_attention/post/b": _n(rng, D, 0.3),
                "pooling_attention_layer_norm/scale": _n(rng, D, 0.3),
                "pooling_attention_layer_norm/bias": _n(rng, D, 0.3)}
        for q in ("query", "key", "value"):
            flat[f"pooling_attention/{q}/w"] = _n(rng, (D, N, 16), 0.25)
            flat[f"pooling_attention/{q}/b"] = _n(rng, (N, 16), 0.3)
        p = job.params(c, flat)
        job.apply(f"{c}/out", "layers.AttenTokenPoolingLayer", dict(hidden_dim=32, num_heads=N), p,
                  job.arr(c, "x", x), None if pd is None else job.arr(c, "paddings", pd), False)

    c = case("l2_normalize")
    job.fn(f"{c}/out", "encoders._l2_normalize", job.arr(c, "x", x))
    c = case("image_to_patch", dict(patch_size=4))
    job.fn(f"{c}/out", "encoders._image_to_patch", job.arr(c, "x", _n(rng, (2, 8, 12, 3))), 4)

    c = case("interp_1d_up", dict(target=16))
    job.fn(f"{c}/out", "encoders._interpolate_emb_1d", job.arr(c, "emb", _n(rng, (1, 8, 5))), 16)
    c = case("interp_1d_down", dict(target=4))
    job.fn(f"{c}/out", "encoders._interpolate_emb_1d", job.arr(c, "emb", _n(rng, (1, 16, 5))), 4)
    c = case("interp_2d_down", dict(source=[16, 16], target=[4, 4]))
    job.fn(f"{c}/out", "encoders._interpolate_emb_2d", job.arr(c, "emb", _n(rng, (1, 256, 3))), (16, 16), (4, 4))
    c = case("interp_2d_up", dict(source=[4, 4], target=[6, 8]))
    job.fn(f"{c}/out", "encoders._interpolate_emb_2d", job.arr(c, "emb", _n(rng, (1, 16, 3))), (4, 4), (6, 8))

    for name, dim in (("sinusoid_even", 16), ("sinusoid_odd", 7)):
        c = case(name, dict(dim=dim, seq_length=10))
        job.apply(f"{c}/out", "encoders.PositionalEmbedding", dict(embedding_dim=dim), None, seq_length=10)

    # the trainable table at, below and past max_seq_length: the last is a lax slice out of range, which the
    # reference's program does not survive -- recorded as such
    table = _n(rng, (6, 8), 0.35)
    for name, length, err in (("trainable_pos_full", 6, False), ("trainable_pos_short", 4, False),
                              ("trainable_pos_past_max", 9, True)):
        c = case(name, dict(max_seq_length=6, seq_length=length))
        p = job.params(c, {"emb_var": table})
        job.calls.append(dict(id=f"{c}/out", kind="apply", cls="encoders.TrainablePositionalEmbedding",
                              ctor=dict(embedding_dim=8, max_seq_length=6), params=p, args=[],
                              kwargs=dict(seq_length=length), expect_error=err))
    return cases


def unroll(flat):
    """Scanned leaves (.../x_layers/<leaf>, leading L) -> the scan=False tree's .../x_layers_<i>/<leaf>."""
    out = {}
    for k, v in flat.items():
        if "/x_layers/" in k:
            for i in range(v.shape[0]):
                out[k.replace("/x_layers/", f"/x_layers_{i}/")] = v[i]
        else:
            out[k] = v
    return out


def tiny_model_cases(job):
    cases = []

    def case(name, cfg):
        cases.append(name)
        job.cfg[name] = cfg
        return name

    tup = lambda cfg: {k: (tuple(v) if k == "pos_emb_shape" else v) for k, v in cfg.items()}  # noqa: E731
    rng = np.random.default_rng(77)
    video = _n(rng, (2, 4, 16, 16, 3), 0.1)
    fp = np.zeros((2, 4), np.float32)
    fp[0, 2:] = 1.0        # encoders_test.py:138-142
    fp[1, 1] = 1.0

    c = case("enc_tiny", dict(TINY))
    flat = params.flatten(params.synthetic_params(TINY, 101)["params"])
    p = job.params(c, flat)
    pu = job.params(c, unroll(flat), tag="param_unrolled", keep=False)
    x, fpa = job.arr(c, "inputs", video), job.arr(c, "frame_paddings", fp)
    job.apply(f"{c}/out_scan", "encoders.FactorizedEncoder", dict(tup(TINY), scan=True), p, x, return_intermediate=True)
    job.apply(f"{c}/out_unrolled", "encoders.FactorizedEncoder", dict(tup(TINY), scan=False), pu, x,
              return_intermediate=True)
    job.apply(f"{c}/out_padded", "encoders.FactorizedEncoder", dict(tup(TINY), scan=True), p, x,
              return_intermediate=True, frame_paddings=fpa)

    # T below, at and above the temporal table (4 rows); the spatial table (4 x 4) fits the 4 x 4 grid as it is
    cfg_t = dict(TINY, pos_emb_shape=(4, 4, 4))
    c = case("enc_t", cfg_t)
    p = job.params(c, params.flatten(params.synthetic_params(cfg_t, 102)["params"]))
    for T in (2, 4, 6):
        job.apply(f"{c}/out_t{T}", "encoders.FactorizedEncoder", dict(tup(cfg_t), scan=True), p,
                  job.arr(c, f"inputs_t{T}", _n(rng, (1, T, 16, 16, 3), 0.1)))

    c = case("clip_tiny", dict(CLIP_TINY))
    flat = params.flatten(params.synthetic_params(CLIP_TINY, 103, specs=params.clip_leaf_specs(CLIP_TINY))["params"])
    p = job.params(c, flat)
    ids = rng.integers(0, 20, (2, 10)).astype(np.int32)
    tp = np.zeros((2, 10), np.float32)
    tp[0, 5:] = 1.0        # encoders_test.py:304-305
    tp[1, 8:] = 1.0
    x, fpa = job.arr(c, "inputs", video), job.arr(c, "frame_paddings", fp)
    ia, ta = job.arr(c, "text_token_ids", ids), job.arr(c, "text_paddings", tp)
    ctor = dict(tup(CLIP_TINY), scan=True)
    job.apply(f"{c}/out_norm", "encoders.FactorizedVideoCLIP", ctor, p, x, ia, ta, return_intermediate=True)
    job.apply(f"{c}/out_raw", "encoders.FactorizedVideoCLIP", ctor, p, x, ia, ta, normalize=False,
              return_intermediate=("frame_embeddings",))
    job.apply(f"{c}/out_padded", "encoders.FactorizedVideoCLIP", ctor, p, x, ia, ta,
              return_intermediate=("frame_embeddings",), frame_paddings=fpa)

    c = case("text_primer", dict(TEXT_PRIMER))
    specs = {"token_emb/emb_var": (20, 8), "cls_emb": (1, 1, 8), "unimodal_ln/scale": (8,), "unimodal_ln/bias": (8,)}
    specs.update(params._stack_specs("unimodal_transformer", 2, {"D": 8, "N": 2, "H": 4, "F": 32}, True,
                                     "primer_hybrid"))
    p = job.params(c, params.flatten(params.synthetic_params(dict(model_dim=8), 104, specs=specs)["params"]))
    job.apply(f"{c}/out", "encoders.TextEncoder", dict(TEXT_PRIMER, scan=True), p,
              job.arr(c, "text_token_ids", ids), job.arr(c, "text_paddings", tp))

    enc_params = dict(TINY, scan=True)
    c = case("classifier_tiny", dict(TINY, num_classes=10))
    flat = params.flatten(params.synthetic_params(TINY, 105, specs=params.classifier_leaf_specs(TINY, 10))["params"])
    p = job.params(c, flat)
    x, fpa = job.arr(c, "inputs", video), job.arr(c, "frame_paddings", fp)
    ctor = dict(encoder_params=tup(enc_params), num_classes=10)
    job.apply(f"{c}/out", "encoders.FactorizedVideoClassifier", ctor, p, x, return_intermediate=True)
    job.apply(f"{c}/out_padded", "encoders.FactorizedVideoClassifier", ctor, p, x, frame_paddings=fpa)
    return cases


def frames_u8(seed, B=2, T=3, size=72):
    """Frames held as bytes (a quarter of the fp32 size); the models see u8 / 255 in float32 (video_utils.py:94)."""
    return np.random.default_rng(seed).integers(0, 256, (B, T, size, size, 3), dtype=np.uint8)


def as_float(u8):
    return u8.astype(np.float32) / np.float32(255.0)


def wide_model_cases(job, which):
    """One of the four cases at shapes the HIP path accepts: real widths, 1 + 1 layers, B = 2, T = 3, 72 x 72 (a
    4 x 4 grid: the spatial table shrinks 16 x 16 -> 4 x 4, the temporal one 16 or 8 -> 3), frame 2 of clip 1
    padded."""
    fp = np.zeros((2, 3), np.float32)
    fp[1, 2] = 1.0
    tup = lambda cfg: {k: (tuple(v) if k == "pos_emb_shape" else v) for k, v in cfg.items()}  # noqa: E731

    for c, base, seed, strides in (("base_encoder", "videoprism_v1_base", 301, (2, 4, 8)),
                                   ("giant_encoder", "videoprism_v1_giant", 304, (3, 8, 16))):
        if c != which:
            continue
        cfg = dict(models.CONFIGS[base], num_spatial_layers=1, num_temporal_layers=1)
        job.cfg[c] = cfg
        u8 = frames_u8(seed)
        job.arrays[f"{c}/in/inputs_u8"] = u8
        job.arrays[f"{c}/in/inputs"] = as_float(u8)
        job.transient.add(f"{c}/in/inputs")
        p = job.seeded_params(c, params.flatten(params.synthetic_params(cfg, seed)["params"]), seed)
        x, fpa = {"$a": f"{c}/in/inputs"}, job.arr(c, "frame_paddings", fp)
        job.apply(f"{c}/out_padded", "encoders.FactorizedEncoder", tup(cfg), p, x, return_intermediate=True,
                  frame_paddings=fpa)
        job.apply(f"{c}/out", "encoders.FactorizedEncoder", tup(cfg), p, x)
        job.subsample.update({f"{c}/out_padded/0": strides[0], f"{c}/out/0": strides[1],
                              f"{c}/out_padded/1/spatial_features": strides[2]})

    if which == "base_lvt":
        _wide_lvt(job, fp, tup)
    if which == "base_classifier":
        _wide_classifier(job, fp, tup)


def _wide_lvt(job, fp, tup):
    c = "base_lvt"
    cfg = dict(models.CONFIGS["videoprism_lvt_v1_base"], vocabulary_size=1000, num_spatial_layers=1,
               num_temporal_layers=1, num_auxiliary_layers=1, num_unimodal_layers=2)
    job.cfg[c] = cfg
    u8 = frames_u8(302)
    job.arrays[f"{c}/in/inputs_u8"] = u8
    job.arrays[f"{c}/in/inputs"] = as_float(u8)
    job.transient.add(f"{c}/in/inputs")
    flat = params.flatten(params.synthetic_params(cfg, 302, specs=params.clip_leaf_specs(cfg))["params"])
    p = job.seeded_params(c, flat, 302)
    rng = np.random.default_rng(302)
    ids = rng.integers(0, 1000, (3, 12)).astype(np.int32)
    tp = np.zeros((3, 12), np.float32)      # three texts of 12, 7 and 3 tokens
    tp[1, 7:] = 1.0
    tp[2, 3:] = 1.0
    x, fpa = {"$a": f"{c}/in/inputs"}, job.arr(c, "frame_paddings", fp)
    ia, ta = job.arr(c, "text_token_ids", ids), job.arr(c, "text_paddings", tp)
    job.apply(f"{c}/out_padded", "encoders.FactorizedVideoCLIP", tup(cfg), p, x, ia, ta,
              return_intermediate=("frame_embeddings",), frame_paddings=fpa)
    job.apply(f"{c}/out", "encoders.FactorizedVideoCLIP", tup(cfg), p, x, ia, ta)



def _wide_classifier(job, fp, tup):
    c = "base_classifier"
    cfg = dict(models.CONFIGS["videoprism_v1_base"], num_spatial_layers=1, num_temporal_layers=1)
    job.cfg[c] = dict(cfg, num_classes=40)
    u8 = frames_u8(303)
    job.arrays[f"{c}/in/inputs_u8"] = u8
    job.arrays[f"{c}/in/inputs"] = as_float(u8)
    job.transient.add(f"{c}/in/inputs")
    flat = params.flatten(params.synthetic_params(cfg, 303, specs=params.classifier_leaf_specs(cfg, 40))["params"])
    p = job.seeded_params(c, flat, 303)
    x, fpa = {"$a": f"{c}/in/inputs"}, job.arr(c, "frame_paddings", fp)
    ctor = dict(encoder_params=tup(cfg), num_classes=40)
    job.apply(f"{c}/out_padded", "encoders.FactorizedVideoClassifier", ctor, p, x,
              return_intermediate=("global_embeddings",), frame_paddings=fpa)
    job.apply(f"{c}/out", "encoders.FactorizedVideoClassifier", ctor, p, x)


BUILDERS = [("videoprism_v1_base", []), ("videoprism_v1_large", []), ("videoprism_v1_giant", []),
            ("videoprism_lvt_v1_base", []), ("videoprism_lvt_v1_large", []), ("videoprism_lvt_v1_giant", []),
            ("videoprism_vc_v1_base", [400]), ("videoprism_vc_v1_large", [174]), ("videoprism_vc_v1_giant", [400])]
CONSTANTS = ["CONFIGS", "K400_NUM_CLASSES", "SSV2_NUM_CLASSES", "TEXT_MAX_LEN", "TEXT_TOKENIZERS", "CHECKPOINTS"]


def settings_case(job):
    """models.py's constants, read before any builder runs (the LvT builders write vocabulary_size into CONFIGS),
    then every builder's module attributes."""
    for name in CONSTANTS:
        job.calls.append(dict(id=f"settings/constant/{name}", kind="constant", fn=f"models.{name}"))
    for name, args in BUILDERS:
        job.calls.append(dict(id=f"settings/builder/{name}", kind="builder", fn=f"models.{name}", args=args))
    job.arrays["settings/builder_args"] = np.array(json.dumps(dict(BUILDERS)))


def run_child(ref_root, job, mode="wide"):
    with tempfile.TemporaryDirectory() as tmp:
        jp, op = os.path.join(tmp, "job.npz"), os.path.join(tmp, "out.npz")
        np.savez(jp, __job__=np.array(json.dumps(job.calls)), **job.arrays)
        env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "PYTHONSTARTUP")}
        env.update(VIDEOPRISM_CACHE_DIR=os.path.join(tmp, "cache"), HF_HUB_OFFLINE="1")
        env.update({k: "2" for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")})
        subprocess.run([sys.executable, CHILD, ref_root, mode, jp, op], check=True, env=env, cwd=tmp)
        with np.load(op, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}


WIDE = ("base_encoder", "giant_encoder", "base_lvt", "base_classifier")


def _small_job():
    job = Job()
    FILES["ref_layers"] = layer_cases(job)
    FILES["ref_models_tiny"] = tiny_model_cases(job)
    settings_case(job)
    return job


def _wide_job(which):
    job = Job()
    wide_model_cases(job, which)
    return job


def _native_runs(ref_root, job):
    """The mask constant depends on the float type (-0.7 * finfo.max): the mask cases once more with float32.  And
    the reference's tiny encoder, to show that the program runs in its own float32 as well."""
    outputs = {}
    native = Job()
    native.arrays = {k: v for k, v in job.arrays.items() if k.startswith(("masks_", "enc_tiny/"))}
    native.calls = [c for c in job.calls if c["id"].startswith("masks_") or c["id"] == "enc_tiny/out_padded"]
    for k, v in run_child(ref_root, native, "native").items():
        assert v.dtype == np.float32, (k, v.dtype)
        case, call, *rest = k.split("/")
        outputs["/".join([case, call + "_native"] + rest)] = v
    return outputs


def generate(ref_root, out_dir):
    """Every part builds its inputs and runs its own child; the parts run side by side."""
    def part(which):
        job = _small_job() if which == "small" else _wide_job(which)
        outputs = run_child(ref_root, job, "wide")
        if which == "small":
            outputs.update(_native_runs(ref_root, job))
        return job, outputs

    job, outputs = Job(), {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(WIDE) + 1) as pool:
        for j, o in pool.map(part, ("small",) + WIDE):
            job.arrays.update(j.arrays)
            job.cfg.update(j.cfg)
            job.transient |= j.transient
            job.subsample.update(j.subsample)
            outputs.update(o)

    stored = {}
    for k, v in {**job.arrays, **outputs}.items():
        if k in job.transient:
            continue
        stride = job.subsample.get(k)
        if stride:
            stored[f"{k}@rows{stride}"] = v[:, ::stride]
            stored[f"{k}@rowsums"] = v.sum(axis=-1)
            stored[f"{k}@tokenmean"] = v.mean(axis=1)
        else:
            stored[k] = v
    for case, cfg in job.cfg.items():
        stored[f"{case}/cfg"] = np.array(json.dumps(cfg, sort_keys=True))
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for fname, cases in FILES.items():
        arrays = {k: v for k, v in stored.items() if k.split("/", 1)[0] in cases}
        assert arrays, fname
        path = os.path.join(out_dir, fname + ".npz")
        np.savez_compressed(path, **arrays)
        written[fname] = os.path.getsize(path)
    left = {k.split("/", 1)[0] for k in stored} - {c for cs in FILES.values() for c in cs}
    assert not left, left
    return written


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("reference", nargs="?", default=os.environ.get("VIDEOPRISM_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    if not os.path.isfile(os.path.join(args.reference, "videoprism", "layers.py")):
        sys.exit(f"no reference checkout at {args.reference}")
    for fname, size in generate(args.reference, args.out).items():
        print(f"{fname}.npz {size}")


if __name__ == "__main__":
    main()
