"""norm_policy='primer_hybrid' restated for the tests: the transformer layer of layers.py:316-430, :749-872 and the
text encoder of encoders.py:656-759 on top of it, once in NumPy from the oracle's own primitives (any Numerics
mode) and once, independently, in plain PyTorch fp64 (the style of torch_restatement.py).

The oracle's text_encoder is 'pre' only; videoprism_lvt_v1_giant's text tower is 'primer_hybrid', where each
sublayer is x + post_layer_norm(f(pre_layer_norm(x))).  In the FFN sublayer the padding multiply comes before the
post LayerNorm (layers.py:409-415), so a padded row's sublayer output is x + beta_post, not x.  With policy 'pre'
the NumPy functions here repeat the oracle's operations in the oracle's order.
"""

import numpy as np
import torch
import torch.nn.functional as F

from oracle import videoprism_oracle as orc

POLICIES = ("pre", "primer_hybrid")


def _ln(x, p, nm):
    return orc.layer_norm(x, p["scale"], p["bias"], nm)


def attention_sublayer(x, p, mask, nm, num_heads, cap, policy):
    """layers.py:819-860 up to the residual: x + [post_layer_norm](attention([pre_]layer_norm(x)))."""
    d = x.shape[-1]
    h = _ln(x, p["pre_layer_norm" if policy == "primer_hybrid" else "layer_norm"], nm)
    sa = p["self_attention"]
    q = orc.attention_projection_in(h, sa["query"]["w"], sa["query"]["b"], nm)
    k = orc.attention_projection_in(h, sa["key"]["w"], sa["key"]["b"], nm)
    v = orc.attention_projection_in(h, sa["value"]["w"], sa["value"]["b"], nm)
    enc = orc.dot_atten(q, k, v, mask, nm, cap, d // num_heads)
    att = orc.attention_projection_out(enc, sa["post"]["w"], sa["post"]["b"], nm)
    if policy == "primer_hybrid":
        att = _ln(att, p["post_layer_norm"], nm)
    return nm.act(att + x)


def ffn_sublayer(x, ff, paddings, nm, policy, activation=orc.relu):
    """layers.py:372-430 TransformerFeedForward with its residual."""
    y = _ln(x, ff["pre_layer_norm" if policy == "primer_hybrid" else "layer_norm"], nm)
    a = nm.act(activation(orc.dense(y, ff["ffn_layer1"]["linear"]["kernel"], ff["ffn_layer1"]["linear"]["bias"], nm)))
    pad = None if paddings is None else nm.act(1.0 - paddings[..., None])
    if pad is not None:
        a = nm.act(a * pad)
    o = orc.dense(a, ff["ffn_layer2"]["linear"]["kernel"], ff["ffn_layer2"]["linear"]["bias"], nm)
    if pad is not None:
        o = nm.act(o * pad)
    if policy == "primer_hybrid":
        o = _ln(o, ff["post_layer_norm"], nm)
    return nm.act(x + o)


def transformer_layer(x, p, paddings, mask, nm, num_heads, cap, policy, activation=orc.relu):
    assert policy in POLICIES, policy
    x = attention_sublayer(x, p, mask, nm, num_heads, cap, policy)
    return ffn_sublayer(x, p["ff_layer"], paddings, nm, policy, activation)


def text_features(params, ids, paddings, cfg, nm, policy):
    """The residual stream [B, L+1, D] after the unimodal transformer, before unimodal_ln, and its paddings."""
    D = cfg["model_dim"]
    ids = np.asarray(ids)
    b, n = ids.shape
    table = nm.param(params["token_emb"]["emb_var"])
    emb = table[np.clip(ids, 0, table.shape[0] - 1)]
    emb = nm.act(emb * nm.act(D ** 0.5))
    pos = nm.act(orc.sinusoidal_positions(n, D))[None]
    feats = nm.act(emb + pos)
    cls = np.tile(nm.param(params["cls_emb"]), (b, 1, 1))
    cls = nm.act(cls * nm.act(D ** 0.5))
    feats = np.concatenate([feats, cls], axis=1)
    pad = np.concatenate([np.asarray(paddings, np.float64), np.zeros((b, 1))], axis=-1)
    causal = cfg.get("enable_causal_atten", True)
    mask = orc.attention_masks_for_fprop(np.asarray(pad, np.float64), causal)
    if not causal and not np.any(pad):
        mask = None
    xl = params["unimodal_transformer"]["x_layers"]
    for i in range(cfg["num_unimodal_layers"]):
        feats = transformer_layer(feats, orc._layer_slice(xl, i), pad, mask, nm, cfg["num_heads"],
                                  cfg.get("atten_logit_cap", 0.0), policy)
    return feats, pad


def text_encoder(params, ids, paddings, cfg, nm, policy=None):
    """encoders.py:656-759 -> [B, L+1, D] after unimodal_ln; policy defaults to cfg['norm_policy']."""
    feats, _ = text_features(params, ids, paddings, cfg, nm, policy or cfg.get("norm_policy", "pre"))
    return _ln(feats, params["unimodal_ln"], nm)


def text_embedding(params, ids, paddings, cfg, mode="f64", normalize=True):
    """FactorizedVideoCLIP's text side (encoders.py:887-908): the CLS row, L2-normalised; `params` is the whole tree."""
    emb = text_encoder(params["text_encoder"], ids, paddings, cfg, orc.Numerics(mode))[:, -1]
    return orc.l2_normalize(emb) if normalize else np.asarray(emb, np.float64)


# ---- the second restatement: plain PyTorch, fp64 ----

def _t(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float64)


def _tln(x, p, i):
    return F.layer_norm(x, (x.shape[-1],), weight=_t(p["scale"][i]) + 1.0, bias=_t(p["bias"][i]), eps=1e-6)


def torch_text_encoder(params, ids, paddings, cfg, policy):
    """Token table * sqrt(D) + sinusoids, CLS appended, L causal ReLU layers, unimodal_ln; fp64 tensors."""
    assert policy in POLICIES, policy
    D, heads = cfg["model_dim"], cfg["num_heads"]
    cap = cfg.get("atten_logit_cap", 0.0)
    dh = D // heads
    ids = torch.as_tensor(np.asarray(ids)).long()
    B, L = ids.shape
    table = _t(params["token_emb"]["emb_var"])
    x = table[ids.clamp(0, table.shape[0] - 1)] * D ** 0.5
    half = D // 2
    inv = torch.exp(torch.arange(half, dtype=torch.float64) * -(np.log(10000.0) / max(half - 1, 1)))
    ang = torch.arange(L, dtype=torch.float64)[:, None] * inv[None]
    x = x + torch.cat([torch.sin(ang), torch.cos(ang)], -1)
    x = torch.cat([x, (_t(params["cls_emb"]) * D ** 0.5).expand(B, 1, D)], 1)
    S = L + 1
    pad = torch.cat([_t(paddings), torch.zeros(B, 1, dtype=torch.float64)], 1)
    # a key is visible to a query when neither is padded and (causal) it does not lie ahead; a query with no
    # visible key attends uniformly to all S keys, which is what equal masked logits give
    valid = (pad < 0.5)
    allowed = valid[:, :, None] & valid[:, None, :]
    if cfg.get("enable_causal_atten", True):
        allowed = allowed & torch.tril(torch.ones(S, S, dtype=torch.bool))[None]
    none = ~allowed.any(-1, keepdim=True)
    allowed = (allowed | none)[:, None]                                   # [B, 1, S, S]
    uniform = none[:, None]                                               # [B, 1, S, 1]
    keep = (1.0 - pad)[..., None]
    pre = "pre_layer_norm" if policy == "primer_hybrid" else "layer_norm"
    xl = params["unimodal_transformer"]["x_layers"]
    for i in range(cfg["num_unimodal_layers"]):
        sa = xl["self_attention"]
        h = _tln(x, xl[pre], i)
        q, k, v = (torch.einsum("bsd,dnh->bsnh", h, _t(sa[n]["w"][i])) + _t(sa[n]["b"][i]) for n in ("query", "key", "value"))
        logits = torch.einsum("btnh,bsnh->bnts", q / dh ** 0.5, k)
        if cap > 0:
            logits = cap * torch.tanh(logits / cap)
        logits = torch.where(uniform, torch.zeros_like(logits), logits)
        probs = torch.softmax(logits.masked_fill(~allowed, float("-inf")), -1)
        att = torch.einsum("bnts,bsnh,dnh->btd", probs, v, _t(sa["post"]["w"][i])) + _t(sa["post"]["b"][i])
        if policy == "primer_hybrid":
            att = _tln(att, xl["post_layer_norm"], i)
        x = x + att
        ff = xl["ff_layer"]
        a = torch.relu(_tln(x, ff[pre], i) @ _t(ff["ffn_layer1"]["linear"]["kernel"][i]) +
                       _t(ff["ffn_layer1"]["linear"]["bias"][i])) * keep
        o = (a @ _t(ff["ffn_layer2"]["linear"]["kernel"][i]) + _t(ff["ffn_layer2"]["linear"]["bias"][i])) * keep
        if policy == "primer_hybrid":
            o = _tln(o, ff["post_layer_norm"], i)
        x = x + o
    return _tln(x, {k: np.asarray(v)[None] for k, v in params["unimodal_ln"].items()}, 0)
