"""CPU restatement of the classifier head's folded forward and backward over frozen tokens (test
infrastructure: the yardstick of tests/test_probe_cpu.py and tests/test_gpu_probe.py).

The forward is a dtype-generic copy of torch_restatement.pooler plus the projection, written the way the
kernels compute it: the query folded into the key projection, U[h] = Wk[:,h,:] q~[h], so that K and V are never
formed.  The backward is the hand-derived one the HIP kernels implement (csrc/probe_kernels.hip), not autograd:
with the tokens frozen its only token-sized work is dp = x . dz and dU = sum dl x.

Parameters and gradients are flat {reference path: tensor} dicts (videoprism.probe.head_leaf_specs).  `split`,
if given, maps an [H, D] tensor to what the bf16 kernels see of it (the hi | lo bf16 pair): it is applied to U and
to each clip's dz.
"""

import torch
import torch.nn.functional as F

PA = "atten_pooler/pooling_attention"
QUERY = "atten_pooler/pooling_attention_query"
PDS = f"{PA}/per_dim_scale/per_dim_scale"
LN_SCALE = "atten_pooler/pooling_attention_layer_norm/scale"
LN_BIAS = "atten_pooler/pooling_attention_layer_norm/bias"
WC, BC = "projection/linear/kernel", "projection/linear/bias"
EPS = 1e-6


def as_dtype(flat, dtype):
    return {k: torch.as_tensor(v).to(dtype) for k, v in flat.items()}


def forward(tokens, p, split=None):
    """-> (logits [B, C], state for backward).  tokens [B, S, D] and every leaf of p in one float dtype."""
    x = tokens
    wq, wk, wv, wp = (p[f"{PA}/{n}/w"] for n in ("query", "key", "value", "post"))
    D, H, dh = wq.shape
    c = 1.442695041 / dh ** 0.5
    qraw = torch.einsum("d,dnh->nh", p[QUERY][0], wq) + p[f"{PA}/query/b"]
    sp = F.softplus(p[PDS])
    qt = qraw * c * sp
    U = torch.einsum("dnh,nh->nd", wk, qt)
    if split is not None:
        U = split(U)
    prob = torch.softmax(torch.einsum("bsd,nd->bns", x, U), dim=-1)  # q~ . bk shifts a row: cancels
    z = torch.einsum("bns,bsd->bnd", prob, x)
    enc = torch.einsum("bnd,dnh->bnh", z, wv) + p[f"{PA}/value/b"]
    pooled = torch.einsum("bnh,dnh->bd", enc, wp) + p[f"{PA}/post/b"]
    mean = pooled.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((pooled - mean) ** 2).mean(-1, keepdim=True) + EPS)
    xh = (pooled - mean) * rstd
    emb = xh * (1.0 + p[LN_SCALE]) + p[LN_BIAS]
    logits = emb @ p[WC] + p[BC]
    st = dict(x=x, qraw=qraw, qt=qt, U=U, prob=prob, z=z, enc=enc, rstd=rstd, xh=xh, emb=emb, split=split, c=c)
    return logits, st


def backward(p, st, dlogits):
    """Steps 1-8 -> {path: gradient}, and the intermediates dz / dl / dU under '_dz' / '_dl' / '_dU'."""
    x, prob, z = st["x"], st["prob"], st["z"]
    wq, wk, wv, wp = (p[f"{PA}/{n}/w"] for n in ("query", "key", "value", "post"))
    g = {}
    # 1. projection
    g[WC] = st["emb"].T @ dlogits
    g[BC] = dlogits.sum(0)
    demb = dlogits @ p[WC].T
    # 2. LayerNorm
    g[LN_SCALE] = (demb * st["xh"]).sum(0)
    g[LN_BIAS] = demb.sum(0)
    gg = demb * (1.0 + p[LN_SCALE])
    dpooled = st["rstd"] * (gg - gg.mean(-1, keepdim=True) - st["xh"] * (gg * st["xh"]).mean(-1, keepdim=True))
    # 3. post projection
    g[f"{PA}/post/w"] = torch.einsum("bd,bnh->dnh", dpooled, st["enc"])
    g[f"{PA}/post/b"] = dpooled.sum(0)
    denc = torch.einsum("bd,dnh->bnh", dpooled, wp)
    # 4. value projection
    g[f"{PA}/value/w"] = torch.einsum("bnd,bnh->dnh", z, denc)
    g[f"{PA}/value/b"] = denc.sum(0)
    dz = torch.einsum("bnh,dnh->bnd", denc, wv)
    if st["split"] is not None:
        dz = torch.stack([st["split"](dz[b]) for b in range(dz.shape[0])])
    # 5. pass 1 over the tokens; the softmax term needs none
    dp = torch.einsum("bsd,bnd->bns", x, dz)
    r = (z * dz).sum(-1)
    dl = prob * (dp - r[..., None])
    # 6. pass 2
    dU = torch.einsum("bns,bsd->nd", dl, x)
    # 7. fold
    g[f"{PA}/key/w"] = torch.einsum("nd,nh->dnh", dU, st["qt"])
    g[f"{PA}/key/b"] = torch.zeros_like(p[f"{PA}/key/b"])
    dqt = torch.einsum("dnh,nd->nh", wk, dU)
    # 8. query
    sp = F.softplus(p[PDS])
    dqraw = dqt * st["c"] * sp
    g[PDS] = st["c"] * torch.sigmoid(p[PDS]) * (dqt * st["qraw"]).sum(0)
    g[f"{PA}/query/w"] = torch.einsum("d,nh->dnh", p[QUERY][0], dqraw)
    g[f"{PA}/query/b"] = dqraw
    g[QUERY] = torch.einsum("dnh,nh->d", wq, dqraw)[None]
    g["_dz"], g["_dl"], g["_dU"] = dz, dl, dU
    return g


def tree(p):
    """The nested 'atten_pooler' subtree torch_restatement.pooler takes."""
    out = {}
    for k, v in p.items():
        if not k.startswith("atten_pooler/"):
            continue
        node = out
        parts = k.split("/")[1:]
        for part in parts[:-1]:
            node = node.setdefault(part, {})
        node[parts[-1]] = v
    return out


def synthetic_head(D, H, C, seed, dtype=torch.float64):
    """Every term exercised: non-zero biases, LN scale and per_dim_scale; values fp32-representable."""
    g = torch.Generator().manual_seed(seed)
    dh = D // H
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    p = {QUERY: r(1, D), PDS: r(dh) * 0.3, LN_SCALE: r(D) * 0.1, LN_BIAS: r(D) * 0.1,
         WC: r(D, C) / D ** 0.5, BC: r(C) * 0.1, f"{PA}/post/b": r(D) * 0.1}
    for n in ("query", "key", "value", "post"):
        p[f"{PA}/{n}/w"] = r(D, H, dh) / D ** 0.5
    for n in ("query", "key", "value"):
        p[f"{PA}/{n}/b"] = r(H, dh) * 0.1
    return {k: v.float().to(dtype) for k, v in p.items()}
