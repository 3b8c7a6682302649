"""CPU restatement of the classifier head's folded forward and backward under token paddings (test infrastructure:
the yardstick of tests/test_probe_masked_cpu.py and tests/test_gpu_probe_masked.py).

tests/probe_restatement.py with the reference's key mask (layers.py:51-72 and :1103-1106): `paddings` [B, S], a token
is padded iff its value is > 0.5, and a padded token's logit becomes exactly MIN = -0.7 * finfo(float32).max in every
head before the softmax.  So in a clip with a valid token the padded tokens get probability exactly 0 (exp(MIN - max)
underflows in any float type), and in a clip whose tokens are all padded the softmax is uniform, 1 / S over all S
tokens.  The key bias still shifts the valid logits of a row equally and still cancels: its gradient is zero.

Contents ignored: the forward selects zeros for the padded tokens of a clip with a valid token before any sum reads
them (what the kernels do by never loading the row), so NaN or Inf there reaches nothing; in a clip of padded tokens
alone every token is read, as in the reference.  The backward's steps are probe_restatement.backward's, written so
that a padded token gives dl == 0 exactly (where prob == 0, and in a clip of padded tokens alone too: MIN is a
constant, nothing flows through it) and adds exactly 0 to dU whatever it holds.  `split` is probe_restatement's hook
for the bf16 hi | lo operands (U, each clip's dz).
"""

import numpy as np
import torch
import torch.nn.functional as F

import probe_restatement as pr
from probe_restatement import BC, LN_BIAS, LN_SCALE, PA, PDS, QUERY, WC, EPS  # noqa: F401

MIN = -0.7 * float(np.finfo(np.float32).max)


def padded(paddings):
    """[B, S] of any dtype -> bool, the reference's rule: mask = paddings * MIN is kept where mask >= 0.5 * MIN."""
    return ~(torch.as_tensor(paddings).double() * MIN >= 0.5 * MIN)


def forward(tokens, p, paddings=None, split=None):
    """-> (logits [B, C], state for backward).  paddings None: probe_restatement.forward itself."""
    if paddings is None:
        return pr.forward(tokens, p, split)
    x = tokens
    pad = padded(paddings)
    assert pad.shape == x.shape[:2], (pad.shape, x.shape)
    wq, wk, wv, wp = (p[f"{PA}/{n}/w"] for n in ("query", "key", "value", "post"))
    D, H, dh = wq.shape
    c = 1.442695041 / dh ** 0.5
    qraw = torch.einsum("d,dnh->nh", p[QUERY][0], wq) + p[f"{PA}/query/b"]
    sp = F.softplus(p[PDS])
    qt = qraw * c * sp
    U = torch.einsum("dnh,nh->nd", wk, qt)
    if split is not None:
        U = split(U)
    # a clip with a valid token never looks at its padded tokens; a clip of padded tokens alone looks at all of them
    live = ~pad | pad.all(-1, keepdim=True)
    xs = torch.where(live[..., None], x, torch.zeros_like(x))
    att = torch.einsum("bsd,nd->bns", xs, U)
    att = torch.where(pad[:, None, :], torch.full_like(att, MIN), att)
    prob = torch.softmax(att, dim=-1)
    z = torch.einsum("bns,bsd->bnd", prob, xs)
    enc = torch.einsum("bnd,dnh->bnh", z, wv) + p[f"{PA}/value/b"]
    pooled = torch.einsum("bnh,dnh->bd", enc, wp) + p[f"{PA}/post/b"]
    mean = pooled.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((pooled - mean) ** 2).mean(-1, keepdim=True) + EPS)
    xh = (pooled - mean) * rstd
    emb = xh * (1.0 + p[LN_SCALE]) + p[LN_BIAS]
    logits = emb @ p[WC] + p[BC]
    # x: the tokens as the sums see them (zero where no sum reads them), so that backward's steps stay as they are
    st = dict(x=xs, qraw=qraw, qt=qt, U=U, prob=prob, z=z, enc=enc, rstd=rstd, xh=xh, emb=emb, split=split, c=c,
              att=att, pad=pad, live=live)
    return logits, st


def backward(p, st, dlogits):
    """Steps 1-8 of probe_restatement.backward on the masked state (an unmasked state: that function itself).  The
    one change is in step 5: a padded token's logit is the constant MIN, so nothing flows through it to U and
    dl = prob (dp - r) is selected to exactly 0 there.  Beside a valid token prob is 0 anyway; in a clip of padded
    tokens alone prob is 1 / S, the tokens still reach every gradient through z, and dU gets nothing from the clip."""
    if "pad" not in st:
        return pr.backward(p, st, dlogits)
    x, prob, z, pad = st["x"], st["prob"], st["z"], st["pad"]
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
    # 5. pass 1 over the valid tokens; the softmax term needs none
    xv = torch.where(pad[..., None], torch.zeros_like(x), x)
    dp = torch.einsum("bsd,bnd->bns", xv, dz)
    r = (z * dz).sum(-1)
    dl = torch.where(pad[:, None, :], torch.zeros_like(dp), prob * (dp - r[..., None]))
    # 6. pass 2
    dU = torch.einsum("bns,bsd->nd", dl, xv)
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
