"""Token paddings in the attentive probe without a GPU: the masked restatement against the oracle's masked layer (and
so against the reference's own recorded output) and against torch autograd, the two helpers of videoprism.probe,
and the C-ABI's new exports and their refusals."""

import ctypes

import numpy as np
import pytest
import torch

import probe_masked_restatement as pm
import probe_restatement as pr
from oracle import videoprism_oracle as orc
from ref_fixtures import Case
from videoprism import _native, params, probe

F64 = torch.float64
NM = orc.Numerics("f64")
B, S, D, H, C = 4, 70, 128, 2, 5


def _head_of(tree, num_classes=3):
    """The reference's pooler subtree -> the flat fp64 head of probe_restatement, with some projection behind it."""
    p = {f"atten_pooler/{k}": torch.from_numpy(np.asarray(v)).double() for k, v in params.flatten(tree).items()}
    g = torch.Generator().manual_seed(3)
    d = p[pr.LN_BIAS].shape[0]
    p[pr.WC] = torch.randn(d, num_classes, generator=g, dtype=F64)
    p[pr.BC] = torch.randn(num_classes, generator=g, dtype=F64)
    return p


def test_masked_forward_is_the_oracles_masked_layer():
    """The reference's pooler_pad case: the restatement's pooled embedding against orc.atten_token_pooling with the
    same paddings (itself held to the reference's recorded output by tests/test_reference_program.py, and checked
    against the record here too), at the 1e-12 max-abs of tests/test_probe_cpu.py's unmasked pair."""
    c = Case("ref_layers", "pooler_pad")
    x, pad = c.inp["x"].astype(np.float64), c.inp["paddings"].astype(np.float64)
    assert pad.any() and not pad.all(axis=1).any()
    ref = orc.atten_token_pooling(x, c.tree, NM, 2, 32, paddings=pad)[:, 0]
    _, st = pm.forward(torch.from_numpy(x), _head_of(c.tree), torch.from_numpy(pad))
    err = np.abs(st["emb"].numpy() - ref).max()
    print(f"masked restatement vs oracle: max-abs {err:.2e}")
    assert err <= 1e-12
    c.check("out", st["emb"].numpy()[:, None])
    # the paddings count: the unmasked restatement is somewhere else
    _, st0 = pr.forward(torch.from_numpy(x), _head_of(c.tree))
    assert (st0["emb"] - st["emb"]).abs().max().item() > 1e-3


def test_fully_padded_clip_is_the_oracles_uniform_softmax():
    """A clip whose tokens are all padded: the oracle's (the reference's) softmax over S equal logits, 1 / S each,
    and every token's contents count."""
    c = Case("ref_layers", "pooler_pad")
    x = c.inp["x"].astype(np.float64)
    pad = np.array([[0, 1, 0, 0, 1], [1, 1, 1, 1, 1]], np.float64)
    ref = orc.atten_token_pooling(x, c.tree, NM, 2, 32, paddings=pad)[:, 0]
    _, st = pm.forward(torch.from_numpy(x), _head_of(c.tree), torch.from_numpy(pad))
    assert np.abs(st["emb"].numpy() - ref).max() <= 1e-12
    assert torch.equal(st["prob"][1], torch.full_like(st["prob"][1], 1.0 / 5))
    assert not st["prob"][0][:, [1, 4]].any() and st["live"][1].all() and not st["live"][0, 1]


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(12)
    p = pr.synthetic_head(D, H, C, 6)
    x = torch.randn(B, S, D, generator=g, dtype=F64)
    dlogits = torch.randn(B, C, generator=g, dtype=F64)
    pad = torch.zeros(B, S)
    pad[0] = (torch.rand(S, generator=g) < 0.4).float()   # scattered, not a suffix
    pad[1, 41:] = 1.0                                      # a suffix
    pad[2] = 1.0                                           # every token padded: the uniform softmax
    assert pad[0].any() and not pad[0].all() and pad[0, -1] + pad[0, -2] < 2 and not pad[3].any()
    return p, x, dlogits, pad


def test_no_paddings_is_the_unmasked_restatement(case):
    p, x, dlogits, _ = case
    want, st_want = pr.forward(x, p)
    for pad in (None, torch.zeros(B, S), torch.zeros(B, S, dtype=torch.bool)):
        got, st = pm.forward(x, p, pad)
        assert torch.equal(got, want) and torch.equal(st["emb"], st_want["emb"]) and torch.equal(st["prob"], st_want["prob"])
        g, g_want = pm.backward(p, st, dlogits), pr.backward(p, st_want, dlogits)
        assert all(torch.equal(g[k], g_want[k]) for k in g_want)


def test_padding_rule_is_the_references():
    """Padded iff > 0.5, from any dtype; the reference's own comparison on paddings * MIN."""
    vals = torch.tensor([[0.0, 0.5, 0.5000001, 1.0, 0.49, 2.0]])
    assert pm.padded(vals).tolist() == [[False, False, True, True, False, True]]
    assert pm.padded(torch.tensor([[True, False]])).tolist() == [[True, False]]
    assert pm.padded(torch.tensor([[0, 1, 3]])).tolist() == [[False, True, True]]
    assert pm.MIN == -0.7 * float(np.finfo(np.float32).max)
    mask = orc.padding_mask(vals.numpy())[:, 0, 0]
    kept = orc.apply_mask_to_logits(np.zeros_like(mask), mask) == 0.0
    assert (~kept).tolist() == pm.padded(vals).tolist()


def test_masked_backward_is_autograd_of_the_masked_forward(case):
    """Steps 1-8 on the masked state against torch autograd of pm.forward in fp64: scattered paddings, a suffix,
    a fully padded clip and an unpadded one in one batch.  1e-12 relative per parameter and the key bias's autograd
    gradient zero to 1e-14, as tests/test_probe_cpu.py holds the unmasked pair."""
    p, x, dlogits, pad = case
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    logits, _ = pm.forward(x, leaves, pad)
    ref = dict(zip(leaves, torch.autograd.grad(logits, list(leaves.values()), dlogits, allow_unused=True)))
    _, st = pm.forward(x, p, pad)
    got = pm.backward(p, st, dlogits)
    kb = f"{pr.PA}/key/b"
    assert ref[kb] is None or ref[kb].abs().max().item() <= 1e-14   # the folded forward never reads it
    assert not got[kb].any()
    for k, r in ref.items():
        if k == kb:
            continue
        rel = ((got[k] - r).norm() / r.norm()).item()
        print(f"{k}: relative {rel:.2e}")
        assert got[k].shape == r.shape and rel <= 1e-12, (k, rel)
    # the unfolded layer (K and V formed, the key bias in the logits) under the same mask gives the same gradients,
    # the key bias's zero included: the bias still cancels
    ref2 = _autograd_unfolded(p, x, dlogits, pad)
    assert ref2[kb].abs().max().item() <= 1e-14
    for k, r in ref2.items():
        if k != kb:
            assert ((got[k] - r).norm() / r.norm()).item() <= 1e-12, k


def _autograd_unfolded(p, x, dlogits, pad):
    """Autograd of the layer as the reference writes it (layers.py:1044-1136): keys and values of every token, the
    key bias included, the mask applied to the logits."""
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    PA = pr.PA
    dh = leaves[f"{PA}/query/w"].shape[2]
    q = torch.einsum("d,dnh->nh", leaves[pr.QUERY][0], leaves[f"{PA}/query/w"]) + leaves[f"{PA}/query/b"]
    q = q * (1.442695041 / dh ** 0.5) * torch.nn.functional.softplus(leaves[pr.PDS])
    k = torch.einsum("bsd,dnh->bsnh", x, leaves[f"{PA}/key/w"]) + leaves[f"{PA}/key/b"]
    v = torch.einsum("bsd,dnh->bsnh", x, leaves[f"{PA}/value/w"]) + leaves[f"{PA}/value/b"]
    att = torch.einsum("nh,bsnh->bns", q, k)
    att = torch.where(pm.padded(pad)[:, None, :], torch.full_like(att, pm.MIN), att)
    enc = torch.einsum("bns,bsnh->bnh", torch.softmax(att, -1), v)
    pooled = torch.einsum("bnh,dnh->bd", enc, leaves[f"{PA}/post/w"]) + leaves[f"{PA}/post/b"]
    mean = pooled.mean(-1, keepdim=True)
    xh = (pooled - mean) / torch.sqrt(((pooled - mean) ** 2).mean(-1, keepdim=True) + pr.EPS)
    logits = (xh * (1.0 + leaves[pr.LN_SCALE]) + leaves[pr.LN_BIAS]) @ leaves[pr.WC] + leaves[pr.BC]
    return dict(zip(leaves, torch.autograd.grad(logits, list(leaves.values()), dlogits)))


def test_padded_contents_never_reach_a_sum(case):
    """NaN, +Inf and 3e38 in the padded tokens of the clips that have a valid token: the same bits as zeros there."""
    p, x, dlogits, pad = case
    dead = pm.padded(pad) & ~pm.padded(pad).all(-1, keepdim=True)
    want_l, st = pm.forward(torch.where(dead[..., None], torch.zeros_like(x), x), p, pad)
    want = pm.backward(p, st, dlogits)
    for junk in (float("nan"), float("inf"), 3e38):
        got_l, st = pm.forward(torch.where(dead[..., None], torch.full_like(x, junk), x), p, pad)
        got = pm.backward(p, st, dlogits)
        assert torch.equal(got_l, want_l)
        assert all(torch.equal(got[k], want[k]) for k in want)


def test_split_hook_reaches_u_and_every_dz(case):
    p, x, dlogits, pad = case
    seen = []

    def split(m):
        seen.append(tuple(m.shape))
        return m

    _, st = pm.forward(x, p, pad, split)
    pm.backward(p, st, dlogits)
    assert seen == [(H, D)] * (1 + B)


# ---- videoprism.probe helpers ----
def test_token_paddings_is_frame_major():
    fp = torch.tensor([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0]])
    tp = probe.token_paddings(fp, 4)
    assert tp.shape == (2, 12) and tp.dtype == fp.dtype
    assert tp.tolist() == [[0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1]]
    assert torch.equal(tp.reshape(2, 3, 4), fp[..., None].expand(2, 3, 4))   # token t * N + n is of frame t
    assert probe.token_paddings(fp.bool(), 1).dtype == torch.bool and probe.token_paddings(fp, 1).shape == (2, 3)
    with pytest.raises(ValueError):
        probe.token_paddings(fp[0], 4)
    with pytest.raises(ValueError):
        probe.token_paddings(fp, 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pad_tokens(dtype):
    g = torch.Generator().manual_seed(2)
    sets = [torch.randn(n, 8, generator=g).to(dtype) for n in (3, 7, 1)]
    tokens, pad = probe.pad_tokens(sets)
    assert tokens.shape == (3, 7, 8) and tokens.dtype == dtype and pad.shape == (3, 7) and pad.dtype == torch.float32
    for b, t in enumerate(sets):
        n = t.shape[0]
        assert torch.equal(tokens[b, :n], t) and not tokens[b, n:].any()
        assert pad[b].tolist() == [0.0] * n + [1.0] * (7 - n)
    with pytest.raises(ValueError):
        probe.pad_tokens([])
    with pytest.raises(ValueError):
        probe.pad_tokens([sets[0], torch.zeros(2, 9, dtype=dtype)])
    with pytest.raises(ValueError):
        probe.pad_tokens([sets[0], sets[1].double()])
    with pytest.raises(ValueError):
        probe.pad_tokens([sets[0], torch.zeros(0, 8, dtype=dtype)])


def test_paddings_are_checked_before_the_library_is_called():
    """The shape refusal needs no device (the tokens' own checks come first and are unchanged)."""
    head = probe.AttentiveProbe(128, 2, 3)
    with pytest.raises(ValueError, match="GPU"):
        head(torch.zeros(1, 4, 128), torch.zeros(1, 4))
    x = torch.zeros(2, 4, 128)
    for bad in (torch.zeros(2, 5), torch.zeros(4), torch.zeros(2, 4, 1)):
        with pytest.raises(ValueError, match="paddings"):
            _native._probe_paddings("vp_op_probe_forward", bad, x)
    with pytest.raises(ValueError, match="paddings"):
        _native._probe_paddings("vp_op_probe_forward", torch.zeros(2, 4, dtype=torch.float64), x)
    assert _native._probe_paddings("vp_op_probe_forward", None, x) == ("vp_op_probe_forward", ())
    entry, args = _native._probe_paddings("vp_op_probe_backward", torch.zeros(2, 4), x)
    assert entry == "vp_op_probe_backward_masked" and len(args) == 1


# ---- C-ABI ----
SYMBOLS = ("vp_op_probe_forward_masked", "vp_op_probe_backward_masked")


def test_symbols_exported_and_abi_version_unchanged():
    lib = ctypes.CDLL(_native.library_path())
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _native.exported_symbols(), s
    assert lib.vp_abi_version() == 8   # additive, as vp_op_topk_groups* were


def _fwd(lib, dims, prm, tokens, dtype, b, s, pad, logits, ws, ws_bytes):
    return lib.vp_op_probe_forward_masked(ctypes.byref(dims) if dims is not None else None,
                                          ctypes.byref(prm) if prm is not None else None, tokens, dtype, b, s, pad,
                                          logits, None, ws, ws_bytes, None)


def _bwd(lib, dims, prm, tokens, dtype, b, s, pad, dlogits, grads, ws, ws_bytes):
    return lib.vp_op_probe_backward_masked(ctypes.byref(dims), ctypes.byref(prm), tokens, dtype, b, s, pad, dlogits,
                                           ctypes.byref(grads) if grads is not None else None, ws, ws_bytes, None)


def test_masked_refusals_without_a_gpu():
    """Every refusal of the unmasked calls, from the masked ones, with paddings given and with NULL: all of them
    come ahead of any device call (the pointers are never followed)."""
    lib = _native.load()
    buf = 256
    prm = _native.vp_probe_params(**{m: buf for m, _ in _native.PROBE_LEAVES})
    dims = _native.vp_probe_dims(768, 12, 400)
    need = _native.op_probe_workspace_bytes(768, 12, 400, 2, 64)
    EINVAL = _native.VP_EINVAL
    for pad in (buf, None):
        assert _fwd(lib, None, None, None, 0, 2, 64, pad, None, None, 0) == EINVAL
        assert b"null" in lib.vp_last_error()
        assert _fwd(lib, dims, prm, None, 0, 2, 64, pad, buf, buf, need) == EINVAL
        assert _fwd(lib, dims, prm, buf, 0, 2, 64, pad, None, buf, need) == EINVAL
        assert _fwd(lib, dims, prm, buf, 0, 2, 64, pad, buf, None, need) == EINVAL
        assert _fwd(lib, dims, None, buf, 0, 2, 64, pad, buf, buf, need) == EINVAL
        assert _bwd(lib, dims, prm, buf, 0, 2, 64, pad, None, prm, buf, need) == EINVAL
        assert _bwd(lib, dims, prm, buf, 0, 2, 64, pad, buf, None, buf, need) == EINVAL
        assert _bwd(lib, dims, prm, None, 0, 2, 64, pad, buf, prm, buf, need) == EINVAL
        for b, s in ((0, 64), (2, 0)):
            assert _fwd(lib, dims, prm, buf, 0, b, s, pad, buf, buf, need) == EINVAL
            assert _bwd(lib, dims, prm, buf, 0, b, s, pad, buf, prm, buf, need) == EINVAL
        assert _fwd(lib, dims, prm, buf, 0, 2, 64, pad, buf, buf, need - 1) == EINVAL
        assert str(need).encode() in lib.vp_last_error()   # the unmasked calls' workspace serves both
        assert _bwd(lib, dims, prm, buf, 1, 2, 64, pad, buf, prm, buf, need - 1) == EINVAL
        assert _fwd(lib, dims, prm, buf, _native.VP_U8, 2, 64, pad, buf, buf, need) == EINVAL
    wide = _native.vp_probe_dims(192, 2, 4)
    assert _fwd(lib, wide, prm, buf, 0, 2, 64, buf, buf, buf, 1 << 40) == _native.VP_ENOTSUP
