"""The classifier head's training ops without a GPU: the folded backward restated on the CPU against torch
autograd, the C-ABI's exports and refusals, and AttentiveProbe's names and variables."""

import ctypes

import numpy as np
import pytest
import torch

import probe_restatement as pr
import torch_restatement as tr
from videoprism import _native, models, params
from videoprism.probe import AttentiveProbe, head_leaf_specs

F64 = torch.float64
B, S, D, H, C = 3, 70, 128, 2, 5


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(11)
    p = pr.synthetic_head(D, H, C, 5)
    x = torch.randn(B, S, D, generator=g, dtype=F64)
    dlogits = torch.randn(B, C, generator=g, dtype=F64)
    return p, x, dlogits


def _autograd(p, x, dlogits):
    """Logits and gradients of torch_restatement.pooler (K and V formed, nothing folded) plus the projection."""
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    emb = tr.pooler(x, pr.tree(leaves), H, hidden=D)
    logits = emb @ leaves[pr.WC] + leaves[pr.BC]
    grads = torch.autograd.grad(logits, list(leaves.values()), dlogits)
    return logits.detach(), dict(zip(leaves, grads))


def test_folded_forward_is_the_pooler(case):
    p, x, dlogits = case
    logits, st = pr.forward(x, p)
    ref, _ = _autograd(p, x, dlogits)
    assert (st["emb"] - tr.pooler(x, pr.tree(p), H, hidden=D)).abs().max().item() <= 1e-12
    assert (logits - ref).abs().max().item() <= 1e-12


def test_folded_backward_is_autograd(case):
    """Steps 1-8 against autograd, 1e-12 relative per parameter; the key bias's autograd gradient is zero to 1e-14."""
    p, x, dlogits = case
    _, st = pr.forward(x, p)
    got = pr.backward(p, st, dlogits)
    _, ref = _autograd(p, x, dlogits)
    assert set(ref) == set(head_leaf_specs(D, H, C))
    kb = f"{pr.PA}/key/b"
    assert ref[kb].abs().max().item() <= 1e-14 and not got[kb].any()
    for k, r in ref.items():
        if k == kb:
            continue
        rel = ((got[k] - r).norm() / r.norm()).item()
        print(f"{k}: relative {rel:.2e}")
        assert got[k].shape == r.shape and rel <= 1e-12, (k, rel)


def test_split_hook_reaches_u_and_every_dz(case):
    p, x, dlogits = case
    seen = []

    def split(m):
        seen.append(tuple(m.shape))
        return m

    _, st = pr.forward(x, p, split)
    pr.backward(p, st, dlogits)
    assert seen == [(H, D)] * (1 + B)


# ---- C-ABI ----
SYMBOLS = ("vp_op_probe_workspace_bytes", "vp_op_probe_forward", "vp_op_probe_backward")


def test_symbols_exported_and_abi_version_unchanged():
    lib = ctypes.CDLL(_native.library_path())
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _native.exported_symbols(), s
    assert lib.vp_abi_version() == 8


def _structs():
    buf = 256  # never dereferenced: every refusal comes ahead of any device call
    prm = _native.vp_probe_params(**{m: buf for m, _ in _native.PROBE_LEAVES})
    return buf, prm


def _fwd(lib, dims, prm, tokens, dtype, b, s, logits, ws, ws_bytes):
    return lib.vp_op_probe_forward(ctypes.byref(dims), ctypes.byref(prm) if prm is not None else None, tokens, dtype,
                                   b, s, logits, None, ws, ws_bytes, None)


def _bwd(lib, dims, prm, tokens, dtype, b, s, dlogits, grads, ws, ws_bytes):
    return lib.vp_op_probe_backward(ctypes.byref(dims), ctypes.byref(prm), tokens, dtype, b, s, dlogits,
                                    ctypes.byref(grads) if grads is not None else None, ws, ws_bytes, None)


def test_refusals_without_a_gpu():
    lib = _native.load()
    buf, prm = _structs()
    dims = _native.vp_probe_dims(768, 12, 400)
    n = ctypes.c_size_t()
    assert lib.vp_op_probe_workspace_bytes(ctypes.byref(dims), 2, 64, ctypes.byref(n)) == _native.VP_OK
    need = n.value
    assert need > 0
    # null pointers
    assert lib.vp_op_probe_workspace_bytes(None, 2, 64, ctypes.byref(n)) == _native.VP_EINVAL
    assert lib.vp_op_probe_workspace_bytes(ctypes.byref(dims), 2, 64, None) == _native.VP_EINVAL
    assert _fwd(lib, dims, prm, None, 0, 2, 64, buf, buf, need) == _native.VP_EINVAL
    assert _fwd(lib, dims, prm, buf, 0, 2, 64, None, buf, need) == _native.VP_EINVAL
    assert _fwd(lib, dims, prm, buf, 0, 2, 64, buf, None, need) == _native.VP_EINVAL
    assert _fwd(lib, dims, None, buf, 0, 2, 64, buf, buf, need) == _native.VP_EINVAL
    assert b"null" in lib.vp_last_error()
    for member, _ in _native.PROBE_LEAVES:  # any leaf, parameter or gradient
        _, hole = _structs()
        setattr(hole, member, None)
        assert _fwd(lib, dims, hole, buf, 0, 2, 64, buf, buf, need) == _native.VP_EINVAL, member
        assert _bwd(lib, dims, prm, buf, 0, 2, 64, buf, hole, buf, need) == _native.VP_EINVAL, member
    assert _bwd(lib, dims, prm, buf, 0, 2, 64, None, prm, buf, need) == _native.VP_EINVAL
    assert _bwd(lib, dims, prm, buf, 0, 2, 64, buf, None, buf, need) == _native.VP_EINVAL
    # B or S < 1
    for b, s in ((0, 64), (2, 0), (-1, 64)):
        assert lib.vp_op_probe_workspace_bytes(ctypes.byref(dims), b, s, ctypes.byref(n)) == _native.VP_EINVAL
        assert _fwd(lib, dims, prm, buf, 0, b, s, buf, buf, need) == _native.VP_EINVAL
        assert _bwd(lib, dims, prm, buf, 0, b, s, buf, prm, buf, need) == _native.VP_EINVAL
    assert b"B >= 1" in lib.vp_last_error()
    # a short workspace, with the size it needs in the message
    assert _fwd(lib, dims, prm, buf, 0, 2, 64, buf, buf, need - 1) == _native.VP_EINVAL
    assert str(need).encode() in lib.vp_last_error()
    assert _bwd(lib, dims, prm, buf, 1, 2, 64, buf, prm, buf, need - 1) == _native.VP_EINVAL
    # a token dtype the head does not take
    assert _fwd(lib, dims, prm, buf, _native.VP_U8, 2, 64, buf, buf, need) == _native.VP_EINVAL


@pytest.mark.parametrize("d,h,what", [(192, 2, "128"), (1664, 13, "1536"), (2176, 17, "16 heads")])
def test_widths_outside_the_poolers_range_are_not_supported(d, h, what):
    lib = _native.load()
    buf, prm = _structs()
    dims = _native.vp_probe_dims(d, h, 4)
    n = ctypes.c_size_t()
    assert lib.vp_op_probe_workspace_bytes(ctypes.byref(dims), 2, 64, ctypes.byref(n)) == _native.VP_ENOTSUP
    assert what.encode() in lib.vp_last_error()
    assert _fwd(lib, dims, prm, buf, 0, 2, 64, buf, buf, 1 << 40) == _native.VP_ENOTSUP
    assert _bwd(lib, dims, prm, buf, 0, 2, 64, buf, prm, buf, 1 << 40) == _native.VP_ENOTSUP
    with pytest.raises(NotImplementedError):
        _native.op_probe_workspace_bytes(d, h, 4, 2, 64)


# ---- AttentiveProbe ----
@pytest.mark.parametrize("name", ["videoprism_v1_base", "videoprism_v1_giant"])
def test_parameter_names_and_shapes_are_the_heads_leaves(name):
    cfg = models.CONFIGS[name]
    specs = params.classifier_leaf_specs(cfg, 400)
    head = {k: v for k, v in specs.items() if not k.startswith("encoder/")}
    probe = AttentiveProbe(cfg["model_dim"], cfg["num_heads"], 400)
    got = {k: tuple(v.shape) for k, v in probe.named_parameters()}
    assert got == head and list(got) == list(head)
    assert [path for _, path in _native.PROBE_LEAVES] == list(head)
    assert all(p.dtype == torch.float32 and p.requires_grad for p in probe.parameters())
    assert head == head_leaf_specs(cfg["model_dim"], cfg["num_heads"], 400)


def test_initialisation_is_as_documented():
    a, b = AttentiveProbe(256, 4, 7, seed=3), AttentiveProbe(256, 4, 7, seed=3)
    for (k, v), w in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(v, w), k
        leaf = k.rsplit("/", 1)[-1]
        if leaf in ("b", "bias", "scale", "per_dim_scale"):
            assert not v.any(), k
        else:
            assert abs(v.std().item() * 256 ** 0.5 - 1.0) < 0.1, k
    assert not torch.equal(a.get_parameter(pr.WC), AttentiveProbe(256, 4, 7, seed=4).get_parameter(pr.WC))


def test_variables_round_trip_and_merge_keeps_the_encoder():
    enc = dict(models.CONFIGS["videoprism_v1_base"])
    enc.update(num_spatial_layers=1, num_temporal_layers=1)
    var = params.synthetic_params(enc, 2, specs=params.classifier_leaf_specs(enc, 6))
    probe = AttentiveProbe(768, 12, 6, seed=1)
    sub = probe.to_variables()
    assert set(sub) == {"atten_pooler", "projection"} and set(sub["projection"]) == {"linear"}
    flat = params.flatten(sub)
    assert {k: v.shape for k, v in flat.items()} == head_leaf_specs(768, 12, 6)
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in flat.values())
    merged = probe.merge_into(var)
    params.validate(params.canonical_params(merged), params.classifier_leaf_specs(enc, 6))
    before, after = params.flatten(var["params"]["encoder"]), params.flatten(merged["params"]["encoder"])
    assert set(before) == set(after) and all(after[k] is before[k] for k in before)
    assert merged["params"]["atten_pooler"] is not var["params"]["atten_pooler"]
    for src in (sub, merged, merged["params"]):
        back = AttentiveProbe.from_variables(src, num_heads=12)
        assert back.dims == probe.dims
        for (k, v), w in zip(probe.named_parameters(), back.parameters()):
            assert torch.equal(v, w), k
    # the given classifier's own head, and a head of another width
    own = AttentiveProbe.from_variables(var, num_heads=12)
    assert np.array_equal(own.to_variables()["projection"]["linear"]["kernel"],
                          var["params"]["projection"]["linear"]["kernel"])
    with pytest.raises(ValueError):
        AttentiveProbe.from_variables(sub, num_heads=16)
    with pytest.raises(ValueError):
        probe.merge_into({"params": sub})


def test_tokens_are_checked_before_the_library_is_called():
    probe = AttentiveProbe(128, 2, 3)
    with pytest.raises(NotImplementedError, match="frozen"):
        probe(torch.zeros(1, 4, 128, requires_grad=True))
    with pytest.raises(ValueError):
        probe(torch.zeros(1, 4, 64))
    with pytest.raises(ValueError, match="GPU"):
        probe(torch.zeros(1, 4, 128))
