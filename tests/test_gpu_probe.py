"""MI355X tests of the classifier head's training ops (vp_op_probe_*, videoprism.probe.AttentiveProbe) against the
fp64 restatement of tests/probe_restatement.py.

Gradient parity: every gradient g of the head and the logits satisfy ||g - g64||_2 <= 2e-5 ||g64||_2, the op-level
fp64 bar of tests/test_gpu_clip_kernels.py taken norm-wise; the key bias's gradient is exactly zero.  With bf16
tokens g64 is the restatement with U and each clip's dz passed through the production hi | lo bf16 split
(vp_dev_pool_split_u): what the kernels are given.  The split reference's own distance from the unsplit one is
printed and written beside the measured errors to profiles/probe/grad_parity.txt; it is not barred.
The shapes are the smallest that reach every branch (see CASES)."""

import os

import numpy as np
import pytest
import torch

import probe_restatement as pr
from videoprism import _native, encoders, models, params
from videoprism.probe import AttentiveProbe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_TXT = os.path.join(ROOT, "profiles", "probe", "grad_parity.txt")
BAR = 2e-5

# (bf16, B, S, D, H, C)
CASES = [
    (False, 1, 40, 128, 2, 1),       # S < one chunk; a single half column block
    (False, 3, 300, 384, 6, 5),      # chunk tail; 256 + 128 column blocks; the sum over clips
    (False, 2, 257, 1408, 16, 70),   # the D > 1024 instantiations with their > 64 KB LDS opt-in; C past one 64-column tile
    (True, 2, 512, 256, 4, 3),       # S % 32 == 0: the MFMA pass 1 and logits
    (True, 3, 300, 384, 6, 5),       # bf16 tokens on the scalar kernels
]


def _split(m):
    """[H, D] -> the fp64 value of the production hi | lo bf16 pair of its fp32 rounding."""
    H = m.shape[0]
    ut = _native.dev_pool_split_u(m.float().numpy())
    f = torch.from_numpy((ut.astype(np.uint32) << 16).view(np.float32)).double()
    assert not f[2 * H:].any()
    return f[:H] + f[H:2 * H]


def _inputs(bf16, B, S, D, H, C):
    g = torch.Generator().manual_seed(1000 * D + 10 * S + B)
    x = torch.randn(B, S, D, generator=g).to(torch.bfloat16)  # bf16-representable in either dtype
    p = pr.synthetic_head(D, H, C, D + S)
    dlogits = torch.randn(B, C, generator=g)
    return (x if bf16 else x.float()), p, dlogits


def _device_run(cuda, x, p, H, dlogits):
    probe = AttentiveProbe.from_variables(params.unflatten({k: v.float().numpy() for k, v in p.items()}), num_heads=H,
                                          device=cuda)
    logits = probe(x.to(cuda))
    logits.backward(dlogits.to(cuda))
    torch.cuda.synchronize()
    return logits.detach().cpu(), {k: v.grad.cpu() for k, v in probe.named_parameters()}


@pytest.fixture(scope="module")
def parity_log():
    lines = []
    yield lines
    os.makedirs(os.path.dirname(PARITY_TXT), exist_ok=True)
    with open(PARITY_TXT, "w") as f:
        f.write("AttentiveProbe gradients on the GPU against the fp64 restatement: ||g - g64|| / ||g64|| per leaf "
                f"(bar {BAR:g}).\nbf16 tokens: g64 is the restatement on the hi | lo split of U and dz; 'split vs "
                "unsplit' is that reference's own distance from the unsplit fp64 gradient (not barred).\n")
        f.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("bf16,B,S,D,H,C", CASES)
def test_gradient_parity(cuda, parity_log, bf16, B, S, D, H, C):
    x, p, dlogits = _inputs(bf16, B, S, D, H, C)
    logits, grads = _device_run(cuda, x, p, H, dlogits)
    ref_logits, st = pr.forward(x.double(), p, _split if bf16 else None)
    ref = pr.backward(p, st, dlogits.double())
    plain = None
    if bf16:
        _, st0 = pr.forward(x.double(), p)
        plain = pr.backward(p, st0, dlogits.double())
    head = f"{'bf16' if bf16 else 'fp32'} B={B} S={S} D={D} H={H} C={C}"
    rel = lambda a, b: ((a.double() - b).norm() / b.norm()).item()  # noqa: E731
    errs = {"logits": rel(logits, ref_logits)}
    kb = f"{pr.PA}/key/b"
    for k, g in grads.items():
        assert g.shape == p[k].shape and g.dtype == torch.float32, k
        if k != kb:
            errs[k] = rel(g, ref[k])
    for k, e in errs.items():
        line = f"{head}  {k}: {e:.3e}"
        if plain is not None and k != "logits":
            line += f"  (split vs unsplit {rel(ref[k], plain[k]):.3e})"
        print(line)
        parity_log.append(line)
    assert not grads[kb].any(), "the key bias's gradient is exactly zero"
    assert len(grads) == len(_native.PROBE_LEAVES)
    bad = {k: e for k, e in errs.items() if not e <= BAR}
    assert not bad, bad


def test_two_runs_give_the_same_bits(cuda):
    bf16, B, S, D, H, C = CASES[4]
    x, p, dlogits = _inputs(bf16, B, S, D, H, C)
    l1, g1 = _device_run(cuda, x, p, H, dlogits)
    l2, g2 = _device_run(cuda, x, p, H, dlogits)
    assert torch.equal(l1, l2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


TINY = dict(patch_size=2, pos_emb_shape=(2, 2, 2), model_dim=128, num_spatial_layers=1, num_temporal_layers=1,
            num_heads=2, mlp_dim=256, atten_logit_cap=50.0)


def _classifier(enc, num_classes, bf16):
    return models.get_model(None, model_fn=lambda: encoders.FactorizedVideoClassifier(encoder_params=enc,
                                                                                      num_classes=num_classes),
                            fprop_dtype=torch.bfloat16 if bf16 else None)


def _head_f64(variables):
    flat = params.flatten(variables["params"])
    return {k: torch.from_numpy(np.asarray(v)).double() for k, v in flat.items() if not k.startswith("encoder/")}


@pytest.mark.parametrize("bf16", [False, True])
def test_forward_agrees_with_the_classifier_handle(cuda, bf16):
    """One finalized reduced-depth classifier, its own spatiotemporal_features, a probe built from the same head:
    the probe's logits and the handle's, each against the fp64 restatement on those features, at
    tests/test_gpu_classifier.py's bars (max-abs: fp32 2e-5, bf16 3e-2).  Not bitwise: the handle folds U on the
    host in fp64, the probe on the device in fp32."""
    enc = dict(models.CONFIGS["videoprism_v1_base"])
    enc.update(num_spatial_layers=1, num_temporal_layers=1)
    m = _classifier(enc, 40, bf16)
    var = params.synthetic_params(enc, 4, specs=m.param_specs())
    video = torch.from_numpy(np.random.default_rng(4).random((2, 2, 144, 144, 3), dtype=np.float32)).to(cuda)
    logits, out = m.apply(var, video, return_intermediate=["spatiotemporal_features"])
    feats = out["spatiotemporal_features"]
    assert feats.dtype == (torch.bfloat16 if bf16 else torch.float32) and feats.shape == (2, 2 * 64, 768)
    probe = AttentiveProbe.from_variables(var, num_heads=enc["num_heads"], device=cuda)
    with torch.no_grad():
        got = probe(feats)
    ref, _ = pr.forward(feats.double().cpu(), _head_f64(var))
    ep = (got.double().cpu() - ref).abs().max().item()
    eh = (logits.double().cpu() - ref).abs().max().item()
    print(f"forward {'bf16' if bf16 else 'fp32'}: probe {ep:.3e}, handle {eh:.3e} (|logits| max {ref.abs().max():.2f})")
    bar = 3e-2 if bf16 else 2e-5
    assert ep < bar and eh < bar


def test_training_round_trip(cuda):
    """40 Adam steps on a separable toy problem bring the cross-entropy below a tenth of its first value (the
    fp32 restatement under this recipe goes from 1.45 to 1e-4 on the CPU); the trained head, merged into a
    reduced-depth classifier's variables, gives through model.apply the logits the probe gives on that model's
    features (fp32 classifier bar, 2e-5 max-abs)."""
    B, S, D, H, C = 16, 96, 128, 2, 4
    g = torch.Generator().manual_seed(7)
    labels = torch.arange(B) % C
    direction = torch.randn(C, D, generator=g)
    where = (torch.rand(B, S, generator=g) < 0.25).float()[..., None]
    tokens = (torch.randn(B, S, D, generator=g) + 2.0 * where * direction[labels][:, None]).to(torch.bfloat16).to(cuda)
    probe = AttentiveProbe(D, H, C, device=cuda, seed=0)
    opt = torch.optim.Adam(probe.parameters(), lr=3e-3)
    losses = []
    for _ in range(40):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(probe(tokens), labels.to(cuda))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"training: loss {losses[0]:.4f} -> {losses[-1]:.3e}")
    assert losses[-1] < 0.1 * losses[0], losses

    m = _classifier(TINY, C, False)
    var = probe.merge_into(params.synthetic_params(TINY, 3, specs=m.param_specs()))
    video = torch.from_numpy(np.random.default_rng(5).random((3, 2, 4, 4, 3), dtype=np.float32)).to(cuda)
    logits, out = m.apply(var, video, return_intermediate=["spatiotemporal_features"])
    with torch.no_grad():
        again = probe(out["spatiotemporal_features"])
    err = (logits - again).abs().max().item()
    print(f"merged head through model.apply vs the probe on its features: max-abs {err:.3e} "
          f"(|logits| max {logits.abs().max().item():.2f})")
    assert logits.shape == (3, C) and err < 2e-5


def test_refusals_on_the_device(cuda):
    probe = AttentiveProbe(128, 2, 3, device=cuda)
    x = torch.zeros(2, 40, 128, device=cuda)
    with pytest.raises(NotImplementedError, match="frozen"):
        probe(x.clone().requires_grad_(True))
    # a workspace one byte short
    dims = (128, 2, 3)
    need = _native.op_probe_workspace_bytes(*dims, 2, 40)
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    tensors = {m: probe.get_parameter(path).detach() for m, path in _native.PROBE_LEAVES}
    logits = torch.empty(2, 3, device=cuda)
    with pytest.raises(ValueError, match=str(need)):
        _native.op_probe_forward(dims, tensors, x, logits, None, ws, ws_bytes=need - 1)
    _native.op_probe_forward(dims, tensors, x, logits, None, ws)
    grads = {m: torch.empty_like(t) for m, t in tensors.items()}
    with pytest.raises(ValueError, match=str(need)):
        _native.op_probe_backward(dims, tensors, x, torch.ones(2, 3, device=cuda), grads, ws, ws_bytes=need - 1)
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError, match="128"):
        AttentiveProbe(192, 3, 3, device=cuda)(torch.zeros(2, 40, 192, device=cuda))
