"""MI355X tests of token paddings in the classifier head's training ops (vp_op_probe_forward_masked /
vp_op_probe_backward_masked, AttentiveProbe.forward(tokens, paddings)) against the fp64 restatement of
tests/probe_masked_restatement.py.

Shapes: tests/test_gpu_probe.py's CASES, the smallest that reach every branch of the kernels, each with paddings
chosen to reach the branches the mask adds (PADDINGS).  Bar of the parity test: that file's, ||g - g64||_2 <=
2e-5 ||g64||_2 for every leaf and for the logits (masking only removes terms from the sums), the key bias's gradient
exactly zero, and for bf16 tokens g64 on the production hi | lo split of U and dz.  The measured errors go to
profiles/probe_masked/grad_parity.txt.  Everything else here is bit for bit."""

import os

import pytest
import torch

import probe_masked_restatement as pm
import probe_restatement as pr
import stream_order as so
import test_gpu_probe as tp
import workspace_guard as wg
from videoprism import _native as nat
from videoprism import params
from videoprism.probe import AttentiveProbe, pad_tokens

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_TXT = os.path.join(ROOT, "profiles", "probe_masked", "grad_parity.txt")
BAR = tp.BAR
CASES = tp.CASES
F32_SMALL, F32_CHUNKS, F32_WIDE, BF16_MFMA, BF16_SCALAR = range(5)


def _paddings(i):
    """The paddings [B, S] (fp32, 1 = padded) of CASES[i]."""
    _, B, S, _, _, _ = CASES[i]
    pad = torch.zeros(B, S)
    g = torch.Generator().manual_seed(50 + i)
    if i == F32_SMALL:       # scattered, not a suffix
        pad[0, [1, 2, 7, 20, 21, 22, 38]] = 1.0
    elif i == F32_CHUNKS:    # clip 0: none; clip 1: the second 256-row chunk holds one valid row; clip 2: the whole
        pad[1, 257:] = 1.0   # first chunk is skipped and the 44-row tail is valid
        pad[2, :256] = 1.0
    elif i == F32_WIDE:      # about half, at random
        pad = (torch.rand(B, S, generator=g) < 0.5).float()
    elif i == BF16_MFMA:     # clip 0: two whole 32-row wave blocks and scattered singles; clip 1: 300 valid rows,
        pad[0, 64:128] = 1.0  # not a multiple of 32
        pad[0, [3, 200, 333, 511]] = 1.0
        pad[1, 300:] = 1.0
    else:                    # bf16 on the scalar kernels: scattered, a fully padded clip (the uniform softmax), a suffix
        pad[0] = (torch.rand(S, generator=g) < 0.3).float()
        pad[1] = 1.0
        pad[2, 150:] = 1.0
    return pad


def _head(p, H, cuda):
    return AttentiveProbe.from_variables(params.unflatten({k: v.float().numpy() for k, v in p.items()}), num_heads=H,
                                         device=cuda)


def _device_run(cuda, x, p, H, dlogits, pad):
    """(logits, {leaf: gradient}) on the CPU; pad None: the unmasked call."""
    probe = _head(p, H, cuda)
    logits = probe(x.to(cuda), None if pad is None else pad.to(cuda))
    logits.backward(dlogits.to(cuda))
    torch.cuda.synchronize()
    return logits.detach().cpu(), {k: v.grad.cpu() for k, v in probe.named_parameters()}


def _same_bits(a, b, what):
    la, ga = a
    lb, gb = b
    d = wg.first_difference(la, lb)
    assert d is None, f"{what}: logits: {d}"
    for k in ga:
        d = wg.first_difference(ga[k], gb[k])
        assert d is None, f"{what}: {k}: {d}"


@pytest.fixture(scope="module")
def parity_log():
    lines = []
    yield lines
    os.makedirs(os.path.dirname(PARITY_TXT), exist_ok=True)
    with open(PARITY_TXT, "w") as f:
        f.write("AttentiveProbe under token paddings on the GPU against the fp64 masked restatement: ||g - g64|| / "
                f"||g64|| per leaf (bar {BAR:g}).\nbf16 tokens: g64 is the restatement on the hi | lo split of U and "
                "dz.  'padded' counts the padded tokens of each clip.\n")
        f.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{'bf16' if c[0] else 'f32'}-B{c[1]}-S{c[2]}-D{c[3]}"
                                                       for c in CASES])
def test_masked_gradient_parity(cuda, parity_log, i):
    bf16, B, S, D, H, C = CASES[i]
    x, p, dlogits = tp._inputs(*CASES[i])
    pad = _paddings(i)
    logits, grads = _device_run(cuda, x, p, H, dlogits, pad)
    ref_logits, st = pm.forward(x.double(), p, pad, tp._split if bf16 else None)
    ref = pm.backward(p, st, dlogits.double())
    if i == BF16_SCALAR:  # the fully padded clip is the reference's uniform softmax, not zeros
        assert torch.equal(st["prob"][1], torch.full_like(st["prob"][1], 1.0 / S))
    head = (f"{'bf16' if bf16 else 'fp32'} B={B} S={S} D={D} H={H} C={C} padded "
            f"{[int(n) for n in pad.sum(1)]}")
    rel = lambda a, b: ((a.double() - b).norm() / b.norm()).item()  # noqa: E731
    errs = {"logits": rel(logits, ref_logits)}
    kb = f"{pr.PA}/key/b"
    for k, g in grads.items():
        assert g.shape == p[k].shape and g.dtype == torch.float32, k
        if k != kb:
            errs[k] = rel(g, ref[k])
    for k, e in errs.items():
        line = f"{head}  {k}: {e:.3e}"
        print(line)
        parity_log.append(line)
    # the paddings count: the unmasked logits are elsewhere
    plain, _ = pr.forward(x.double(), p, tp._split if bf16 else None)
    assert rel(plain, ref_logits) > 1e-3
    assert not grads[kb].any(), "the key bias's gradient is exactly zero"
    assert len(grads) == len(nat.PROBE_LEAVES)
    bad = {k: e for k, e in errs.items() if not e <= BAR}
    assert not bad, bad


@pytest.mark.parametrize("i", [F32_CHUNKS, BF16_MFMA], ids=["f32", "bf16-mfma"])
def test_padded_contents_are_never_observable(cuda, i):
    """NaN, +Inf and 3e38 in the padded tokens (no clip of these two cases is fully padded): the logits and every
    gradient hold the bits of the run with zeros there."""
    bf16, B, S, D, H, C = CASES[i]
    x, p, dlogits = tp._inputs(*CASES[i])
    pad = _paddings(i)
    assert not pad.all(1).any() and pad.any()
    hole = pad.bool()[..., None]
    want = _device_run(cuda, torch.where(hole, torch.zeros_like(x), x), p, H, dlogits, pad)
    assert all(bool(torch.isfinite(t).all()) for t in [want[0], *want[1].values()])
    for junk in (float("nan"), float("inf"), 3e38):
        got = _device_run(cuda, torch.where(hole, torch.full_like(x, junk), x), p, H, dlogits, pad)
        _same_bits(got, want, f"padded tokens = {junk}")


@pytest.mark.parametrize("i", [F32_CHUNKS, BF16_MFMA, BF16_SCALAR], ids=["f32", "bf16-mfma", "bf16-scalar"])
def test_zero_paddings_are_no_paddings(cuda, i):
    """The masked kernels with nothing padded form the same sums in the same order as the unmasked ones; paddings of
    any dtype arrive as fp32."""
    bf16, B, S, D, H, C = CASES[i]
    x, p, dlogits = tp._inputs(*CASES[i])
    want = _device_run(cuda, x, p, H, dlogits, None)
    for zeros in (torch.zeros(B, S), torch.zeros(B, S, dtype=torch.bool), torch.zeros(B, S, dtype=torch.int64),
                  torch.full((B, S), 0.5, dtype=torch.bfloat16)):   # 0.5 is not padded: the rule is > 0.5
        _same_bits(_device_run(cuda, x, p, H, dlogits, zeros), want, f"all-zero {zeros.dtype} paddings")


@pytest.mark.parametrize("i", [F32_CHUNKS, BF16_MFMA], ids=["f32", "bf16-mfma"])
def test_clips_do_not_see_each_others_paddings(cuda, i):
    bf16, B, S, D, H, C = CASES[i]
    x, p, _ = tp._inputs(*CASES[i])
    probe = _head(p, H, cuda)
    pad = _paddings(i)
    other = pad.clone()
    other[1] = 0.0
    other[1, 5:S // 2] = 1.0
    with torch.no_grad():
        a = probe(x.to(cuda), pad.to(cuda)).cpu()
        b = probe(x.to(cuda), other.to(cuda)).cpu()
    assert wg.first_difference(a[0], b[0]) is None
    assert wg.first_difference(a[1], b[1]) is not None   # clip 1's own logits did move
    if B > 2:
        assert wg.first_difference(a[2], b[2]) is None


@pytest.mark.parametrize("valid", [200, 257])
def test_suffix_padded_clip_is_the_clip_alone(cuda, valid):
    """One fp32 clip of 300 tokens with a padded suffix against its first `valid` tokens alone, both on the scalar
    pass 1: bit for bit, by construction.  A logit is a function of its own row; the padded rows add exp(..) = +0
    exactly to the softmax's sum in pool_stats_kernel (each thread's partial sum and the block's tree keep their
    order, and x + 0 == x); pass 2 skips them, so every chunk sum is formed from the same rows in the same order, and a
    chunk with no valid row adds an exact zero in pool_reduce; dl is 0 at them and the same holds for dU."""
    _, _, S, D, H, C = CASES[F32_CHUNKS]
    x, p, dlogits = tp._inputs(False, 1, S, D, H, C)
    tokens, pad = pad_tokens([x[0, :valid], x[0]])   # [2, 300, D]; row 0 is the suffix-padded clip
    assert pad[0].tolist() == [0.0] * valid + [1.0] * (S - valid) and not pad[1].any()
    got = _device_run(cuda, tokens[:1], p, H, dlogits, pad[:1])
    want = _device_run(cuda, x[:, :valid].contiguous(), p, H, dlogits, None)
    _same_bits(got, want, f"{valid} of {S} tokens valid against those {valid} alone")


def test_two_masked_runs_give_the_same_bits(cuda):
    for i in (BF16_SCALAR, BF16_MFMA):
        bf16, B, S, D, H, C = CASES[i]
        x, p, dlogits = tp._inputs(*CASES[i])
        pad = _paddings(i)
        _same_bits(_device_run(cuda, x, p, H, dlogits, pad), _device_run(cuda, x, p, H, dlogits, pad), "second run")


# ---------------------------------------------------------------------------------------------------------------
# the stream and workspace contracts, on the harnesses of tests/stream_order.py and tests/workspace_guard.py
# ---------------------------------------------------------------------------------------------------------------
Dm, Hm, Cm, Bm, Sm = 256, 4, 5, 2, 40   # the unmasked probe cases' shape (tests/test_gpu_workspace.py)


def _contract_paddings():
    pad = torch.zeros(Bm, Sm)
    pad[0, [0, 3, 4, 17, 30]] = 1.0
    pad[1, 23:] = 1.0
    return pad


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_masked_stream_contract(cuda, bf16):
    """Forward + backward masked in one chain: deferred inputs (the paddings are an input like the tokens: the
    poisoned ones are NaN, which reads as padded and faults nothing), then capture and replay."""
    dims = (Dm, Hm, Cm)
    head = pr.synthetic_head(Dm, Hm, Cm, 77)
    dt = torch.bfloat16 if bf16 else torch.float32
    g = torch.Generator().manual_seed(78)
    named = {m: so.staged(head[path].float().contiguous().to(cuda)) for m, path in nat.PROBE_LEAVES}
    named["tokens"] = so.staged(torch.randn(Bm, Sm, Dm, generator=g).to(dt).to(cuda))
    named["dlogits"] = so.staged(torch.randn(Bm, Cm, generator=g).to(cuda))
    named["paddings"] = so.staged(_contract_paddings().to(cuda))
    tensors = {m: named[m][0] for m, _ in nat.PROBE_LEAVES}
    x, dl, pad = named["tokens"][0], named["dlogits"][0], named["paddings"][0]
    ws = torch.empty(nat.op_probe_workspace_bytes(*dims, Bm, Sm), dtype=torch.uint8, device=cuda)
    logits, emb = torch.empty(Bm, Cm, device=cuda), torch.empty(Bm, Dm, device=cuda)
    grads = {m: torch.empty_like(t) for m, t in tensors.items()}
    outs = [logits, emb] + [grads[m] for m, _ in nat.PROBE_LEAVES]

    def call(stream):
        nat.op_probe_forward(dims, tensors, x, logits, emb, ws, stream=stream, paddings=pad)
        nat.op_probe_backward(dims, tensors, x, dl, grads, ws, stream=stream, paddings=pad)
        return tuple(outs)

    label = f"vp_op_probe_forward_masked+backward_masked D=256 H=4 C=5 B=2 S=40 {'bf16' if bf16 else 'f32'} tokens"
    failures = so.check_case(so.case_from(label, named, outs, lambda: [ws], call, capture=True),
                             torch.cuda.Stream(cuda))
    assert not failures, failures


def test_masked_workspace_contract(cuda):
    """vp_op_probe_forward_masked + two vp_op_probe_backward_masked in exactly vp_op_probe_workspace_bytes: guard
    bands, the four fills, the refusal one byte short, and the fp64 masked restatement at 2e-5."""
    dims = (Dm, Hm, Cm)
    g = torch.Generator().manual_seed(77)
    p = pr.synthetic_head(Dm, Hm, Cm, 77)
    tensors = {m: p[path].float().contiguous().to(cuda) for m, path in nat.PROBE_LEAVES}
    x64 = torch.randn(Bm, Sm, Dm, generator=g).to(torch.bfloat16).double()
    x = x64.float().to(cuda)
    dl64 = torch.randn(Bm, Cm, generator=g).float().double()
    dlogits = dl64.float().to(cuda)
    pad64 = _contract_paddings()
    pad = pad64.to(cuda)
    need = nat.op_probe_workspace_bytes(*dims, Bm, Sm)
    xs = torch.randn(3, 17, Dm, generator=g).to(cuda)
    dls = torch.randn(3, Cm, generator=g).to(cuda)
    pads = (torch.rand(3, 17, generator=g) < 0.5).float().to(cuda)

    def call(ws, x, dlogits, pad, backwards):
        logits = torch.empty(x.shape[0], Cm, device=cuda)
        emb = torch.empty(x.shape[0], Dm, device=cuda)
        nat.op_probe_forward(dims, tensors, x, logits, emb, ws, paddings=pad)
        grads = []
        for _ in range(backwards):
            gr_ = {m: torch.empty_like(t) for m, t in tensors.items()}
            nat.op_probe_backward(dims, tensors, x, dlogits, gr_, ws, paddings=pad)
            grads.append(gr_)
        return (logits, emb) + tuple(gr_[m] for gr_ in grads for m, _ in nat.PROBE_LEAVES)

    def run(ws):
        outs = call(ws, x, dlogits, pad, 2)
        n = len(nat.PROBE_LEAVES)
        for a, b, (m, _) in zip(outs[2:2 + n], outs[2 + n:], nat.PROBE_LEAVES):
            d = wg.first_difference(a, b)
            assert d is None, f"second backward on the same workspace: {m}: {d}"
        return outs

    def oracle(outs):
        ref_logits, st = pm.forward(x64, p, pad64)
        ref = pm.backward(p, st, dl64)
        rel = lambda a, b: ((a.double().cpu() - b).norm() / b.norm()).item()  # noqa: E731
        errs = {"logits": rel(outs[0], ref_logits)}
        for i, (m, path) in enumerate(nat.PROBE_LEAVES):
            if m == "key_b":
                assert not outs[2 + i].any(), "the key bias's gradient is exactly zero"
            else:
                errs[m] = rel(outs[2 + i], ref[path])
        assert max(errs.values()) <= 2e-5, errs
        return f"oracle largest relative error {max(errs.values()):.2e} (bar 2e-05)"

    case = wg.Case("vp_op_probe_forward_masked+backward_masked D=256 H=4 C=5 B=2 S=40 f32 tokens",
                   ("vp_op_probe_forward_masked", "vp_op_probe_backward_masked"), need, run,
                   lambda take: call(take(nat.op_probe_workspace_bytes(*dims, 3, 17)), xs, dls, pads, 1),
                   lambda: call(torch.empty(need + 4096, dtype=torch.uint8, device=cuda), x, dlogits, pad, 2),
                   oracle, pointers="any")
    wg.check_case(case, cuda)
    wg.check_short_slice(case, cuda)


def test_paddings_refusals_on_the_device(cuda):
    probe = AttentiveProbe(128, 2, 3, device=cuda)
    x = torch.zeros(2, 40, 128, device=cuda)
    for bad in (torch.zeros(2, 41, device=cuda), torch.zeros(3, 40, device=cuda), torch.zeros(80, device=cuda),
                torch.zeros(2, 40, 1, device=cuda)):
        with pytest.raises(ValueError, match="paddings"):
            probe(x, bad)
    with pytest.raises(ValueError, match="device"):
        probe(x, torch.zeros(2, 40))
    # paddings take no gradient, and the tokens' own refusals are unchanged
    pad = torch.zeros(2, 40, device=cuda, requires_grad=True)
    probe(x, pad).sum().backward()
    assert pad.grad is None
    with pytest.raises(NotImplementedError, match="frozen"):
        probe(x.clone().requires_grad_(True), torch.zeros(2, 40, device=cuda))
    torch.cuda.synchronize()
