"""tests/attention_bar.py on the inputs of tests/test_gpu_attention_exact.py (tests/attention_cases.py), before a GPU sees
them.  CPU only.

The kernels' arithmetic is emulated in NumPy: fp32 logits of the bf16 inputs, capped_exp_exact numerators (its fp32
restatement in tests/test_capped_exp_cpu.py), the masks, P rounded to bf16, the row sum and P.V summed in fp32, 1 / sum,
the product, the bf16 output.
  (a) the emulation is inside B at every element of every case of the GPU file (largest err / B about 0.9): the inputs
      keep an arithmetically faithful kernel inside the bar;
  (b) three wrong emulations are past B somewhere in every family they apply to, and the share of elements the older
      bar 2^-8 (|ref| + max|v|) would have flagged is printed beside B's:
        - one extra key: row S - 1 counted twice, as `>` for `>=` in attn_seq_kernel's `slot - j*Sp >= S` would do.  It
          applies where S < Sp and no mask is given (the slot past S is a padded key under MASK, and past every query
          under the causal mask);
        - the numerator constants of cap 50 used at caps 20 and 5: every case at those caps with more than one key
          (a row with a single allowed key has one weight whatever its numerator is), the narrow family included;
        - the padding vector applied one key to the side: every masked case.
  (c) the long kernel's calls (four tiers, no fp32-sums term) give the arrays the function gave before it moved to
      attention_bar.py, bit for bit, on one of test_gpu_attention_tiers.py's inputs;
  (d) the masks: the unrounded reference sum_j n_ij v_jd / sum_j n_ij equals the oracle's masked attention.
"""

import numpy as np
import pytest
import torch

import test_capped_exp_cpu as cx
import attention_cases as gx
from attention_bar import _bf16_round, _split, allowed_keys, census, reference_and_bound
from oracle import videoprism_oracle as orc

f32 = np.float32


def emulate(q, k, v, cap, allowed, numerators=None, extra_key=False):
    """The kernels' arithmetic on [P, S, 64] fp64 copies of the bf16 inputs -> the bf16 output as fp64.
    numerators: x (fp32) -> fp32 numerators, capped_exp_exact at `cap` by default.  extra_key: key S - 1 twice."""
    if extra_key:
        k, v = np.concatenate([k, k[:, -1:]], 1), np.concatenate([v, v[:, -1:]], 1)
        if allowed is not None:
            allowed = np.concatenate([allowed, allowed[:, :, -1:]], 2)
    x = np.matmul(q.astype(f32), k.astype(f32).transpose(0, 2, 1))
    e = (numerators or (lambda t: cx.capped_exp_exact(t, cap)))(x).astype(f32)
    if allowed is not None:
        none = ~allowed.any(-1, keepdims=True)
        e = np.where(none, f32(1.0), np.where(allowed, e, f32(0.0))).astype(f32)
    rho = _bf16_round(e.astype(np.float64)).astype(f32)  # (bf16 values are fp32 values)
    lsum = e.sum(-1, keepdims=True, dtype=f32)
    y = np.matmul(rho, v.astype(f32))
    inv = (f32(1.0) / lsum).astype(f32)
    return _bf16_round((y * inv).astype(f32).astype(np.float64))


def _old_bar(O, v):
    return 2.0 ** -8 * (np.abs(O) + np.abs(v).max())


def _shares(out, O, B, v):
    err = np.abs(out - O)
    return float((err / B).max()), float((err > B).mean()), float((err > _old_bar(O, v)).mean())


@pytest.mark.parametrize("c", gx.ALL_CASES, ids=gx.case_id)
def test_faithful_emulation_is_inside_the_bar(c):
    _, kp, q, k, v, x, allowed = gx.problem(c)
    gx.check_inputs(c, x, kp)
    O, B = gx.reference(c, q, k, v, allowed)
    ratio = np.abs(emulate(q, k, v, c.cap, allowed) - O) / B
    print(f"{gx.case_id(c)}: emulation largest err / B {ratio.max():.3f}, median B {np.median(B):.3e}")
    assert np.all(ratio <= 1.0), ratio.max()


EXTRA_KEY_CASES = [c for c in gx.SEQ_CASES if c.S % 32 and c.mask is None and not c.causal]


@pytest.mark.parametrize("c", EXTRA_KEY_CASES, ids=gx.case_id)
def test_an_extra_key_is_past_the_bar(c):
    _, _, q, k, v, _, allowed = gx.problem(c)
    assert allowed is None
    O, B = gx.reference(c, q, k, v, None)
    worst, past, old = _shares(emulate(q, k, v, c.cap, None, extra_key=True), O, B, v)
    print(f"{gx.case_id(c)}: extra key, largest err / B {worst:.2f}, past B {past:.1%}, past the older bar {old:.1%}")
    assert worst > 1.0


WRONG_CAP_CASES = [c for c in gx.ALL_CASES if c.cap != 50.0]


@pytest.mark.parametrize("c", WRONG_CAP_CASES, ids=gx.case_id)
def test_cap_50_constants_at_another_cap_are_past_the_bar(c):
    _, _, q, k, v, _, allowed = gx.problem(c)
    O, B = gx.reference(c, q, k, v, allowed)
    out = emulate(q, k, v, c.cap, allowed, numerators=lambda t: cx.capped_exp_exact(t, 50.0))
    worst, past, old = _shares(out, O, B, v)
    print(f"{gx.case_id(c)}: cap 50's constants, largest err / B {worst:.2f}, past B {past:.1%}, "
          f"past the older bar {old:.1%}")
    if c.S > 1 and (allowed is None or bool((allowed.sum(-1) > 1).any())):
        assert worst > 1.0


SHIFTED_MASK_CASES = [c for c in gx.ALL_CASES if c.mask and c.S > 1]


@pytest.mark.parametrize("c", SHIFTED_MASK_CASES, ids=gx.case_id)
def test_paddings_one_key_to_the_side_are_past_the_bar(c):
    _, kp, q, k, v, _, allowed = gx.problem(c)
    O, B = gx.reference(c, q, k, v, allowed)
    kpp = np.repeat(np.roll(kp, 1, axis=1).reshape(c.num_seq, 1, c.S), c.heads, axis=1).reshape(-1, c.S)
    shifted = allowed_keys(q.shape[0], c.S, kpp, c.causal)
    if np.array_equal(shifted, allowed):
        pytest.fail("the case's paddings are invariant under the shift: choose others")
    worst, past, old = _shares(emulate(q, k, v, c.cap, shifted), O, B, v)
    print(f"{gx.case_id(c)}: shifted paddings, largest err / B {worst:.3g}, past B {past:.1%}, "
          f"past the older bar {old:.1%}")
    assert worst > 1.0


def test_fused_probabilities_emulated():
    """Launch 0 of the fused pair on the temporal family at T = 16: fp32 logits and numerators, fp32 row sum,
    1 / sum, the product, bf16 -- inside fused_p_bar at every probability; with cap 50's constants at cap 20, past it."""
    for cap in (50.0, 20.0):
        c = gx.Case("TEMPORAL", "video", "mid", 16, 32, 3, cap, None, False)
        _, _, q, k, v, _, _ = gx.problem(c)
        x, p, bar = gx.fused_p_bar(q, k, cap)
        for wrong in (False, True):
            e = cx.capped_exp_exact(np.matmul(q.astype(f32), k.astype(f32).transpose(0, 2, 1)), 50.0 if wrong else cap)
            inv = (f32(1.0) / e.sum(-1, keepdims=True, dtype=f32)).astype(f32)
            P = _bf16_round((e * inv).astype(f32).astype(np.float64))
            worst = float((np.abs(P - p) / bar).max())
            print(f"fused P cap {cap:g}{' with cap 50 constants' if wrong else ''}: largest err / bar {worst:.3f}")
            assert worst > 1.0 if (wrong and cap != 50.0) else worst <= 1.0


def test_unpack_p_is_the_kernels_layout():
    """Lane lid = r16 + 16 g4 stores P[r16][4 g4 + r] at element 4 lid + r of the block (lane_off = 8 lid bytes)."""
    P = np.arange(2 * 256, dtype=np.float64).reshape(2, 16, 16)
    buf = np.zeros(2 * 256)
    for blk in range(2):
        for lid in range(64):
            for r in range(4):
                buf[blk * 256 + 4 * lid + r] = P[blk, lid % 16, 4 * (lid // 16) + r]
    assert np.array_equal(gx.unpack_p(buf, 2), P)


def _reference_and_bound_as_merged(q, k, v, cap):
    """reference_and_bound of tests/test_gpu_attention_tiers.py as it stood when the long kernel's tests were merged,
    kept here only to pin the generalised function to it."""
    S = q.shape[1]
    thr = [float(f32(cx.FACTORS[t]) * f32(cap)) for t in ("LIN", "QUAD", "CUBIC")]
    x, acc, m, may = census(q, k, cap, thr)
    bars = [cx.tier_bar(t, cap) + 2.0 ** -23 for t in ("LIN", "QUAD", "CUBIC")]
    up = lambda g: np.repeat(np.repeat(g, 32, axis=1), 32, axis=2)[:, :S, :S]
    d = np.zeros_like(x)
    for t in range(4):
        bar_t = bars[t] if t < 3 else cx.exact_bar(x, cap)
        d = np.maximum(d, np.where(up(may[..., t]), bar_t, 0.0))
    d = d + acc
    n = np.exp(cap * np.tanh(x / cap))
    rho = _bf16_round(n)
    den = n.sum(-1, keepdims=True)
    O = np.matmul(rho, v) / den
    flip = (_bf16_round(n * (1 + d)) != rho) | (_bf16_round(n * (1 - d)) != rho)
    w = (d + flip * 2.0 ** -7) * n
    B = 2.0 ** -8 * np.abs(O) + (np.matmul(w, np.abs(v)) + np.abs(O) * w.sum(-1, keepdims=True)) / den
    return O, B, m, may


@pytest.mark.parametrize("cap", [50.0, 20.0])
def test_long_kernel_bar_is_unchanged(cap):
    """test_attention_long_all_tiers_in_one_row's S = 300 input (partial groups, every tier)."""
    import test_gpu_attention_tiers as tiers  # (its input builders; the module imports the native package)
    S, num_seq, heads = 300, 4, 2
    qkv = tiers._for_cap(tiers._qkv_grid(num_seq, S, heads, 7 + S), heads, cap).to(torch.bfloat16)
    q, k, v = _split(qkv, num_seq, S, heads)
    new, old = reference_and_bound(q, k, v, cap), _reference_and_bound_as_merged(q, k, v, cap)
    for a, b in zip(new, old):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    tiers._all_tiers(new[2], new[3], tiers._long_thresholds(cap))  # and the census conditions hold on it


MASK_CASES = [c for c in gx.ALL_CASES if (c.mask or c.causal) and c.S in (1, 5, 16, 33, 100, 256) and c.cap == 20.0
              and c.family in ("wide", "mid")]


@pytest.mark.parametrize("c", MASK_CASES, ids=gx.case_id)
def test_allowed_keys_are_the_oracles_masks(c):
    _, kp, q, k, v, x, allowed = gx.problem(c)
    n = np.exp(c.cap * np.tanh(x / c.cap))
    none = ~allowed.any(-1, keepdims=True)
    n = np.where(none, 1.0, np.where(allowed, n, 0.0))
    mine = np.matmul(n, v) / n.sum(-1, keepdims=True)
    kpp = np.zeros(q.shape[:2]) if kp is None else np.repeat(kp.reshape(c.num_seq, 1, c.S), c.heads, 1).reshape(-1, c.S)
    ref = orc.masked_attention(q, k, v, c.cap, kpp, c.causal)
    assert np.abs(mine - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
