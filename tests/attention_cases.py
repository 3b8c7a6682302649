"""The cases and input builders of tests/test_gpu_attention_exact.py (a helper module, no tests, no native library):
tests/test_attention_bar_cpu.py runs the same builders through a NumPy emulation before a GPU sees them.

Input families (logit std at cap 50; q and k scaled by sqrt(cap / 50) at other caps, as the long kernel's tests do):
    narrow     0.7   near-uniform rows, what synthetic parameters produce; every |x| < 0.10 cap
    mid        8     the spread of test_gpu_kernels' attention inputs
    wide       20    at least 20 % of the logits past 0.48 cap (a Gaussian of std 8 has 0.3 % there)
    saturated  32    |x| up to 4 cap, the end of the range exact_bar is pinned on (largest |x| past 3 cap)
Every family keeps max |x| <= 4 cap.  The wide share is 23 % in expectation, so a case of few logits (the temporal
kernel's 9 S^2) can miss 20 % by chance: make_qkv draws such a case again, from the next seed, until its own logits
meet the condition.  The choice looks at the inputs only, and check_inputs asserts the condition for every wide case,
S = 1 included (there: 2 of the 9 logits).
"""

import collections

import numpy as np
import torch

import test_capped_exp_cpu as cx
from attention_bar import EXACT_ONLY, _split, allowed_keys, reference_and_bound

FAMILY_STD = {"narrow": 0.7, "mid": 8.0, "wide": 20.0, "saturated": 32.0}
EXTRA_D = 2.0 ** -23
WIDE_EDGE, WIDE_SHARE = 0.48, 0.20

# kernel: the name dev_attention_choice must give; entry: "video" (op_attention) or "text" (op_attention_masked);
# mask: None or "pad"
Case = collections.namedtuple("Case", "kernel entry family S num_seq heads cap mask causal")


def case_id(c):
    return (f"{c.kernel}-{c.entry}-{c.family}-S{c.S}x{c.num_seq}-cap{c.cap:g}-{c.mask or 'nomask'}"
            + ("-causal" if c.causal else ""))


def _seed(c):
    """One seed per case: the two entry points get inputs of their own."""
    return (1000 * c.S + 10 * int(c.cap) + len(c.family) + (5 if c.mask else 0) + (3 if c.causal else 0)
            + (500000 if c.entry == "text" else 0))


def wide_share(x, cap):
    return float((np.abs(x) > WIDE_EDGE * cap).mean())


def make_qkv(c):
    """bf16 q|k|v [num_seq S, 3 D] of the case's family (wide: drawn again until the case's logits meet the share)."""
    D = c.heads * 64
    s = float(np.sqrt(FAMILY_STD[c.family] / 8.0 * c.cap / 50.0))
    for draw in range(50):
        g = torch.Generator(device="cpu").manual_seed(_seed(c) + 7919 * draw)
        q = torch.randn(c.num_seq * c.S, D, generator=g) * s
        k = torch.randn(c.num_seq * c.S, D, generator=g) * s
        v = torch.randn(c.num_seq * c.S, D, generator=g)
        qkv = torch.cat([q, k, v], dim=1).to(torch.bfloat16)
        if c.family != "wide":
            return qkv
        qd, kd, _ = _split(qkv, c.num_seq, c.S, c.heads)
        if wide_share(np.matmul(qd, kd.transpose(0, 2, 1)), c.cap) >= WIDE_SHARE:
            return qkv
    raise AssertionError(f"no draw of {case_id(c)} meets the wide condition")


def make_paddings(c):
    """fp32 [num_seq, S], 1 = padded key; None without a mask.  Random at 30 %, the last sequence fully padded; at
    S = 256 through the spatial kernel also sequence 1 with a single valid key."""
    if c.mask is None:
        return None
    g = torch.Generator(device="cpu").manual_seed(_seed(c) + 1)
    kp = (torch.rand(c.num_seq, c.S, generator=g) < 0.3).float()
    if c.kernel == "SPATIAL":
        kp[1] = 1.0
        kp[1, 77] = 0.0
    kp[-1] = 1.0
    return kp.numpy()


def problem(c):
    """(qkv, key paddings, q, k, v [P, S, 64] fp64, logits x, allowed or None) of a case."""
    qkv, kp = make_qkv(c), make_paddings(c)
    q, k, v = _split(qkv, c.num_seq, c.S, c.heads)
    kpp = None if kp is None else np.repeat(kp.reshape(c.num_seq, 1, c.S), c.heads, axis=1).reshape(-1, c.S)
    allowed = allowed_keys(q.shape[0], c.S, kpp, c.causal) if (kp is not None or c.causal) else None
    x = np.matmul(q, k.transpose(0, 2, 1))
    return qkv, kp, q, k, v, x, allowed


def reference(c, q, k, v, allowed):
    O, B, _, _ = reference_and_bound(q, k, v, c.cap, tiers=EXACT_ONLY, allowed=allowed, extra_d=EXTRA_D, fp32_sums=True)
    return O, B


def check_inputs(c, x, kp):
    """The conditions on the inputs, before any kernel runs."""
    ax = np.abs(x)
    assert ax.max() <= 4.0 * c.cap, ax.max()  # the range exact_bar is pinned on (tests/test_capped_exp_cpu.py)
    if c.family == "narrow":
        assert ax.max() < 0.10 * c.cap, ax.max()
    if c.family == "wide":
        assert wide_share(x, c.cap) >= WIDE_SHARE, wide_share(x, c.cap)
    if c.family == "saturated":
        assert ax.max() > 3.0 * c.cap, ax.max()
    if kp is not None:
        assert bool((kp[-1] == 1).all())  # a fully padded sequence: uniform rows
        if c.kernel == "SPATIAL":
            # partial paddings inside every 32-key tile of sequence 0 (the kernel's kp[key] select), one valid key
            tiles = kp[0].reshape(8, 32)
            assert bool(((tiles == 1).any(1) & (tiles == 0).any(1)).all())
            assert int((kp[1] == 0).sum()) == 1
        if c.causal:
            assert bool((kp[:-1] == 1).any())  # a padded query outside the fully padded sequence


# ---- spatial: 3 sequences x 3 heads (the reversed block order and the bid % heads split), every family at every cap
SPATIAL_CASES = [Case("SPATIAL", "video", fam, 256, 3, 3, cap, mask, False)
                 for fam in ("narrow", "mid", "wide", "saturated") for cap in (50.0, 20.0, 5.0) for mask in (None, "pad")]


def _seq_cases():
    """Sp = S rounded up to 32 / 64 / 128 / 256 holds 256 / Sp sequences per workgroup; num_seq leaves the last
    workgroup with fewer (Sp = 32: 11 = 8 + 3; 64: 5 = 4 + 1; 128: 3 = 2 + 1).  S = Sp - 1, Sp and Sp + 1 at every
    width, S = 256 through the text kind only (the video kind's S = 256 is the spatial kernel).  Both entry points
    get no mask and paddings (the same kernel variants on inputs of their own), the text one also causal and
    causal + paddings."""
    out = []
    for S in (17, 31, 32, 33, 64, 100, 127, 128, 129, 200, 255, 256):
        num_seq = 11 if S <= 32 else 5 if S <= 64 else 3 if S <= 128 else 2
        for cap in (50.0, 20.0):
            variants = [("text", None, False), ("text", "pad", False), ("text", None, True), ("text", "pad", True)]
            if S < 256:
                variants = [("video", None, False), ("video", "pad", False)] + variants
            for entry, mask, causal in variants:
                out.append(Case("SEQ", entry, "wide", S, num_seq, 2, cap, mask, causal))
    return out


SEQ_CASES = _seq_cases()
# ---- temporal: every S, 9 (sequence, head) pairs: two workgroups of 4 waves and a last one running a single wave
TEMPORAL_CASES = [Case("TEMPORAL", "video", "wide", S, 3, 3, cap, mask, False)
                  for S in range(1, 17) for cap in (50.0, 20.0, 5.0) for mask in (None, "pad")]
ALL_CASES = SPATIAL_CASES + SEQ_CASES + TEMPORAL_CASES


# ---- the fused temporal pair
def fused_p_bar(q, k, cap):
    """p_ij = n_ij / sum_j n_ij and the bar of launch 0's stored bf16 probabilities for [P, T, 64] problems:
        |P - p| <= 2^-8 p + p (d_ij + sum_j d_ij p_ij) + 24 2^-24 p
    the bf16 rounding of the stored value; the numerator's own error and the row sum's (a p-weighted mean of the
    d_ij); the fp32 sum of T <= 16 numerators (15 2^-24), the reciprocal (1 ulp, 2 2^-24), the product and slack."""
    x = np.matmul(q, k.transpose(0, 2, 1))
    d = cx.exact_bar(x, cap) + EXTRA_D + 64 * 2.0 ** -24 * np.matmul(np.abs(q), np.abs(k).transpose(0, 2, 1))
    n = np.exp(cap * np.tanh(x / cap))
    p = n / n.sum(-1, keepdims=True)
    return x, p, 2.0 ** -8 * p + p * (d + (d * p).sum(-1, keepdims=True)) + 24 * 2.0 ** -24 * p


def unpack_p(pbuf, blocks):
    """Launch 0's P buffer -> [blocks, query, key]: 512 B per (sequence, head) at block sq * heads + head; lane
    lid = r16 + 16 g4 writes its 8 B at lane_off = 8 lid (gemm_w4_kernel.h), the four bf16 P[query r16][key 4 g4 + r],
    r = 0 .. 3.  So element (g4, r16, r) of the block viewed as [4][16][4] is P[r16][4 g4 + r]."""
    return pbuf.reshape(blocks, 4, 16, 4).transpose(0, 2, 1, 3).reshape(blocks, 16, 16)
