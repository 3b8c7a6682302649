"""The S <= 256 bf16 attention kernels one element at a time: attn_spatial_kernel (S = 256), attn_seq_kernel
(16 < S <= 256, sequences packed into 256 slots, optionally causal), attn_temporal_kernel (S <= 16) and the fused
temporal pair of gemm_w4_kernel.h (EPI_QK_TATTN_LN writes P, EPI_V_TATTN_LN writes O).  All four form the numerators with
capped_exp_exact, round P to bf16 for the P.V MFMA and keep the row sum in fp32.

Reference and bar: tests/attention_bar.py with the exact form only, d_ij = exact_bar(x_ij) + 2^-23 + 64 2^-24 sum_e
|q_ie| |k_je|, the masks as `allowed`, and the fp32-accumulation term (S + 4) 2^-24 (|O| + sum_j rho_ij |v_jd| / sum_j
n_ij).  B has a median of 2e-4 to 4.4e-3 where the older tests' bar, 2^-8 (|ref| + max|v|), is 1.8e-2 to 2e-2.  Nothing
in B is measured from a kernel; tests/test_attention_bar_cpu.py proves on this file's own inputs that an arithmetically
faithful kernel stays inside B (largest err / B about 0.9) and that three wrong ones do not.

Every case asserts the kernel it reaches (dev_attention_choice) and its input conditions before the launch, poisons
the q|k|v rows past the last sequence with NaN, prefills the output and checks nothing past the last query is written,
and compares every element.

The cases, the input families and their conditions, and the fused pair's P layout: tests/attention_cases.py.
"""

import numpy as np
import pytest
import torch

from attention_bar import _split, _unmerge
from attention_cases import (SEQ_CASES, SPATIAL_CASES, TEMPORAL_CASES, Case, case_id, check_inputs, fused_p_bar, problem,
                             reference, unpack_p)
from videoprism import _native as nat

pytestmark = pytest.mark.gpu


def _choice_kind(c):
    return nat.ATT_OP if c.entry == "video" else nat.ATT_TEXT


def run_kernel(cuda, c, qkv, kp):
    """The case's kernel on q|k|v with the rows past the last sequence poisoned and the output prefilled; returns the
    [P, S, 64] output as fp64."""
    assert nat.dev_attention_choice(_choice_kind(c), nat.VP_BF16, c.S, c.cap, kp is not None) == c.kernel
    D, rows = c.heads * 64, c.num_seq * c.S
    buf = torch.full((rows + 512, 3 * D), float("nan"), dtype=torch.bfloat16, device=cuda)
    buf[:rows] = qkv.to(cuda)
    out = torch.full((rows + 256, D), 7.0, dtype=torch.bfloat16, device=cuda)
    kpd = None
    if kp is not None:
        kpd = torch.full((rows + 256,), float("nan"), device=cuda)
        kpd[:rows] = torch.from_numpy(kp).reshape(-1).to(cuda)
    if c.entry == "video":
        assert not c.causal
        nat.op_attention(buf, c.num_seq, c.S, c.heads, c.cap, key_pad=kpd, out=out)
    else:
        nat.op_attention_masked(buf, c.num_seq, c.S, c.heads, c.cap, key_pad=kpd, causal=c.causal, out=out)
    torch.cuda.synchronize()
    assert bool((out[rows:] == 7.0).all())  # no store past the last query
    return _unmerge(out[:rows].double().cpu().numpy(), c.num_seq, c.S, c.heads)


def _check(cuda, c):
    qkv, kp, q, k, v, x, allowed = problem(c)
    check_inputs(c, x, kp)
    O, B = reference(c, q, k, v, allowed)
    out = run_kernel(cuda, c, qkv, kp)
    bad = ~np.isfinite(out)
    err = np.where(bad, 0.0, np.abs(out - O))
    ratio = err / B
    print(f"{case_id(c)}: max err {err.max():.3e}, median B {np.median(B):.3e}, largest err / B {ratio.max():.3f}"
          + (f", {int(bad.sum())} values not finite" if bad.any() else ""))
    assert not bad.any() and np.all(ratio <= 1.0), (ratio.max(), err.max(), int(bad.sum()))


@pytest.mark.parametrize("c", SPATIAL_CASES, ids=case_id)
def test_spatial(cuda, c):
    _check(cuda, c)


@pytest.mark.parametrize("c", SEQ_CASES, ids=case_id)
def test_sequence_packed(cuda, c):
    _check(cuda, c)


@pytest.mark.parametrize("c", TEMPORAL_CASES, ids=case_id)
def test_temporal(cuda, c):
    _check(cuda, c)


# ---- the fused temporal pair
@pytest.mark.parametrize("cap", [50.0, 20.0])
def test_fused_temporal_pair(cuda, cap):
    """M = 512 rows (32 sequences of T = 16), D = 768.  The reference inputs are the bf16 q|k|v of the unfused
    EPI_BF16_LN GEMM: both paths round the same fold4 values to bf16 (gemm_w4_kernel.h fold2blk, fold_write); the
    precondition is asserted by holding the unfused temporal kernel on that q|k|v to B.  Launch 0: every stored
    probability against fused_p_bar.  Launch 1: O against sum_j P_ij v_jd formed in fp64 from the P launch 0 wrote,
    bar 2^-8 |O| + 20 2^-24 sum_j |P_ij| |v_jd| (bf16 rounding of the result; the MFMA's fp32 sum of 16 products), so
    a defect is attributed to one launch."""
    heads, S, M = 12, 16, 512
    D, nseq = heads * 64, M // S
    g = torch.Generator(device="cpu").manual_seed(int(cap))
    x = (torch.randn(M, D, generator=g) * 2 + 0.3).to(torch.bfloat16)
    w = torch.randn(3 * D, D, generator=g) / D ** 0.5
    w[:D] *= cap / 50.0  # logit std about 8 at cap 50 (the q rows would carry dh^-0.5; here they carry the spread)
    wp = w.to(torch.bfloat16)
    b = (torch.randn(3 * D, generator=g) * 0.1).float()
    cc = wp.double().sum(1).float()
    xc, wpc, bc, ccd = x.to(cuda), wp.to(cuda), b.to(cuda), cc.to(cuda)
    rs = torch.empty(M, 2, device=cuda)
    nat.dev_ln_stats(xc, M, D, rs, from_partials=False)
    qkv = torch.empty(M, 3 * D, device=cuda, dtype=torch.bfloat16)
    nat.dev_gemm_ln(xc, wpc, bc, nat.EPI_BF16_LN, qkv, ln_rs=rs, ln_c=ccd)
    torch.cuda.synchronize()
    q, k, v = _split(qkv, nseq, S, heads)
    xl, p, pbar = fused_p_bar(q, k, cap)
    print(f"fused cap {cap:g}: logits std {xl.std():.2f}, max |x| {np.abs(xl).max():.1f}")
    assert np.abs(xl).max() <= 4.0 * cap and xl.std() >= 0.1 * cap
    # the precondition: the unfused kernel on this q|k|v
    c = Case("TEMPORAL", "video", "fused", S, nseq, heads, cap, None, False)
    O, B = reference(c, q, k, v, None)
    o_u = run_kernel(cuda, c, qkv.cpu(), None)
    ru = np.abs(o_u - O) / B
    print(f"fused cap {cap:g}: unfused on the same q|k|v, largest err / B {ru.max():.3f}")
    # launch 0
    perm = torch.cat([torch.cat([torch.arange(h * 64, h * 64 + 64), D + torch.arange(h * 64, h * 64 + 64)])
                      for h in range(heads)]).to(cuda)
    blocks = nseq * heads
    pb = torch.full(((blocks + 4) * 256,), 7.0, device=cuda, dtype=torch.bfloat16)
    nat.dev_gemm_tattn(0, xc, wpc[perm].contiguous(), bc[perm].contiguous(), rs, ccd[perm].contiguous(), pb, heads, cap)
    torch.cuda.synchronize()
    assert bool((pb[blocks * 256:] == 7.0).all())  # no store past the last (sequence, head) block
    pg = unpack_p(pb[:blocks * 256].double().cpu().numpy(), blocks)
    rp = np.abs(pg - p) / pbar
    print(f"fused cap {cap:g} launch 0: max |P - p| {np.abs(pg - p).max():.3e}, largest err / bar {rp.max():.3f}")
    # launch 1
    of = torch.full((M + 256, D), 7.0, device=cuda, dtype=torch.bfloat16)
    nat.dev_gemm_tattn(1, xc, wpc[2 * D:].contiguous(), bc[2 * D:].contiguous(), rs, ccd[2 * D:].contiguous(), of,
                       heads, cap, p=pb)
    torch.cuda.synchronize()
    assert bool((of[M:] == 7.0).all())
    og = _unmerge(of[:M].double().cpu().numpy(), nseq, S, heads)
    ref = np.matmul(pg, v)
    obar = 2.0 ** -8 * np.abs(ref) + 20 * 2.0 ** -24 * np.matmul(np.abs(pg), np.abs(v))
    ro = np.abs(og - ref) / obar
    print(f"fused cap {cap:g} launch 1: max |O - P v| {np.abs(og - ref).max():.3e}, largest err / bar {ro.max():.3f}")
    # every figure is printed before the first assertion, so one run tells which of the three is off
    assert np.all(ru <= 1.0), ("unfused kernel on the same q|k|v", ru.max())
    assert np.all(np.isfinite(pg)) and np.all(rp <= 1.0), ("launch 0", rp.max())
    assert np.all(np.isfinite(og)) and np.all(ro <= 1.0), ("launch 1", ro.max())
