"""Every numerator tier of attention_long_bf16 (capped_exp16: LIN / QUAD / cubic / exact) and both forms of
attention_f32_mfma's capped_exp_f32x16, at caps 50 and 20, on inputs whose tiers are counted before the kernel runs.

Which tier a logit takes is decided per ballot group: one wave's 32 queries x the 32 keys of one tile.  In
attention_long_kernel.h a workgroup owns queries qb 256 .. + 255 and wave w of it rows q0 = qb 256 + 32 w .. + 31
(:68, loaded :77-81, the MFMA's B operand); a 64-key chunk is two tiles kt = 0, 1 of keys c 64 + kt 32 .. + 31
(:151, :174); capped_exp16 takes the tile's 16 values per lane and ballots over the wave (vp_common.h, mx and
__builtin_amdgcn_ballot_w64).  So group (g, j) of a (sequence, head) is rows 32 g .. 32 g + 31 x keys 32 j .. 32 j + 31.
In TAIL builds (S % 256 != 0) a row or key past S is read from row S - 1 (:77, :92) and its numerators are zeroed only
after the ballot (:171-179): the census clamps the same way, so the past-S entries of a partial group are copies of
row / key S - 1, which lies in that group.  attention_f32_mfma has the same 32 x 32 groups (attention.hip: q = qb 256 +
32 w + l32, keys c 128 + kt 32 ..).

Reference and bar (bf16 kernel), per element, no element left out.  With x_ij the fp64 logit of the bf16 inputs,
    n_ij = exp(cap tanh(x_ij / cap)),  rho_ij = n_ij rounded to bf16 (nearest even, as pack_bf16x2),
    O_id = sum_j rho_ij v_jd / sum_j n_ij
is what the kernel computes with exact numerators: it rounds P to bf16 for the P.V MFMA and sums the row in fp32.  The
kernel's bf16 output may differ by its own rounding, 2^-8 |O_id|, by the numerator error d_ij (in the row sum), and by
rounding flips of rho_ij where a numerator within d_ij of a bf16 tie lands on the other side (one bf16 ulp, at most
2^-7 n_ij).  With f_ij = 1 where n_ij (1 +- d_ij) rounds to another bf16 value than n_ij:
    B_id = 2^-8 |O_id| + (1 / sum_j n_ij) sum_j (d_ij + f_ij 2^-7) n_ij (|v_jd| + |O_id|)
    d_ij = the tier's bar of tests/test_capped_exp_cpu.py (polynomial tiers: fit * edge + 4 * 2^-24 * edge; exact form:
           exact_bar(x_ij)) + 2^-23 for v_exp_f32's result (1 ulp, which the polynomial bars leave out)
           + 64 * 2^-24 * sum_e |q_ie| |k_je|, the MFMA's fp32 accumulation of the logit (64 terms);
           where the group's largest |x| is within that accumulation error of a threshold, the worse of the two tiers.
Nothing in B is measured from the kernel.  It comes to a few 1e-4 where test_gpu_clip.py's bar for this kernel,
2^-8 (|ref| + max|v|), is 1.8e-2: that bar is the size of the bf16 rounding of P, which this reference makes itself.

fp32 kernel: the fp64 oracle and test_attention_f32_mfma's bar, 3e-5 max(1, |ref|).
"""

import numpy as np
import pytest
import torch

from attention_bar import _merge, _split, _thresholds as _long_thresholds, _unmerge, census, reference_and_bound
from oracle import videoprism_oracle as orc
from videoprism import _native as nat

pytestmark = pytest.mark.gpu

ALPHA = (0.25, 0.5, 0.8, 1.4)  # per 32-row query group, in runs
BETA = (0.5, 0.8, 1.4, 2.2)    # per 32-row key group, repeating


def _qkv(num_seq, S, heads, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    D = heads * 64
    q = torch.randn(num_seq * S, D, generator=g) * scale
    k = torch.randn(num_seq * S, D, generator=g) * scale
    v = torch.randn(num_seq * S, D, generator=g)
    return torch.cat([q, k, v], dim=1)


def _qkv_grid(num_seq, S, heads, seed):
    """q of query group g scaled by ALPHA (runs of ceil(groups / 4) groups), k of key group j by BETA[j % 4]: logit
    std 8 alpha beta from 1 to 25, so one query group meets several tiers along its keys."""
    qkv = _qkv(num_seq, S, heads, seed)
    D = heads * 64
    grp = torch.arange(S) // 32
    run = -(-int(grp[-1] + 1) // 4)
    a = torch.tensor(ALPHA)[grp // run].repeat(num_seq)[:, None]
    b = torch.tensor(BETA)[grp % 4].repeat(num_seq)[:, None]
    qkv[:, :D] *= a
    qkv[:, D:2 * D] *= b
    return qkv


def _for_cap(qkv, heads, cap):
    """The same tiers at another cap: q and k scaled by sqrt(cap / 50), so the logits scale with the thresholds."""
    qkv = qkv.clone()
    qkv[:, :2 * heads * 64] *= float(np.sqrt(cap / 50.0))
    return qkv


def _counts(may):
    """Groups per tier (a group that may take two tiers counts for neither)."""
    sure = may.sum(-1) == 1
    return [int((may[..., t] & sure).sum()) for t in range(may.shape[-1])], int(may[..., 0].size)


def _run_long(cuda, qkv, num_seq, S, heads, cap):
    """The kernel on bf16 q|k|v with the rows past the last sequence poisoned and the output prefilled (as
    test_attention_long_bf16_partial_blocks); returns the [num_seq S, D] output as fp64."""
    assert nat.dev_attention_choice(nat.ATT_OP, nat.VP_BF16, S, cap, False) == "LONG"
    D = heads * 64
    buf = torch.full((num_seq * S + 512, 3 * D), float("nan"), dtype=torch.bfloat16, device=cuda)
    buf[:num_seq * S] = qkv.to(cuda)
    out = torch.full((num_seq * S + 256, D), 7.0, dtype=torch.bfloat16, device=cuda)
    nat.op_attention(buf, num_seq, S, heads, cap, out=out)
    torch.cuda.synchronize()
    assert bool((out[num_seq * S:] == 7.0).all())  # no store past the last query
    return out[:num_seq * S].double().cpu().numpy()


def _check_long(cuda, qkv, num_seq, S, heads, cap, census_conditions, label):
    qkv = qkv.to(torch.bfloat16)
    q, k, v = _split(qkv, num_seq, S, heads)
    O, B, m, may = reference_and_bound(q, k, v, cap)
    counts, total = _counts(may)
    print(f"{label} cap {cap:g} S {S}: groups LIN / QUAD / cubic / exact {counts} of {total}")
    census_conditions(m, may, _long_thresholds(cap))  # conditions on the inputs, before the kernel runs
    out = _unmerge(_run_long(cuda, qkv, num_seq, S, heads, cap), num_seq, S, heads)
    err = np.abs(out - O)
    ratio = err / B
    # largest err / B over the rows of the query groups that meet each tier along their keys
    met = np.repeat(may.any(axis=2), 32, axis=1)[:, :S]  # [P, S, 4]
    per = [float(ratio[met[..., t]].max()) if met[..., t].any() else 0.0 for t in range(4)]
    print(f"{label} cap {cap:g} S {S}: max err {err.max():.3e}, median B {np.median(B):.3e}, err / B per tier met "
          + " / ".join(f"{p:.3f}" for p in per) + f", overall {ratio.max():.3f}")
    assert np.all(ratio <= 1.0), (ratio.max(), err.max())


def _straddles(t):
    """At least 20 % of the groups on each side of threshold t, and at least 10 within 3 % below and above it."""
    def cond(m, may, thr):
        sure = may.sum(-1) == 1
        below, above = int((may[..., t] & sure).sum()), int((may[..., t + 1] & sure).sum())
        assert below >= 0.2 * m.size and above >= 0.2 * m.size, (below, above, m.size)
        r = m / thr[t]
        assert int(((r >= 0.97) & (r <= 0.999)).sum()) >= 10 and int(((r >= 1.001) & (r <= 1.03)).sum()) >= 10
    return cond


def _all_tiers(m, may, thr):
    """Every tier holds at least 5 % of the groups, and at least half of the query groups meet three or more tiers
    along their keys, so one row sum mixes numerators of different forms."""
    counts, total = _counts(may)
    assert min(counts) >= 0.05 * total, (counts, total)
    sure = (may.sum(-1) == 1)[..., None]
    met = (may & sure).any(axis=2).sum(-1)  # [P, G]: tiers per query group
    assert int((met >= 3).sum()) * 2 >= met.size, (int((met >= 3).sum()), met.size)


# scale s of q and k at cap 50 -> logit std 8 s^2: 1.4 / 3.4 / 6.8, group maxima around 5 / 12 / 24
STRADDLE = {"LIN|QUAD": (0, 0.42), "QUAD|cubic": (1, 0.65), "cubic|exact": (2, 0.92)}


@pytest.mark.parametrize("cap", [50.0, 20.0])
@pytest.mark.parametrize("pair", sorted(STRADDLE))
def test_attention_long_straddling_a_threshold(cuda, pair, cap):
    t, s = STRADDLE[pair]
    S, num_seq, heads = 512, 1, 2
    qkv = _for_cap(_qkv(num_seq, S, heads, 100 + t, s), heads, cap)
    _check_long(cuda, qkv, num_seq, S, heads, cap, _straddles(t), pair)


@pytest.mark.parametrize("cap", [50.0, 20.0])
@pytest.mark.parametrize("S,num_seq", [(512, 1), (300, 4)])
def test_attention_long_all_tiers_in_one_row(cuda, S, num_seq, cap):
    """The separable grid; S = 300 has a partial last block of queries, a partial last chunk and a tail tile (keys
    288 .. 299 of 288 .. 319)."""
    heads = 2
    qkv = _for_cap(_qkv_grid(num_seq, S, heads, 7 + S), heads, cap)
    _check_long(cuda, qkv, num_seq, S, heads, cap, _all_tiers, "grid")


@pytest.mark.parametrize("cap", [50.0, 20.0])
def test_attention_f32_mfma_both_forms(cuda, cap):
    """attention_f32_mfma at both caps with groups on both sides of capped_exp_f32x16's 0.55 cap threshold."""
    S, num_seq, heads = 512, 1, 2
    assert nat.dev_attention_choice(nat.ATT_OP, nat.VP_F32, S, cap, False) == "F32_MFMA"
    qkv = _for_cap(_qkv(num_seq, S, heads, 11, 1.0), heads, cap)
    q, k, v = _split(qkv, num_seq, S, heads)
    thr = float(np.float32(0.55) * np.float32(cap))
    _, _, m, may = census(q, k, cap, [thr])
    counts, total = _counts(may)
    print(f"f32 cap {cap:g}: groups polynomial / exp form {counts} of {total}")
    assert min(counts) >= 0.2 * total, (counts, total)
    out = nat.op_attention(qkv.to(cuda), num_seq, S, heads, cap)
    torch.cuda.synchronize()
    ref = _merge(orc.capped_softmax_attention(q, k, v, cap), num_seq, S, heads)
    err = np.abs(out.double().cpu().numpy() - ref)
    bar = 3e-5 * np.maximum(1.0, np.abs(ref))
    print(f"f32 cap {cap:g}: max-abs {err.max():.3e}, largest err / bar {(err / bar).max():.3f}")
    assert np.all(err <= bar), err.max()
