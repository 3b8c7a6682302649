"""Reference and per-element bar of the bf16 attention kernels that form exact-or-tiered numerators in fp32, round P
to bf16 for the P.V MFMA and keep the row sum in fp32.  A helper module (no tests): tests/test_gpu_attention_tiers.py
(attention_long_bf16, four numerator tiers), tests/test_gpu_attention_exact.py (the S <= 256 kernels, exact form only)
and tests/test_attention_bar_cpu.py import it.

For a query i, with x_ij the fp64 logit of the bf16 inputs and `allowed` the keys the masks leave (key paddings, the
causal mask, their merge):
    n_ij   = exp(cap tanh(x_ij / cap)) where allowed, 0 where not; a row with no allowed key gets n_ij = 1 for all S
             keys (what the kernels do, and what the reference's softmax of equal logits gives), with d_ij = 0 there;
    rho_ij = n_ij rounded to bf16 (nearest even, as pack_bf16x2);
    O_id   = sum_j rho_ij v_jd / sum_j n_ij.
The kernel's bf16 output may differ by its own rounding, 2^-8 |O_id|, by the numerator error d_ij (in the row sum),
and by rounding flips of rho_ij where a numerator within d_ij of a bf16 tie lands on the other side (one bf16 ulp, at
most 2^-7 n_ij).  With f_ij = 1 where n_ij (1 +- d_ij) rounds to another bf16 value than n_ij:
    B_id = 2^-8 |O_id| + (1 / sum_j n_ij) sum_j (d_ij + f_ij 2^-7) n_ij (|v_jd| + |O_id|)
           [ + (S + 4) 2^-24 (|O_id| + sum_j rho_ij |v_jd| / sum_j n_ij)      with fp32_sums ]
    d_ij = the tier's bar of tests/test_capped_exp_cpu.py (polynomial tiers: fit * edge + 4 * 2^-24 * edge + 2^-23 for
           v_exp_f32's result, 1 ulp, which the polynomial bars leave out; exact form: exact_bar(x_ij)) + extra_d
           + 64 * 2^-24 * sum_e |q_ie| |k_je|, the MFMA's fp32 accumulation of the logit (64 terms);
           where the group's largest |x| is within that accumulation error of a threshold, the worse of the two tiers.
The fp32_sums term is the worst-case fp32 accumulation of the row sum and of P.V, each over S terms ((S - 1) 2^-24
relative to sum_j n_ij and to sum_j rho_ij |v_jd|), plus the reciprocal (1 ulp, 2 * 2^-24), the product with it and the
rounding of the quotient's fp32 value before the bf16 conversion (2^-24 each, rounded up to (S + 4) in all).  It is
derived, not measured; it is what bounds a fully masked row (d = 0 there: the bar would otherwise be exactly bf16's
half ulp) and the near-uniform rows of small logits.  The long kernel's tests do not take it: their calls give the
arrays they gave before this module existed (tests/test_attention_bar_cpu.py pins that).
Nothing in B is measured from a kernel.
"""

import numpy as np

import test_capped_exp_cpu as cx

LONG_TIERS = ("LIN", "QUAD", "CUBIC", "EXACT")  # capped_exp16 (attention_long_bf16)
EXACT_ONLY = ("EXACT",)                        # capped_exp_exact alone (the S <= 256 kernels)


def _split(qkv, num_seq, S, heads):
    x = qkv.double().cpu().numpy().reshape(num_seq, S, 3, heads, 64)
    return [x[:, :, i].transpose(0, 2, 1, 3).reshape(num_seq * heads, S, 64) for i in range(3)]


def _merge(o, num_seq, S, heads):
    return o.reshape(num_seq, heads, S, 64).transpose(0, 2, 1, 3).reshape(num_seq * S, heads * 64)


def _unmerge(o, num_seq, S, heads):
    return o.reshape(num_seq, S, heads, 64).transpose(0, 2, 1, 3).reshape(num_seq * heads, S, 64)


def _group_max(a, S):
    """[P, S, S] -> [P, G, G] maxima over the ballot groups (32 queries x 32 keys), rows and keys past S clamped to
    S - 1 as the long kernel's loads are."""
    G = -(-S // 32)
    idx = np.minimum(np.arange(G * 32), S - 1)
    a = a[:, idx][:, :, idx]
    return a.reshape(a.shape[0], G, 32, G, 32).max(axis=(2, 4))


def census(q, k, cap, thresholds):
    """Per ballot group of fp64 logits of the (already rounded) inputs: the largest |x|, the largest accumulation
    error bound, and the tiers the group may take (a [P, G, G, len(thresholds) + 1] mask: one tier per group, two
    where the maximum is within the accumulation error of a threshold)."""
    S = q.shape[1]
    x = np.matmul(q, k.transpose(0, 2, 1))
    acc = 64 * 2.0 ** -24 * np.matmul(np.abs(q), np.abs(k).transpose(0, 2, 1))
    m, a = _group_max(np.abs(x), S), _group_max(acc, S)
    thr = np.asarray(thresholds, np.float64)
    lo = (m - a)[..., None] > thr   # certainly past threshold t
    hi = (m + a)[..., None] > thr   # possibly past it
    tier_lo, tier_hi = lo.sum(-1), hi.sum(-1)
    may = (np.arange(len(thr) + 1) >= tier_lo[..., None]) & (np.arange(len(thr) + 1) <= tier_hi[..., None])
    return x, acc, m, may


def _thresholds(cap, tiers=LONG_TIERS):
    """0.10 / 0.24 / 0.48 cap as fp32 products (make_cap_poly's x2, x1, x0) for the polynomial tiers in `tiers`:
    written here, not read from the header (tests/test_capped_exp_cpu.py pins the header's), so a moved threshold in
    the kernel is an error past B."""
    return [float(np.float32(cx.FACTORS[t]) * np.float32(cap)) for t in tiers if t != "EXACT"]


def _bf16_round(n):
    """fp64 -> the nearest bf16 value (8 significant bits), ties to even."""
    m, e = np.frexp(n)
    return np.ldexp(np.rint(m * 256.0), e - 8)


def reference_and_bound(q, k, v, cap, tiers=LONG_TIERS, allowed=None, extra_d=0.0, fp32_sums=False):
    """O and B of the module docstring for [P, S, 64] problems, and the census (group maxima of |x| and the tiers
    each group may take, in the order of `tiers`).

    tiers: the numerator forms a logit may take, a tail of LONG_TIERS (a group below a threshold takes the first).
    allowed: boolean [P, S, S] (query, key), or None for every key.
    extra_d: added to every d_ij.  fp32_sums: add the accumulation term."""
    assert tuple(tiers) == LONG_TIERS[len(LONG_TIERS) - len(tiers):] and tiers[-1] == "EXACT", tiers
    S = q.shape[1]
    x, acc, m, may = census(q, k, cap, _thresholds(cap, tiers))
    up = lambda g: np.repeat(np.repeat(g, 32, axis=1), 32, axis=2)[:, :S, :S]
    d = np.zeros_like(x)
    for t, name in enumerate(tiers):
        bar_t = cx.exact_bar(x, cap) if name == "EXACT" else cx.tier_bar(name, cap) + 2.0 ** -23
        d = np.maximum(d, np.where(up(may[..., t]), bar_t, 0.0))
    d = d + acc + extra_d
    n = np.exp(cap * np.tanh(x / cap))
    if allowed is not None:
        none = ~allowed.any(-1, keepdims=True)  # rows with no allowed key: uniform over all S keys, exactly
        n = np.where(none, 1.0, np.where(allowed, n, 0.0))
        d = np.where(none, 0.0, d)
    rho = _bf16_round(n)
    den = n.sum(-1, keepdims=True)
    O = np.matmul(rho, v) / den
    flip = (_bf16_round(n * (1 + d)) != rho) | (_bf16_round(n * (1 - d)) != rho)
    w = (d + flip * 2.0 ** -7) * n
    B = 2.0 ** -8 * np.abs(O) + (np.matmul(w, np.abs(v)) + np.abs(O) * w.sum(-1, keepdims=True)) / den
    if fp32_sums:
        B = B + (S + 4) * 2.0 ** -24 * (np.abs(O) + np.matmul(rho, np.abs(v)) / den)
    return O, B, m, may


def allowed_keys(P, S, key_pad=None, causal=False):
    """The keys each query may attend, [P, S, S] booleans: key j not padded (key_pad [P, S], 1 = padded), and with
    `causal` j <= i and query i not padded either -- the reference merges the causal mask with the paddings of both
    sides (the reference's merge_masks in compute_attention_masks_for_fprop), so a padded query keeps no key."""
    ok = np.ones((P, S, S), bool)
    if key_pad is not None:
        ok &= (np.asarray(key_pad) == 0)[:, None, :]
    if causal:
        ok &= np.tril(np.ones((S, S), bool))[None]
        if key_pad is not None:
            ok &= (np.asarray(key_pad) == 0)[:, :, None]
    return ok
