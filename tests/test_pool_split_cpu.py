"""The bf16 hi/lo split of the pooler's folded key vectors U (vp_clip.cpp pool_split_u, called by pack_pooler and
by vp_dev_pool_split_u): host code only, no GPU.

pool_logits_mfma_kernel multiplies bf16 tokens with the bf16 operand Ut [32][D] = (U_hi | U_lo | 0) and adds column
H + h to column h, so the fp32 U reaches the logits only as hi + lo.

The bar |U - (hi + lo)| <= 2^-17 |U| is a bound, not a margin: bf16 keeps 8 significant bits, so for |U| in
[2^e, 2^(e+1)) the residual r = U - hi (exact in fp32) is at most half an ulp of hi, 2^(e-8); unless it is that
power of two itself (then lo = r) it lies in a binade [2^f, 2^(f+1)) with f <= e - 9, where rounding to 8 bits
moves it by at most 2^(f-8) <= 2^(e-17) <= 2^-17 |U|.  Values just above a power of two come close to it
(measured 7.6e-6 = 0.998 * 2^-17), so a split that rounded either half any worse would cross the bar."""

import numpy as np
import pytest
import torch

from videoprism import _native as nat


def _decode(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _torch_bf16_bits(a):
    """torch's own round-to-nearest-even bf16 of a float32 array, as uint16 bits."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16)


def _wide_u(H, D, seed):
    """0.04 * exp(N(0, 1)) * sign: a wide dynamic range, plus exact zeros, exact bf16 values (lo must be 0)
    and values a hair off a bf16 rounding boundary."""
    rng = np.random.default_rng(seed)
    U = (0.04 * np.exp(rng.standard_normal((H, D))) * rng.choice([-1.0, 1.0], (H, D))).astype(np.float32)
    flat = U.reshape(-1)
    n = flat.size
    idx = rng.permutation(n)
    k = max(n // 16, 1)
    flat[idx[:k]] = 0.0
    flat[idx[k:2 * k]] = _decode(_torch_bf16_bits(flat[idx[k:2 * k]]))            # exact bf16 values
    ties = _decode(_torch_bf16_bits(flat[idx[2 * k:3 * k]])).view(np.uint32) | np.uint32(0x8000)
    flat[idx[2 * k:3 * k]] = ties.view(np.float32)                                  # exact ties (to even)
    flat[idx[3 * k:4 * k]] = (ties + np.uint32(1)).view(np.float32)                 # one ulp above the tie
    flat[0] = -0.0
    return U


@pytest.mark.parametrize("D", [64, 768, 1024])
@pytest.mark.parametrize("H", [1, 12, 16])
def test_pool_split_u(H, D):
    U = _wide_u(H, D, 100 * H + D)
    ut = nat.dev_pool_split_u(U)
    assert ut.shape == (32, D) and ut.dtype == np.uint16
    hi_bits, lo_bits = ut[:H], ut[H:2 * H]
    # bit for bit torch's round-to-nearest-even, of U and of the fp32 residual U - hi
    want_hi = _torch_bf16_bits(U)
    np.testing.assert_array_equal(hi_bits, want_hi)
    resid = U - _decode(want_hi)                                                     # fp32 subtraction (exact)
    np.testing.assert_array_equal(lo_bits, _torch_bf16_bits(resid))
    # rows 2H..31 are the MFMA operand's zero padding
    assert not ut[2 * H:].any()
    hi, lo = _decode(hi_bits).astype(np.float64), _decode(lo_bits).astype(np.float64)
    err = np.abs(U.astype(np.float64) - (hi + lo))
    nz = U != 0
    rel = float((err[nz] / np.abs(U[nz].astype(np.float64))).max())
    print(f"pool_split_u H={H} D={D}: max |U - (hi + lo)| / |U| = {rel:.3e} (bar {2.0 ** -17:.3e})")
    assert np.all(err <= 2.0 ** -17 * np.abs(U.astype(np.float64)))
    # exact zeros and exact bf16 values split to (U, 0)
    exact = _decode(want_hi) == U
    assert exact.sum() >= U.size // 16 and not (lo_bits[exact] & 0x7FFF).any()


def test_pool_split_u_refusals():
    lib = nat.load()
    U = np.zeros((17, 64), np.float32)
    ut = np.zeros((32, 64), np.uint16)
    p = lambda a: a.ctypes.data_as(nat.c_void_p)  # noqa: E731
    assert lib.vp_dev_pool_split_u(p(U), 17, 64, p(ut)) == nat.VP_EINVAL
    assert lib.vp_dev_pool_split_u(p(U), 0, 64, p(ut)) == nat.VP_EINVAL
    assert lib.vp_dev_pool_split_u(None, 1, 64, p(ut)) == nat.VP_EINVAL
    assert lib.vp_dev_pool_split_u(p(U), 1, 64, None) == nat.VP_EINVAL
    assert nat.dev_pool_chunks(1) == 1 and nat.dev_pool_chunks(256) == 1 and nat.dev_pool_chunks(257) == 2
