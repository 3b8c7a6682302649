"""The fp8 gallery's storage format restated in torch on the CPU (DESIGN.md §4 "fp8 gallery"): what
vp_op_quantize_rows_f8 must write and what a stored row stands for.  A helper module, not a test module.

A row is D codes in OCP e4m3 (torch.float8_e4m3fn) and one fp32 scale 2^-e:
  amax  the largest magnitude among the row's finite elements
  e     the largest integer with amax * 2^e <= 448, from frexp and not from a logarithm: amax = m * 2^p with m in
        [0.5, 1) gives 9 - p where m <= 0.875 and 8 - p otherwise; clamped to [-100, 100]; 0 where amax is 0 or the
        row has no finite element
  code  RNE_e4m3(x * 2^e) (the product is exact, or underflows far below e4m3's smallest subnormal); the NaN code
        for a non-finite x
bf16 input is widened to fp32 first.
"""

import numpy as np
import torch

E4M3_MAX = 448.0
E_CLAMP = 100


def exponents(x):
    """e per row of x [N, D] (fp32 or bf16): int32 [N]."""
    x = x.to(torch.float32)
    mag = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x))
    amax = mag.max(dim=1).values
    m, p = torch.frexp(amax)  # amax = m * 2^p, m in [0.5, 1); (0, 0) for 0; exact for denormals too
    e = torch.where(m <= 0.875, 9 - p, 8 - p).clamp(-E_CLAMP, E_CLAMP)
    return torch.where(amax == 0, torch.zeros_like(e), e).to(torch.int32)


def quantize(x):
    """(codes float8_e4m3fn [N, D], scales fp32 [N]) of x [N, D], fp32 or bf16."""
    x = x.to(torch.float32)
    e = exponents(x)
    y = torch.ldexp(x, e[:, None])  # exact: a power of two within 2^+-100
    codes = y.to(torch.float8_e4m3fn)
    nan = torch.tensor([0x7f], dtype=torch.uint8).view(torch.float8_e4m3fn)
    codes = torch.where(torch.isfinite(x), codes.view(torch.uint8), nan.view(torch.uint8)).view(torch.float8_e4m3fn)
    scales = torch.ldexp(torch.ones_like(e, dtype=torch.float32), -e)
    return codes, scales


def dequantize(codes, scales, dtype=torch.float64):
    """The values the stored rows stand for: codes * scales[:, None], exact in bf16 and so in `dtype`."""
    if codes.dtype == torch.uint8:
        codes = codes.view(torch.float8_e4m3fn)
    return codes.to(torch.float64).mul(scales.to(torch.float64)[:, None]).to(dtype)


def decode_table():
    """float64 [256]: the value of every e4m3 code, spelled out from the format (NaN for 0x7f and 0xff)."""
    out = np.empty(256, dtype=np.float64)
    for b in range(256):
        s, ex, m = b >> 7, (b >> 3) & 15, b & 7
        if ex == 15 and m == 7:
            v = np.nan
        elif ex == 0:
            v = m * 2.0 ** -9
        else:
            v = (1 + m / 8) * 2.0 ** (ex - 7)
        out[b] = -v if s else v
    return out


def same_codes(a, b):
    """Codes equal by value, NaNs in the same places (the two NaN codes count as one; +0 and -0 do not differ in
    value, and neither changes a score)."""
    t = decode_table()
    va, vb = t[a.view(torch.uint8).cpu().numpy()], t[b.view(torch.uint8).cpu().numpy()]
    return np.array_equal(np.isnan(va), np.isnan(vb)) and np.array_equal(np.nan_to_num(va), np.nan_to_num(vb))


def unit_rows(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, d), generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.float32)
