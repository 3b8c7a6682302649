"""The 4-wave bf16 GEMM's scalar addressing (gemm_w4_kernel.h): the load stream's running piece
offsets, its per-tile bases, and the tile coordinates a workgroup steps from tile to tile.  None of it
may move an output bit, so every check is bitwise against a launch shape that takes another path
through the same arithmetic:

  * row ranges of at most CUs / 8 M-blocks (no workgroup owns two tiles, so no tile change in the load
    stream) against one launch in which some workgroups own two (the kernel documents row-range
    launches as bitwise one launch);
  * contiguous copies against column slices of wider tensors (row pitch != K);
  * the row-blocked A operand against the row-major pair;
  * the patch embedding staged from frames against the GEMM over patches gathered into the same K order.

fp64 bounds where stated are test_gemm_bf16_store's: one bf16 rounding, 2^-8 |ref| + 1e-3.
"""

import pytest
import torch

from videoprism import _native as nat

pytestmark = pytest.mark.gpu


def _bf(x):
    return x.to(torch.bfloat16)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ranges(M, rows):
    return [(r0, min(r0 + rows, M)) for r0 in range(0, M, rows)]


def _unblock(h):
    """Inverse of nat.to_row_blocked."""
    M, F = h.shape
    return h.reshape(M // 16, F // 32, 16, 32).permute(0, 2, 1, 3).reshape(M, F)


@pytest.mark.parametrize("epi", [nat.EPI_STORE, nat.EPI_RESID_BF16_ST, nat.EPI_BF16_LN_BLK])
@pytest.mark.parametrize("K", [128, 192])
def test_load_stream_across_tile_change(cuda, K, epi):
    """More tiles than CUs (M = 256 (CUs / 8 + 1), N = 2048: 8 (CUs / 8 + 1) tiles), two and three
    K-tiles (the S3 kernels' A ring wraps differently): the 2-stage kernel (epilogue 0), the S3 kernel
    with the peeled last K-tile (10) and the S3 row-blocked q|k|v store (19).  One launch == row ranges
    of CUs / 8 M-blocks, bit for bit; and within one bf16 rounding of fp64."""
    mb = _cus() // 8
    M, N = 256 * (mb + 1), 2048
    g = torch.Generator(device="cpu").manual_seed(K + epi)
    a = _bf(torch.randn(M, K, generator=g)).to(cuda)
    w = _bf(torch.randn(N, K, generator=g) / K ** 0.5).to(cuda)
    b = (torch.randn(N, generator=g) * 0.1).to(cuda)
    y = a.double() @ w.double().T
    rngs = _ranges(M, 256 * mb)
    if epi == nat.EPI_STORE:
        one = nat.op_gemm(a, w, b, epi)
        parts = torch.empty_like(one)
        for r0, r1 in rngs:
            nat.op_gemm(a[r0:r1], w, b, epi, out=parts[r0:r1])
        torch.cuda.synchronize()
        assert torch.equal(one, parts)
        ref, got = y + b.double(), one.double()
    elif epi == nat.EPI_RESID_BF16_ST:
        x0 = _bf(torch.randn(M, N, generator=g) * 2).to(cuda)
        one, parts = x0.clone(), x0.clone()
        st_one = torch.full((N // 128, M, 2), float("nan"), device=cuda)
        nat.dev_gemm_ln(a, w, b, epi, one, resid=one, st_part=st_one)
        st_parts = []
        for r0, r1 in rngs:
            st = torch.full((N // 128, r1 - r0, 2), float("nan"), device=cuda)
            nat.dev_gemm_ln(a[r0:r1], w, b, epi, parts[r0:r1], resid=parts[r0:r1], st_part=st)
            st_parts.append(st)
        torch.cuda.synchronize()
        assert torch.equal(one, parts)
        assert torch.equal(st_one, torch.cat(st_parts, 1))
        ref, got = x0.double() + y + b.double(), one.double()
    else:
        # (rstd, -mean rstd) rows as the epilogue takes them: any finite values pin the fold
        rs = torch.stack([torch.rand(M, generator=g) + 0.5, torch.randn(M, generator=g) * 0.1], 1).contiguous().to(cuda)
        c = (torch.randn(N, generator=g) * 0.1).to(cuda)
        perm = torch.from_numpy(nat.ffn1_blk_rows(N)).to(cuda)
        wp, bp, cp = w[perm].contiguous(), b[perm].contiguous(), c[perm].contiguous()
        one = torch.empty(M, N, device=cuda, dtype=torch.bfloat16)
        parts = torch.empty_like(one)
        nat.dev_gemm_ln(a, wp, bp, epi, one, ln_rs=rs, ln_c=cp)
        for r0, r1 in rngs:
            nat.dev_gemm_ln(a[r0:r1], wp, bp, epi, parts[r0:r1], ln_rs=rs[r0:r1], ln_c=cp)
        torch.cuda.synchronize()
        assert torch.equal(one, parts)
        ref = rs[:, :1].double() * y + rs[:, 1:].double() * c.double() + b.double()
        got = _unblock(one).double()
    err = (got - ref).abs()
    assert bool((err <= 2 ** -8 * ref.abs() + 1e-3).all()), float(err.max())


def test_grouped_tile_order_with_wrap(cuda):
    """ffn_layer1's kernel (EPI_GELU_LN_BLK without padded rows) in the N-grouped tile order (w4_ngrp = 6
    of 12 N-tiles) with 288 tiles, so workgroups step to a second tile across the M-block and group
    carries: bitwise the same launch over row ranges of 2048 rows (96 tiles each, grouped as well)."""
    M, N, K = 6144, 3072, 768
    g = torch.Generator(device="cpu").manual_seed(16)
    x = _bf(torch.randn(M, K, generator=g) * 2 + 0.5).to(cuda)
    w = _bf(torch.randn(N, K, generator=g) / K ** 0.5)
    b = torch.randn(N, generator=g) * 0.1
    c = w.double().sum(1).float()
    perm = torch.from_numpy(nat.ffn1_blk_rows(N))
    wp, bp, cp = w[perm].contiguous().to(cuda), b[perm].to(cuda), c[perm].to(cuda)
    rs = torch.empty(M, 2, device=cuda)
    nat.dev_ln_stats(x, M, K, rs, from_partials=False)
    one = torch.empty(M, N, device=cuda, dtype=torch.bfloat16)
    parts = torch.empty_like(one)
    nat.dev_gemm_ln(x, wp, bp, nat.EPI_GELU_LN_BLK, one, ln_rs=rs, ln_c=cp)
    for r0, r1 in _ranges(M, 2048):
        nat.dev_gemm_ln(x[r0:r1], wp, bp, nat.EPI_GELU_LN_BLK, parts[r0:r1], ln_rs=rs[r0:r1], ln_c=cp)
    torch.cuda.synchronize()
    assert torch.equal(one, parts)
    assert bool(one.float().abs().sum() > 0)


def test_row_pitch_not_k(cuda):
    """A and W as column slices of wider tensors (row pitch K + 64 elements, 16-byte aligned): bitwise
    the contiguous copies -- the piece step and the tile base are products of the pitch, not of K."""
    M, N, K = 512, 512, 192
    g = torch.Generator(device="cpu").manual_seed(3)
    big_a = _bf(torch.randn(M, K + 64, generator=g)).to(cuda)
    big_w = _bf(torch.randn(N, K + 64, generator=g) / K ** 0.5).to(cuda)
    b = (torch.randn(N, generator=g) * 0.1).to(cuda)
    a, w = big_a[:, :K], big_w[:, :K]
    assert a.stride(0) == K + 64 and w.stride(0) == K + 64
    strided = nat.op_gemm(a, w, b, nat.EPI_STORE)
    packed = nat.op_gemm(a.contiguous(), w.contiguous(), b, nat.EPI_STORE)
    torch.cuda.synchronize()
    assert torch.equal(strided, packed)
    ref = a.double() @ w.double().T + b.double()
    err = (strided.double() - ref).abs()
    assert bool((err <= 2 ** -8 * ref.abs() + 1e-3).all()), float(err.max())


@pytest.mark.parametrize("epi", [nat.EPI_RESID_FFN_BF16_ST_BLK, nat.EPI_RESID_FFN_BF16_BLK])
def test_row_blocked_a_across_tile_change(cuda, epi):
    """ffn_layer2 over the row-blocked hidden activation (the S3 path, K = 2048) with more tiles than
    CUs: bitwise the row-major pair, as test_ffn_pair_row_blocked_bitwise has it at small M."""
    M, N, K = 256 * (_cus() // 8 + 1), 2048, 2048
    g = torch.Generator(device="cpu").manual_seed(epi)
    h = _bf(torch.randn(M, K, generator=g)).to(cuda)
    w = _bf(torch.randn(N, K, generator=g) / K ** 0.5).to(cuda)
    b = (torch.randn(N, generator=g) * 0.1).to(cuda)
    r0 = _bf(torch.randn(M, N, generator=g)).to(cuda)
    hb = nat.to_row_blocked(h).contiguous()
    y_rm, y_bk = r0.clone(), r0.clone()
    if epi == nat.EPI_RESID_FFN_BF16_ST_BLK:
        st_rm = torch.full((N // 128, M, 2), float("nan"), device=cuda)
        st_bk = torch.full_like(st_rm, float("nan"))
        nat.dev_gemm_ln(h, w, b, nat.EPI_RESID_FFN_BF16_ST, y_rm, resid=y_rm, st_part=st_rm)
        nat.dev_gemm_ln(hb, w, b, epi, y_bk, resid=y_bk, st_part=st_bk)
        torch.cuda.synchronize()
        assert torch.equal(st_rm, st_bk)
    else:
        nat.dev_gemm_kernel(4, h, w, b, nat.EPI_RESID_FFN_BF16, y_rm, resid=y_rm)
        nat.dev_gemm_ln(hb, w, b, epi, y_bk, resid=y_bk)
        torch.cuda.synchronize()
    assert torch.equal(y_rm, y_bk)
    assert not torch.equal(y_rm, r0)


def test_patch_embed_from_frames_across_tile_change(cuda):
    """The patch embedding staged straight from 288 x 288 frames with 3 frames > CUs tiles (N = 768: three
    N-tiles per frame), so workgroups change frame in the load stream.  Bitwise against patchify + GEMM
    with the patches' columns gathered into the fused kernel's K order (K-tile py = pixel row py in eight
    8-value slots at value offsets min(8 j, 3P - 8), the slots past the row re-reading chunk 0; the same
    packed weights): the same products summed in the same order.  Against the two-kernel path in its
    natural column order the sums differ in fp32 order only, at most one bf16 ulp, as
    test_patch_embed_fused_from_frames bounds it."""
    P, D = 18, 768
    frames = _cus() // 3 + 1
    g = torch.Generator(device="cpu").manual_seed(frames)
    v = _bf(torch.rand(frames, 16 * P, 16 * P, 3, generator=g) * 4 - 1).to(cuda)
    kb = _bf(torch.randn(P * P * 3, D, generator=g) / (P * P * 3) ** 0.5)
    b = (torch.randn(D, generator=g) * 0.1).to(cuda)
    pos = (torch.randn(256, D, generator=g) * 0.1).to(cuda)
    wv = _bf(nat.video_patch_w(kb, P)).to(cuda)
    fused = torch.empty(frames * 256, D, device=cuda, dtype=torch.bfloat16)
    nat.dev_patch_embed(v, P, wv, b, pos, fused)
    patches = nat.op_patchify(v, P, 1024, torch.bfloat16)
    cpr = (3 * P + 7) // 8
    idx = torch.tensor([py * 3 * P + (0 if j >= cpr else min(8 * j, 3 * P - 8)) + e
                        for py in range(P) for j in range(8) for e in range(8)], device=cuda)
    gathered = nat.op_gemm(patches[:, idx].contiguous(), wv, b, nat.EPI_POS_BF16, pos=pos)
    wk = torch.zeros(D, 1024)
    wk[:, :P * P * 3] = kb.T
    two = nat.op_gemm(patches, _bf(wk).to(cuda), b, nat.EPI_POS_BF16, pos=pos)
    torch.cuda.synchronize()
    assert torch.equal(fused, gathered)
    d = (fused.double() - two.double()).abs()
    assert bool((d <= 2 ** -7 * two.double().abs() + 1e-5).all()), float(d.max())
