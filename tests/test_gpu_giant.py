"""The Giant encoder's widths on the GPU in fp32: 88-wide heads (1408 / 16) through the three fp32 attention
kernels, LayerNorm at D = 1408 = 11 x 128, and reduced-depth forwards at Giant's widths against the fp64 oracle.

Attention bar: test_gpu_kernels.test_attention_f32_mfma's, err <= 3e-5 max(1, |ref|).  The inputs are that
file's _qkv with 88-wide heads and q scaled by sqrt(64 / 88) more, so q.k over 88 values has the variance it
has over 64 there (logits reach |q.k| ~ 100 at scale 2 - 4, where the fp32 rounding of the logit alone moves a
probability ~1e-5 relative): plain fp32 attention on these inputs stays at or below 1.23e-5 on the CPU.
Forward bar: the project's fp32 bar, max-abs <= 1e-5 against oracle mode 'f64'.

Measured on an MI355X (2 + 1 layers, max-abs against 'f64'; beside it the oracle's own 'f32' NumPy graph on the
same inputs, the floor):
  288 x 288, T = 2   uniform 6.12e-6 (floor 3.65e-6)   normal 6.87e-6 (floor 3.90e-6)
  72 x 72, T = 3     uniform 5.37e-6 (floor 3.34e-6)   normal 7.25e-6 (floor 4.59e-6; spatial_features 6.84e-6)
These are with the two-chain fp32 GEMM that handles of Giant's widths run (gemm_f32.hip TWO, vp_internal.h
f32_two_chains).  On the one-chain kernel the same four cases measured 8.67e-6, 9.79e-6, 9.07e-6 and 1.135e-5, the
last outside the bar: a single k-ordered chain's error grows as sqrt(K), and Giant has K = 1408 and 6144 where Base
(6.2e-6 - 7.2e-6 on the same test) has 768 and 3072.  test_gemm_f32_two_chains pins the kernel itself."""

import numpy as np
import pytest
import torch

from oracle import videoprism_oracle as orc
from videoprism import _native as nat
from videoprism import models, params

pytestmark = pytest.mark.gpu

DH = 88
HEADS = 2
GUARD = 64  # poisoned rows behind the last sequence, in q|k|v and in o


def _qkv88(num_seq, S, seed, scale):
    g = torch.Generator(device="cpu").manual_seed(seed)
    D = HEADS * DH
    q = torch.randn(num_seq * S, D, generator=g) * scale * 0.125 * 8 * (64.0 / DH) ** 0.5
    k = torch.randn(num_seq * S, D, generator=g) * scale
    v = torch.randn(num_seq * S, D, generator=g)
    return torch.cat([q, k, v], dim=1)


def _split(qkv, num_seq, S):
    x = qkv.double().cpu().numpy().reshape(num_seq, S, 3, HEADS, DH)
    return tuple(x[:, :, i].transpose(0, 2, 1, 3).reshape(num_seq * HEADS, S, DH) for i in range(3))


def _merge(o, num_seq, S):
    return o.reshape(num_seq, HEADS, S, DH).transpose(0, 2, 1, 3).reshape(num_seq * S, HEADS * DH)


def _paddings(pad, num_seq, S):
    """test_attention_f32_mfma's: random keys with one fully padded sequence, or one fully padded frame."""
    if pad is None:
        return None
    if pad == "frame":
        kp = torch.zeros(num_seq, S)
        kp[num_seq - 1] = 1.0
        return kp
    g = torch.Generator(device="cpu").manual_seed(5)
    kp = (torch.rand(num_seq, S, generator=g) < 0.3).float()
    kp[-1] = 1.0
    return kp


def _run_op(cuda, qkv, num_seq, S, cap, kp, causal=None):
    """The op on q|k|v followed by GUARD rows of NaN, into an o whose last GUARD rows are NaN: a read past the last
    sequence poisons the result, a store past the last query shows in the band."""
    rows, D = num_seq * S, HEADS * DH
    buf = torch.full((rows + GUARD, 3 * D), float("nan"), device=cuda)
    buf[:rows] = qkv.to(cuda)
    out = torch.full((rows + GUARD, D), float("nan"), device=cuda)
    kpd = None if kp is None else kp.reshape(-1).to(cuda)
    if causal is None:
        nat.op_attention(buf, num_seq, S, HEADS, cap, key_pad=kpd, out=out, dim_per_head=DH)
    else:
        nat.op_attention_masked(buf, num_seq, S, HEADS, cap, key_pad=kpd, causal=causal, out=out, dim_per_head=DH)
    torch.cuda.synchronize()
    o = out.double().cpu().numpy()
    assert np.isnan(o[rows:]).all(), "store past the last query"
    assert np.isfinite(o[rows - 1]).all(), "last query's 88 columns"
    assert np.isfinite(o[:rows]).all()
    return o[:rows]


def _check(tag, o, ref):
    err = np.abs(o - ref)
    print(f"{tag}: max-abs {err.max():.3e}")
    assert np.all(err <= 3e-5 * np.maximum(1.0, np.abs(ref))), err.max()


def _check_uniform(o, qkv, kp, num_seq, S):
    """A sequence whose every key is padded: all logits equal, so uniform weights over all S keys in every tier
    (with the causal merge too: a padded query's row is fully masked) -- every row of o is the mean of v."""
    D = HEADS * DH
    v = qkv[:, 2 * D:].double().numpy().reshape(num_seq, S, D)
    for s in range(num_seq):
        if kp is not None and bool(kp[s].all()):
            assert np.abs(o[s * S:(s + 1) * S] - v[s].mean(axis=0)).max() <= 3e-5


# (S, num_seq, scale, paddings, cap, the kernel vp_dev_attention_choice names).  attention_f32 ("F32") runs its MFMA
# kernel from S = 128 with 0 < cap <= 50 and its generic kernel otherwise; past 256 keys the MFMA kernel is named itself.
ATTENTION_CASES = [
    # the MFMA kernel: whole blocks, paddings, and TAIL with two and three query blocks
    (128, 2, 1.0, None, 50.0, "F32"),
    (256, 3, 1.0, None, 50.0, "F32"),
    (256, 3, 4.0, "random", 50.0, "F32"),
    (300, 2, 2.0, "random", 50.0, "F32_MFMA"),
    (520, 1, 2.0, None, 50.0, "F32_MFMA"),
    (256, 3, 1.0, "frame", 50.0, "F32"),
    # the generic kernel
    (5, 3, 1.0, "random", 50.0, "F32"),
    (16, 5, 2.0, None, 50.0, "F32"),
    (100, 3, 2.0, "random", 50.0, "F32"),
    (200, 2, 1.0, None, 0.0, "F32"),
    (224, 1, 1.0, "random", 0.0, "F32"),      # its last S: K|V fill the LDS
    # past the generic kernel's LDS without a fast cap: the online-softmax kernel
    (225, 1, 1.0, None, 0.0, "MASKED"),
    (256, 2, 1.0, None, 0.0, "MASKED"),
    (300, 2, 1.0, "random", 0.0, "MASKED"),
]


@pytest.mark.parametrize("S,num_seq,scale,pad,cap,kernel", ATTENTION_CASES)
def test_attention_88(cuda, S, num_seq, scale, pad, cap, kernel):
    kp = _paddings(pad, num_seq, S)
    assert nat.dev_attention_choice(nat.ATT_OP, nat.VP_F32, S, cap, kp is not None, dim_per_head=DH) == kernel
    if kernel == "F32":  # which of attention_f32's two kernels the case is meant for
        assert S <= (256 if 0.0 < cap <= 50.0 and S >= 128 else 224)
    qkv = _qkv88(num_seq, S, 31 + S + num_seq, scale)
    o = _run_op(cuda, qkv, num_seq, S, cap, kp)
    q, k, v = _split(qkv, num_seq, S)
    kpp = None if kp is None else np.repeat(kp.numpy().reshape(num_seq, 1, S), HEADS, axis=1).reshape(-1, S)
    ref = _merge(orc.capped_softmax_attention(q, k, v, cap, kpp), num_seq, S)
    _check(f"88-wide S={S} scale {scale} pad {pad} cap {cap} ({kernel})", o, ref)
    _check_uniform(o, qkv, kp, num_seq, S)


@pytest.mark.parametrize("S,num_seq,scale,pad,cap", [(65, 3, 1.0, "random", 50.0), (300, 1, 1.0, None, 0.0)])
def test_attention_masked_causal_88(cuda, S, num_seq, scale, pad, cap):
    kp = _paddings(pad, num_seq, S)
    assert nat.dev_attention_choice(nat.ATT_TEXT, nat.VP_F32, S, cap, kp is not None, dim_per_head=DH) == "MASKED"
    qkv = _qkv88(num_seq, S, 77 + S, scale)
    o = _run_op(cuda, qkv, num_seq, S, cap, kp, causal=True)
    q, k, v = _split(qkv, num_seq, S)
    kpp = np.zeros((num_seq * HEADS, S)) if kp is None else \
        np.repeat(kp.numpy().reshape(num_seq, 1, S), HEADS, axis=1).reshape(-1, S)
    ref = _merge(orc.masked_attention(q, k, v, cap, kpp, True), num_seq, S)
    _check(f"88-wide causal S={S} pad {pad} cap {cap}", o, ref)
    _check_uniform(o, qkv, kp, num_seq, S)


def test_attention_88_bf16_is_refused(cuda):
    qkv = torch.zeros(16, 3 * HEADS * DH, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(NotImplementedError, match="dim_per_head"):
        nat.op_attention(qkv, 1, 16, HEADS, 50.0, dim_per_head=DH)
    with pytest.raises(NotImplementedError, match="dim_per_head"):
        nat.op_attention_masked(qkv, 1, 16, HEADS, 50.0, causal=True, dim_per_head=DH)


# 96 rows, and 45: not a multiple of the 8 (D = 1408) or 16 (D = 768) rows of a workgroup, nor of a wave's 2 or 4
@pytest.mark.parametrize("B,T,N", [(2, 3, 16), (1, 3, 15)])
@pytest.mark.parametrize("perm", [nat.PERM_NONE, nat.PERM_BTN_TO_BNT, nat.PERM_BNT_TO_BTN])
@pytest.mark.parametrize("in_bf16", [False, True])
@pytest.mark.parametrize("D", [1408, 768])
def test_layernorm_1408(cuda, D, in_bf16, perm, B, T, N):
    """test_gpu_kernels.test_layernorm at D = 11 x 128 (the last 128 columns on half a wave), fp32 out; 768 is the
    control."""
    g = torch.Generator(device="cpu").manual_seed(D + perm)
    x = (torch.randn(B * T * N, D, generator=g) * 3 + 1).to(cuda)
    if in_bf16:
        x = x.to(torch.bfloat16)
    scale = torch.randn(D, generator=g) * 0.1
    bias = torch.randn(D, generator=g) * 0.1
    add = torch.randn(T, D, generator=g).to(cuda) if perm == nat.PERM_BTN_TO_BNT else None
    rows = B * T * N
    out = nat.op_layernorm(x, (1 + scale).to(cuda), bias.to(cuda), torch.float32, perm, T, N, add)
    torch.cuda.synchronize()
    ref = orc.layer_norm(x.double().cpu().numpy(), scale.double().numpy(), bias.double().numpy(), orc.Numerics("f64"))
    if perm == nat.PERM_BTN_TO_BNT:
        ref = (ref.reshape(B, T, N, D).transpose(0, 2, 1, 3) + add.double().cpu().numpy()[None, None]).reshape(-1, D)
    elif perm == nat.PERM_BNT_TO_BTN:
        ref = ref.reshape(B, N, T, D).transpose(0, 2, 1, 3).reshape(-1, D)
    err = np.abs(out.double().cpu().numpy() - ref)
    print(f"layernorm D={D} rows {rows} perm {perm} in_bf16 {in_bf16}: max-abs {err.max():.3e}")
    assert np.all(err <= 2e-5), err.max()


def test_layernorm_1408_bf16_out_and_refusal(cuda):
    """bf16 out at 1408 (the bf16 bar of test_layernorm), and a width that is no multiple of 128."""
    D, rows = 1408, 45
    g = torch.Generator(device="cpu").manual_seed(3)
    x = (torch.randn(rows, D, generator=g) * 3 + 1).to(cuda)
    scale, bias = torch.randn(D, generator=g) * 0.1, torch.randn(D, generator=g) * 0.1
    out = nat.op_layernorm(x, (1 + scale).to(cuda), bias.to(cuda), torch.bfloat16)
    torch.cuda.synchronize()
    ref = orc.layer_norm(x.double().cpu().numpy(), scale.double().numpy(), bias.double().numpy(), orc.Numerics("f64"))
    err = np.abs(out.double().cpu().numpy() - ref)
    assert np.all(err <= 2 ** -8 * np.abs(ref) + 1e-5), err.max()
    with pytest.raises(NotImplementedError, match="128"):
        nat.op_layernorm(torch.zeros(4, 1408 + 64, device=cuda), torch.ones(1408 + 64, device=cuda),
                         torch.zeros(1408 + 64, device=cuda), torch.float32)


@pytest.mark.parametrize("K,epi", [(1408, nat.EPI_STORE), (6144, nat.EPI_RESID_FFN), (1408, nat.EPI_GELU)])
def test_gemm_f32_two_chains(cuda, K, epi):
    """The fp32 GEMM Giant-width handles run (two accumulation chains per output, vp_dev_gemm_kernel 34) at Giant's
    K against fp64: test_gemm_f32's bar (2e-5 on unit-variance sums), and, the chain being half as long, an rms
    error below the one-chain kernel's (33) on the same operands."""
    M, N = 256, 1408
    g = torch.Generator(device="cpu").manual_seed(K)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) * 0.1
    x = torch.randn(M, N, generator=g)
    pad = (torch.rand(M, generator=g) < 0.2).float()
    y = a.double() @ w.double().T + b.double()
    if epi == nat.EPI_GELU:
        ref = 0.5 * y * (1 + torch.erf(y / 2 ** 0.5)) * (1 - pad.double())[:, None]
    elif epi == nat.EPI_RESID_FFN:
        ref = x.double() + y * (1 - pad.double())[:, None]
    else:
        ref = y
    rms = {}
    for which in (33, 34):
        o = x.clone().to(cuda)
        nat.dev_gemm_kernel(which, a.to(cuda), w.to(cuda), b.to(cuda), epi, o,
                            resid=o if epi == nat.EPI_RESID_FFN else None,
                            rowpad=None if epi == nat.EPI_STORE else pad.to(cuda))
        torch.cuda.synchronize()
        err = (o.double().cpu() - ref).abs()
        rms[which] = float(err.pow(2).mean().sqrt())
        print(f"gemm_f32 kernel {which} K={K} epilogue {epi}: max-abs {float(err.max()):.3e} rms {rms[which]:.3e}")
        assert float(err.max()) < 2e-5
    assert rms[34] < rms[33]


# ---- reduced-depth forwards at Giant's widths ----

def _cfg(**kw):
    c = dict(models.CONFIGS["videoprism_v1_giant"])
    c.update(kw)
    return c


def _video(B, T, H, seed, dist="uniform"):
    rng = np.random.default_rng(seed)
    if dist == "uniform":
        return rng.random((B, T, H, H, 3), dtype=np.float32)
    return rng.normal(0.0, 0.1, (B, T, H, H, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def giant21():
    """2 spatial + 1 temporal layer at model_dim 1408, 16 heads, mlp_dim 6144: one parameter tree and one engine."""
    cfg = _cfg(num_spatial_layers=2, num_temporal_layers=1)
    var = params.synthetic_params(cfg, seed=1)
    mdl = models.get_model(None, model_fn=lambda: models.encoders.FactorizedEncoder(**cfg))
    return cfg, var, mdl


@pytest.mark.parametrize("dist", ["uniform", "normal"])
def test_giant_dims_f32(cuda, giant21, dist):
    """B = 1, T = 2, 288 x 288: the spatial attention (S = 256) on the MFMA kernel, the temporal (S = 2) on the
    generic one."""
    cfg, var, mdl = giant21
    assert nat.dev_attention_choice(nat.ATT_VIDEO, nat.VP_F32, 256, 50.0, False, dim_per_head=88) == "F32"
    video = _video(1, 2, 288, 3, dist)
    emb, _ = mdl.apply(var, video, train=False)
    ref, _ = orc.factorized_encoder(var["params"], video, cfg, mode="f64")
    err = np.abs(emb - ref)
    print(f"f32 giant-dims {dist} max-abs {err.max():.3e} mean-abs {err.mean():.3e}")
    assert emb.shape == (1, 2 * 256, 1408)
    assert err.max() <= 1e-5


@pytest.mark.parametrize("dist", ["uniform", "normal"])
def test_giant_dims_small_grid_paddings_f32(cuda, giant21, dist):
    """B = 2, T = 3, 72 x 72: S = 16, 96 rows padded to the GEMM's 128, one padded frame, spatial_features, the
    positional tables interpolated 16 x 16 -> 4 x 4 and 8 -> 3; NumPy and device input."""
    cfg, var, mdl = giant21
    video = _video(2, 3, 72, 5, dist)
    fp = np.zeros((2, 3), np.float32)
    fp[1, 2] = 1.0
    emb, out = mdl.apply(var, video, train=False, frame_paddings=fp, return_intermediate=["spatial_features"])
    ref, rout = orc.factorized_encoder(var["params"], video, cfg, mode="f64", frame_paddings=fp,
                                       return_intermediate=["spatial_features"])
    assert set(out) == {"spatial_features"} and emb.shape == (2, 3 * 16, 1408)
    e1, e2 = np.abs(emb - ref).max(), np.abs(out["spatial_features"] - rout["spatial_features"]).max()
    print(f"f32 giant-dims 72x72 {dist}: embeddings max-abs {e1:.3e}, spatial_features {e2:.3e}")
    assert e1 <= 1e-5 and e2 <= 1e-5
    demb, _ = mdl.apply(var, torch.from_numpy(video).to(cuda), train=False, frame_paddings=fp)
    np.testing.assert_array_equal(demb.cpu().numpy() if isinstance(demb, torch.Tensor) else demb, emb)


@pytest.mark.parametrize("H,T,kernel", [(72, 3, "F32"), (270, 2, "MASKED")])
def test_giant_dims_no_cap_f32(cuda, H, T, kernel):
    """atten_logit_cap = 0 (outside the fast range), 1 + 1 layers: 72 x 72 keeps both stacks on the generic kernel
    (S = 16 and 3); 270 x 270 is a 15 x 15 grid, S = 225, one past what the generic kernel's LDS holds at 88, so
    the spatial stack runs the online-softmax kernel end to end."""
    cfg = _cfg(num_spatial_layers=1, num_temporal_layers=1, atten_logit_cap=0.0)
    S = (H // 18) ** 2
    assert nat.dev_attention_choice(nat.ATT_VIDEO, nat.VP_F32, S, 0.0, False, dim_per_head=88) == kernel
    var = params.synthetic_params(cfg, seed=1)
    mdl = models.get_model(None, model_fn=lambda: models.encoders.FactorizedEncoder(**cfg))
    B = 2 if H == 72 else 1
    video = _video(B, T, H, 7)
    fp = np.zeros((B, T), np.float32)
    fp[B - 1, T - 1] = 1.0
    emb, _ = mdl.apply(var, video, train=False, frame_paddings=fp)
    ref, _ = orc.factorized_encoder(var["params"], video, cfg, mode="f64", frame_paddings=fp)
    err = np.abs(emb - ref)
    print(f"f32 giant-dims no cap {H}x{H} ({kernel}): max-abs {err.max():.3e}")
    assert err.max() <= 1e-5


def test_giant_bf16_is_refused(cuda):
    """The full Giant configuration in bf16: the library's refusal arrives as NotImplementedError before any weight
    is read (the leaves are zero-stride views, no 4.4 GB tree)."""
    mdl = models.get_model(None, model_fn=models.videoprism_v1_giant, fprop_dtype=torch.bfloat16)
    flat = {k: torch.zeros(()).expand(*shape) for k, shape in mdl.param_specs().items()}
    with pytest.raises(NotImplementedError, match="dim_per_head"):
        mdl.apply(flat, _video(1, 2, 72, 0), train=False)


def test_giant_dims_vs_reference_program(cuda):
    """The reference's own program as the yardstick (tests/golden/ref_giant_encoder.npz: its FactorizedEncoder run
    in float64 on the NumPy stand-ins, oracle/make_ref_fixtures.py): Giant widths, 1 + 1 layers, B = 2, T = 3,
    72 x 72, one padded frame, spatial_features.  fp32 only (bf16 is refused at 88-wide heads); this file's bar,
    max-abs <= 1e-5, on the recorded token rows and token means, 1408 x 1e-5 on the sums of the rows."""
    from ref_fixtures import Case
    c = Case("ref_giant_encoder", "giant_encoder")
    cfg, var, video, fp = c.cfg, c.seeded_variables(), c.video, c.inp["frame_paddings"].astype(np.float32)
    mdl = models.get_model(None, model_fn=lambda: models.encoders.FactorizedEncoder(**cfg))
    emb, out = mdl.apply(var, video, train=False, frame_paddings=fp, return_intermediate=True)
    plain, _ = mdl.apply(var, video, train=False)
    assert emb.shape == (2, 3 * 16, 1408)
    for key, got in (("out_padded/0", emb), ("out_padded/1/spatial_features", out["spatial_features"]),
                     ("out/0", plain)):
        for k, g, ref in c.records(key, got):
            err = np.abs(g - ref).max()
            print(f"f32 giant-dims vs reference program {k}: max-abs {err:.3e}")
            assert err <= (1408 * 1e-5 if k.endswith("@rowsums") else 1e-5), (k, err)
