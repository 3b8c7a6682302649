"""MI355X op-level parity of the kernels in csrc/clip_kernels.hip that the LvT and classifier heads run after
the encoder -- pool_logits (scalar and MFMA), pool_stats / pool_wsum / pool_reduce, small_gemm,
small_gemm_splitk, ln_l2_rows, text_embed -- and of the whole pooler on caller-supplied tokens, each against a
plain fp64 restatement of the same operation (through the vp_dev_* entries; similarity has its test in
test_gpu_clip.py).

The end-to-end tests reach these kernels only with params.synthetic_params, whose pooler gives near-uniform
softmaxes over logits of about N(0, 1): a dropped U_lo row, a missing max subtraction, a chunk tail of one row
or a split-K slice read past its end all stay below their 1e-3 / 2e-5 embedding bars.  Here every kernel sees
the shapes where it changes path (chunk and tile edges, a half-empty last workgroup, K slices that are no
multiple of the 128-wide K step) and inputs that make the guarded term matter (logits of +-100, one-hot
softmaxes, biases of std 1).

Bars are the ones the project uses for fp32 math elsewhere (written at each test; the measured maxima are
printed and recorded in DESIGN.md §2).  Every output and scratch buffer starts as NaN; where an output has a
leading dimension larger than its width the padding columns must come back bit for bit."""

import math

import numpy as np
import pytest
import torch

from oracle import videoprism_oracle as orc
from videoprism import _native as nat
from videoprism import encoders, models, params

pytestmark = pytest.mark.gpu

F64 = orc.Numerics("f64")


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def _untouched(t):
    """Every element still holds the NaN prefill's bits."""
    return torch.equal(_bits(t), _bits(_nan(*t.shape, dtype=t.dtype)))


def _tokens(rows, D, bf16, seed):
    """N(0, 1) tokens on the host in the kernel's input dtype; the references read these very values."""
    x = torch.randn(rows, D, generator=_gen(seed))
    return x.to(torch.bfloat16) if bf16 else x


def _rel_bar(ref, bar):
    return bar * np.maximum(1.0, np.abs(ref))


# ------------------------------------------------------------------------------------------------------
# pool_logits: logits[g][h][s] = x[g*S+s] . U[h]
# ------------------------------------------------------------------------------------------------------
def _folded_keys(H, D, seed):
    """U ~ N(0, 4/D): logits of std 2 (|logit| <= 10) over N(0, 1) tokens."""
    return torch.randn(H, D, generator=_gen(seed)) * (2.0 / math.sqrt(D))


def _bf16_rows(bits):
    return torch.from_numpy((bits.astype(np.uint32) << 16).view(np.float32).copy()).double()


# D / 16 MFMA steps: 48 and 64 (the unrolled loop only), 20 (two unrolled steps + a tail of 4), 4 (tail only);
# (2, 96): 6 waves of 32 rows, so the second workgroup is half empty
@pytest.mark.parametrize("G,S", [(1, 32), (2, 96), (3, 256)])
@pytest.mark.parametrize("D,H", [(768, 12), (1024, 16), (320, 1), (64, 5)])
def test_pool_logits_mfma(cuda, D, H, G, S):
    """bf16 tokens on v_mfma_f32_32x32x16_bf16 against Ut = (U_hi | U_lo | 0) from the production split.
    (a) 2e-5 max(1, |ref|) against fp64 x . (hi + lo): exact bf16 products summed in fp32 (the split's own error
    is test_pool_split_cpu's).  (b) against fp64 x . U the error is at most 1/32 of what dropping U_lo costs on
    the same inputs: a correct kernel sits near 1/600 (the 2^-17 split against the 2^-9 of hi alone), a kernel
    that loses or misplaces U_lo at 1."""
    x = _tokens(G * S, D, True, 7 * D + S)
    U = _folded_keys(H, D, D + H)
    ut = nat.dev_pool_split_u(U.numpy())
    hi, lo = _bf16_rows(ut[:H]), _bf16_rows(ut[H:2 * H])
    logits = _nan(G, H, S)
    nat.dev_pool_logits(x.to(cuda), S, U.to(cuda), torch.from_numpy(ut.view(np.int16)).to(cuda), logits)
    torch.cuda.synchronize()
    out = logits.double().cpu().numpy()
    lay = lambda m: (x.double() @ m.T).reshape(G, S, H).permute(0, 2, 1).numpy()  # noqa: E731
    ref_split, ref_u, ref_hi = lay(hi + lo), lay(U.double()), lay(hi)
    err = np.abs(out - ref_split)
    lost = np.abs(ref_hi - ref_u).max()
    got = np.abs(out - ref_u).max()
    print(f"pool_logits mfma D={D} H={H} G={G} S={S}: max err {err.max():.3e} (|ref| max {np.abs(ref_split).max():.2f}); "
          f"vs fp64 U {got:.3e} = 1/{lost / got:.0f} of the U_lo term {lost:.3e}")
    assert np.all(err <= _rel_bar(ref_split, 2e-5)), err.max()
    assert got <= lost / 32, (got, lost)


def _scalar_cases():
    dh = [(64, 1), (768, 12), (1024, 16), (64, 16), (1024, 1)]
    out = [("f32", D, H, G, S) for D, H in dh for G, S in [(1, 7), (3, 49), (2, 196), (1, 300)]]
    out += [("bf16", D, H, G, S) for D, H in dh[:3] for G, S in [(3, 49), (1, 300), (2, 96)]]
    out += [("bf16_ut", D, H, 2, 196) for D, H in dh[:3]]  # Ut given, S % 32 != 0: falls back
    return out


@pytest.mark.parametrize("mode,D,H,G,S", _scalar_cases())
def test_pool_logits_scalar(cuda, mode, D, H, G, S):
    """The U-in-LDS kernel (fp32 tokens; bf16 tokens without Ut or with S % 32 != 0) against fp64 x . U at
    2e-5 max(1, |ref|).  No row count here is a multiple of 64 but 192, so the per-wave `break` runs."""
    x = _tokens(G * S, D, mode != "f32", 3 * D + S + H)
    U = _folded_keys(H, D, D + 2 * H)
    Ut = None
    if mode == "bf16_ut":
        Ut = torch.from_numpy(nat.dev_pool_split_u(U.numpy()).view(np.int16)).to(cuda)
    logits = _nan(G, H, S)
    nat.dev_pool_logits(x.to(cuda), S, U.to(cuda), Ut, logits)
    torch.cuda.synchronize()
    ref = (x.double() @ U.double().T).reshape(G, S, H).permute(0, 2, 1).numpy()
    err = np.abs(logits.double().cpu().numpy() - ref)
    print(f"pool_logits scalar {mode} D={D} H={H} G={G} S={S}: max err {err.max():.3e}")
    assert np.all(err <= _rel_bar(ref, 2e-5)), err.max()


@pytest.mark.parametrize("rows,S,D,H", [(8, 4, 96, 2), (8, 4, 1088, 2), (8, 4, 64, 17), (10, 3, 64, 2)])
def test_pool_logits_refusals(cuda, rows, S, D, H):
    """D % 64, D > 1024, H > 16, rows % S: VP_EINVAL and nothing launched."""
    x = torch.zeros(rows, D, device=cuda)
    U = torch.zeros(H, D, device=cuda)
    logits = _nan(rows * H + 64)
    with pytest.raises(ValueError, match="pool_logits"):
        nat.dev_pool_logits(x, S, U, None, logits)
    torch.cuda.synchronize()
    assert _untouched(logits)


# ------------------------------------------------------------------------------------------------------
# pool_softmax_wsum: stats = (max, 1 / sum exp(l - max)), z[g][h] = sum_s softmax(l)[s] x[g*S+s]
# ------------------------------------------------------------------------------------------------------
def _logit_patterns(G, H, S, seed):
    g = _gen(seed)
    normal = torch.randn(G, H, S, generator=g)
    wide = torch.rand(G, H, S, generator=g) * 200.0 - 100.0   # exp overflows without the max subtraction
    equal = torch.full((G, H, S), 3.25)                        # z = the mean of the rows
    onehot = torch.randn(G, H, S, generator=g)                 # one logit 60 above the rest: z = that row
    pos = torch.randint(0, S, (G, H), generator=g)
    if S in (257, 300):
        pos[:] = S - 1                                         # the last row of the last chunk
    top = onehot.max(-1).values + 60.0
    onehot.scatter_(2, pos[..., None], top[..., None])
    return {"normal": normal, "wide": wide, "equal": equal, "onehot": (onehot, pos)}


# S: below one 16-row step, one step, a step + 1, a chunk - 1, one chunk, a chunk + a single row, a chunk + a
# tail with two 16-row steps and 12 rows, four chunks
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("D,H", [(256, 1), (768, 12), (1024, 16)])
@pytest.mark.parametrize("S", [1, 16, 17, 255, 256, 257, 300, 1024])
def test_pool_softmax_wsum(cuda, S, D, H, bf16):
    """fp64 softmax and weighted sum.  z: 2e-5 max(1, |ref|); stats[0] (the row maximum) exact; stats[1] rtol
    1e-5; the probabilities sum to 1 within 1e-5, both rebuilt in fp64 from the logits and the kernel's stats
    (pool_stats_kernel's expf sum) and as pool_wsum_kernel itself forms them with __expf: column 0 of the
    tokens is 1, so z[..., 0] is the kernel's own sum of p."""
    worst = dict(z=0.0, s1=0.0, psum=0.0, ksum=0.0)
    for G in (1, 3):
        x = _tokens(G * S, D, bf16, 11 * S + D + G)
        x[:, 0] = 1.0
        xd = x.double().reshape(G, S, D)
        C = nat.dev_pool_chunks(S)
        assert C == (S + 255) // 256
        for name, l in _logit_patterns(G, H, S, S + D + G).items():
            pos = None
            if name == "onehot":
                l, pos = l
            stats, zpart, z = _nan(G * H, 2), _nan(G, C, H, D), _nan(G, H, D)
            nat.dev_pool_softmax_wsum(x.to(cuda), G, S, H, l.to(cuda), stats, zpart, z)
            torch.cuda.synchronize()
            ld = l.double()
            m = ld.max(-1, keepdim=True).values
            e = torch.exp(ld - m)
            p = e / e.sum(-1, keepdim=True)
            zref = torch.einsum("ghs,gsd->ghd", p, xd).numpy()
            zo = z.double().cpu().numpy()
            st = stats.double().cpu().reshape(G, H, 2)
            err = np.abs(zo - zref)
            assert np.all(err <= _rel_bar(zref, 2e-5)), (name, G, err.max())
            assert torch.equal(st[..., 0], m[..., 0]), (name, G)
            s1 = ((st[..., 1] - 1.0 / e.sum(-1)).abs() * e.sum(-1)).max().item()
            assert s1 <= 1e-5, (name, G, s1)
            psum = (torch.exp(ld - st[..., :1]) * st[..., 1:]).sum(-1)
            gap = (psum - 1.0).abs().max().item()
            kgap = np.abs(zo[..., 0] - 1.0).max()
            assert gap <= 1e-5 and kgap <= 1e-5, (name, G, gap, kgap)
            if name == "equal":
                assert np.all(np.abs(zo - xd.mean(1, keepdim=True).numpy()) <= _rel_bar(zref, 2e-5))
            if name == "onehot":
                rows = xd[torch.arange(G)[:, None], pos]            # [G, H, D]
                assert np.all(np.abs(zo - rows.numpy()) <= _rel_bar(zref, 2e-5))
            worst = dict(z=max(worst["z"], err.max()), s1=max(worst["s1"], s1), psum=max(worst["psum"], gap),
                         ksum=max(worst["ksum"], kgap))
    print(f"pool_softmax_wsum S={S} D={D} H={H} {'bf16' if bf16 else 'f32'}: z max err {worst['z']:.3e}, "
          f"stats[1] rel {worst['s1']:.3e}, |sum p - 1| rebuilt {worst['psum']:.3e} kernel {worst['ksum']:.3e}")


@pytest.mark.parametrize("D,H", [(320, 2), (256, 17)])
def test_pool_softmax_wsum_refusals(cuda, D, H):
    """D % 256, H > 16: VP_EINVAL and nothing launched."""
    G, S = 2, 4
    x = torch.zeros(G * S, D, device=cuda)
    l = torch.zeros(G, H, S, device=cuda)
    stats, zpart, z = _nan(G * H, 2), _nan(G, 1, H, D), _nan(G, H, D)
    with pytest.raises(ValueError, match="pool_softmax_wsum"):
        nat.dev_pool_softmax_wsum(x, G, S, H, l, stats, zpart, z)
    torch.cuda.synchronize()
    assert _untouched(stats) and _untouched(zpart) and _untouched(z)


# ------------------------------------------------------------------------------------------------------
# small_gemm / small_gemm_splitk: out[m][n] = A[m][:] . Wt[:][n] + bias[n], fp32
# ------------------------------------------------------------------------------------------------------
def _gemm_inputs(M, N, K, seed, batch=None):
    """A ~ N(0, 1), Wt ~ N(0, 1/K): outputs of O(1)."""
    g = _gen(seed)
    b = () if batch is None else (batch,)
    return (torch.randn(*b, M, K, generator=g), torch.randn(*b, K, N, generator=g) / math.sqrt(K),
            torch.randn(*b, N, generator=g))


def _padded(t, ld):
    """t [M, W] inside a NaN buffer [M, ld] on the device: a kernel that read a padding column would show it."""
    buf = _nan(t.shape[0], ld)
    buf[:, :t.shape[1]] = t.to(buf.device)
    return buf


# tile 32 rows x 64 columns, K step 128 split over 4 waves: below, at and above each, and several tiles of each
@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (31, 63, 127), (32, 64, 128), (33, 65, 129), (70, 400, 768),
                                   (1, 768, 768), (33, 1, 129), (70, 64, 1), (32, 400, 127), (31, 768, 128),
                                   (1, 65, 768), (70, 63, 129)])
def test_small_gemm(cuda, M, N, K, use_bias):
    """fp64 reference, 2e-5 max(1, |ref|); packed (lda = K, ldo = N) and padded (lda = K + 3 with NaN in the
    padding, ldo = N + 5 whose padding columns must survive)."""
    A, Wt, bias = _gemm_inputs(M, N, K, M + 3 * N + 7 * K)
    ref = (A.double() @ Wt.double() + (bias.double() if use_bias else 0.0)).numpy()
    b = bias.to(cuda) if use_bias else None
    for lda, ldo in ((K, N), (K + 3, N + 5)):
        out = _nan(M, ldo)
        nat.dev_small_gemm(_padded(A, lda), lda, 0, Wt.to(cuda), 0, b, 0, out, ldo, 0, M, N, K)
        torch.cuda.synchronize()
        err = np.abs(out[:, :N].double().cpu().numpy() - ref)
        assert np.all(err <= _rel_bar(ref, 2e-5)), (lda, ldo, err.max())
        assert _untouched(out[:, N:])
    print(f"small_gemm M={M} N={N} K={K} bias={use_bias}: max err {err.max():.3e} (|ref| max {np.abs(ref).max():.2f})")


@pytest.mark.parametrize("G,H,D,dp", [(3, 12, 768, 256), (2, 16, 1024, 64)])
def test_small_gemm_batched_value_projection(cuda, G, H, D, dp):
    """The strides of run_pooler's value projection: A = z [G][H*D] (lda = H*D, sA = D), Wt [H][D][dp],
    bias [H][dp], out = enc [G][H*dp] (ldo = H*dp, sO = dp), one batch entry per head."""
    g = _gen(G + H + D)
    z = torch.randn(G, H, D, generator=g)
    Wt = torch.randn(H, D, dp, generator=g) / math.sqrt(D)
    bias = torch.randn(H, dp, generator=g)
    out = _nan(G, H * dp)
    nat.dev_small_gemm(z.to(cuda), H * D, D, Wt.to(cuda), D * dp, bias.to(cuda), dp, out, H * dp, dp, G, dp, D, batch=H)
    torch.cuda.synchronize()
    ref = (torch.einsum("ghd,hdp->ghp", z.double(), Wt.double()) + bias.double()).reshape(G, H * dp).numpy()
    err = np.abs(out.double().cpu().numpy() - ref)
    print(f"small_gemm batched G={G} H={H} D={D} dp={dp}: max err {err.max():.3e}")
    assert np.all(err <= _rel_bar(ref, 2e-5)), err.max()


def _splitk(A, Wt, bias, splits, ldo=None):
    M, K = A.shape
    N = Wt.shape[1]
    ldo = ldo or N
    out, part = _nan(M, ldo), _nan(splits, M, N)
    nat.dev_small_gemm(A.cuda(), K, 0, Wt.cuda(), 0, None if bias is None else bias.cuda(), 0, out, ldo, 0, M, N, K,
                       splits=splits, part=part)
    torch.cuda.synchronize()
    return out, part


# K / splits: 512 and 384 (whole K steps), 96 (less than one step: a slice that read on to the step's end
# would count the next slice's rows twice), 384 with 2 slices, and 1 slice
@pytest.mark.parametrize("M,N,K,splits", [(1, 1024, 4096, 8), (33, 768, 3072, 8), (3, 768, 768, 8), (5, 64, 768, 2),
                                          (2, 256, 512, 1)])
def test_small_gemm_splitk(cuda, M, N, K, splits):
    """fp64 reference at 2e-5 max(1, |ref|), bias added once, the padding columns of out (ldo = N + 5) kept,
    and every partial equal to its own K slice's product."""
    A, Wt, bias = _gemm_inputs(M, N, K, M + N + K + splits)
    out, part = _splitk(A, Wt, bias, splits, ldo=N + 5)
    ref = (A.double() @ Wt.double() + bias.double()).numpy()
    err = np.abs(out[:, :N].double().cpu().numpy() - ref)
    Kc = K // splits
    pref = torch.einsum("mzk,zkn->zmn", A.double().reshape(M, splits, Kc), Wt.double().reshape(splits, Kc, N)).numpy()
    perr = np.abs(part.double().cpu().numpy() - pref)
    print(f"small_gemm_splitk M={M} N={N} K={K} splits={splits}: max err {err.max():.3e}, partials {perr.max():.3e}")
    assert np.all(err <= _rel_bar(ref, 2e-5)), err.max()
    assert np.all(perr <= _rel_bar(pref, 2e-5)), perr.max()
    assert _untouched(out[:, N:])


def test_small_gemm_splitk_same_bits_for_any_m(cuda):
    """small_gemm_splitk's documented claim: a row's bits do not depend on how many rows ride along.  Row m
    of an M = 33 run equals an M = 1 run on that row alone and that row in an M = 2 run, bit for bit."""
    M, N, K, splits = 33, 768, 3072, 8
    A, Wt, bias = _gemm_inputs(M, N, K, 5)
    Wt, bias = Wt.to(cuda), bias.to(cuda)
    full, _ = _splitk(A, Wt, bias, splits)
    for m in (0, 17, 31, 32):
        one, _ = _splitk(A[m:m + 1].contiguous(), Wt, bias, splits)
        assert torch.equal(_bits(one[0]), _bits(full[m])), m
        other = (m + 5) % M
        for rows, at in (([m, other], 0), ([other, m], 1)):
            two, _ = _splitk(A[rows].contiguous(), Wt, bias, splits)
            assert torch.equal(_bits(two[at]), _bits(full[m])), (m, rows)


def test_small_gemm_refusals(cuda):
    """K % splits != 0, split-K over a batch or without partials: VP_EINVAL and nothing launched."""
    M, N, K = 2, 64, 100
    A, Wt, out, part = torch.zeros(M, K, device=cuda), torch.zeros(K, N, device=cuda), _nan(M, N), _nan(8, M, N)
    with pytest.raises(ValueError, match="multiple of splits"):
        nat.dev_small_gemm(A, K, 0, Wt, 0, None, 0, out, N, 0, M, N, K, splits=8, part=part)
    with pytest.raises(ValueError, match="batch == 1"):
        nat.dev_small_gemm(A, K, 0, Wt, 0, None, 0, out, N, 0, M, N, K, batch=2, splits=4, part=part)
    with pytest.raises(ValueError, match="partials"):
        nat.dev_small_gemm(A, K, 0, Wt, 0, None, 0, out, N, 0, M, N, K, splits=4, part=None)
    with pytest.raises(ValueError, match="positive"):
        nat.dev_small_gemm(A, K, 0, Wt, 0, None, 0, out, N, 0, 0, N, K)
    torch.cuda.synchronize()
    assert _untouched(out) and _untouched(part)


# ------------------------------------------------------------------------------------------------------
# ln_l2_rows: LayerNorm and / or L2 normalisation of strided rows, fp32 out
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("D", [1, 255, 256, 257, 768, 1000, 1024])
def test_ln_l2_rows(cuda, D, bf16):
    """LayerNorm only (2e-5, test_layernorm's bar), L2 only (gamma = NULL) and both (1e-6, test_pool_l2's bar)
    against orc.layer_norm / orc.l2_normalize in fp64, over rows laid out as the text tower's CLS rows are:
    stride 3 D, starting at row 2 of each group of 3.  Five rows: random, constant (variance 0), all zero
    (L2 of it alone is 0 / sqrt(1e-12)), random, random; and the first row alone."""
    g = _gen(D)
    rows = 5
    x = torch.randn(rows, 3, D, generator=g) * 3 + 1
    x[1, 2] = 2.5
    x[2, 2] = 0.0
    if bf16:
        x = x.to(torch.bfloat16)
    gamma1p = 1 + torch.randn(D, generator=g) * 0.1
    beta = torch.randn(D, generator=g) * 0.1
    xd = x[:, 2].double().numpy()
    ln_ref = orc.layer_norm(xd, gamma1p.double().numpy() - 1.0, beta.double().numpy(), F64)
    refs = {"ln": ln_ref, "l2": orc.l2_normalize(xd), "ln_l2": orc.l2_normalize(ln_ref)}
    assert np.all(refs["l2"][2] == 0.0)
    xg = x.to(cuda)
    start = xg.reshape(-1)[2 * D:]          # the pointer of row 2 of group 0
    worst = {}
    for name, ref in refs.items():
        for n in (rows, 1):
            out = _nan(n, D)
            nat.dev_ln_l2_rows(start, 3 * D, n, D, gamma1p.to(cuda) if "ln" in name else None,
                               beta.to(cuda) if "ln" in name else None, "l2" in name, out)
            torch.cuda.synchronize()
            err = np.abs(out.double().cpu().numpy() - ref[:n])
            worst[name] = max(worst.get(name, 0.0), err.max())
            assert np.all(err <= (2e-5 if name == "ln" else 1e-6)), (name, n, err.max())
    print(f"ln_l2_rows D={D} {'bf16' if bf16 else 'f32'}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


def test_ln_l2_rows_refusals(cuda):
    x, out = torch.zeros(2, 1025, device=cuda), _nan(2, 1025)
    with pytest.raises(ValueError, match="ln_l2_rows"):
        nat.dev_ln_l2_rows(x, 1025, 2, 1025, None, None, True, out)
    with pytest.raises(ValueError, match="stride"):
        nat.dev_ln_l2_rows(x, 8, 2, 16, None, None, True, out)
    torch.cuda.synchronize()
    assert _untouched(out)


# ------------------------------------------------------------------------------------------------------
# text_embed: table[clamp(id)] * scale + pos, CLS appended; paddings with the CLS token's 0 appended
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,V", [(64, 7), (768, 1000), (1000, 50)])
@pytest.mark.parametrize("Q,L", [(1, 1), (3, 16), (2, 63), (2, 0)])
def test_text_embed(cuda, Q, L, D, V):
    """Table and output each in fp32 and bf16.  ids hold 0, V-1, V, V+5, -1 and -3 (clamped as
    oracle.text_encoder clamps them).  Rows t < L: |out - ref| <= 2^-23 (|table scale| + |pos|), one rounding
    of at most 2^-24 for the product and one for the sum; CLS rows the same with cls scale and no pos; a bf16
    output adds 2^-8 |ref|.  pad_out = [pad_in | 0] exactly."""
    g = _gen(Q + L + D + V)
    ids = torch.randint(0, V, (Q, L), generator=g, dtype=torch.int32)
    special = torch.tensor([V + 5, -3, 0, V - 1, V, -1], dtype=torch.int32)
    n = min(6, Q * L)
    ids.view(-1)[:n] = special[:n]
    pad_in = (torch.rand(Q, L, generator=g) < 0.5).float()
    table32 = torch.randn(V, D, generator=g) / math.sqrt(D)
    cls = torch.randn(D, generator=g) / math.sqrt(D)
    pos = torch.from_numpy(orc.sinusoidal_positions(max(L, 1), D).astype(np.float32))[:L]
    scale = float(np.float32(math.sqrt(D)))
    want_pad = torch.cat([pad_in, torch.zeros(Q, 1)], 1)
    clamped = ids.long().clamp(0, V - 1)
    worst = {}
    for table in (table32, table32.to(torch.bfloat16)):
        ts = table.double()[clamped] * scale                                # [Q, L, D]
        ref = torch.cat([ts + pos.double(), (cls.double() * scale).expand(Q, 1, D)], 1)
        mag = torch.cat([ts.abs() + pos.double().abs(), (cls.double() * scale).abs().expand(Q, 1, D)], 1)
        for odt in (torch.float32, torch.bfloat16):
            out, pad_out = _nan(Q, L + 1, D, dtype=odt), _nan(Q, L + 1)
            nat.dev_text_embed(ids.to(cuda), table.to(cuda), cls.to(cuda), pos.to(cuda) if L else None, scale, out,
                               pad_in.to(cuda), pad_out)
            torch.cuda.synchronize()
            assert torch.equal(pad_out.cpu(), want_pad)
            err = (out.double().cpu() - ref).abs()
            bar = 2.0 ** -23 * mag + (2.0 ** -8 * ref.abs() if odt == torch.bfloat16 else 0.0)
            assert bool((err <= bar).all()), (table.dtype, odt, (err - bar).max().item())
            worst[odt] = max(worst.get(odt, 0.0), (err / bar.clamp_min(1e-300)).max().item())
    print(f"text_embed Q={Q} L={L} D={D} V={V}: largest err / bar, fp32 out {worst[torch.float32]:.3f}, "
          f"bf16 out {worst[torch.bfloat16]:.3f}")


# ------------------------------------------------------------------------------------------------------
# the whole pooler (run_pooler with a finalized handle's packed weights) on caller-supplied tokens
# ------------------------------------------------------------------------------------------------------
_POOL_DIMS = {"base": ("videoprism_lvt_v1_base", "videoprism_v1_base"),
              "large": ("videoprism_lvt_v1_large", "videoprism_v1_large")}


def _pooler_logits(p, tokens, H, dp):
    """fp64 logits of the pooler without the key bias (the form the kernels use): [rows, H]."""
    pa = p["pooling_attention"]
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    q = np.einsum("d,dhj->hj", f(p["pooling_attention_query"])[0], f(pa["query"]["w"])) + f(pa["query"]["b"])
    q = q * (1.442695041 / math.sqrt(dp)) * orc.softplus(f(pa["per_dim_scale"]["per_dim_scale"]))
    U = np.einsum("dhj,hj->hd", f(pa["key"]["w"]), q)
    return tokens @ U.T


@pytest.fixture(scope="module", params=[(kind, size) for kind in ("clip", "classifier") for size in ("base", "large")],
                ids=lambda p: f"{p[0]}-{p[1]}")
def pooler_handles(request, cuda):
    """Reduced-depth handles (1+1 vision layers; 1 auxiliary and 1 text layer for the clip) at Base (D 768,
    12 heads) / Large (D 1024, 16 heads) dims, one per fprop dtype, over one synthetic tree whose pooler
    leaves are overridden: per_dim_scale holds 35, 31 (softplus(x) = x past 30), 0, -5, -20; key and value
    biases of std 1 (the key bias must cancel in the softmax, the value bias must come through once); the
    query (weights' input and bias alike) scaled so the largest |logit| over 1024 N(0, 1) probe tokens is 30
    for the fp32 handle (peaked softmax) and 8 for the bf16 one (|logit| <= 10 on the tests' tokens: there the
    2^-17 split of U alone moves a logit by about 3e-5, which would otherwise dominate)."""
    kind, size = request.param
    lvt, enc = _POOL_DIMS[size]
    if kind == "clip":
        cfg = dict(models.CONFIGS[lvt], vocabulary_size=16, num_spatial_layers=1, num_temporal_layers=1,
                   num_auxiliary_layers=1, num_unimodal_layers=1)
        make = lambda: encoders.FactorizedVideoCLIP(**cfg)  # noqa: E731
        specs, root = params.clip_leaf_specs(cfg), "contrastive_vision_pooler"
    else:
        cfg = dict(models.CONFIGS[enc], num_spatial_layers=1, num_temporal_layers=1)
        make = lambda: encoders.FactorizedVideoClassifier(encoder_params=cfg, num_classes=3)  # noqa: E731
        specs, root = params.classifier_leaf_specs(cfg, 3), "atten_pooler"
    D, H = cfg["model_dim"], cfg["num_heads"]
    hidden = 4 * D if kind == "clip" else D
    dp = hidden // H
    tree = params.synthetic_params(cfg, 31, specs=specs)["params"]
    rng = np.random.default_rng(32)
    base = dict(tree[root])
    pa = dict(base["pooling_attention"])
    pds = pa["per_dim_scale"]["per_dim_scale"].copy()
    pds[:5] = [35.0, 31.0, 0.0, -5.0, -20.0]
    pa["per_dim_scale"] = {"per_dim_scale": pds}
    for name in ("key", "value"):
        pa[name] = dict(pa[name], b=rng.standard_normal((H, dp)).astype(np.float32))
    base["pooling_attention"] = pa
    probe = np.random.default_rng(33).standard_normal((1024, D))
    out = {}
    for bf16, target in ((False, 30.0), (True, 8.0)):
        p = dict(base)
        a = np.float32(target / np.abs(_pooler_logits(base, probe, H, dp)).max())
        p["pooling_attention_query"] = base["pooling_attention_query"] * a
        p["pooling_attention"] = dict(pa, query=dict(pa["query"], b=pa["query"]["b"] * a))
        var = {"params": dict(tree, **{root: p})}
        m = models.get_model(None, model_fn=make, fprop_dtype=torch.bfloat16 if bf16 else None)
        out[bf16] = (m.engine(var, torch.cuda.current_device()), p, m)
    return dict(kind=0 if kind == "clip" else 1, name=f"{kind}-{size}", D=D, H=H, hidden=hidden, dp=dp, by_dtype=out)


# S: one chunk; a tail of 196; a chunk + 44 rows (S % 32 != 0: the scalar logits kernel in bf16 too); four chunks
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("G,S", [(1, 256), (3, 196), (2, 300), (1, 1024)])
def test_pooler_on_tokens(cuda, pooler_handles, G, S, bf16):
    """vp_dev_pooler against orc.atten_token_pooling in fp64 (which projects keys and values of every token,
    key bias included) on N(0, 1) tokens, rounded to bf16 first for the bf16 handles.  Bar: 3e-5 max(1, |ref|)
    on the LayerNorm output and on the L2-normalised output -- test_attention_f32's bar and reasoning: at
    |logit| of about 30 the fp32 rounding of a logit alone moves a probability by about 1e-5.  The Large clip
    handle (heads x dim_per_head = 4096) takes the 8-way split-K output projection, the others one launch."""
    hs = pooler_handles
    eng, p, _ = hs["by_dtype"][bf16]
    D, H = hs["D"], hs["H"]
    x = _tokens(G * S, D, bf16, 13 * S + G + D)
    xd = x.double().numpy()
    ref = orc.atten_token_pooling(xd.reshape(G, S, D), p, F64, H, hs["hidden"])[:, 0]
    lmax = np.abs(_pooler_logits(p, xd, H, hs["dp"])).max()
    refs = {False: ref, True: orc.l2_normalize(ref)}
    nbytes = nat.dev_pooler_scratch_bytes(hs["kind"], eng.handle(), G, S)
    worst = {}
    for do_l2 in (False, True):
        scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=cuda)   # NaN in every float
        dst = _nan(G, D)
        nat.dev_pooler(hs["kind"], eng.handle(), x.to(cuda), G, S, do_l2, dst, scratch)
        torch.cuda.synchronize()
        err = np.abs(dst.double().cpu().numpy() - refs[do_l2])
        worst[do_l2] = (err / _rel_bar(refs[do_l2], 3e-5)).max()
        print(f"pooler {hs['name']} {'bf16' if bf16 else 'f32'} G={G} S={S} {'l2' if do_l2 else 'ln'}: max err "
              f"{err.max():.3e} (|ref| max {np.abs(refs[do_l2]).max():.2f}, |logit| max {lmax:.1f}), "
              f"largest err / bar {worst[do_l2]:.3f}")
    assert worst[False] <= 1.0 and worst[True] <= 1.0, worst


def test_pooler_refusals(cuda, pooler_handles):
    hs = pooler_handles
    eng = hs["by_dtype"][False][0]
    with pytest.raises(ValueError, match="kind"):
        nat.dev_pooler_scratch_bytes(2, eng.handle(), 1, 16)
    with pytest.raises(ValueError, match="bad G or S"):
        nat.dev_pooler_scratch_bytes(hs["kind"], eng.handle(), 0, 16)
    n = nat.dev_pooler_scratch_bytes(hs["kind"], eng.handle(), 1, 16)
    dst = _nan(1, hs["D"])
    with pytest.raises(ValueError, match="scratch too small"):
        nat.dev_pooler(hs["kind"], eng.handle(), torch.zeros(16, hs["D"], device=cuda), 1, 16, False, dst,
                       torch.zeros(n - 256, dtype=torch.uint8, device=cuda))
    torch.cuda.synchronize()
    assert _untouched(dst)
