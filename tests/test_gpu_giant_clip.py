"""videoprism_lvt_v1_giant and videoprism_vc_v1_giant on the GPU in fp32: the pooler kernels at D = 1408 (and the
other widths the *_wide entry points add), the LayerNorm-then-residual kernel of norm_policy 'primer_hybrid', and
reduced-depth forwards of both models against fp64.

Op level: the input recipes and bars of test_gpu_clip_kernels.py (2e-5 max(1, |ref|) against fp64; every output
starts as NaN).  Model level: oracle mode 'f64' for the video side, tests/primer_restatement.py for the primer
text tower; L2-normalised video / frame / text embeddings 2e-5 in fp32 and 1e-3 in bf16 (test_gpu_clip.py),
spatiotemporal_features 1e-5 (test_gpu_giant.py), classifier logits and global_embeddings 2e-5
(test_gpu_classifier.py).  Each model test prints the error of the oracle's own 'f32' NumPy graph beside the
library's: the floor.

Measured on an MI355X (max-abs against fp64; in brackets the floor):
  Giant LvT (a) 72 x 72, T = 3    video 9.6e-8 (4.8e-8)  frames 1.0e-7 (5.5e-8)  text 9.5e-8 (6.2e-8)  st 5.06e-6 (3.35e-6)
  Giant LvT (b) 144 x 144, T = 5  video 1.2e-7 (3.9e-8)  frames 1.0e-7 (4.8e-8)  text 9.5e-8 (6.2e-8)  st 5.12e-6 (2.93e-6)
  Giant classifier (a)            logits 2.3e-6 (3.6e-6)  global_embeddings 2.0e-6 (1.2e-6)
  Giant classifier (b)            logits 1.9e-6 (1.0e-6)  global_embeddings 1.9e-6 (1.1e-6)
  primer text tower, Base widths  fp32 1.1e-7 (7.7e-8)    bf16 7.2e-4 (1.4e-3)
  layernorm_residual              <= 8.4e-7 in all eight cases; ln_l2_rows wide LayerNorm <= 4.9e-7"""

import numpy as np
import pytest
import torch

import primer_restatement as pr
from oracle import videoprism_oracle as orc
from test_gpu_clip import _text
from test_gpu_clip_kernels import (_bf16_rows, _bits, _folded_keys, _gen, _logit_patterns, _nan, _rel_bar, _tokens,
                                   _untouched)
from videoprism import _native as nat
from videoprism import encoders, models, params

pytestmark = pytest.mark.gpu

F64 = orc.Numerics("f64")
LIMIT = 1536  # vp::kPoolMaxD


# ------------------------------------------------------------------------------------------------------
# pool_logits, wide
# ------------------------------------------------------------------------------------------------------
# 1408: 22 column steps of 64 and, at 16 heads, 90,112 B of U in LDS (past the 64 KB default); 1088: 17 steps, a
# width that is no multiple of 128; H = 1 keeps U below 64 KB on the same kernel
@pytest.mark.parametrize("G,S", [(1, 7), (3, 49), (1, 300)])
@pytest.mark.parametrize("D,H", [(1408, 16), (1408, 1), (1088, 16), (1088, 1)])
@pytest.mark.parametrize("bf16", [False, True])
def test_pool_logits_wide(cuda, bf16, D, H, G, S):
    x = _tokens(G * S, D, bf16, 3 * D + S + H)
    U = _folded_keys(H, D, D + 2 * H)
    logits = _nan(G, H, S)
    nat.dev_pool_logits(x.to(cuda), S, U.to(cuda), None, logits, wide=True)
    torch.cuda.synchronize()
    ref = (x.double() @ U.double().T).reshape(G, S, H).permute(0, 2, 1).numpy()
    err = np.abs(logits.double().cpu().numpy() - ref)
    print(f"pool_logits wide {'bf16' if bf16 else 'f32'} D={D} H={H} G={G} S={S}: max err {err.max():.3e}")
    assert np.all(err <= _rel_bar(ref, 2e-5)), err.max()


# D / 16 MFMA steps: 88 = 11 unrolled groups of 8; 68 = 8 groups and a tail of 4
@pytest.mark.parametrize("D,H", [(1408, 16), (1408, 1), (1088, 16), (1088, 1)])
def test_pool_logits_wide_mfma(cuda, D, H):
    """bf16 tokens with Ut at S = 96 (S % 32 == 0: the MFMA kernel); test_pool_logits_mfma's two bars."""
    G, S = 2, 96
    x = _tokens(G * S, D, True, 7 * D + S)
    U = _folded_keys(H, D, D + H)
    ut = nat.dev_pool_split_u(U.numpy())
    hi, lo = _bf16_rows(ut[:H]), _bf16_rows(ut[H:2 * H])
    logits = _nan(G, H, S)
    nat.dev_pool_logits(x.to(cuda), S, U.to(cuda), torch.from_numpy(ut.view(np.int16)).to(cuda), logits, wide=True)
    torch.cuda.synchronize()
    out = logits.double().cpu().numpy()
    lay = lambda m: (x.double() @ m.T).reshape(G, S, H).permute(0, 2, 1).numpy()  # noqa: E731
    ref_split, ref_u, ref_hi = lay(hi + lo), lay(U.double()), lay(hi)
    err = np.abs(out - ref_split)
    lost, got = np.abs(ref_hi - ref_u).max(), np.abs(out - ref_u).max()
    print(f"pool_logits wide mfma D={D} H={H}: max err {err.max():.3e}; vs fp64 U {got:.3e}, U_lo term {lost:.3e}")
    assert np.all(err <= _rel_bar(ref_split, 2e-5)), err.max()
    assert got <= lost / 32, (got, lost)


@pytest.mark.parametrize("D", [LIMIT + 64, 1408 + 32, 2048])
def test_pool_logits_wide_refusals(cuda, D):
    rows, S, H = 8, 4, 2
    logits = _nan(rows * H + 64)
    with pytest.raises(ValueError, match="pool_logits"):
        nat.dev_pool_logits(torch.zeros(rows, D, device=cuda), S, torch.zeros(H, D, device=cuda), None, logits, wide=True)
    torch.cuda.synchronize()
    assert _untouched(logits)


# ------------------------------------------------------------------------------------------------------
# pool_softmax_wsum, wide
# ------------------------------------------------------------------------------------------------------
GUARD = 256  # poisoned floats behind zpart and z: two 128-wide half blocks


def _wsum(cuda, x, G, S, H, l, wide, guard=GUARD):
    """-> stats, zpart, z as the kernels left them, zpart and z with `guard` NaN floats behind them."""
    D = x.shape[1]
    C = nat.dev_pool_chunks(S)
    stats = _nan(G * H, 2)
    zpart, z = _nan(G * C * H * D + guard), _nan(G * H * D + guard)
    nat.dev_pool_softmax_wsum(x.to(cuda), G, S, H, l.to(cuda), stats, zpart, z, wide=wide)
    torch.cuda.synchronize()
    return stats, zpart, z


# D: five 256-column blocks and a half, no half block, a half block alone.  S: one row, a 16-row step + 1, one chunk,
# a chunk + a single row, a chunk + a tail of two steps and 12 rows
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("D,H", [(1408, 16), (1408, 1), (1280, 16), (1280, 1), (128, 16), (128, 1)])
@pytest.mark.parametrize("S", [1, 17, 256, 257, 300])
def test_pool_softmax_wsum_wide(cuda, S, D, H, bf16):
    """test_pool_softmax_wsum's checks on z and the stats, all four logit patterns; the floats behind zpart and z
    keep their bits, so the 128-wide last block wrote no column past D (the last head's row ends the buffer)."""
    worst = 0.0
    for G in (1, 3):
        x = _tokens(G * S, D, bf16, 11 * S + D + G)
        x[:, 0] = 1.0
        xd = x.double().reshape(G, S, D)
        for name, l in _logit_patterns(G, H, S, S + D + G).items():
            pos = None
            if name == "onehot":
                l, pos = l
            stats, zpart, z = _wsum(cuda, x, G, S, H, l, True)
            assert _untouched(zpart[-GUARD:]) and _untouched(z[-GUARD:]), (name, G)
            ld = l.double()
            m = ld.max(-1, keepdim=True).values
            e = torch.exp(ld - m)
            p = e / e.sum(-1, keepdim=True)
            zref = torch.einsum("ghs,gsd->ghd", p, xd).numpy()
            zo = z[:-GUARD].reshape(G, H, D).double().cpu().numpy()
            st = stats.double().cpu().reshape(G, H, 2)
            err = np.abs(zo - zref)
            assert np.all(err <= _rel_bar(zref, 2e-5)), (name, G, err.max())
            assert torch.equal(st[..., 0], m[..., 0]), (name, G)
            assert ((st[..., 1] - 1.0 / e.sum(-1)).abs() * e.sum(-1)).max().item() <= 1e-5, (name, G)
            assert np.abs(zo[..., 0] - 1.0).max() <= 1e-5, (name, G)
            if name == "equal":
                assert np.all(np.abs(zo - xd.mean(1, keepdim=True).numpy()) <= _rel_bar(zref, 2e-5))
            if name == "onehot":
                rows = xd[torch.arange(G)[:, None], pos]
                assert np.all(np.abs(zo - rows.numpy()) <= _rel_bar(zref, 2e-5))
            worst = max(worst, err.max())
    print(f"pool_softmax_wsum wide S={S} D={D} H={H} {'bf16' if bf16 else 'f32'}: z max err {worst:.3e}")


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("D,H", [(768, 12), (1024, 16)])
def test_pool_softmax_wsum_wide_keeps_the_old_bits(cuda, D, H, bf16):
    """Whole 256-column blocks: the new entry point runs the same blocks in the same order as the old one."""
    G, S = 3, 300
    x = _tokens(G * S, D, bf16, D + 5)
    for name, l in _logit_patterns(G, H, S, D).items():
        l = l[0] if name == "onehot" else l
        old, new = _wsum(cuda, x, G, S, H, l, False), _wsum(cuda, x, G, S, H, l, True)
        for a, b in zip(old, new):
            assert torch.equal(_bits(a), _bits(b)), name


@pytest.mark.parametrize("D,H", [(1408 + 64, 2), (LIMIT + 128, 2), (64, 2), (1408, 17)])
def test_pool_softmax_wsum_wide_refusals(cuda, D, H):
    G, S = 2, 4
    stats, zpart, z = _nan(G * H, 2), _nan(G, 1, H, D), _nan(G, H, D)
    with pytest.raises(ValueError, match="pool_softmax_wsum"):
        nat.dev_pool_softmax_wsum(torch.zeros(G * S, D, device=cuda), G, S, H, torch.zeros(G, H, S, device=cuda), stats,
                                  zpart, z, wide=True)
    torch.cuda.synchronize()
    assert _untouched(stats) and _untouched(zpart) and _untouched(z)


# ------------------------------------------------------------------------------------------------------
# ln_l2_rows, wide
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("D", [1408, 1025, LIMIT])
def test_ln_l2_rows_wide(cuda, D, bf16):
    """test_ln_l2_rows at the new widths: LayerNorm only (2e-5), L2 only and both (1e-6), rows at stride 3 D."""
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
    start = x.to(cuda).reshape(-1)[2 * D:]
    worst = {}
    for name, ref in refs.items():
        for n in (rows, 1):
            out = _nan(n + 1, D)  # a guard row
            nat.dev_ln_l2_rows(start, 3 * D, n, D, gamma1p.to(cuda) if "ln" in name else None,
                               beta.to(cuda) if "ln" in name else None, "l2" in name, out, wide=True)
            torch.cuda.synchronize()
            assert _untouched(out[n:])
            err = np.abs(out[:n].double().cpu().numpy() - ref[:n])
            worst[name] = max(worst.get(name, 0.0), err.max())
            assert np.all(err <= (2e-5 if name == "ln" else 1e-6)), (name, n, err.max())
    print(f"ln_l2_rows wide D={D} {'bf16' if bf16 else 'f32'}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


def test_ln_l2_rows_wide_refusal(cuda):
    D = LIMIT + 1
    out = _nan(2, D)
    with pytest.raises(ValueError, match="ln_l2_rows"):
        nat.dev_ln_l2_rows(torch.zeros(2, D, device=cuda), D, 2, D, None, None, True, out, wide=True)
    torch.cuda.synchronize()
    assert _untouched(out)


# ------------------------------------------------------------------------------------------------------
# LayerNorm, then the residual (norm_policy 'primer_hybrid')
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_pad", [False, True])
@pytest.mark.parametrize("y_bf16", [False, True])
@pytest.mark.parametrize("D", [1408, 768])
def test_layernorm_residual(cuda, D, y_bf16, with_pad):
    """xs += LN(y (1 - pad)) in place, 45 rows (no multiple of a workgroup's 8 or a wave's 2), rows 3 and 44 padded.
    Bar: test_layernorm's for fp32 output, 2e-5, on the LayerNorm term (out - xs), plus the one rounding of the
    stored sum, 2^-24 |xs + LN| (half an ulp).  A padded row is xs + beta to the same bar; the 8 rows behind xs
    keep their NaN."""
    rows, guard = 45, 8
    g = _gen(D + 2 * y_bf16 + with_pad)
    y = torch.randn(rows, D, generator=g) * 3 + 1
    if y_bf16:
        y = y.to(torch.bfloat16)
    xs = torch.randn(rows, D, generator=g)
    scale, bias = torch.randn(D, generator=g) * 0.1, torch.randn(D, generator=g) * 0.1
    pad = torch.zeros(rows)
    pad[[3, 44]] = 1.0
    buf = _nan(rows + guard, D)
    buf[:rows] = xs.to(cuda)
    nat.dev_layernorm_residual(y.to(cuda), (1 + scale).to(cuda), bias.to(cuda), buf, pad.to(cuda) if with_pad else None)
    torch.cuda.synchronize()
    assert _untouched(buf[rows:])
    yd = y.double().numpy() * ((1.0 - pad.double().numpy())[:, None] if with_pad else 1.0)
    ln = orc.layer_norm(yd, scale.double().numpy(), bias.double().numpy(), F64)
    ref = xs.double().numpy() + ln
    out = buf[:rows].double().cpu().numpy()
    err = np.abs((out - xs.double().numpy()) - ln)
    bar = 2e-5 + 2.0 ** -24 * np.abs(ref)
    print(f"layernorm_residual D={D} y {'bf16' if y_bf16 else 'f32'} pad {with_pad}: max err {err.max():.3e}")
    assert np.all(err <= bar), err.max()
    if with_pad:
        want = xs.double().numpy()[[3, 44]] + bias.double().numpy()
        assert np.all(np.abs(out[[3, 44]] - want) <= bar[[3, 44]])
    else:
        assert np.abs(out[[3, 44]] - (xs.double().numpy()[[3, 44]] + bias.double().numpy())).max() > 1e-2


def test_layernorm_residual_refusal(cuda):
    D = 1408 + 64
    buf = _nan(4, D)
    with pytest.raises(NotImplementedError, match="128"):
        nat.dev_layernorm_residual(torch.zeros(4, D, device=cuda), torch.ones(D, device=cuda),
                                   torch.zeros(D, device=cuda), buf)
    torch.cuda.synchronize()
    assert _untouched(buf)


# ------------------------------------------------------------------------------------------------------
# reduced-depth forwards
# ------------------------------------------------------------------------------------------------------
def _video(B, T, H, seed):
    return np.random.default_rng(seed).random((B, T, H, H, 3), dtype=np.float32)


def _frame_pad(B, T):
    fp = np.zeros((B, T), np.float32)
    fp[B - 1, T - 1] = 1.0
    return fp


# (B, T, H, padded frame): (a) 16 tokens per frame, auxiliary S = 48, pooler groups G = 2 and 6; (b) 64 tokens per
# frame, auxiliary S = 320 (>= 128, no multiple of 128), the pooler's row chunks 256 + 64
GEOMETRIES = {"a": (2, 3, 72, True), "b": (1, 5, 144, False)}


@pytest.fixture(scope="module")
def giant_lvt():
    """Giant LvT at reduced depth: 1 + 1 vision, 1 auxiliary and 2 primer text layers, vocabulary 1000."""
    cfg = dict(models.CONFIGS["videoprism_lvt_v1_giant"], vocabulary_size=1000, num_spatial_layers=1,
               num_temporal_layers=1, num_auxiliary_layers=1, num_unimodal_layers=2)
    var = params.synthetic_params(cfg, 17, specs=params.clip_leaf_specs(cfg))
    mdl = models.get_model(None, model_fn=lambda: encoders.FactorizedVideoCLIP(**cfg))
    return cfg, var, mdl


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_giant_lvt_f32(cuda, giant_lvt, geo):
    cfg, var, mdl = giant_lvt
    B, T, H, padded = GEOMETRIES[geo]
    if geo == "b":
        assert nat.dev_attention_choice(nat.ATT_LONG, nat.VP_F32, 320, 50.0, False, dim_per_head=88) == "F32_MFMA"
        assert nat.dev_pool_chunks(320) == 2
    video = _video(B, T, H, 23)
    fp = _frame_pad(B, T) if padded else None
    ids, pads = _text(3, 16, 23, cfg["vocabulary_size"])
    want = ("frame_embeddings", "spatiotemporal_features")
    v, t, out = mdl.apply(var, video, ids, pads, frame_paddings=fp, return_intermediate=want)
    assert set(out) == set(want)
    assert v.shape == (B, 1408) and t.shape == (3, 1408) and out["frame_embeddings"].shape == (B, T, 1408)
    errs, floors = {}, {}
    refs = {}
    for mode in ("f64", "f32"):
        rv, _, rout = orc.video_clip(var["params"], cfg, video, None, None, mode, return_intermediate=want,
                                     frame_paddings=fp)
        refs[mode] = dict(video=rv, frames=rout["frame_embeddings"], st=rout["spatiotemporal_features"],
                          text=pr.text_embedding(var["params"], ids, pads, cfg, mode))
    got = dict(video=v, frames=out["frame_embeddings"], st=out["spatiotemporal_features"], text=t)
    for k in got:
        errs[k] = np.abs(got[k] - refs["f64"][k]).max()
        floors[k] = np.abs(np.asarray(refs["f32"][k], np.float64) - refs["f64"][k]).max()
    print(f"giant LvT f32 ({geo}): " + ", ".join(f"{k} {errs[k]:.3e} (floor {floors[k]:.3e})" for k in errs))
    np.testing.assert_allclose(np.linalg.norm(v, axis=-1), 1.0, rtol=1e-5)
    assert errs["video"] <= 2e-5 and errs["frames"] <= 2e-5 and errs["text"] <= 2e-5, errs
    assert errs["st"] <= 1e-5, errs


def test_giant_lvt_text_only_video_only_unnormalized(cuda, giant_lvt):
    """apply with one tower at a time, normalize=False, spatial_features, and device tensors in."""
    cfg, var, mdl = giant_lvt
    ids, pads = _text(3, 16, 23, cfg["vocabulary_size"])
    v, t, out = mdl.apply(var, None, ids, pads, normalize=False)
    assert v is None and out == {} and t.shape == (3, 1408)
    ref = pr.text_embedding(var["params"], ids, pads, cfg, "f64", normalize=False)
    err = np.abs(t - ref).max()
    print(f"giant LvT text only, unnormalised: max-abs {err:.3e} (|ref| max {np.abs(ref).max():.2f})")
    assert np.all(np.abs(t - ref) <= _rel_bar(ref, 2e-5)), err
    B, T, H, _ = GEOMETRIES["a"]
    video = _video(B, T, H, 23)
    v, t, out = mdl.apply(var, torch.from_numpy(video).to(cuda), normalize=False, return_intermediate=["spatial_features"])
    assert t is None and set(out) == {"spatial_features"} and isinstance(v, torch.Tensor)
    rv, _, rout = orc.video_clip(var["params"], cfg, video, None, None, "f64", normalize=False,
                                 return_intermediate=["spatial_features"])
    assert np.all(np.abs(v.cpu().numpy() - rv) <= _rel_bar(rv, 2e-5))
    assert np.abs(out["spatial_features"].cpu().numpy() - rout["spatial_features"]).max() <= 1e-5


@pytest.fixture(scope="module")
def giant_vc():
    enc = dict(models.CONFIGS["videoprism_v1_giant"], num_spatial_layers=1, num_temporal_layers=1)
    mdl = models.get_model(None, model_fn=lambda: encoders.FactorizedVideoClassifier(encoder_params=enc, num_classes=40))
    var = params.synthetic_params(enc, 19, specs=mdl.param_specs())
    return enc, var, mdl


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_giant_classifier_f32(cuda, giant_vc, geo):
    enc, var, mdl = giant_vc
    B, T, H, padded = GEOMETRIES[geo]
    video = _video(B, T, H, 29)
    fp = _frame_pad(B, T) if padded else None
    logits, out = mdl.apply(var, video, frame_paddings=fp, return_intermediate=["global_embeddings"])
    assert logits.shape == (B, 40) and set(out) == {"global_embeddings"}
    ref, rout = orc.video_classifier(var["params"], enc, video, "f64", ["global_embeddings"], fp)
    flo, fout = orc.video_classifier(var["params"], enc, video, "f32", ["global_embeddings"], fp)
    el, eg = np.abs(logits - ref).max(), np.abs(out["global_embeddings"] - rout["global_embeddings"]).max()
    fl = np.abs(flo.astype(np.float64) - ref).max()
    fg = np.abs(fout["global_embeddings"].astype(np.float64) - rout["global_embeddings"]).max()
    print(f"giant classifier f32 ({geo}): logits {el:.3e} (floor {fl:.3e}, |logits| max {np.abs(ref).max():.2f}), "
          f"global_embeddings {eg:.3e} (floor {fg:.3e})")
    assert el <= 2e-5 and eg <= 2e-5, (el, eg)


@pytest.mark.parametrize("bf16", [False, True])
def test_primer_text_tower_base_widths(cuda, bf16):
    """norm_policy 'primer_hybrid' at LvT-Base widths (D 768, 12 heads of 64), text only, 2 layers: the one bf16 use
    of layernorm_residual and of the small-M GEMM's plain store after `post` and `ffn_layer2`."""
    cfg = dict(models.CONFIGS["videoprism_lvt_v1_base"], vocabulary_size=1000, num_spatial_layers=1,
               num_temporal_layers=1, num_auxiliary_layers=1, num_unimodal_layers=2, norm_policy="primer_hybrid")
    var = params.synthetic_params(cfg, 31, specs=params.clip_leaf_specs(cfg))
    mdl = models.get_model(None, model_fn=lambda: encoders.FactorizedVideoCLIP(**cfg),
                           fprop_dtype=torch.bfloat16 if bf16 else None)
    ids, pads = _text(3, 16, 31, cfg["vocabulary_size"])
    v, t, _ = mdl.apply(var, None, ids, pads)
    assert v is None and t.shape == (3, 768)
    ref = pr.text_embedding(var["params"], ids, pads, cfg, "f64")
    floor = np.abs(pr.text_embedding(var["params"], ids, pads, cfg, "bf16" if bf16 else "f32") - ref).max()
    err = np.abs(t - ref).max()
    print(f"primer text tower, Base widths, {'bf16' if bf16 else 'f32'}: max-abs {err:.3e} (floor {floor:.3e})")
    assert err <= (1e-3 if bf16 else 2e-5), err


def test_giant_leaf_counts_and_bf16_refusal(cuda):
    """Full-size Giant LvT and classifier: leaf counts, and in bf16 the library's dim_per_head refusal arrives as
    NotImplementedError before any weight is read (zero-stride leaves, no multi-GB tree)."""
    lvt = models.get_model(None, model_fn=models.videoprism_lvt_v1_giant, fprop_dtype=torch.bfloat16)
    vc = models.get_model(None, model_fn=lambda: models.videoprism_vc_v1_giant(40), fprop_dtype=torch.bfloat16)
    assert len(lvt.param_specs()) == 92 and len(vc.param_specs()) == 54
    video = _video(1, 2, 72, 0)
    for mdl in (lvt, vc):
        flat = {k: torch.zeros(()).expand(*shape) for k, shape in mdl.param_specs().items()}
        with pytest.raises(NotImplementedError, match="dim_per_head"):
            mdl.apply(flat, video)
