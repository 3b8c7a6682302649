"""Sliding windows over per-frame spatial states on the MI355X: the frame gather bitwise against a materialised copy
(and, with the LayerNorm that follows it, against an fp64 restatement), its index clamp, frame-locality of the
states, and `apply_windows` bit for bit against `apply` on the gathered clips for the encoder, the LvT model and the
classifier.

Bars.  Gather + LayerNorm: those of test_gpu_kernels.test_layernorm / test_gpu_giant at the same widths (fp32 out
2e-5, bf16 out 2^-8 |ref| + 1e-5); its out_rs: test_gpu_kernels' bar for row statistics (rtol 2e-5, atol 1e-5).
Oracle anchor: test_gpu_encoder's fp32 bar, 1e-5.  Everything else is bitwise."""

import ctypes

import numpy as np
import pytest
import torch

from oracle import videoprism_oracle as orc
from videoprism import _native as nat
from videoprism import encoders, models, params, video_utils

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert not torch.isnan(a.float()).any(), what
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


# ---------------------------------------------------------------------------------------------------------------
# 1. the frame gather, op level
# ---------------------------------------------------------------------------------------------------------------
def _indices(rng, F, count):
    """Frame indices with repeats, a reversed run and gaps."""
    idx = rng.integers(0, F, count)
    lead = [F - 1, F - 1, F - 3, 0, 0, 2][:count]
    idx[:len(lead)] = lead
    return idx.astype(np.int32)


@pytest.mark.parametrize("N,T,Wn", [(4, 1, 3), (64, 16, 2), (256, 20, 1), (4, 20, 3), (1, 16, 1)])
@pytest.mark.parametrize("D,bf16", [(768, True), (768, False), (1024, True), (1024, False), (1408, False)])
def test_gather_frames(cuda, D, bf16, N, T, Wn):
    """Frames from 1536 bytes (a fraction of the 16 KiB piece one workgroup copies) over 22528 (two pieces, the second
    partial) to 256 x 1408 x 4 (88 pieces): bitwise the materialised copy, every output value written."""
    F = 7
    rng = np.random.default_rng(D + N + T)
    g = torch.Generator(device="cpu").manual_seed(D + N + T + Wn)
    dt = torch.bfloat16 if bf16 else torch.float32
    states = (torch.randn(F, N, D, generator=g) * 3 + 1).to(dt).to(cuda)
    idx = _indices(rng, F, Wn * T)
    idx_d = torch.from_numpy(idx).to(cuda)
    out = torch.full((Wn * T, N, D), float("nan"), dtype=dt, device=cuda)
    nat.dev_gather_frames(states, idx_d, out)
    torch.cuda.synchronize()
    _same(out, states[idx_d.long()], "gathered frames")


@pytest.mark.parametrize("N,T,Wn", [(4, 1, 3), (64, 16, 2), (256, 20, 1), (4, 20, 3), (4, 16, 1)])
@pytest.mark.parametrize("D,in_bf16,out_bf16", [(768, True, True), (768, False, False), (768, True, False),
                                                (768, False, True), (1024, True, True), (1024, False, False),
                                                (1024, False, True), (1408, False, False), (1408, False, True)])
def test_layernorm_gather(cuda, D, in_bf16, out_bf16, N, T, Wn):
    """The gather followed by the LayerNorm, the two launches with which vp_forward_temporal enters the temporal half
    (vp_dev_layernorm_gather), against the fp64 restatement: both output orders (PERM_NONE is the spatial_features
    launch, PERM_BTN_TO_BNT the one into the temporal stack), with and without the `add` table, out_rs, outputs
    prefilled with NaN, row counts from 12 (less than a workgroup's rows) up; and bitwise the LayerNorm on a
    materialised copy of the gathered rows.  Bars: test_layernorm's at these widths; out_rs against the statistics of
    the stored rows at test_gpu_kernels' bar for row statistics (rtol 2e-5, atol 1e-5)."""
    F = 7
    rng = np.random.default_rng(D + N + T)
    g = torch.Generator(device="cpu").manual_seed(D + N + T + Wn)
    states = torch.randn(F, N, D, generator=g) * 3 + 1
    if in_bf16:
        states = states.to(torch.bfloat16)
    states = states.to(cuda)
    scale = torch.randn(D, generator=g) * 0.1
    bias = torch.randn(D, generator=g) * 0.1
    gamma, beta = (1 + scale).to(cuda), bias.to(cuda)
    add = torch.randn(T, D, generator=g).to(cuda)
    idx = _indices(rng, F, Wn * T)
    idx_d = torch.from_numpy(idx).to(cuda)
    rows = Wn * T * N
    odt = torch.bfloat16 if out_bf16 else torch.float32
    gathered = states[idx_d.long()].reshape(rows, D).contiguous()  # the materialised copy
    ln = orc.layer_norm(gathered.double().cpu().numpy(), scale.double().numpy(), bias.double().numpy(),
                        orc.Numerics("f64"))
    for perm in (nat.PERM_NONE, nat.PERM_BTN_TO_BNT):
        for a in (None, add):
            out = torch.full((rows, D), float("nan"), dtype=odt, device=cuda)
            rs = torch.full((rows, 2), float("nan"), dtype=torch.float32, device=cuda)
            nat.dev_layernorm_gather(states, idx_d, T, gamma, beta, out, perm, a, rs)
            plain = nat.op_layernorm(gathered, gamma, beta, odt, perm, T, N, a)
            torch.cuda.synchronize()
            ref = ln
            if perm == nat.PERM_BTN_TO_BNT:
                ref = ref.reshape(Wn, T, N, D).transpose(0, 2, 1, 3)
                if a is not None:
                    ref = ref + a.double().cpu().numpy()[None, None]
                ref = ref.reshape(rows, D)
            elif a is not None:  # no permutation: every output row counts as t = 0
                ref = ref + a.double().cpu().numpy()[0]
            got = out.double().cpu().numpy()
            err = np.abs(got - ref)
            print(f"layernorm_gather D={D} N={N} T={T} Wn={Wn} rows {rows} in_bf16 {in_bf16} out_bf16 {out_bf16} "
                  f"perm {perm} add {a is not None}: max-abs {np.nanmax(err):.3e}")
            tol = 2 ** -8 * np.abs(ref) + 1e-5 if out_bf16 else 2e-5
            assert np.all(err <= tol), np.nanmax(err)
            _same(out, plain, "gather + LayerNorm vs LayerNorm on the gathered rows")
            # out_rs: (rstd, -mean * rstd) of the stored (rounded) rows, by output row
            mean = got.mean(-1)
            rstd = 1.0 / np.sqrt(got.var(-1) + 1e-6)
            want = np.stack([rstd, -mean * rstd], -1)
            got_rs = rs.double().cpu().numpy()
            e_rs = np.abs(got_rs - want)
            print(f"  out_rs max-abs {np.nanmax(e_rs):.3e}")
            assert np.all(e_rs <= 2e-5 * np.abs(want) + 1e-5), np.nanmax(e_rs)


def test_gather_frames_refusals(cuda):
    st = torch.zeros(2, 4, 768, device=cuda)
    i = torch.zeros(2, dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError, match="gather_frames"):  # frames of 12 bytes
        nat.dev_gather_frames(torch.zeros(2, 3, device=cuda), i, torch.zeros(2, 3, device=cuda))
    with pytest.raises(ValueError, match="gather_frames"):  # a source 4 bytes off a 16-byte boundary
        nat.dev_gather_frames(st.reshape(-1)[1:1 + 768 * 4].reshape(1, 4, 768), i, torch.zeros(2, 4, 768, device=cuda))
    with pytest.raises(ValueError, match="null"):  # no slots: an empty index tensor has no address
        nat.dev_gather_frames(st, i[:0], torch.zeros(1, 4, 768, device=cuda))


# ---------------------------------------------------------------------------------------------------------------
# 2. the clamp
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,bf16", [(768, True), (1024, False), (1408, False)])
def test_gather_frames_clamps_indices(cuda, D, bf16):
    """The states are a slice of a larger allocation with two guard frames of NaN on each side: indices -2, -1, F and
    F + 1 must give bitwise what 0 and F - 1 give.  Without the clamp the kernel would read the guards' NaN (inside
    the allocation) and fail here."""
    F, N = 5, 4
    dt = torch.bfloat16 if bf16 else torch.float32
    g = torch.Generator(device="cpu").manual_seed(D)
    big = torch.full((F + 4, N, D), float("nan"), dtype=dt, device=cuda)
    big[2:F + 2] = torch.randn(F, N, D, generator=g).to(dt).to(cuda)
    states = big[2:F + 2]
    assert states.is_contiguous() and states.data_ptr() == big.data_ptr() + 2 * N * D * big.element_size()
    wild = torch.tensor([-1, F, 2, -2, F + 1, F - 1, 0, -1], dtype=torch.int32, device=cuda)
    tame = wild.clamp(0, F - 1)
    outs = []
    for idx in (wild, tame):
        out = torch.full((idx.numel(), N, D), float("nan"), dtype=dt, device=cuda)
        nat.dev_gather_frames(states, idx, out)
        outs.append(out)
    torch.cuda.synchronize()
    _same(outs[0], outs[1], "clamped gather")
    _same(outs[0], states[tame.long()], "clamped gather against the copy")
    assert torch.isnan(big[:2].float()).all() and torch.isnan(big[F + 2:].float()).all()


# ---------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------
def _cfg(name, **kw):
    c = dict(models.CONFIGS[name])
    c.update(kw)
    return c


BASE22 = _cfg("videoprism_v1_base", num_spatial_layers=2, num_temporal_layers=2)
_cache = {}


def _encoder(cfg, bf16, seed=11):
    key = (tuple(sorted((k, str(v)) for k, v in cfg.items())), bf16, seed)
    if key not in _cache:
        var = params.synthetic_params(cfg, seed=seed)
        m = models.get_model(None, model_fn=lambda: encoders.FactorizedEncoder(**cfg),
                             fprop_dtype=torch.bfloat16 if bf16 else None)
        _cache[key] = (m, var)
    return _cache[key]


def _frames(F, size, seed, device):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand(F, size, size, 3, generator=g).to(device)


def _base_fixture(cuda, bf16):
    """Base widths, 2 + 2 layers, 20 frames of 288 x 288: the model, the frames, their paddings (frames 3 and 10
    padded) and the frame states without and with those paddings, computed once per dtype."""
    key = ("base-fixture", bf16)
    if key not in _cache:
        m, var = _encoder(BASE22, bf16)
        frames = _frames(20, 288, 5, cuda)
        pads = torch.zeros(20, device=cuda)
        pads[3] = pads[10] = 1.0
        _cache[key] = (m, var, frames, pads, m.encode_frames(var, frames), m.encode_frames(var, frames, pads))
    return _cache[key]


def _check_windows_equal_apply(m, var, frames, pads, fs, idx):
    """apply_windows(fs, idx) against apply on the gathered clips of the same model object: embeddings and
    spatial_features, bit for bit."""
    idx_d = torch.as_tensor(np.asarray(idx), device=frames.device).long()
    clips = frames[idx_d]
    fp = None if pads is None else pads[idx_d]
    want, wout = m.apply(var, clips, return_intermediate=["spatial_features"], frame_paddings=fp)
    got, gout = m.apply_windows(var, fs, idx_d, return_intermediate=["spatial_features"])
    torch.cuda.synchronize()
    assert got.shape == (idx_d.shape[0], idx_d.shape[1] * fs.states.shape[1], fs.states.shape[2])
    _same(got, want, "embeddings")
    _same(gout["spatial_features"], wout["spatial_features"], "spatial_features")
    return got


# 3. states are frame-local
@pytest.mark.parametrize("bf16", [False, True])
def test_states_are_frame_local(cuda, bf16):
    m, var = _encoder(BASE22, bf16)
    frames = _frames(5, 288, 7, cuda)
    pads = torch.tensor([0.0, 0.0, 1.0, 0.0, 0.0], device=cuda)
    fs = m.encode_frames(var, frames, pads)
    assert fs.states.shape == (5, 256, 768) and fs.frame_size == (288, 288)
    assert fs.states.dtype == (torch.bfloat16 if bf16 else torch.float32)
    assert torch.equal(fs.paddings, pads)
    for f in range(5):  # each frame alone
        one = m.encode_frames(var, frames[f:f + 1], pads[f:f + 1])
        _same(one.states[0], fs.states[f], f"frame {f} alone")
    order = [3, 0, 4, 2, 1]
    perm = m.encode_frames(var, frames[order], pads[order])
    _same(perm.states, fs.states[order], "permuted frames")
    # numpy frames in: the same states
    host = m.encode_frames(var, frames.cpu().numpy(), pads.cpu().numpy())
    _same(host.states, fs.states, "numpy frames")


# 4. windows equal apply
@pytest.mark.parametrize("bf16", [False, True])
def test_windows_t16_stride1(cuda, bf16):
    """T = 16, no paddings: in bf16 the fused temporal q|k|v attention."""
    m, var, frames, _, fs, _ = _base_fixture(cuda, bf16)
    idx = video_utils.sliding_windows(20, 16, 1)
    assert idx.shape == (5, 16)
    _check_windows_equal_apply(m, var, frames, None, fs, idx)


@pytest.mark.parametrize("bf16", [False, True])
def test_windows_t8_dilation2_padded(cuda, bf16):
    """T = 8 at dilation 2 with two padded frames among the states: the unfused temporal kernel."""
    m, var, frames, pads, _, fs = _base_fixture(cuda, bf16)
    idx = video_utils.sliding_windows(20, 8, 1, dilation=2)
    assert idx.shape == (6, 8) and {3, 10} <= set(idx.ravel().tolist())
    _check_windows_equal_apply(m, var, frames, pads, fs, idx)


@pytest.mark.parametrize("bf16", [False, True])
def test_windows_t20_interpolated_table(cuda, bf16):
    """T = 20: the sequence-packed attention and a temporal table interpolated from 16 to 20 rows."""
    m, var, frames, _, fs, _ = _base_fixture(cuda, bf16)
    idx = np.stack([np.arange(20), np.random.default_rng(3).permutation(20)]).astype(np.int32)
    _check_windows_equal_apply(m, var, frames, None, fs, idx)


@pytest.mark.parametrize("bf16", [False, True])
def test_windows_repeated_and_reversed(cuda, bf16):
    m, var, frames, pads, fs, fsp = _base_fixture(cuda, bf16)
    idx = np.array([[5, 5, 4, 3, 3, 2, 1, 0], [19, 19, 19, 19, 0, 0, 0, 0], [10, 9, 10, 9, 3, 3, 11, 12]], np.int32)
    _check_windows_equal_apply(m, var, frames, None, fs, idx)
    _check_windows_equal_apply(m, var, frames, pads, fsp, idx)


@pytest.mark.parametrize("bf16", [False, True])
def test_windows_host_index_numpy_out_and_slices(cuda, bf16):
    """A numpy frame_index gives numpy results equal to the tensor path's; sliced and re-concatenated states (a
    stream dropping and appending frames) give the same windows."""
    m, var, frames, _, fs, _ = _base_fixture(cuda, bf16)
    idx = video_utils.sliding_windows(12, 8, 4)
    t_emb, t_out = m.apply_windows(var, fs, torch.from_numpy(idx).to(cuda), return_intermediate=True)
    n_emb, n_out = m.apply_windows(var, fs, idx, return_intermediate=True)
    assert isinstance(n_emb, np.ndarray) and n_emb.dtype == np.float32 and set(n_out) == {"spatial_features"}
    np.testing.assert_array_equal(n_emb, t_emb.float().cpu().numpy())
    np.testing.assert_array_equal(n_out["spatial_features"], t_out["spatial_features"].float().cpu().numpy())
    rolled = encoders.FrameStates.cat([fs[4:12], fs[0:4]])  # frames 4..11, then 0..3
    r_emb, _ = m.apply_windows(var, rolled, torch.from_numpy((idx + 8) % 12).to(cuda))
    _same(r_emb, t_emb, "rolled states")
    with pytest.raises(IndexError):
        m.apply_windows(var, fs, [[0, 20]])
    # a host tensor index: range-checked like the numpy one, tensors out
    h_emb, _ = m.apply_windows(var, fs, torch.from_numpy(idx))
    _same(h_emb, t_emb, "host tensor index")


@pytest.mark.parametrize("bf16", [False, True])
def test_windows_large_widths_t16(cuda, bf16):
    """Large widths (16 heads, temporal table of 8 rows interpolated to 16), 1 + 1 layers."""
    cfg = _cfg("videoprism_v1_large", num_spatial_layers=1, num_temporal_layers=1)
    m, var = _encoder(cfg, bf16, seed=12)
    frames = _frames(17, 288, 6, cuda)
    fs = m.encode_frames(var, frames)
    _check_windows_equal_apply(m, var, frames, None, fs, video_utils.sliding_windows(17, 16, 1))


@pytest.mark.parametrize("bf16", [False, True])
def test_windows_small_grid_padded_rows(cuda, bf16):
    """Base at 144 x 144 (N = 64, interpolated spatial table, patchify route), T = 3, F = 5: neither the 320 rows of
    the states nor the 576 of the windows fill the GEMM row tile; uint8 frames."""
    m, var = _encoder(BASE22, bf16)
    g = torch.Generator(device="cpu").manual_seed(9)
    frames = torch.randint(0, 256, (5, 144, 144, 3), generator=g, dtype=torch.uint8).to(cuda)
    pads = torch.tensor([0.0, 1.0, 0.0, 0.0, 0.0], device=cuda)
    fs = m.encode_frames(var, frames, pads)
    assert fs.states.shape == (5, 64, 768)
    _check_windows_equal_apply(m, var, frames, pads, fs, video_utils.sliding_windows(5, 3, 1))


def test_windows_giant_f32(cuda):
    """Giant widths (1408, 16 heads of 88) in fp32, 1 + 1 layers, F = 4, T = 4."""
    cfg = _cfg("videoprism_v1_giant", num_spatial_layers=1, num_temporal_layers=1)
    m, var = _encoder(cfg, False, seed=13)
    frames = _frames(4, 288, 8, cuda)
    fs = m.encode_frames(var, frames)
    assert fs.states.shape == (4, 256, 1408)
    _check_windows_equal_apply(m, var, frames, None, fs, np.array([[0, 1, 2, 3], [3, 2, 1, 0]], np.int32))


# 5. oracle anchor
def test_windows_against_oracle_f32(cuda):
    """The small-grid case in fp32 against the NumPy oracle on the gathered clips: both paths wrong together would
    pass every bitwise test above."""
    m, var = _encoder(BASE22, False)
    frames = np.random.default_rng(21).random((5, 144, 144, 3), dtype=np.float32)
    pads = np.array([0.0, 1.0, 0.0, 0.0, 0.0], np.float32)
    idx = video_utils.sliding_windows(5, 3, 1)
    fs = m.encode_frames(var, frames, pads)
    emb, out = m.apply_windows(var, fs, idx, return_intermediate=True)
    ref, rout = orc.factorized_encoder(var["params"], frames[idx], BASE22, mode="f64", frame_paddings=pads[idx],
                                       return_intermediate=True)
    e, es = np.abs(emb - ref).max(), np.abs(out["spatial_features"] - rout["spatial_features"]).max()
    print(f"windows vs oracle f32: embeddings max-abs {e:.3e}, spatial_features {es:.3e}")
    assert emb.shape == (3, 3 * 64, 768)
    assert e <= 1e-5 and es <= 1e-5, (e, es)


# 6. LvT and classifier
@pytest.mark.parametrize("bf16", [False, True])
def test_lvt_windows(cuda, bf16):
    cfg = _cfg("videoprism_lvt_v1_base", vocabulary_size=1000, num_spatial_layers=1, num_temporal_layers=1,
               num_auxiliary_layers=1, num_unimodal_layers=2)
    var = params.synthetic_params(cfg, 17, specs=params.clip_leaf_specs(cfg))
    m = models.get_model(None, model_fn=lambda: encoders.FactorizedVideoCLIP(**cfg),
                         fprop_dtype=torch.bfloat16 if bf16 else None)
    frames = _frames(6, 288, 17, cuda)
    pads = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0], device=cuda)
    g = torch.Generator(device="cpu").manual_seed(17)
    ids = torch.randint(0, 1000, (3, 16), generator=g, dtype=torch.int32).to(cuda)
    tp = torch.zeros(3, 16, device=cuda)
    tp[1, 9:] = 1.0
    idx = torch.tensor([[0, 1, 2, 3], [2, 3, 4, 5], [5, 5, 1, 0]], device=cuda)
    fs = m.encode_frames(var, frames, pads)
    v0, t0, o0 = m.apply(var, frames[idx], ids, tp, return_intermediate=True, frame_paddings=pads[idx])
    v1, t1, o1 = m.apply_windows(var, fs, idx, ids, tp, return_intermediate=True)
    torch.cuda.synchronize()
    assert v1.shape == (3, 768) and v1.dtype == (torch.bfloat16 if bf16 else torch.float32)
    _same(v1, v0, "video embeddings")
    _same(t1, t0, "text embeddings")
    assert set(o1) == set(o0) == {"spatial_features", "spatiotemporal_features", "frame_embeddings"}
    for k in o0:
        _same(o1[k], o0[k], k)
    # either side alone, and one intermediate asked for by name
    v2, t2, o2 = m.apply_windows(var, fs, idx, normalize=False, return_intermediate=["frame_embeddings"])
    v3, _, o3 = m.apply(var, frames[idx], normalize=False, return_intermediate=["frame_embeddings"],
                        frame_paddings=pads[idx])
    assert t2 is None and set(o2) == {"frame_embeddings"}
    _same(v2, v3, "unnormalised video embeddings")
    _same(o2["frame_embeddings"], o3["frame_embeddings"], "frame_embeddings")
    v4, t4, _ = m.apply_windows(var, None, None, ids, tp)
    assert v4 is None
    _same(t4, t0, "text only")


@pytest.mark.parametrize("bf16", [False, True])
def test_classifier_windows(cuda, bf16):
    enc = _cfg("videoprism_v1_base", num_spatial_layers=1, num_temporal_layers=1)
    m = models.get_model(None, model_fn=lambda: encoders.FactorizedVideoClassifier(encoder_params=enc,
                                                                                  num_classes=40),
                         fprop_dtype=torch.bfloat16 if bf16 else None)
    var = params.synthetic_params(enc, 19, specs=m.param_specs())
    frames = _frames(5, 288, 19, cuda)
    pads = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0], device=cuda)
    idx = torch.tensor([[0, 1], [1, 2], [4, 3], [2, 2]], device=cuda)
    fs = m.encode_frames(var, frames, pads)
    l0, o0 = m.apply(var, frames[idx], return_intermediate=True, frame_paddings=pads[idx])
    l1, o1 = m.apply_windows(var, fs, idx, return_intermediate=True)
    torch.cuda.synchronize()
    assert l1.shape == (4, 40)
    _same(l1, l0, "logits")
    assert set(o1) == set(o0) == {"spatial_features", "spatiotemporal_features", "global_embeddings"}
    for k in o0:
        _same(o1[k], o0[k], k)
    l2, o2 = m.apply_windows(var, fs, idx)
    assert o2 == {}
    _same(l2, l0, "logits without intermediates")


# 7. contract
def test_windows_contract(cuda):
    m, var = _encoder(BASE22, True)
    frames = _frames(3, 288, 23, cuda)
    fs = m.encode_frames(var, frames)
    eng = m.engine(var, cuda.index or 0)
    lib = nat.load()
    h = eng.handle()
    need = ctypes.c_size_t()
    nat.call("vp_spatial_workspace_bytes", h, 3, 288, 288, ctypes.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=cuda)
    out = torch.empty_like(fs.states)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = frames.to(torch.bfloat16)
    # a too-small workspace
    assert lib.vp_forward_spatial(h, p(x), nat.VP_BF16, 3, 288, 288, None, p(out), p(ws), need.value - 1,
                                  stream) == nat.VP_EINVAL
    assert b"workspace too small" in lib.vp_last_error()
    idx = torch.zeros((1, 33), dtype=torch.int32, device=cuda)
    nat.call("vp_temporal_workspace_bytes", h, 1, 33, 288, 288, ctypes.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=cuda)
    emb = torch.empty((1, 33 * 256, 768), dtype=torch.bfloat16, device=cuda)
    args = (h, p(fs.states), 3, p(idx), 1, 33, 288, 288, None, p(emb), nat.VP_BF16, None, p(ws))
    assert lib.vp_forward_temporal(*args, need.value - 1, stream) == nat.VP_EINVAL
    # the index is required
    assert lib.vp_forward_temporal(h, p(fs.states), 3, None, 1, 33, 288, 288, None, p(emb), nat.VP_BF16, None, p(ws),
                                   need.value, stream) == nat.VP_EINVAL
    assert b"null" in lib.vp_last_error()
    # T = 33 has no temporal table until vp_prepare_frames (vp_finalize precomputes 1..32)
    assert lib.vp_forward_temporal(*args, need.value, stream) == nat.VP_ESTATE
    assert b"vp_prepare_frames" in lib.vp_last_error()
    torch.cuda.synchronize()
    # no windows, no frames: zero-size results, nothing launched
    emb, outs = m.apply_windows(var, fs, torch.zeros((0, 16), dtype=torch.int64, device=cuda),
                                return_intermediate=True)
    assert emb.shape == (0, 16 * 256, 768) and outs["spatial_features"].shape == emb.shape
    emb, _ = m.apply_windows(var, fs, np.zeros((0, 4), np.int32))
    assert emb.shape == (0, 4 * 256, 768)
    none = m.encode_frames(var, frames[:0])
    assert none.states.shape == (0, 256, 768) and len(none) == 0
    emb, _ = m.apply_windows(var, none, np.zeros((0, 16), np.int32))
    assert emb.shape == (0, 16 * 256, 768)
    with pytest.raises(IndexError):
        m.apply_windows(var, none, torch.zeros((1, 16), dtype=torch.int64, device=cuda))
    # states of another width or dtype are refused on use
    with pytest.raises(ValueError, match="fprop dtype"):
        m.apply_windows(var, encoders.FrameStates(fs.states.float(), None, (288, 288)), [[0, 1]])
    with pytest.raises(ValueError, match=r"\[F, 256, 768\]"):
        m.apply_windows(var, encoders.FrameStates(fs.states[:, :, :512], None, (288, 288)), [[0, 1]])
    with pytest.raises(ValueError, match="cuda"):
        m.apply_windows(var, encoders.FrameStates(fs.states.cpu(), None, (288, 288)), [[0, 1]])
