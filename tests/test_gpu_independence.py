"""Independence properties of the forward off the headline shape, bit for bit, in fp32 and bf16 (cases:
tests/offsize_cases.py; the properties are the reference's own, tests/test_independence_cpu.py):

  (a) a clip's `embeddings` and `spatial_features` do not depend on the batch it runs in (B = 3 with different
      paddings per clip against B = 1), at Base and Large widths, and the video-text model's and the classifier's
      heads likewise;
  (b) the rows of valid frames do not depend on the pixels of padded frames (and the padded frames' own rows do:
      the test has teeth);
  (c) a text embedding depends neither on the ids under its paddings nor on the other queries of its batch -- as long
      as the batch stays on one side of clip_text_ws's switch between the 64-row and the 256-row bf16 GEMM (4096
      rows): the two sum K in different orders, so across it the distance is printed, not asserted.

What (a) can and cannot see.  Alone and in a batch a clip's rows lie in other GEMM tiles and, where sequences are
packed several to a workgroup, in other slots: at 144 x 144, T = 3 clips 1 and 2 move by 3 and 2 of the spatial
kernel's 4 slots (offsize_cases.frame_paddings keeps the fully padded clip, whose uniform attention tells nothing, at
clip 0, which never moves).  At 144 x 144, T = 20 a clip is a whole number of workgroups in both stacks, so no clip
changes slots there; a slot-dependent error at that case is test_gpu_bf16_offsize.py's to find.

Not pinned, because the reference does not promise it: the pooled heads (logits, video embedding) depend on the
pixels of padded frames (the poolers take no paddings)."""

import numpy as np
import pytest
import torch

import offsize_cases as oc
from videoprism import _native as nat
from videoprism import encoders, models, params

pytestmark = pytest.mark.gpu

B = 3
_runs = {}


def _same(a, b, what):
    """Bit for bit (finite values, so equal values of one dtype are equal bits but for the sign of a zero, which
    the integer view compares too)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all(), what
    ints = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    diff = a.contiguous().view(ints) != b.contiguous().view(ints)
    if diff.any():
        i = tuple(int(x) for x in diff.nonzero()[0])
        d = (a.double() - b.double()).abs().max().item()
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} elements differ, the first at {i}: "
                             f"{a[i].item()!r} vs {b[i].item()!r}; max-abs difference {d:.3e}")


def _apply(m, var, video, fp):
    emb, out = m.apply(var, video, return_intermediate=True,
                       frame_paddings=None if fp is None else torch.from_numpy(fp).to(video.device))
    torch.cuda.synchronize()
    return emb, out["spatial_features"]


def _batch_run(cuda, c, cfg, bf16, tag="base"):
    """The B = 3 run of a case, once per (case, widths, dtype): model, variables, clips, paddings, outputs."""
    key = (tag, c, bf16)
    if key not in _runs:
        oc.assert_kernels(c, cfg, bf16)
        m, var = oc.encoder(cfg, bf16)
        video = oc.clips(c, B, bf16, cuda)
        fp = oc.frame_paddings(B, c.T) if c.padded else None
        _runs[key] = (m, var, video, fp) + _apply(m, var, video, fp)
    return _runs[key]


def _check_clip_independence(cuda, c, cfg, bf16, tag):
    m, var, video, fp, emb, spf = _batch_run(cuda, c, cfg, bf16, tag)
    N = oc.patches(cfg, c.hw)
    assert emb.shape == spf.shape == (B, c.T * N, cfg["model_dim"])
    for b in range(B):
        e1, s1 = _apply(m, var, video[b:b + 1].contiguous(), None if fp is None else fp[b:b + 1])
        _same(e1[0], emb[b], f"{oc.case_id(c)} clip {b}: embeddings alone vs in the batch")
        _same(s1[0], spf[b], f"{oc.case_id(c)} clip {b}: spatial_features alone vs in the batch")


# (a) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", oc.CASES, ids=oc.case_id)
def test_clip_independent_of_batch(cuda, c, bf16):
    _check_clip_independence(cuda, c, oc.BASE22, bf16, "base")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_clip_independent_of_batch_large_widths(cuda, bf16):
    """Large widths (1024, 16 heads, the temporal table of 8 rows interpolated to 3) at 144 x 144, T = 3, padded."""
    _check_clip_independence(cuda, oc.CASES[2], oc.LARGE22, bf16, "large")


def _head_batch(cuda, bf16):
    c = oc.CASES[2]  # 144 x 144, T = 3
    return oc.clips(c, B, bf16, cuda, seed=1), torch.from_numpy(oc.frame_paddings(B, c.T)).to(cuda)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_lvt_video_independent_of_batch(cuda, bf16):
    """LvT-Base (1 + 1 vision, 1 auxiliary, 1 text layer) at 144 x 144, T = 3, B = 3, without and with frame
    paddings: each clip's video and frame embeddings are those of its B = 1 run (the 288 x 288 counterpart:
    test_gpu_lvt_large.test_lvt_large_bench_batch_bitwise)."""
    cfg = oc.cfg_of("videoprism_lvt_v1_base", num_spatial_layers=1, num_temporal_layers=1, num_auxiliary_layers=1,
                    num_unimodal_layers=1, vocabulary_size=100)
    var = params.synthetic_params(cfg, 43, specs=params.clip_leaf_specs(cfg))
    m = models.get_model(None, model_fn=lambda: encoders.FactorizedVideoCLIP(**cfg),
                         fprop_dtype=torch.bfloat16 if bf16 else None)
    eng = m.engine(var, torch.cuda.current_device())
    video, fp = _head_batch(cuda, bf16)
    for pads in (None, fp):
        v, f, _, _ = eng.encode_video(video, pads, want_frames=True)
        v, f = v.clone(), f.clone()
        for b in range(B):
            v1, f1, _, _ = eng.encode_video(video[b:b + 1].contiguous(), None if pads is None else pads[b:b + 1],
                                            want_frames=True)
            torch.cuda.synchronize()
            _same(v1[0], v[b], f"video embedding, clip {b}, paddings {pads is not None}")
            _same(f1[0], f[b], f"frame embeddings, clip {b}, paddings {pads is not None}")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_classifier_independent_of_batch(cuda, bf16):
    """The Base classifier (1 + 1 layers, 40 classes) at 144 x 144, T = 3, B = 3: logits and global embedding of each
    clip are those of its B = 1 run (the 288 x 288 counterpart: test_classifier_forward_chunks_bitwise)."""
    enc = oc.cfg_of("videoprism_v1_base", num_spatial_layers=1, num_temporal_layers=1)
    m = models.get_model(None, model_fn=lambda: encoders.FactorizedVideoClassifier(encoder_params=enc, num_classes=40),
                         fprop_dtype=torch.bfloat16 if bf16 else None)
    var = params.synthetic_params(enc, 44, specs=m.param_specs())
    eng = m.engine(var, torch.cuda.current_device())
    video, fp = _head_batch(cuda, bf16)
    for pads in (None, fp):
        lg, emb, _, _ = eng.forward(video, pads, want_embeddings=True)
        lg, emb = lg.clone(), emb.clone()
        for b in range(B):
            l1, e1, _, _ = eng.forward(video[b:b + 1].contiguous(), None if pads is None else pads[b:b + 1],
                                       want_embeddings=True)
            torch.cuda.synchronize()
            _same(l1[0], lg[b], f"logits, clip {b}, paddings {pads is not None}")
            _same(e1[0], emb[b], f"global embedding, clip {b}, paddings {pads is not None}")


# (b) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["random", "constant"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [c for c in oc.CASES if c.padded], ids=oc.case_id)
def test_valid_frames_ignore_padded_frames(cuda, c, bf16, how):
    cfg = oc.BASE22
    m, var, video, fp, emb, spf = _batch_run(cuda, c, cfg, bf16)
    changed = oc.replace_padded_frames(video, fp, how)
    pad = torch.from_numpy(fp > 0).to(cuda)
    assert torch.isfinite(changed.float()).all() and torch.equal(changed[~pad], video[~pad])
    assert not torch.equal(changed[pad], video[pad])
    emb2, spf2 = _apply(m, var, changed, fp)
    N, D = oc.patches(cfg, c.hw), cfg["model_dim"]
    for name, a, b in (("embeddings", emb, emb2), ("spatial_features", spf, spf2)):
        a, b = a.view(B, c.T, N, D), b.view(B, c.T, N, D)
        _same(a[~pad], b[~pad], f"{oc.case_id(c)} {name}: rows of valid frames")
        assert not torch.equal(a[pad], b[pad]), f"{name}: no padded frame's rows moved with its pixels"


# (c) ---------------------------------------------------------------------------------------------------------------
VOCAB = 1000


def _text_engine(bf16):
    key = ("text", bf16)
    if key not in _runs:
        cfg = oc.cfg_of("videoprism_lvt_v1_base", num_spatial_layers=1, num_temporal_layers=1,
                        num_auxiliary_layers=1, num_unimodal_layers=2, vocabulary_size=VOCAB)
        var = params.synthetic_params(cfg, 45, specs=params.clip_leaf_specs(cfg))
        m = models.get_model(None, model_fn=lambda: encoders.FactorizedVideoCLIP(**cfg),
                             fprop_dtype=torch.bfloat16 if bf16 else None)
        _runs[key] = (cfg, m.engine(var, torch.cuda.current_device()))
    return _runs[key]


def _queries(L, Q, seed):
    """ids [Q, L] and causal (trailing) paddings: query 0 full length, 1 half, 2 fully padded, 3 one token,
    4 all but the last token; further queries of random lengths."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, VOCAB, (Q, L)).astype(np.int32)
    lengths = [L, L // 2, 0, 1, L - 1] + list(rng.integers(0, L + 1, max(Q - 5, 0)))
    pads = np.zeros((Q, L), np.float32)
    for q in range(Q):
        pads[q, lengths[q]:] = 1.0
    return ids, pads


@pytest.mark.parametrize("L", [7, 16, 63])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_text_ignores_padded_ids_and_other_queries(cuda, bf16, L):
    cfg, eng = _text_engine(bf16)
    prec = nat.VP_BF16 if bf16 else nat.VP_F32
    want = "SEQ" if bf16 and L + 1 > 16 else "MASKED"
    assert nat.dev_attention_choice(nat.ATT_TEXT, prec, L + 1, cfg["atten_logit_cap"], True) == want

    def encode(ids, pads):
        out = eng.encode_text(torch.from_numpy(ids).to(cuda), torch.from_numpy(pads).to(cuda)).clone()
        torch.cuda.synchronize()
        return out

    ids, pads = _queries(L, 5, L)
    assert pads[2].all() and not pads[0].any()
    base = encode(ids, pads)
    rng = np.random.default_rng(L + 100)
    ids2 = np.where(pads > 0, (ids + 1 + rng.integers(0, VOCAB - 1, ids.shape)) % VOCAB, ids).astype(np.int32)
    assert (ids2 != ids)[pads > 0].all() and (ids2 == ids)[pads == 0].all()
    _same(encode(ids2, pads), base, f"L = {L}: ids under the paddings changed")
    for q in range(5):
        _same(encode(ids[q:q + 1], pads[q:q + 1])[0], base[q], f"L = {L}: query {q} alone vs among 5")
    if L != 63:
        return
    # past clip_text_ws's switch to the 256-row GEMM (4096 rows): 70 x 64 = 4480 and 130 x 64 = 8320 rows
    big_ids, big_pads = _queries(L, 130, 7)
    big_ids[60:65], big_pads[60:65] = ids, pads  # the five queries in the middle of both batches
    e130 = encode(big_ids, big_pads)
    e70 = encode(big_ids[:70], big_pads[:70])
    _same(e70, e130[:70], "L = 63: a query among 70 vs among 130")
    d = (e70[60:65] - base).abs().max().item()
    print(f"L = 63 {'bf16' if bf16 else 'f32'}: among 5 vs among 70 (across the 4096-row switch) max-abs {d:.3e}")
    if not bf16:  # fp32 has one GEMM kernel at every row count
        _same(e70[60:65], base, "L = 63 f32: a query among 5 vs among 70")
