"""The video cases off the headline shape (288 x 288, T = 16, no paddings) that tests/test_gpu_independence.py and
tests/test_gpu_bf16_offsize.py share (a helper module, no tests): frame size, clip length, whether frames are padded,
and the attention kernels the bf16 forward reaches there.  Base widths (the production kernel instantiations are
chosen by D = 768 and 12 heads), 2 spatial + 2 temporal layers (the `_ST` producers of a non-last layer and the plain
epilogues of the last one both run), synthetic parameters; models are built once per dtype.

    H = W   T   paddings   patches   spatial attention                 temporal stack
     72    16   none          16     TEMPORAL (S = 16)                 fused q|k|v attention
     72    16   some          16     TEMPORAL                          unfused TEMPORAL
    144     3   some          64     SEQ, 4 sequences per workgroup    TEMPORAL; 192 rows per clip
    144    20   none          64     SEQ                               SEQ (S = 20)
    216     5   some         144     SEQ (S = 144)                     TEMPORAL; 720 rows per clip
    360     2   some         400     MASKED (S = 400)                  TEMPORAL; 800 rows per clip
"""

import collections

import numpy as np
import torch

from videoprism import _native as nat
from videoprism import encoders, models, params

# spatial / temporal: the names dev_attention_choice must give the bf16 stacks; *_f32: the fp32 stacks
Case = collections.namedtuple("Case", "hw T padded spatial temporal spatial_f32 temporal_f32")

CASES = [
    Case(72, 16, False, "TEMPORAL", "TEMPORAL", "F32", "F32"),
    Case(72, 16, True, "TEMPORAL", "TEMPORAL", "F32", "F32"),
    Case(144, 3, True, "SEQ", "TEMPORAL", "F32", "F32"),
    Case(144, 20, False, "SEQ", "SEQ", "F32", "F32"),
    Case(216, 5, True, "SEQ", "TEMPORAL", "F32", "F32"),
    Case(360, 2, True, "MASKED", "TEMPORAL", "F32_MFMA", "F32"),
]


def case_id(c):
    return f"{c.hw}x{c.hw}-T{c.T}-{'padded' if c.padded else 'plain'}"


def cfg_of(name, **kw):
    c = dict(models.CONFIGS[name])
    c.update(kw)
    return c


BASE22 = cfg_of("videoprism_v1_base", num_spatial_layers=2, num_temporal_layers=2)
LARGE22 = cfg_of("videoprism_v1_large", num_spatial_layers=2, num_temporal_layers=2)
PARAM_SEED = 41
_cache = {}


def encoder(cfg, bf16, seed=PARAM_SEED):
    """(model, variables) of a FactorizedEncoder, built once per configuration and dtype."""
    key = (tuple(sorted((k, str(v)) for k, v in cfg.items())), bf16, seed)
    if key not in _cache:
        var = params.synthetic_params(cfg, seed=seed)
        m = models.get_model(None, model_fn=lambda: encoders.FactorizedEncoder(**cfg),
                             fprop_dtype=torch.bfloat16 if bf16 else None)
        _cache[key] = (m, var)
    return _cache[key]


def patches(cfg, hw):
    return (hw // cfg["patch_size"]) ** 2


def assert_kernels(c, cfg, bf16):
    """The case reaches the kernels its row of the table names (no GPU call)."""
    prec = nat.VP_BF16 if bf16 else nat.VP_F32
    cap = cfg["atten_logit_cap"]
    dh = cfg["model_dim"] // cfg["num_heads"]
    got = (nat.dev_attention_choice(nat.ATT_VIDEO, prec, patches(cfg, c.hw), cap, c.padded, dim_per_head=dh),
           nat.dev_attention_choice(nat.ATT_VIDEO, prec, c.T, cap, c.padded, dim_per_head=dh))
    want = (c.spatial, c.temporal) if bf16 else (c.spatial_f32, c.temporal_f32)
    assert got == want, (case_id(c), got, want)


def frame_paddings(B, T):
    """[B, T] float32, the patterns of test_gpu_encoder.py and one more: clip 0 fully padded (uniform attention
    everywhere), clip 1 with its first and last frame padded, clip 2 with its second half padded
    (encoders_test.py:138-142).  At T = 2 clip 1 pads frame 0 and clip 2 frame 1.  Further clips repeat the three.

    The fully padded clip comes first on purpose.  Clip 0 sits at the same rows, and so in the same slots of a
    sequence-packed attention workgroup, alone and in a batch; only the later clips move (at 144 x 144, T = 3: clip 1
    by 3 of a workgroup's 4 slots, clip 2 by 2), and a clip of uniform attention cannot tell one row sum from
    another."""
    fp = np.zeros((B, T), np.float32)
    for b in range(B):
        if b % 3 == 0:
            fp[b, :] = 1.0
        elif b % 3 == 1:
            fp[b, 0] = 1.0
            if T > 2:
                fp[b, T - 1] = 1.0
        else:
            fp[b, T // 2:] = 1.0
    return fp


def clips(c, B, bf16, device, seed=0):
    """B clips of the case, uniform in [0, 1), as a device tensor in the model's dtype (bf16 values for a bf16
    model, so that the oracle can be given the very same frames)."""
    rng = np.random.default_rng(1000 * c.hw + 10 * c.T + seed)
    v = torch.from_numpy(rng.random((B, c.T, c.hw, c.hw, 3), dtype=np.float32)).to(device)
    return v.to(torch.bfloat16) if bf16 else v


def replace_padded_frames(video, fp, how, seed=0):
    """A copy of `video` with the pixels of the padded frames (fp [B, T] == 1) replaced: "random": other values,
    uniform in [-1, 2); "constant": 0.75.  All finite; nothing else changes."""
    out = video.clone()
    mask = torch.from_numpy(fp > 0).to(video.device)
    if how == "constant":
        out[mask] = 0.75
    else:
        g = torch.Generator(device="cpu").manual_seed(977 + seed)
        n = int(mask.sum())
        out[mask] = (torch.rand((n,) + tuple(video.shape[2:]), generator=g) * 3.0 - 1.0).to(video.device, video.dtype)
    return out
