"""What the reference promises about paddings, on the NumPy oracle at a tiny configuration (no GPU).  The bitwise GPU
tests in test_gpu_independence.py rely on these as properties of the reference itself, the negative one included:

  * the rows of valid frames ignore the pixels of padded frames, exactly, in every mode of the oracle;
  * a text embedding ignores the ids under its paddings, exactly;
  * the pooled heads (the classifier's logits, the video-text model's video embedding) do see the padded frames'
    pixels: the poolers are applied without paddings (encoders.py:583-653, :846-876), so nothing pins independence
    there.
"""

import numpy as np
import pytest

from oracle import videoprism_oracle as orc
from videoprism import params

ENC = dict(patch_size=2, pos_emb_shape=(4, 4, 4), model_dim=32, num_spatial_layers=1, num_temporal_layers=2,
           num_heads=2, mlp_dim=64, atten_logit_cap=50.0)
CLIP = dict(ENC, num_auxiliary_layers=1, num_unimodal_layers=2, vocabulary_size=50, enable_causal_atten=True)
B, T, HW, N = 2, 5, 6, 9
# both clips have padded frames: clip 0 its first and last, clip 1 one in the middle
FRAME_PADS = np.array([[1, 0, 0, 0, 1], [0, 0, 1, 0, 0]], np.float32)


def _videos():
    """The clips, and the same clips with the padded frames' pixels replaced (other random values; a constant)."""
    rng = np.random.default_rng(0)
    video = rng.random((B, T, HW, HW, 3), dtype=np.float32)
    padded = FRAME_PADS.astype(bool)
    other, const = video.copy(), video.copy()
    other[padded] = rng.random((int(padded.sum()), HW, HW, 3), dtype=np.float32) * 3.0 - 1.0
    const[padded] = 0.75
    return video, other, const


def _frame_rows(x):
    return x.reshape(B, T, N, x.shape[-1])


@pytest.mark.parametrize("mode", ["f64", "f32", "bf16"])
def test_valid_frames_ignore_padded_frames_pixels(mode):
    var = params.synthetic_params(ENC, seed=5)
    video, other, const = _videos()
    valid = FRAME_PADS == 0
    ref, rout = orc.factorized_encoder(var["params"], video, ENC, mode, frame_paddings=FRAME_PADS,
                                       return_intermediate=True)
    for changed in (other, const):
        got, gout = orc.factorized_encoder(var["params"], changed, ENC, mode, frame_paddings=FRAME_PADS,
                                           return_intermediate=True)
        for a, b in ((ref, got), (rout["spatial_features"], gout["spatial_features"])):
            a, b = _frame_rows(np.asarray(a, np.float64)), _frame_rows(np.asarray(b, np.float64))
            assert np.abs(a[valid] - b[valid]).max() == 0.0
            assert np.abs(a[~valid] - b[~valid]).max() > 0.0  # the padded frames' own rows do change


def test_text_ignores_ids_under_paddings():
    var = params.synthetic_params(CLIP, 6, specs=params.clip_leaf_specs(CLIP))
    rng = np.random.default_rng(1)
    L = 7
    ids = rng.integers(0, 50, (3, L)).astype(np.int32)
    pads = np.zeros((3, L), np.float32)
    pads[0, 4:] = 1.0
    pads[1, :] = 1.0  # a fully padded query
    ids2 = np.where(pads > 0, (ids + 1 + rng.integers(0, 48, ids.shape)) % 50, ids).astype(np.int32)
    assert (ids2 != ids)[pads > 0].all() and (ids2 == ids)[pads == 0].all()
    for mode in ("f64", "f32", "bf16"):
        _, t1, _ = orc.video_clip(var["params"], CLIP, None, ids, pads, mode)
        _, t2, _ = orc.video_clip(var["params"], CLIP, None, ids2, pads, mode)
        assert np.abs(np.asarray(t1, np.float64) - np.asarray(t2, np.float64)).max() == 0.0


def test_pooled_heads_see_padded_frames():
    """The negative fact: the pooler does not mask padded frames, so the logits and the video embedding move with
    their pixels, by far more than rounding."""
    video, other, _ = _videos()
    cvar = params.synthetic_params(ENC, 7, specs=params.classifier_leaf_specs(ENC, 10))
    l1, _ = orc.video_classifier(cvar["params"], ENC, video, frame_paddings=FRAME_PADS)
    l2, _ = orc.video_classifier(cvar["params"], ENC, other, frame_paddings=FRAME_PADS)
    var = params.synthetic_params(CLIP, 6, specs=params.clip_leaf_specs(CLIP))
    v1, _, _ = orc.video_clip(var["params"], CLIP, video, frame_paddings=FRAME_PADS)
    v2, _, _ = orc.video_clip(var["params"], CLIP, other, frame_paddings=FRAME_PADS)
    dl, dv = np.abs(l1 - l2).max(), np.abs(v1 - v2).max()
    print(f"padded frames' pixels replaced: logits move by {dl:.3e}, the video embedding by {dv:.3e}")
    assert dl > 1e-3 and dv > 1e-3
