"""Which attention kernel the library picks (vpi::choose_attention through vp_dev_attention_choice; no GPU
call).  The forward (run_stack) and the op-level entry points the kernel parity tests call share that one
choice; the tables below are written out by hand from the three ladders it replaced, not computed."""

import pytest

from videoprism import _native
from videoprism._native import ATT_LONG, ATT_OP, ATT_TEXT, ATT_VIDEO, VP_BF16, VP_F32

S_VALUES = (1, 16, 17, 127, 128, 255, 256, 257, 4096)
CAPS = (0.0, 50.0, 50.5)  # no capping / the largest cap of the max-free softmax / just past it

ALL_MASKED = ("MASKED",) * 9
F32_SHORT = ("F32",) * 7

# (kind, precision, cap) -> the kernel at each of S_VALUES; key paddings never change a stack's kernel
STACK_TABLE = {
    (ATT_TEXT, VP_BF16, 0.0): ALL_MASKED,
    (ATT_TEXT, VP_BF16, 50.0): ("MASKED", "MASKED", "SEQ", "SEQ", "SEQ", "SEQ", "SEQ", "MASKED", "MASKED"),
    (ATT_TEXT, VP_BF16, 50.5): ALL_MASKED,
    (ATT_TEXT, VP_F32, 0.0): ALL_MASKED,
    (ATT_TEXT, VP_F32, 50.0): ALL_MASKED,
    (ATT_TEXT, VP_F32, 50.5): ALL_MASKED,
    (ATT_VIDEO, VP_BF16, 0.0): ALL_MASKED,
    (ATT_VIDEO, VP_BF16, 50.0): ("TEMPORAL", "TEMPORAL", "SEQ", "SEQ", "SEQ", "SEQ", "SPATIAL", "MASKED", "MASKED"),
    (ATT_VIDEO, VP_BF16, 50.5): ALL_MASKED,
    (ATT_VIDEO, VP_F32, 0.0): F32_SHORT + ("MASKED", "MASKED"),
    (ATT_VIDEO, VP_F32, 50.0): F32_SHORT + ("F32_MFMA", "F32_MFMA"),
    (ATT_VIDEO, VP_F32, 50.5): F32_SHORT + ("MASKED", "MASKED"),
    (ATT_LONG, VP_BF16, 0.0): ALL_MASKED,
    (ATT_LONG, VP_BF16, 50.0): ("TEMPORAL", "TEMPORAL", "SEQ", "SEQ", "SEQ", "SEQ", "LONG", "LONG", "LONG"),
    (ATT_LONG, VP_BF16, 50.5): ALL_MASKED,
    (ATT_LONG, VP_F32, 0.0): ALL_MASKED,
    (ATT_LONG, VP_F32, 50.0): ("F32_MFMA",) * 9,
    (ATT_LONG, VP_F32, 50.5): ALL_MASKED,
}

# vp_op_attention before the shared dispatch: (precision, cap, key paddings) -> the kernel at each of S_VALUES.
# bf16: online softmax outside the fast cap range; else the spatial kernel at 256, the auxiliary encoder's past
# 256 without paddings, the online softmax past 256 with them, the temporal kernel up to 16, the sequence
# kernel between.  fp32: attention_f32 up to 256, then the MFMA kernel (fast caps) or the online softmax.
OP_TABLE = {
    (VP_BF16, 0.0, False): ALL_MASKED,
    (VP_BF16, 0.0, True): ALL_MASKED,
    (VP_BF16, 50.0, False): ("TEMPORAL", "TEMPORAL", "SEQ", "SEQ", "SEQ", "SEQ", "SPATIAL", "LONG", "LONG"),
    (VP_BF16, 50.0, True): ("TEMPORAL", "TEMPORAL", "SEQ", "SEQ", "SEQ", "SEQ", "SPATIAL", "MASKED", "MASKED"),
    (VP_BF16, 50.5, False): ALL_MASKED,
    (VP_BF16, 50.5, True): ALL_MASKED,
    (VP_F32, 0.0, False): F32_SHORT + ("MASKED", "MASKED"),
    (VP_F32, 0.0, True): F32_SHORT + ("MASKED", "MASKED"),
    (VP_F32, 50.0, False): F32_SHORT + ("F32_MFMA", "F32_MFMA"),
    (VP_F32, 50.0, True): F32_SHORT + ("F32_MFMA", "F32_MFMA"),
    (VP_F32, 50.5, False): F32_SHORT + ("MASKED", "MASKED"),
    (VP_F32, 50.5, True): F32_SHORT + ("MASKED", "MASKED"),
}


def test_tables_cover_every_case():
    assert set(STACK_TABLE) == {(k, p, c) for k in (ATT_VIDEO, ATT_LONG, ATT_TEXT) for p in (VP_F32, VP_BF16)
                                for c in CAPS}
    assert set(OP_TABLE) == {(p, c, kp) for p in (VP_F32, VP_BF16) for c in CAPS for kp in (False, True)}


@pytest.mark.parametrize("key_pad", [False, True])
@pytest.mark.parametrize("kind,precision,cap", sorted(STACK_TABLE))
def test_stack_choice(kind, precision, cap, key_pad):
    got = tuple(_native.dev_attention_choice(kind, precision, S, cap, key_pad) for S in S_VALUES)
    assert got == STACK_TABLE[(kind, precision, cap)]


@pytest.mark.parametrize("precision,cap,key_pad", sorted(OP_TABLE))
def test_op_attention_choice(precision, cap, key_pad):
    """vp_op_attention's mapping (past 256 keys without paddings: ATT_LONG, else ATT_VIDEO) gives the kernels its
    own ladder gave."""
    got = tuple(_native.dev_attention_choice(ATT_OP, precision, S, cap, key_pad) for S in S_VALUES)
    assert got == OP_TABLE[(precision, cap, key_pad)]
    for S, want in zip(S_VALUES, got):
        kind = ATT_LONG if S > 256 and not key_pad else ATT_VIDEO
        assert _native.dev_attention_choice(kind, precision, S, cap, key_pad) == want


def test_op_attention_masked_is_the_text_stack():
    """vp_op_attention_masked before the shared dispatch: bf16 with a fast cap and 16 < S <= 256 on the
    sequence kernel, everything else on the online-softmax kernel."""
    for precision in (VP_F32, VP_BF16):
        for cap in CAPS:
            for S in S_VALUES:
                seq = precision == VP_BF16 and cap == 50.0 and S in (17, 127, 128, 255, 256)
                assert _native.dev_attention_choice(ATT_TEXT, precision, S, cap, True) == ("SEQ" if seq else "MASKED")


@pytest.mark.parametrize("kind,precision,S", [(3, VP_BF16, 16), (ATT_VIDEO, 2, 16), (ATT_VIDEO, VP_BF16, 0)])
def test_bad_arguments(kind, precision, S):
    with pytest.raises(ValueError):
        _native.dev_attention_choice(kind, precision, S, 50.0)
