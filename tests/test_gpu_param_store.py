"""Parameter intake of the three handle types (vp_*, vp_clip_*, vp_classifier_*) through raw ctypes: leaf
enumeration, validation messages and states.  They share one store (csrc/vp_params.h) and the two wrapping
handles one base (vp_clip.cpp WrapHandle), so every case runs for all three.  *_create needs a device count;
no kernel is launched.  One more case: an Engine built and dropped at interpreter exit leaves cleanly."""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from videoprism import _native
from videoprism import params as params_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the smallest configuration the library accepts (dim_per_head 64, dims multiples of 256)
CFG = dict(patch_size=2, pos_emb_shape=(2, 2, 2), model_dim=256, num_spatial_layers=1, num_temporal_layers=1,
           num_heads=4, mlp_dim=256, atten_logit_cap=50.0)
LVT = dict(CFG, num_auxiliary_layers=1, vocabulary_size=8, num_unimodal_layers=1, enable_causal_atten=True)
NUM_CLASSES = 3


def _vp_config():
    return _native.vp_config(patch_size=2, pos_emb_t=2, pos_emb_h=2, pos_emb_w=2, model_dim=256, num_spatial_layers=1,
                             num_temporal_layers=1, num_heads=4, mlp_dim=256, atten_logit_cap=50.0,
                             fprop_dtype=_native.VP_BF16)


def _create_args(family):
    if family == "vp":
        return (ctypes.byref(_vp_config()),)
    if family == "vp_clip":
        return (ctypes.byref(_native.vp_clip_config(video=_vp_config(), num_auxiliary_layers=1, vocabulary_size=8,
                                                    num_unimodal_layers=1, enable_causal_atten=1)),)
    return (ctypes.byref(_vp_config()), NUM_CLASSES)


# family -> (the expected leaves, the prefix of the wrapped encoder's leaves)
FAMILIES = {
    "vp": (params_lib.encoder_leaf_specs(CFG), ""),
    "vp_clip": (params_lib.clip_leaf_specs(LVT), "vision_encoder/"),
    "vp_classifier": (params_lib.classifier_leaf_specs(CFG, NUM_CLASSES), "encoder/"),
}
WRAPPERS = ("vp_clip", "vp_classifier")


class Handle:
    def __init__(self, family):
        self.lib = _native.load()
        self.family = family
        self.specs, self.prefix = FAMILIES[family]
        self.h = ctypes.c_void_p()
        assert self.fn("create")(*_create_args(family), 0, ctypes.byref(self.h)) == _native.VP_OK, self.error()

    def fn(self, name):
        return getattr(self.lib, f"{self.family}_{name}")

    def error(self):
        return self.lib.vp_last_error().decode()

    def set(self, name, shape=None, handle=None, family=None):
        shape = tuple(self.specs[name] if shape is None else shape)
        a = np.zeros(max(int(np.prod(shape)), 1), dtype=np.float32)
        fn = getattr(self.lib, f"{family or self.family}_set_param")
        return fn(handle or self.h, name.encode(), a.ctypes.data_as(ctypes.c_void_p),
                  (ctypes.c_int64 * len(shape))(*shape), len(shape))

    def set_all(self, skip=()):
        for name in self.specs:
            if name not in skip:
                assert self.set(name) == _native.VP_OK, self.error()

    def names(self):
        n = ctypes.c_int()
        assert self.fn("param_count")(self.h, ctypes.byref(n)) == _native.VP_OK
        out = []
        for i in range(n.value):
            s = ctypes.c_char_p()
            assert self.fn("param_name")(self.h, i, ctypes.byref(s)) == _native.VP_OK
            out.append(s.value.decode())
        s = ctypes.c_char_p()
        assert self.fn("param_name")(self.h, n.value, ctypes.byref(s)) == _native.VP_EINVAL
        return out

    def video_handle(self):
        v = ctypes.c_void_p()
        assert self.fn("video_handle")(self.h, ctypes.byref(v)) == _native.VP_OK
        return v


@pytest.fixture(params=sorted(FAMILIES))
def handle(request, cuda):
    h = Handle(request.param)
    yield h
    assert h.fn("destroy")(h.h) == _native.VP_OK


def _own(h):
    """A leaf of the handle itself (for a wrapper: not one of the wrapped encoder's)."""
    return [n for n in h.specs if not (h.prefix and n.startswith(h.prefix))][-1]


def test_enumeration(handle):
    names = handle.names()
    assert len(names) == len(set(names)) == len(handle.specs)
    assert set(names) == set(handle.specs)
    if handle.prefix:  # the wrapped encoder's leaves first, under their prefix
        n_enc = len(params_lib.encoder_leaf_specs(CFG))
        assert all(n.startswith(handle.prefix) for n in names[:n_enc])
        assert not any(n.startswith(handle.prefix) for n in names[n_enc:])
        assert {n[len(handle.prefix):] for n in names[:n_enc]} == set(params_lib.encoder_leaf_specs(CFG))


def test_unknown_name(handle):
    for name in ("no/such/leaf", handle.prefix + "no/such/leaf"):
        assert handle.set(name, shape=(1,)) == _native.VP_EINVAL
        assert handle.error() == f"unexpected parameter: {name}"


def test_wrong_shape(handle):
    for name in {_own(handle), next(iter(handle.specs))}:  # a leaf of its own and (wrappers) one of the encoder's
        want = handle.specs[name]
        given = tuple(want) + (2,)
        assert handle.set(name, shape=given) == _native.VP_EINVAL
        msg = handle.error()
        assert msg.startswith(f"shape mismatch for {name}")
        assert "expected (" + ", ".join(map(str, want)) + ")" in msg
        assert "got (" + ", ".join(map(str, given)) + ")" in msg


def test_missing_leaf(handle):
    missing = {_own(handle), next(iter(handle.specs))}  # a leaf of its own and (wrappers) one of the encoder's
    handle.set_all(skip=missing)
    while missing:  # finalize names one missing leaf at a time
        assert handle.fn("finalize")(handle.h) == _native.VP_ESTATE
        msg = handle.error()
        assert msg.startswith("missing parameter: ") and msg[len("missing parameter: "):] in missing
        name = msg[len("missing parameter: "):]
        assert handle.set(name) == _native.VP_OK, handle.error()
        missing.remove(name)
    # complete: now it finalizes, and then takes no more leaves
    assert handle.fn("finalize")(handle.h) == _native.VP_OK, handle.error()
    for name in {_own(handle), next(iter(handle.specs))}:
        assert handle.set(name) == _native.VP_ESTATE
    assert handle.fn("finalize")(handle.h) == _native.VP_OK  # idempotent


@pytest.mark.parametrize("family", WRAPPERS)
def test_prefixed_leaves_land_in_the_wrapped_handle(cuda, family):
    h = Handle(family)
    try:
        video = h.video_handle()
        enc = [n for n in h.specs if n.startswith(h.prefix)]
        assert len(enc) == len(params_lib.encoder_leaf_specs(CFG))
        n = ctypes.c_int()
        assert h.lib.vp_param_count(video, ctypes.byref(n)) == _native.VP_OK and n.value == len(enc)
        for name in enc[:-1]:
            assert h.set(name) == _native.VP_OK, h.error()
        # the wrapped handle holds all but the last of its leaves: it names that one
        assert h.lib.vp_finalize(video) == _native.VP_ESTATE
        assert h.error() == f"missing parameter: {enc[-1]}"
        # a leaf of the wrapper's own is none of the wrapped handle's
        assert h.set(_own(h), handle=video, family="vp") == _native.VP_EINVAL
        assert h.error() == f"unexpected parameter: {_own(h)}"
        assert h.set(enc[-1]) == _native.VP_OK
        assert h.lib.vp_finalize(video) == _native.VP_OK, h.error()
    finally:
        assert h.fn("destroy")(h.h) == _native.VP_OK


CHILD = """
import sys
sys.path[:0] = [ROOT, ROOT + "/videoprism-mlx_amd"]
import numpy as np
from videoprism import encoders, params
cfg = CFG
flat = {k: np.zeros(s, np.float32) for k, s in params.encoder_leaf_specs(cfg).items()}
eng = encoders.Engine(cfg, flat, 0, True)
assert eng.video_handle() is eng._h
print("built")
"""


def test_engine_is_destroyed_cleanly_at_interpreter_exit(cuda):
    """The engine is still alive when the interpreter shuts down: its handle must be destroyed then without an
    "Exception ignored in __del__" (the module globals are already gone by then)."""
    code = CHILD.replace("ROOT", repr(ROOT)).replace("CFG", repr(CFG))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "built" in r.stdout
    assert "Exception ignored" not in r.stderr and "Traceback" not in r.stderr, r.stderr[-2000:]
