"""Reader of tests/golden/ref_*.npz: what the reference's own program computed (oracle/make_ref_fixtures.py).

Shared by tests/test_reference_program.py (the oracle against the records) and by the GPU tests that hold the HIP
forward against the same records.  Reads the fixture files only: the GPU machines have no reference checkout.
"""

import json
import os

import numpy as np

from videoprism import params

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 1e-10          # |oracle - ref| <= BAR * max(1, |ref|): the bar between the project's fp64 restatements
MEASURED = {}        # largest |got - ref| per checked record, for the report

_FILES = {}


def fixture(name):
    if name not in _FILES:
        with np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False) as z:
            _FILES[name] = {k: z[k] for k in z.files}
    return _FILES[name]


class Case:
    """One case of a fixture file: inputs, parameter tree, configuration, recorded outputs."""

    def __init__(self, file, name):
        z = fixture(file)
        pre = name + "/"
        assert any(k.startswith(pre) for k in z), name
        self.name = name
        self.cfg = json.loads(str(z[pre + "cfg"]))
        if "pos_emb_shape" in self.cfg:
            self.cfg["pos_emb_shape"] = tuple(self.cfg["pos_emb_shape"])
        # float32 inputs are exact in float64, which is what the reference's program was handed
        self.inp = {k[len(pre) + 3:]: (v.astype(np.float64) if v.dtype.kind == "f" else v) for k, v in z.items()
                    if k.startswith(pre + "in/")}
        self.out = {k[len(pre):]: v for k, v in z.items()
                    if k.startswith(pre) and k.split("/")[1] not in ("in", "param", "cfg") and
                    not k.split("/")[1].startswith("param_")}
        self._flat = {k[len(pre) + 6:]: v for k, v in z.items() if k.startswith(pre + "param/")}
        self.seed = int(z[pre + "param_seed"]) if pre + "param_seed" in z else None
        self._z, self._pre = z, pre

    @property
    def tree(self):
        return params.unflatten(self._flat)

    def seeded_variables(self, specs=None):
        """Parameters recorded as seed + checksums: drawn again, and checked against the record."""
        z, pre = self._z, self._pre
        var = params.synthetic_params(self.cfg, self.seed, specs=specs)
        flat = params.flatten(var["params"])
        names = sorted(flat)
        assert names == list(z[pre + "param_names"])
        np.testing.assert_array_equal(np.stack([flat[k].ravel()[:4] for k in names]), z[pre + "param_heads"])
        np.testing.assert_allclose([float(np.sum(flat[k], dtype=np.float64)) for k in names], z[pre + "param_sums"],
                                   rtol=0, atol=1e-9)
        return var

    @property
    def video(self):
        """float32 frames: the bytes / 255 where the case holds bytes."""
        if "inputs_u8" in self.inp:
            return self.inp["inputs_u8"].astype(np.float32) / np.float32(255.0)
        return self.inp["inputs"].astype(np.float32)

    def records(self, key, got):
        """(record name, the part of `got` it covers, the record): the output itself, or -- for an output stored
        as a subsample -- every k-th token row, the sum of every row and the mean over the tokens."""
        got = np.asarray(got, np.float64)
        if key in self.out:
            return [(key, got, self.out[key])]
        rows = [k for k in self.out if k.startswith(key + "@rows") and not k.endswith("sums")]
        assert len(rows) == 1, (key, sorted(self.out))
        stride = int(rows[0].rsplit("@rows", 1)[1])
        return [(rows[0], got[:, ::stride], self.out[rows[0]]),
                (key + "@rowsums", got.sum(axis=-1), self.out[key + "@rowsums"]),
                (key + "@tokenmean", got.mean(axis=1), self.out[key + "@tokenmean"])]

    def check(self, key, got, bar=BAR):
        for k, g, ref in self.records(key, got):
            assert g.shape == ref.shape, (self.name, k, g.shape, ref.shape)
            assert ref.dtype == np.float64
            err = np.abs(g - ref)
            MEASURED[f"{self.name}/{k}"] = float(err.max())
            assert np.all(err <= bar * np.maximum(1.0, np.abs(ref))), (self.name, k, float(err.max()))
