"""The integer-valued inputs of the exact cases of the grouped gallery search, shared by
tests/test_retrieval_groups_cpu.py (which asserts the ties they hold) and tests/test_gpu_retrieval_groups.py.  Products
and sums of -1, 0, 1 are exact in every format, so the GPU must return the restatement's result bit for bit."""

import functools

import numpy as np


@functools.lru_cache(maxsize=None)
def ternary_case():
    """The inputs of tests/test_gpu_retrieval.py's exact case, with labels that exceed 2^32."""
    rng = np.random.default_rng(1)
    q = rng.integers(-1, 2, size=(33, 128)).astype(np.float32)
    g = rng.integers(-1, 2, size=(517, 128)).astype(np.float32)
    labels = np.random.default_rng(7).integers(0, 60, 517).astype(np.int64) * (1 << 33) + 5
    return q, g, g.astype(np.float64) @ q.astype(np.float64).T, labels


@functools.lru_cache(maxsize=None)
def many_ranges_case():
    rng = np.random.default_rng(11)
    q = rng.integers(-1, 2, size=(3, 64)).astype(np.float32)
    g = rng.integers(-1, 2, size=(20483, 64)).astype(np.float32)
    return q, g, g.astype(np.float64) @ q.astype(np.float64).T, np.arange(20483, dtype=np.int64) % 97
