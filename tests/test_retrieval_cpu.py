"""Gallery search without a device: the three C-ABI symbols, every argument check of vp_op_topk / vp_op_topk_merge
(they run before any device call, so fake device addresses are enough), the workspace size, and the NumPy statement
of the order rule (tests/retrieval_restatement.py) on a hand-written case and on shards against the whole."""

import ctypes

import numpy as np
import pytest

import retrieval_restatement as rr
from videoprism import _native

P = 0x10000  # a 16-byte aligned address no check dereferences
VP_OK, VP_EINVAL, VP_ENOTSUP = _native.VP_OK, _native.VP_EINVAL, _native.VP_ENOTSUP


def _topk(**kw):
    a = dict(queries=P, Q=4, gallery=P, dtype=_native.VP_BF16, N=100, ld=768, D=768, k=10, id_base=0, scores=P,
             ids=P, ws=P, ws_bytes=_native.op_topk_workspace_bytes(4, 10), stream=None)
    a.update(kw)
    rc = _native.load().vp_op_topk(a["queries"], a["Q"], a["gallery"], a["dtype"], a["N"], a["ld"], a["D"], a["k"],
                                   a["id_base"], a["scores"], a["ids"], a["ws"], a["ws_bytes"], a["stream"])
    return rc, _native.load().vp_last_error().decode()


def _merge(**kw):
    a = dict(scores_in=P, ids_in=P, parts=3, Q=4, k_in=10, k=10, scores=P, ids=P, stream=None)
    a.update(kw)
    rc = _native.load().vp_op_topk_merge(a["scores_in"], a["ids_in"], a["parts"], a["Q"], a["k_in"], a["k"],
                                         a["scores"], a["ids"], a["stream"])
    return rc, _native.load().vp_last_error().decode()


def test_symbols_exported_and_bound():
    lib = _native.load()
    for name in ("vp_op_topk_workspace_bytes", "vp_op_topk", "vp_op_topk_merge"):
        assert name in _native.exported_symbols()
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
    assert lib.vp_abi_version() == 8


@pytest.mark.parametrize("kw, code, word", [
    (dict(queries=None), VP_EINVAL, "queries"),
    (dict(gallery=None), VP_EINVAL, "gallery"),
    (dict(scores=None), VP_EINVAL, "scores"),
    (dict(ids=None), VP_EINVAL, "ids"),
    (dict(ws=None), VP_EINVAL, "ws"),
    (dict(k=0), VP_EINVAL, "k"),
    (dict(ld=760), VP_EINVAL, "ld"),
    (dict(ld=772), VP_EINVAL, "ld"),
    (dict(queries=P + 4), VP_EINVAL, "queries"),
    (dict(gallery=P + 8), VP_EINVAL, "gallery"),
    (dict(ws_bytes=1024), VP_EINVAL, "ws_bytes"),
    (dict(D=800, ld=800), VP_ENOTSUP, "D"),
    (dict(D=1600, ld=1600), VP_ENOTSUP, "D"),
    (dict(k=129, ws_bytes=1 << 40), VP_ENOTSUP, "k"),
    (dict(dtype=_native.VP_U8), VP_ENOTSUP, "gallery_dtype"),
    (dict(dtype=7), VP_ENOTSUP, "gallery_dtype"),
])
def test_topk_argument_checks(kw, code, word):
    rc, msg = _topk(**kw)
    assert rc == code, (rc, msg)
    assert word in msg, msg


def test_topk_no_queries_is_ok_without_a_device():
    rc, msg = _topk(Q=0)
    assert rc == VP_OK, msg


@pytest.mark.parametrize("kw, code, word", [
    (dict(scores_in=None), VP_EINVAL, "scores_in"),
    (dict(ids_in=None), VP_EINVAL, "ids_in"),
    (dict(scores=None), VP_EINVAL, "scores"),
    (dict(ids=None), VP_EINVAL, "ids"),
    (dict(k=0), VP_EINVAL, "k"),
    (dict(k=11), VP_EINVAL, "k_in"),
    (dict(parts=0), VP_EINVAL, "parts"),
    (dict(k_in=129, k=129), VP_ENOTSUP, "k_in"),
])
def test_merge_argument_checks(kw, code, word):
    rc, msg = _merge(**kw)
    assert rc == code, (rc, msg)
    assert word in msg, msg
    assert _merge(Q=0)[0] == VP_OK


def test_workspace_bytes_needs_no_device_and_does_not_shrink():
    n = ctypes.c_size_t()
    lib = _native.load()
    assert lib.vp_op_topk_workspace_bytes(4, 10, None) == VP_EINVAL
    assert lib.vp_op_topk_workspace_bytes(4, 0, ctypes.byref(n)) == VP_EINVAL
    assert lib.vp_op_topk_workspace_bytes(4, 129, ctypes.byref(n)) == VP_ENOTSUP
    prev = 0
    for Q in (0, 1, 2, 31, 32, 33, 256, 1000):
        row = [_native.op_topk_workspace_bytes(Q, k) for k in (1, 2, 10, 64, 128)]
        assert all(a <= b for a, b in zip(row, row[1:])), (Q, row)
        assert row[0] >= prev
        prev = row[0]
        if Q:
            assert row[2] >= 12 * Q * 10  # at least one list of (fp32 score, int64 id) per query


def test_restatement_hand_written_ties():
    nan, inf = np.nan, np.inf
    #          row: 0    1    2    3     4    5    6
    s = np.array([[2.0, 5.0, 2.0, nan, -inf, 5.0, 1.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]).T
    sc, ids = rr.topk(s, 4, id_base=100)
    assert ids.tolist() == [[101, 105, 100, 102], [100, 101, 102, 103]]
    assert sc.tolist() == [[5.0, 5.0, 2.0, 2.0], [0.0, 0.0, 0.0, 0.0]]
    sc, ids = rr.topk(s, 7)
    assert ids[0].tolist() == [1, 5, 0, 2, 6, -1, -1]  # the NaN and the -inf row are never returned
    assert sc[0].tolist() == [5.0, 5.0, 2.0, 2.0, 1.0, -inf, -inf]
    # merge: padding last, ties across lists by id
    ms, mi = rr.merge(np.array([[[3.0, 1.0, -inf]], [[3.0, 2.0, 1.0]]]), np.array([[[7, 9, -1]], [[4, 5, 8]]]), 5)
    assert mi.tolist() == [[4, 7, 5, 8, 9]] and ms.tolist() == [[3.0, 3.0, 2.0, 1.0, 1.0]]
    ms, mi = rr.merge(np.array([[[3.0, -inf]], [[-inf, -inf]]]), np.array([[[7, -1]], [[-1, -1]]]), 2)
    assert mi.tolist() == [[7, -1]] and ms.tolist() == [[3.0, -inf]]


def test_restatement_shards_merge_to_the_whole():
    rng = np.random.default_rng(3)
    s = rng.integers(-3, 4, size=(400, 6)).astype(np.float64)  # many ties
    s[rng.integers(0, 400, 20), rng.integers(0, 6, 20)] = np.nan
    for k in (1, 7, 50):
        whole = rr.topk(s, k, id_base=10)
        cuts = [0, 130, 131, 131, 400]  # one single-row and one empty shard
        lists = [rr.topk(s[a:b], k, id_base=10 + a) for a, b in zip(cuts, cuts[1:])]
        got = rr.merge(np.stack([l[0] for l in lists]), np.stack([l[1] for l in lists]), k)
        assert np.array_equal(got[1], whole[1]) and np.array_equal(got[0], whole[0])
