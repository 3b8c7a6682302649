"""Grouped gallery search without a device: the three C-ABI symbols, every argument check of vp_op_topk_groups /
vp_op_topk_groups_merge (they run before any device call, so fake device addresses are enough), the workspace size,
the NumPy statement of the rule (tests/grouped_retrieval_restatement.py) against the ungrouped one and on row ranges
that cut through groups, and the input conditions of the exact GPU cases (tests/test_gpu_retrieval_groups.py)."""

import ctypes
import os
import re

import numpy as np
import pytest

import grouped_retrieval_restatement as gr
import retrieval_restatement as rr
from grouped_retrieval_cases import many_ranges_case, ternary_case
from videoprism import _native

P = 0x10000  # a 16-byte aligned address no check dereferences
VP_OK, VP_EINVAL, VP_ENOTSUP = _native.VP_OK, _native.VP_EINVAL, _native.VP_ENOTSUP
NAMES = ("vp_op_topk_groups_workspace_bytes", "vp_op_topk_groups", "vp_op_topk_groups_merge")


def _groups(**kw):
    a = dict(queries=P, Q=4, gallery=P, dtype=_native.VP_BF16, N=100, ld=768, D=768, labels=P, k=10, id_base=0,
             scores=P, groups=P, ids=P, ws=P, ws_bytes=_native.op_topk_groups_workspace_bytes(4, 10), stream=None)
    a.update(kw)
    rc = _native.load().vp_op_topk_groups(a["queries"], a["Q"], a["gallery"], a["dtype"], a["N"], a["ld"], a["D"],
                                          a["labels"], a["k"], a["id_base"], a["scores"], a["groups"], a["ids"],
                                          a["ws"], a["ws_bytes"], a["stream"])
    return rc, _native.load().vp_last_error().decode()


def _merge(**kw):
    a = dict(scores_in=P, groups_in=P, ids_in=P, parts=3, Q=4, k_in=10, k=10, scores=P, groups=P, ids=P, stream=None)
    a.update(kw)
    rc = _native.load().vp_op_topk_groups_merge(a["scores_in"], a["groups_in"], a["ids_in"], a["parts"], a["Q"],
                                                a["k_in"], a["k"], a["scores"], a["groups"], a["ids"], a["stream"])
    return rc, _native.load().vp_last_error().decode()


def test_symbols_in_the_header_exported_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "videoprism_hip.h")) as f:
        header = f.read()
    lib = _native.load()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _native.exported_symbols()
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
    for name in ("op_topk_groups_workspace_bytes", "op_topk_groups", "op_topk_groups_merge"):
        assert callable(getattr(_native, name))


@pytest.mark.parametrize("kw, code, word", [
    (dict(queries=None), VP_EINVAL, "queries"),
    (dict(gallery=None), VP_EINVAL, "gallery"),
    (dict(labels=None), VP_EINVAL, "labels"),
    (dict(scores=None), VP_EINVAL, "scores"),
    (dict(groups=None), VP_EINVAL, "groups"),
    (dict(ids=None), VP_EINVAL, "ids"),
    (dict(ws=None), VP_EINVAL, "ws"),
    (dict(k=0), VP_EINVAL, "k"),
    (dict(N=-1), VP_EINVAL, "N"),
    (dict(ld=760), VP_EINVAL, "ld"),
    (dict(ld=772), VP_EINVAL, "ld"),
    (dict(queries=P + 4), VP_EINVAL, "queries"),
    (dict(gallery=P + 8), VP_EINVAL, "gallery"),
    (dict(labels=P + 4), VP_EINVAL, "labels"),
    (dict(ws=P + 8), VP_EINVAL, "ws"),
    (dict(ws_bytes=1024), VP_EINVAL, "ws_bytes"),
    (dict(ws_bytes=_native.op_topk_workspace_bytes(4, 10)), VP_EINVAL, "ws_bytes"),  # the ungrouped size is too small
    (dict(D=800, ld=800), VP_ENOTSUP, "D"),
    (dict(D=1600, ld=1600), VP_ENOTSUP, "D"),
    (dict(k=129, ws_bytes=1 << 40), VP_ENOTSUP, "k"),
    (dict(dtype=_native.VP_U8), VP_ENOTSUP, "gallery_dtype"),
    (dict(dtype=7), VP_ENOTSUP, "gallery_dtype"),
])
def test_topk_groups_argument_checks(kw, code, word):
    rc, msg = _groups(**kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("topk_groups: ") and word in msg[len("topk_groups: "):], msg


def test_topk_groups_no_queries_is_ok_without_a_device():
    rc, msg = _groups(Q=0)
    assert rc == VP_OK, msg
    rc, msg = _groups(Q=0, N=0, gallery=None, labels=None)
    assert rc == VP_OK, msg


@pytest.mark.parametrize("kw, code, word", [
    (dict(scores_in=None), VP_EINVAL, "scores_in"),
    (dict(groups_in=None), VP_EINVAL, "groups_in"),
    (dict(ids_in=None), VP_EINVAL, "ids_in"),
    (dict(scores=None), VP_EINVAL, "scores"),
    (dict(groups=None), VP_EINVAL, "groups"),
    (dict(ids=None), VP_EINVAL, "ids"),
    (dict(k=0), VP_EINVAL, "k"),
    (dict(k=11), VP_EINVAL, "k_in"),
    (dict(parts=0), VP_EINVAL, "parts"),
    (dict(Q=-1), VP_EINVAL, "Q"),
    (dict(k_in=129, k=129), VP_ENOTSUP, "k_in"),
])
def test_merge_argument_checks(kw, code, word):
    rc, msg = _merge(**kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("topk_groups_merge: ") and word in msg[len("topk_groups_merge: "):], msg
    assert _merge(Q=0)[0] == VP_OK


def test_workspace_bytes_needs_no_device_and_holds_three_lists():
    n = ctypes.c_size_t()
    lib = _native.load()
    assert lib.vp_op_topk_groups_workspace_bytes(4, 10, None) == VP_EINVAL
    assert lib.vp_op_topk_groups_workspace_bytes(4, 0, ctypes.byref(n)) == VP_EINVAL
    assert lib.vp_op_topk_groups_workspace_bytes(4, 129, ctypes.byref(n)) == VP_ENOTSUP
    prev = 0
    for Q in (0, 1, 2, 31, 32, 33, 256, 1000):
        row = [_native.op_topk_groups_workspace_bytes(Q, k) for k in (1, 2, 10, 64, 128)]
        assert all(a <= b for a, b in zip(row, row[1:])), (Q, row)
        assert row[0] >= prev
        prev = row[0]
        if Q:
            assert row[2] >= 20 * Q * 10  # at least one list of (fp32 score, int64 group, int64 id) per query
            assert row[2] > _native.op_topk_workspace_bytes(Q, 10)


def test_queries_per_workgroup_against_16_bytes_an_entry():
    """The grouped lists take 16 B an entry, so at D = 1024 a workgroup holds 32 queries only up to k = 63; the
    ungrouped choice keeps its meaning."""
    lib = _native.load()
    assert [lib.vp_dev_topk_groups_group(1024, k) for k in (1, 40, 63, 64, 128)] == [32, 32, 32, 16, 16]
    assert [lib.vp_dev_topk_group(1024, k) for k in (1, 63, 64, 127, 128)] == [32, 32, 32, 32, 16]
    # D = 768: 96 KB of queries and 512 k B of lists against 160 KB less the flags' 64 B
    assert [lib.vp_dev_topk_groups_group(768, k) for k in (10, 127, 128)] == [32, 32, 16]
    assert lib.vp_dev_topk_groups_group(1088, 1) == 16
    for D in range(64, 1537, 64):  # what it chooses fits the LDS of a CU
        for k in (1, 63, 64, 128):
            G = lib.vp_dev_topk_groups_group(D, k)
            assert D * G * 4 + G * k * 16 + 64 <= 160 * 1024, (D, k, G)


# ---- the restatement ----
def _scores(seed, N, Q):
    rng = np.random.default_rng(seed)
    s = rng.integers(-3, 4, size=(N, Q)).astype(np.float64)  # many ties
    s[rng.integers(0, N, 20), rng.integers(0, Q, 20)] = np.nan
    s[rng.integers(0, N, 5), rng.integers(0, Q, 5)] = -np.inf
    return s


def test_restatement_every_row_its_own_group_is_the_row_rule():
    s = _scores(3, 400, 6)
    for k in (1, 7, 50):
        want_s, want_i = rr.topk(s, k, id_base=10)
        got_s, got_g, got_i = gr.group_topk(s, np.arange(400), k, id_base=10)
        assert np.array_equal(got_s, want_s) and np.array_equal(got_i, want_i)
        assert np.array_equal(got_g, np.where(want_i < 0, -1, want_i - 10))


def test_restatement_one_group_is_the_smallest_argmax_then_padding():
    s = _scores(4, 300, 5)
    got_s, got_g, got_i = gr.group_topk(s, np.full(300, 1 << 40), 4, id_base=7)
    col = np.where(np.isnan(s), -np.inf, s)
    assert got_i[:, 0].tolist() == (7 + col.argmax(axis=0)).tolist()  # argmax returns the first of equal maxima
    assert got_s[:, 0].tolist() == col.max(axis=0).tolist() and (got_g[:, 0] == 1 << 40).all()
    assert np.isneginf(got_s[:, 1:]).all() and (got_g[:, 1:] == -1).all() and (got_i[:, 1:] == -1).all()


def test_restatement_hand_written():
    nan, inf = np.nan, np.inf
    #           row: 0    1    2    3     4    5    6    7
    s = np.array([[2.0, 5.0, 2.0, nan, -inf, 5.0, 1.0, 9.0]]).T
    lab = np.array([30, 20, 10, 10, 40, 30, 10, -1])
    sc, g, i = gr.group_topk(s, lab, 4, id_base=100)
    # group 30's best row is 5, which ties group 20's row 1: the smaller id first; row 7 is blanked, group 40 only -inf
    assert sc.tolist() == [[5.0, 5.0, 2.0, -inf]] and g.tolist() == [[20, 30, 10, -1]]
    assert i.tolist() == [[101, 105, 102, -1]]
    ms, mg, mi = gr.group_merge(np.array([[[5.0, 2.0, -inf]], [[5.0, 3.0, 1.0]]]),
                                np.array([[[20, 10, -1]], [[30, 10, 50]]]), np.array([[[7, 9, -1]], [[4, 5, 8]]]), 3)
    assert mg.tolist() == [[30, 20, 10]] and mi.tolist() == [[4, 7, 5]] and ms.tolist() == [[5.0, 5.0, 3.0]]


def test_restatement_row_ranges_that_cut_through_groups_merge_to_the_whole():
    s = _scores(5, 400, 6)
    lab = np.random.default_rng(5).integers(0, 40, 400) * 1000
    lab[::17] = -1
    cuts = [0, 130, 131, 131, 400]  # one single-row and one empty range
    for k_in, k_out in ((1, 1), (7, 7), (50, 50), (50, 12)):
        whole = gr.group_topk(s, lab, k_out, id_base=10)
        lists = [gr.group_topk(s[a:b], lab[a:b], k_in, id_base=10 + a) for a, b in zip(cuts, cuts[1:])]
        got = gr.group_merge(*(np.stack([l[j] for l in lists]) for j in range(3)), k_out)
        for a, b in zip(got, whole):
            assert np.array_equal(a, b)


# ---- the inputs of the exact GPU cases ----
def test_ternary_case_has_the_ties_it_is_for():
    _, _, s, lab = ternary_case()
    assert len(np.unique(lab)) == 60 and lab.max() > 1 << 32
    _, rows = rr.topk(s, 20)
    assert sum(len(set(lab[rows[r]].tolist())) < 20 for r in range(33)) == 33  # a repeated group in the plain top-20
    gs, gg, _ = gr.group_topk(s, lab, 21)
    assert sum(len(np.unique(gs[r, :20])) < 20 for r in range(33)) == 33  # tied group scores inside the top 20
    assert sum(gs[r, 19] == gs[r, 20] for r in range(33)) == 22  # a tie across the 20 / 21 boundary
    several = sum((s[lab == gg[r, j], r] == gs[r, j]).sum() > 1 for r in range(33) for j in range(20))
    assert several == 17  # returned groups that reach their maximum in more than one row
    both = sum((np.nonzero(lab == u)[0] < 512).any() and (np.nonzero(lab == u)[0] >= 512).any() for u in np.unique(lab))
    assert both == 5  # groups with rows on both sides of row 512, the first tile's end


def test_many_ranges_case_has_ties_across_ranges():
    _, _, s, lab = many_ranges_case()
    gs, _, _ = gr.group_topk(s, lab, 97)
    assert not np.isneginf(gs).any()
    for r in range(3):
        assert len(np.unique(gs[r])) in (11, 12)  # distinct group maxima
        assert gs[r, 63] == gs[r, 64]  # a tie across the k = 64 boundary
        spread = 0
        for u in range(97):
            rows = np.nonzero(lab == u)[0]
            best = rows[s[rows, r] == s[rows, r].max()]
            spread += len(set((best // 512).tolist())) > 1
        assert 19 <= spread <= 25, spread  # groups whose maximum occurs in more than one range of 512 rows
