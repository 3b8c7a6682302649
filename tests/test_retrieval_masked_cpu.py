"""The masked gallery search without a device: the new C-ABI symbols, every argument check of vp_op_topk_masked,
vp_op_topk_groups_masked and vp_op_rowmask_pack (they run before any device call, so fake device addresses are
enough), the workspace rule (the unmasked calls' sizes), the Python-side checks of EmbeddingIndex.remove / compact /
search(allow=...) on a CPU index, and the NumPy restatement (tests/masked_retrieval_cases.py) against itself."""

import ctypes

import numpy as np
import pytest
import torch

import grouped_retrieval_restatement as gr
import masked_retrieval_cases as mc
import retrieval_restatement as rr
from videoprism import _native
from videoprism.retrieval import EmbeddingIndex

P = 0x10000  # a 16-byte aligned address no check dereferences
VP_OK, VP_EINVAL, VP_ENOTSUP = _native.VP_OK, _native.VP_EINVAL, _native.VP_ENOTSUP


def _masked(**kw):
    a = dict(queries=P, Q=4, gallery=P, dtype=_native.VP_BF16, N=100, ld=768, D=768, k=10, id_base=0, mask=P, stride=0,
             scores=P, ids=P, ws=P, ws_bytes=_native.op_topk_workspace_bytes(4, 10), stream=None)
    a.update(kw)
    rc = _native.load().vp_op_topk_masked(a["queries"], a["Q"], a["gallery"], a["dtype"], a["N"], a["ld"], a["D"],
                                          a["k"], a["id_base"], a["mask"], a["stride"], a["scores"], a["ids"], a["ws"],
                                          a["ws_bytes"], a["stream"])
    return rc, _native.load().vp_last_error().decode()


def _groups_masked(**kw):
    a = dict(queries=P, Q=4, gallery=P, dtype=_native.VP_BF16, N=100, ld=768, D=768, labels=P, k=10, id_base=0, mask=P,
             stride=0, scores=P, groups=P, ids=P, ws=P, ws_bytes=_native.op_topk_groups_workspace_bytes(4, 10),
             stream=None)
    a.update(kw)
    rc = _native.load().vp_op_topk_groups_masked(a["queries"], a["Q"], a["gallery"], a["dtype"], a["N"], a["ld"],
                                                 a["D"], a["labels"], a["k"], a["id_base"], a["mask"], a["stride"],
                                                 a["scores"], a["groups"], a["ids"], a["ws"], a["ws_bytes"],
                                                 a["stream"])
    return rc, _native.load().vp_last_error().decode()


def _pack(**kw):
    a = dict(allow=P, Q=4, N=100, and_words=None, and_stride=0, out=P, stride=4, stream=None)
    a.update(kw)
    rc = _native.load().vp_op_rowmask_pack(a["allow"], a["Q"], a["N"], a["and_words"], a["and_stride"], a["out"],
                                           a["stride"], a["stream"])
    return rc, _native.load().vp_last_error().decode()


def test_symbols_exported_and_bound_and_the_abi_version_stays():
    lib = _native.load()
    for name in ("vp_op_rowmask_pack", "vp_op_topk_masked", "vp_op_topk_groups_masked"):
        assert name in _native.exported_symbols()
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
    assert lib.vp_abi_version() == 8


COMMON = [
    (dict(queries=None), VP_EINVAL, "queries"),
    (dict(gallery=None), VP_EINVAL, "gallery"),
    (dict(scores=None), VP_EINVAL, "scores"),
    (dict(ids=None), VP_EINVAL, "ids"),
    (dict(ws=None), VP_EINVAL, "ws"),
    (dict(mask=None), VP_EINVAL, "null mask"),
    (dict(mask=P + 2), VP_EINVAL, "mask must be 4-byte aligned"),
    (dict(mask=P + 1, stride=4), VP_EINVAL, "mask must be 4-byte aligned"),
    (dict(stride=-1), VP_EINVAL, "mask_query_stride_words"),
    (dict(stride=3), VP_EINVAL, "mask_query_stride_words"),  # 100 rows are 4 words
    (dict(N=-1), VP_EINVAL, "N"),
    (dict(Q=-1), VP_EINVAL, "Q"),
    (dict(k=0), VP_EINVAL, "k"),
    (dict(ld=760), VP_EINVAL, "ld"),
    (dict(queries=P + 4), VP_EINVAL, "queries"),
    (dict(gallery=P + 8), VP_EINVAL, "gallery"),
    (dict(ws_bytes=1024), VP_EINVAL, "ws_bytes"),
    (dict(D=800, ld=800), VP_ENOTSUP, "D"),
    (dict(k=129, ws_bytes=1 << 40), VP_ENOTSUP, "k"),
    (dict(dtype=_native.VP_U8), VP_ENOTSUP, "gallery_dtype"),
]


@pytest.mark.parametrize("kw, code, word", COMMON)
def test_topk_masked_argument_checks(kw, code, word):
    rc, msg = _masked(**kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("topk_masked: ") and word in msg, msg


@pytest.mark.parametrize("kw, code, word", COMMON + [
    (dict(labels=None), VP_EINVAL, "labels"),
    (dict(labels=P + 4), VP_EINVAL, "labels"),
    (dict(groups=None), VP_EINVAL, "groups"),
])
def test_topk_groups_masked_argument_checks(kw, code, word):
    rc, msg = _groups_masked(**kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("topk_groups_masked: ") and word in msg, msg


def test_masked_calls_that_launch_nothing_need_no_device():
    assert _masked(Q=0)[0] == VP_OK and _groups_masked(Q=0)[0] == VP_OK
    # a mask 4-byte but not 16-byte aligned, and a stride of exactly a mask's words, pass the checks (Q = 0 stops the
    # call before the launch)
    assert _masked(Q=0, mask=P + 4, stride=4)[0] == VP_OK
    # N == 0: the mask may be null (the refusal of a null mask is for N > 0); Q = 0 again keeps the device out of it
    assert _masked(Q=0, N=0, mask=None, gallery=None)[0] == VP_OK
    assert _groups_masked(Q=0, N=0, mask=None, gallery=None, labels=None)[0] == VP_OK


@pytest.mark.parametrize("kw, code, word", [
    (dict(allow=None), VP_EINVAL, "allow"),
    (dict(out=None), VP_EINVAL, "out_words"),
    (dict(out=P + 2), VP_EINVAL, "out_words"),
    (dict(and_words=P + 2), VP_EINVAL, "and_words"),
    (dict(and_words=P, and_stride=3), VP_EINVAL, "and_stride"),
    (dict(and_stride=-1), VP_EINVAL, "and_stride"),
    (dict(stride=3), VP_EINVAL, "stride"),
    (dict(N=-1), VP_EINVAL, "N"),
    (dict(Q=-1), VP_EINVAL, "Q"),
])
def test_rowmask_pack_argument_checks(kw, code, word):
    rc, msg = _pack(**kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("rowmask_pack: ") and word in msg, msg
    assert _pack(Q=0)[0] == VP_OK and _pack(N=0, stride=0)[0] == VP_OK


def test_the_unmasked_messages_keep_their_names():
    lib = _native.load()
    assert lib.vp_op_topk(None, 4, P, _native.VP_BF16, 100, 768, 768, 10, 0, P, P, P, 1 << 30, None) == VP_EINVAL
    assert lib.vp_last_error().decode() == "topk: null queries"
    assert lib.vp_op_topk_groups(P, 4, P, _native.VP_BF16, 100, 768, 768, None, 10, 0, P, P, P, P, 1 << 30,
                                 None) == VP_EINVAL
    assert lib.vp_last_error().decode() == "topk_groups: null labels"


def test_the_workspace_is_the_unmasked_calls():
    """The masked calls take vp_op_topk_workspace_bytes / vp_op_topk_groups_workspace_bytes: one byte fewer is
    refused, and the refusal names that number (that exactly that many are enough is the GPU tests' to show)."""
    for Q, k in ((1, 1), (4, 10), (33, 128)):
        for call, need in ((_masked, _native.op_topk_workspace_bytes(Q, k)),
                           (_groups_masked, _native.op_topk_groups_workspace_bytes(Q, k))):
            rc, msg = call(Q=Q, k=k, ws_bytes=need - 1)
            assert rc == VP_EINVAL and "too small" in msg and f"need {need}" in msg, msg


# ---- Python-side checks (a CPU index: nothing here reaches the library) ----
def _cpu_index(n=10, labels=False):
    index = EmbeddingIndex(64, dtype=torch.float32, device="cpu")
    emb = torch.arange(n, dtype=torch.float32)[:, None].repeat(1, 64)
    index.add(emb, group=torch.arange(n) // 2 if labels else None)
    return index


def test_remove_bookkeeping():
    index = _cpu_index()
    assert len(index) == 10 and index.live == 10
    index.remove([])
    assert index.live == 10
    index.remove(3)
    index.remove([3, 7])
    index.remove(np.array([7], dtype=np.int32))
    index.remove(torch.tensor([9]))
    assert len(index) == 10 and index.live == 7
    for bad in ([10], [-1], [0, 99], np.array([4, 10])):
        with pytest.raises(ValueError, match="out of range"):
            index.remove(bad)
    assert index.live == 7  # a refused call removed nothing, not even its valid ids
    with pytest.raises(ValueError):
        index.remove([1.5])
    with pytest.raises(ValueError):
        index.remove(np.zeros((2, 2), dtype=np.int64))
    # ids stay stable: add keeps appending, and the new rows are live
    assert index.add(torch.ones((30, 64))) == range(10, 40)
    assert len(index) == 40 and index.live == 37
    index.remove(39)
    assert index.live == 36


def test_compact_bookkeeping():
    index = _cpu_index(labels=True)
    index.remove([0, 3, 7, 9])
    old = index.compact()
    assert old.dtype == torch.int64 and old.tolist() == [1, 2, 4, 5, 6, 8]
    assert len(index) == 6 and index.live == 6
    assert index.embeddings[:, 0].tolist() == [1.0, 2.0, 4.0, 5.0, 6.0, 8.0]
    assert index.groups.tolist() == [0, 1, 2, 2, 3, 4]
    assert index.compact().tolist() == list(range(6))  # no tombstones: the identity
    assert index.add(torch.zeros((2, 64)), group=9) == range(6, 8)
    index.remove(range(8))
    assert index.live == 0 and index.compact().numel() == 0 and len(index) == 0
    plain = _cpu_index()
    assert plain.compact().tolist() == list(range(10)) and len(plain) == 10


def test_allow_argument_checks():
    index = _cpu_index()
    q = torch.zeros((3, 64))
    for allow, exc in ((np.ones(9, dtype=bool), ValueError), (np.ones((2, 10), dtype=bool), ValueError),
                       (np.ones((3, 10, 1), dtype=bool), ValueError), (torch.ones(11, dtype=torch.bool), ValueError),
                       (np.ones(10, dtype=np.float32), TypeError), (torch.ones(10, dtype=torch.int64), TypeError),
                       ([True] * 10, TypeError)):
        with pytest.raises(exc, match="allow"):
            index.search(q, 2, allow=allow)
    labelled = _cpu_index(labels=True)
    with pytest.raises(ValueError, match="allow"):
        labelled.search_groups(q, 2, allow=np.ones(9, dtype=bool))
    with pytest.raises(TypeError, match="allow"):
        labelled.search_groups(q, 2, allow=np.ones(10, dtype=np.int32))


def test_native_mask_argument_checks():
    q, g = torch.zeros((3, 64)), torch.zeros((40, 64))
    with pytest.raises(TypeError, match="mask"):
        _native.op_topk_masked(q, g, 2, torch.zeros(2, dtype=torch.int64))
    for mask in (torch.zeros(1, dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int32),
                 torch.zeros((3, 1), dtype=torch.int32)):
        with pytest.raises(ValueError, match="mask"):
            _native.op_topk_masked(q, g, 2, mask)
    with pytest.raises(TypeError, match="allow"):
        _native.op_rowmask_pack(torch.zeros(40))
    with pytest.raises(ValueError, match="allow"):
        _native.op_rowmask_pack(torch.zeros((2, 2, 2), dtype=torch.bool))


# ---- the restatement against itself ----
def test_pack_restatement():
    assert mc.pack([True]).tolist() == [1] and mc.pack([True], spare=1).tolist() == [0xFFFFFFFF]
    a = np.zeros(65, dtype=bool)
    a[[0, 31, 32, 64]] = True
    assert mc.pack(a).tolist() == [0x80000001, 1, 1]
    assert mc.pack(a, spare=1).tolist() == [0x80000001, 1, 0xFFFFFFFF]
    assert mc.pack(np.stack([a, ~a])).shape == (2, 3) and mc.pack(np.zeros(0, dtype=bool)).shape == (0,)
    for N in mc.NS:
        m = mc.make_mask("random.5", N, 1, seed=N)
        w = mc.pack(m)
        assert w.shape == (mc.words(N),)
        assert [(int(w[r >> 5]) >> (r & 31)) & 1 for r in range(N)] == m.astype(int).tolist()


def test_every_mask_kind_is_what_its_name_says():
    for c in mc.CASES:
        m = mc.make_mask(c.mask, c.N, c.Q)
        assert m.shape == ((c.Q, c.N) if c.mask.startswith("pq") else (c.N,)), c
        if c.mask.startswith("one@"):
            assert m.sum() == 1
        if c.mask == "few":
            assert 0 < m.sum() < max(c.k, 4)
        if c.mask in ("wave_clear", "tile_clear", "part_clear"):
            assert m.any() and not m.all()
        if c.mask == "pq_mixed" and c.Q > 2:
            assert not m[0].any() and m[1].all() and not m[-1].any() and m[-2].all()
    kinds = {c.mask for c in mc.CASES}
    assert {"ones", "zeros", "alternating", "wave_clear", "tile_clear", "part_clear", "few", "random.5", "random.03",
            "pq_random", "pq_mixed", "one@0", "one@31", "one@32", "one@63", "one@64", "one@511", "one@512",
            "one@last"} <= kinds
    assert {c.N for c in mc.CASES} == set(mc.NS)
    for c in mc.CASES:  # the workgroups of 16 queries are among the cases, plain and grouped
        assert c.D in (64, 1024, 1536) and c.k in (1, 5, 64, 128) and (c.Q in (1, 32, 33) or c.Q == 4096)
    assert any(_native.load().vp_dev_topk_group(c.D, c.k) == 16 and c.D == 1024 for c in mc.CASES if not c.grouped)
    assert any(_native.load().vp_dev_topk_groups_group(c.D, c.k) == 16 and c.D == 1024 for c in mc.CASES if c.grouped)


def test_an_all_ones_mask_is_the_unmasked_restatement():
    rng = np.random.default_rng(5)
    s = rng.integers(-3, 4, size=(70, 5)).astype(np.float64)
    s[rng.integers(0, 70, 6), rng.integers(0, 5, 6)] = np.nan
    labels = mc.masked_labels(70)
    for k in (1, 5, 128):
        for allow in (np.ones(70, dtype=bool), np.ones((5, 70), dtype=bool)):
            got = mc.masked_topk(s, allow, k, id_base=40)
            want = rr.topk(s, k, id_base=40)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            got = mc.masked_group_topk(s, labels, allow, k, id_base=40)
            want = gr.group_topk(s, labels, k, id_base=40)
            assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_the_restatement_leaves_out_what_is_not_allowed():
    #          row: 0    1    2    3    4
    s = np.array([[5.0, 5.0, 3.0, 9.0, 1.0]]).T
    sc, ids = mc.masked_topk(s, np.array([0, 1, 1, 0, 1], dtype=bool), 4, id_base=10)
    assert ids.tolist() == [[11, 12, 14, -1]] and sc.tolist() == [[5.0, 3.0, 1.0, -np.inf]]
    sc, ids = mc.masked_topk(s, np.zeros(5, dtype=bool), 2)
    assert ids.tolist() == [[-1, -1]] and np.isneginf(sc).all()
    # a group's best row is its best allowed row
    sc, g, ids = mc.masked_group_topk(s, np.array([7, 7, 8, 8, 8]), np.array([0, 1, 1, 0, 1], dtype=bool), 3)
    assert g.tolist() == [[7, 8, -1]] and ids.tolist() == [[1, 2, -1]] and sc[0, :2].tolist() == [5.0, 3.0]
    # per query
    s2 = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]]).T
    sc, ids = mc.masked_topk(s2, np.array([[1, 1, 0], [0, 0, 0]], dtype=bool), 2)
    assert ids.tolist() == [[1, 0], [-1, -1]]
