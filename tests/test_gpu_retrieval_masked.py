"""The masked gallery search on the GPU (vp_op_topk_masked, vp_op_topk_groups_masked, vp_op_rowmask_pack,
EmbeddingIndex.remove / compact / search(allow=...)) at the shapes and masks of tests/masked_retrieval_cases.py.

The main check is the equivalence law: a masked search returns, bit for bit, what the unmasked vp_op_topk /
vp_op_topk_groups return on the gallery gathered to the allowed rows, ids mapped back.  The table's inputs are
ternary (-1, 0, 1): every product and sum is exact in both gallery dtypes, so against the NumPy restatement ids and
scores are equal exactly, through all the ties such inputs hold.  The unit-norm cases meet the bar of
tests/test_gpu_retrieval.py (2e-5, both dtypes) on inputs whose fp64 scores have no near-ties among the allowed
rows, which the test asserts first, so there too the ids are decided.
"""

import functools
import os

import numpy as np
import pytest
import torch

import grouped_retrieval_restatement as gr
import masked_retrieval_cases as mc
import retrieval_restatement as rr
import workspace_guard as wg
from videoprism import _native, distributed
from videoprism.retrieval import EmbeddingIndex

pytestmark = pytest.mark.gpu

BAR = 2e-5  # tests/test_gpu_retrieval.py's, for both gallery dtypes
DTYPES = [torch.float32, torch.bfloat16]


# ---- inputs ----
@functools.lru_cache(maxsize=None)
def _ternary(n, D, seed):
    return np.random.default_rng([seed, n, D]).integers(-1, 2, size=(n, D)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _dev(kind, n, D, seed, bf16=False):
    x = (_ternary if kind == "ternary" else mc.unit_rows)(n, D, seed)
    return torch.from_numpy(x).cuda().to(torch.bfloat16 if bf16 else torch.float32)


@functools.lru_cache(maxsize=None)
def _scores64(kind, N, Q, D, bf16):
    """fp64 scores [N, Q] of the stored gallery (seed 2) against the queries (seed 1): computed once per shape."""
    g = _dev(kind, N, D, 2, bf16).double().cpu().numpy()
    q = (_ternary if kind == "ternary" else mc.unit_rows)(Q, D, 1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return g @ q.T


def _labels(N):
    return torch.from_numpy(mc.masked_labels(N)).cuda()


def _words(allow):
    """allow bool NumPy [N] or [Q, N] -> the packed mask on the device, by the pack kernel."""
    return _native.op_rowmask_pack(torch.from_numpy(np.ascontiguousarray(allow)).cuda())


def _masked(q, g, k, words, labels=None, **kw):
    if labels is None:
        return _native.op_topk_masked(q, g, k, words, **kw)
    return _native.op_topk_groups_masked(q, g, labels, k, words, **kw)


def _unmasked(q, g, k, labels=None, **kw):
    if labels is None:
        return _native.op_topk(q, g, k, **kw)
    return _native.op_topk_groups(q, g, labels, k, **kw)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want):
    """None, or where two result tuples differ in their bits."""
    for name, a, b in zip(("scores", "groups" if len(got) == 3 else "ids", "ids"), got, want):
        d = wg.first_difference(a.contiguous(), b.contiguous())
        if d:
            return f"{name}: {d}"
    return None


def _gathered(q, g, k, allow, labels=None, id_base=0):
    """The law's right-hand side: per set of queries that share a mask, the unmasked call on the gallery gathered to
    that mask's rows, the ids mapped back through the rows."""
    Q, N = q.shape[0], g.shape[0]
    allow = np.broadcast_to(allow, (Q, N))
    outs = None
    uniq, inverse = np.unique(allow, axis=0, return_inverse=True)
    for u in range(uniq.shape[0]):
        qs = torch.from_numpy(np.nonzero(inverse.reshape(-1) == u)[0]).cuda()
        rows = torch.from_numpy(np.nonzero(uniq[u])[0]).cuda()
        res = list(_unmasked(q[qs].contiguous(), g[rows].contiguous(), k,
                             labels=None if labels is None else labels[rows].contiguous()))
        ids = res[-1]
        res[-1] = torch.where(ids >= 0, id_base + rows[ids.clamp(min=0)] if rows.numel() else ids, ids)
        if outs is None:
            outs = [torch.empty((Q,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in res]
        for o, t in zip(outs, res):
            o[qs] = t
    return tuple(outs)


# ---- 1, 2, 3: the table ----
@pytest.mark.parametrize("c", mc.CASES, ids=mc.case_id)
def test_masked_search_is_the_search_of_the_allowed_rows(cuda, c):
    q, g = _dev("ternary", c.Q, c.D, 1), _dev("ternary", c.N, c.D, 2, c.bf16)
    labels = _labels(c.N) if c.grouped else None
    allow = mc.make_mask(c.mask, c.N, c.Q)
    words = _words(allow)
    assert np.array_equal(words.cpu().numpy().view(np.uint32), mc.pack(allow))
    got = _masked(q, g, c.k, words, labels, id_base=c.id_base)
    # 1. the equivalence law, bit for bit
    want = _gathered(q, g, c.k, allow, labels, id_base=c.id_base)
    torch.cuda.synchronize()
    assert got[0].shape == (c.Q, c.k) and got[0].dtype == torch.float32 and got[-1].dtype == torch.int64
    assert _same(got, want) is None, _same(got, want)
    # 2. an all-ones mask is the unmasked call on the same gallery
    if c.mask == "ones":
        plain = _unmasked(q, g, c.k, labels, id_base=c.id_base)
        assert _same(got, plain) is None, _same(got, plain)
    # 3. the NumPy restatement: exact inputs, so ids and scores are equal exactly (inside the bar a fortiori)
    s64 = _scores64("ternary", c.N, c.Q, c.D, c.bf16)
    if c.grouped:
        ref = mc.masked_group_topk(s64, mc.masked_labels(c.N), allow, c.k, id_base=c.id_base)
    else:
        ref = mc.masked_topk(s64, allow, c.k, id_base=c.id_base)
    for a, b in zip(got[1:], ref[1:]):
        assert np.array_equal(a.cpu().numpy(), b)
    gs = got[0].cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isneginf(gs), np.isneginf(ref[0]))
    live = ~np.isneginf(gs)
    assert np.abs(gs[live] - ref[0][live]).max(initial=0.0) <= BAR
    assert np.array_equal(gs, ref[0])
    allowed = np.broadcast_to(allow, (c.Q, c.N)).sum(1)
    n_live = (got[-1].cpu().numpy() >= 0).sum(1)
    assert (n_live <= np.minimum(allowed, c.k)).all() and (c.grouped or (n_live == np.minimum(allowed, c.k)).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("N, D, Q, kind", [(1025, 1024, 33, "random.5"), (513, 64, 32, "pq_random"),
                                           (1025, 1536, 1, "wave_clear"), (65, 64, 33, "ones")])
def test_unit_norm_rows_meet_the_bar(cuda, dtype, N, D, Q, kind):
    bf16, k = dtype == torch.bfloat16, 5
    q, g = _dev("unit", Q, D, 1), _dev("unit", N, D, 2, bf16)
    allow = mc.make_mask(kind, N, Q, seed=3)
    s64 = _scores64("unit", N, Q, D, bf16)
    ref_s, ref_i = mc.masked_topk(s64, allow, k + 1)
    # a property of the inputs alone: where a query's best k + 1 allowed fp64 scores lie more than two bars apart,
    # scores inside the bar leave no choice of ids.  Most queries are such, and their ids must be exact; the others
    # (a near-tie in fp64) are held to the bar on the sorted scores
    with np.errstate(invalid="ignore"):
        gaps = -np.diff(ref_s, axis=1)
    decided = ((gaps > 2 * BAR) | ~np.isfinite(gaps)).all(1)
    assert decided.mean() >= 0.8, decided.mean()
    got_s, got_i = _native.op_topk_masked(q, g, k, _words(allow))
    torch.cuda.synchronize()
    assert np.array_equal(got_i.cpu().numpy()[decided], ref_i[decided, :k])
    assert np.array_equal(np.isneginf(got_s.cpu().numpy()), np.isneginf(ref_s[:, :k]))
    fin = np.isfinite(ref_s[:, :k])
    err = np.abs(got_s.cpu().numpy().astype(np.float64)[fin] - ref_s[:, :k][fin]).max()
    print(f"masked topk N={N} D={D} Q={Q} {kind} {dtype}: |score - fp64| max {err:.3e} (bar {BAR:.0e})")
    assert err <= BAR
    for labels in (None, _labels(N)):  # and the law on these inputs, both searches
        got = _masked(q, g, k, _words(allow), labels)
        want = _gathered(q, g, k, allow, labels)
        assert _same(got, want) is None, _same(got, want)
    if kind == "ones":
        assert _same((got_s, got_i), _native.op_topk(q, g, k)) is None
        pq = _native.op_topk_masked(q, g, k, _words(np.ones((Q, N), dtype=bool)))
        assert _same((got_s, got_i), pq) is None


# ---- 2 again: all-ones at every N, both forms, both searches ----
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_all_ones_is_the_unmasked_search_at_every_size(cuda, dtype):
    for N in mc.NS:
        Q, D, k = 33, 64, 5
        q, g = _dev("unit", Q, D, 1), _dev("unit", N, D, 2, dtype == torch.bfloat16)
        for labels in (None, _labels(N)):
            want = _unmasked(q, g, k, labels, id_base=11)
            for allow in (np.ones(N, dtype=bool), np.ones((Q, N), dtype=bool)):
                got = _masked(q, g, k, _words(allow), labels, id_base=11)
                assert _same(got, want) is None, (N, labels is not None, allow.shape, _same(got, want))


# ---- 4. ties ----
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_of_two_equal_rows_the_smaller_allowed_id_wins(cuda, dtype):
    N, D, Q = 1025, 64, 3
    q = _dev("unit", Q, D, 1)
    g = _dev("unit", N, D, 2, dtype == torch.bfloat16).clone()
    lo, hi = 40, 700  # in different waves and tiles
    g[lo] = g[hi] = q[0].to(dtype)  # query 0 itself: scores about 1, above every other row
    both = np.ones(N, dtype=bool)
    s, i = _native.op_topk_masked(q, g, 3, _words(both))
    assert i[0, :2].tolist() == [lo, hi] and s[0, 0].item() == s[0, 1].item()
    only_hi = both.copy()
    only_hi[lo] = False
    s2, i2 = _native.op_topk_masked(q, g, 3, _words(only_hi))
    assert i2[0, 0].item() == hi and s2[0, 0].item() == s[0, 0].item() and lo not in i2[0].tolist()
    assert i2[0, 1].item() == i[0, 2].item()
    # per query: query 0 sees only the larger copy, query 1 both
    pq = np.ones((Q, N), dtype=bool)
    pq[0, lo] = False
    s3, i3 = _native.op_topk_masked(q, g, 3, _words(pq))
    assert i3[0, 0].item() == hi and _same((s3[1:], i3[1:]), (s[1:], i[1:])) is None
    # groups: the copies in one group, the group's id is the smaller allowed one
    labels = torch.arange(N, device=cuda) % 50
    labels[lo] = labels[hi] = 1 << 35
    _, gg, gi = _native.op_topk_groups_masked(q, g, labels, 3, _words(both))
    assert (gg[0, 0].item(), gi[0, 0].item()) == (1 << 35, lo)
    _, gg, gi = _native.op_topk_groups_masked(q, g, labels, 3, _words(only_hi))
    assert (gg[0, 0].item(), gi[0, 0].item()) == (1 << 35, hi)


# ---- 5. bits past N, and nothing read past the mask's words ----
BAND = 129  # words on each side of the mask: an odd number, so the mask itself is only 4-byte aligned


def _banded_mask(words_np, band_fill):
    buf = torch.full((BAND + words_np.size + BAND,), band_fill, dtype=torch.int32, device="cuda")
    mid = buf[BAND:BAND + words_np.size].view(words_np.shape)
    mid.copy_(torch.from_numpy(words_np.view(np.int32)).cuda())
    assert words_np.size == 0 or mid.data_ptr() % 16 == 4
    return buf, mid


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "groups"])
@pytest.mark.parametrize("N", [1, 31, 33, 63, 65, 511, 513, 1025])
def test_spare_bits_and_what_follows_the_mask_do_not_matter(cuda, N, grouped):
    Q, D, k = 33, 64, 5
    q, g = _dev("ternary", Q, D, 1), _dev("ternary", N, D, 2, True)
    labels = _labels(N) if grouped else None
    for allow in (mc.make_mask("random.5", N, Q, seed=N), mc.make_mask("pq_random", N, Q, seed=N)):
        first = None
        for spare in (0, 1):
            for band in (0, -1):  # what lies around the mask: all zeros, all ones
                buf, words = _banded_mask(mc.pack(allow, spare=spare), band)
                got = _masked(q, g, k, words, labels)
                torch.cuda.synchronize()
                first = first or got
                assert _same(got, first) is None, (spare, band, _same(got, first))
                assert bool((buf[:BAND] == band).all()) and bool((buf[BAND + words.numel():] == band).all())
        want = _gathered(q, g, k, allow, labels)
        assert _same(first, want) is None


# ---- 6. rows that are not allowed may hold anything ----
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["random.5", "pq_random", "wave_clear"])
def test_nan_and_inf_in_rows_that_are_not_allowed(cuda, dtype, kind):
    N, D, Q, k = 513, 64, 33, 128
    q = _dev("ternary", Q, D, 1)
    clean = _dev("ternary", N, D, 2, dtype == torch.bfloat16)
    allow = mc.make_mask(kind, N, Q, seed=6).copy()
    allow[..., np.r_[64:128, 200:512:7]] = False  # a whole wave and scattered rows that no query allows
    never =torch.from_numpy(np.nonzero(~np.broadcast_to(allow, (Q, N)).any(0))[0]).cuda()  # allowed by no query
    assert never.numel() >= 30
    dirty = clean.clone()
    dirty[never[0::3]] = float("nan")
    dirty[never[1::3]] = float("inf")
    dirty[never[2::3], 0] = float("inf")
    words = _words(allow)
    for labels in (None, _labels(N)):
        got = _masked(q, dirty, k, words, labels)
        want = _masked(q, clean, k, words, labels)
        assert _same(got, want) is None, _same(got, want)
        assert not torch.isin(got[-1], never).any() and not torch.isnan(got[0]).any()
        assert not torch.isposinf(got[0]).any()
    s64 = _scores64("ternary", N, Q, D, dtype == torch.bfloat16)
    ref_s, ref_i = mc.masked_topk(s64, allow, k)
    got_s, got_i = _native.op_topk_masked(q, dirty, k, words)
    assert np.array_equal(got_i.cpu().numpy(), ref_i) and np.array_equal(got_s.cpu().numpy().astype(np.float64), ref_s)


# ---- 7. the pack kernel ----
@pytest.mark.parametrize("N", mc.NS + (0, 64, 2049))
def test_pack_kernel(cuda, N):
    rng = np.random.default_rng(70 + N)
    W = mc.words(N)
    for shape in ((N,), (3, N), (1, N)):
        allow = rng.random(shape) < 0.5
        want = mc.pack(allow)
        a_bool = torch.from_numpy(allow).cuda()
        a_u8 = torch.from_numpy(allow.astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)).cuda()  # any nonzero
        for a in (a_bool, a_u8):
            got = _native.op_rowmask_pack(a)
            assert got.dtype == torch.int32 and tuple(got.shape) == shape[:-1] + (W,)
            assert np.array_equal(got.cpu().numpy().view(np.uint32).reshape(want.shape), want)
        # the AND operand: one packed mask for every row of allow, or one each; its spare bits do not reach the output
        shared = mc.pack(rng.random(N) < 0.5, spare=1)
        got = _native.op_rowmask_pack(a_bool, and_words=torch.from_numpy(shared.view(np.int32)).cuda())
        assert np.array_equal(got.cpu().numpy().view(np.uint32).reshape(want.shape), want & shared)
        if len(shape) == 2:
            each = mc.pack(rng.random(shape) < 0.5, spare=1)
            got = _native.op_rowmask_pack(a_bool, and_words=torch.from_numpy(each.view(np.int32)).cuda())
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want & each)
    # only the words that hold a row are written: a banded output
    out, band = wg.banded((3, W), torch.int32, cuda, band_rows=4) if W else (None, None)
    if W:
        allow = rng.random((3, N)) < 0.5
        _native.op_rowmask_pack(torch.from_numpy(allow).cuda(), out=out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), mc.pack(allow)) and wg.band_intact(band)


# ---- 8. shards, on one GPU ----
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["random.5", "pq_mixed", "part_clear"])
def test_masked_shards_merge_to_the_bits_of_the_whole(cuda, dtype, kind):
    N, D, Q, k, base = 1025, 64, 33, 10, 5
    q, g = _dev("unit", Q, D, 1), _dev("unit", N, D, 2, dtype == torch.bfloat16)
    allow = mc.make_mask(kind, N, Q, seed=8)
    cuts = ((0, 333), (333, 334), (334, 847), (847, N))  # no boundary on a multiple of 32
    assert all(a % 32 for a, _ in cuts[1:])
    for labels in (None, _labels(N)):
        whole = _masked(q, g, k, _words(allow), labels, id_base=base)
        lists = [_masked(q, g[a:b], k, _words(allow[..., a:b]), None if labels is None else labels[a:b],
                         id_base=base + a) for a, b in cuts]
        stacked = [torch.stack([l[j] for l in lists]) for j in range(len(whole))]
        got = _native.op_topk_merge(*stacked, k) if labels is None else _native.op_topk_groups_merge(*stacked, k)
        torch.cuda.synchronize()
        assert _same(got, whole) is None, _same(got, whole)


# ---- 9. stream and workspace ----
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "groups"])
def test_side_stream_and_a_poisoned_workspace_of_the_exact_size(cuda, grouped):
    N, D, Q, k = 1025, 64, 33, 5
    q, g = _dev("unit", Q, D, 1), _dev("unit", N, D, 2, True)
    labels = _labels(N) if grouped else None
    words = _words(mc.make_mask("pq_random", N, Q, seed=9))
    want = _masked(q, g, k, words, labels)
    need = (_native.op_topk_groups_workspace_bytes if grouped else _native.op_topk_workspace_bytes)(Q, k)
    gw = wg.GuardedWorkspace(need, cuda)
    side = torch.cuda.Stream(device=cuda)
    entry = "vp_op_topk_groups_masked" if grouped else "vp_op_topk_masked"
    for fill in (0x00, 0xFF, 0x7F):
        gw.fill(fill)
        side.wait_stream(torch.cuda.current_stream())
        with gw.watch((entry,)):
            got = _masked(q, g, k, words, labels, stream=side, ws=gw.ws)
        side.synchronize()
        assert gw.damaged_guard() is None
        assert _same(got, want) is None, (fill, _same(got, want))
    assert [n for n, _ in gw.calls] == [entry] * 3
    short = wg.GuardedWorkspace(need, cuda, shrink=1)
    short.fill(0x00)
    with pytest.raises(ValueError, match=f"need {need}"), short.watch((entry,)):
        _masked(q, g, k, words, labels, ws=short.ws)


# ---- EmbeddingIndex ----
def _index(dtype, N=700, D=64, labels=False):
    index = EmbeddingIndex(D, dtype=dtype, device="cuda", capacity=4)
    g = mc.unit_rows(N, D, 2)
    lab = mc.masked_labels(N)
    for a, b in ((0, 300), (300, 301), (301, N)):
        index.add(g[a:b], group=lab[a:b] if labels else None)
    return index


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_index_allow_is_the_search_of_the_allowed_rows(cuda, dtype):
    index, Q, k = _index(dtype), 33, 10
    q = _dev("unit", Q, 64, 1)
    for kind in ("random.03", "pq_mixed", "zeros"):
        allow = mc.make_mask(kind, len(index), Q, seed=12)
        want = _gathered(q, index.embeddings, k, allow, id_base=1000)
        for a in (allow, allow.astype(np.uint8), torch.from_numpy(allow), torch.from_numpy(allow).cuda()):
            got = index.search(q, k, id_base=1000, allow=a)
            assert _same(got, want) is None, (kind, _same(got, want))
        np_s, np_i = index.search(q.cpu().numpy(), k, id_base=1000, allow=allow)
        assert isinstance(np_s, np.ndarray) and np.array_equal(np_i, want[1].cpu().numpy())
        assert np.array_equal(np_s.view(np.int32), want[0].cpu().numpy().view(np.int32))
    plain = index.search(q, k)
    assert _same(index.search(q, k, allow=np.ones(len(index), dtype=bool)), plain) is None


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "groups"])
def test_remove_then_search_is_compact_then_search(cuda, dtype, grouped):
    Q, k = 33, 10
    q = _dev("unit", Q, 64, 1)
    index = _index(dtype, labels=grouped)
    search = index.search_groups if grouped else index.search
    before = search(q, k)
    gone = np.unique(np.concatenate([before[-1][:, 0].cpu().numpy(),  # every query's best row, a whole wave, the ends
                                     np.arange(128, 192), [0, len(index) - 1]]))
    index.remove(gone)
    index.remove(gone[:3])
    assert len(index) == 700 and index.live == 700 - len(gone)
    alive = np.ones(700, dtype=bool)
    alive[gone] = False
    after = search(q, k)
    assert not np.isin(after[-1].cpu().numpy(), gone).any()
    stored, labels = index.embeddings.clone(), index.groups.clone() if grouped else None
    want = _gathered(q, stored, k, alive, labels)
    assert _same(after, want) is None, _same(after, want)
    # tombstones and a caller's filter: both hold
    allow = mc.make_mask("pq_random", 700, Q, seed=13)
    got = search(q, k, allow=allow)
    want2 = _gathered(q, stored, k, allow & alive, labels)
    assert _same(got, want2) is None, _same(got, want2)
    # rows added after a removal are live, and the mask follows the new length
    extra = mc.unit_rows(40, 64, 5)
    assert index.add(extra, group=7 if grouped else None) == range(700, 740)
    grown = search(q, k)
    want3 = _gathered(q, index.embeddings.clone(), k, np.concatenate([alive, np.ones(40, dtype=bool)]),
                      index.groups.clone() if grouped else None)
    assert _same(grown, want3) is None, _same(grown, want3)
    index.remove(range(700, 740))
    assert _same(search(q, k), after) is None
    # compact: the same lists with the ids mapped through old_ids, and then the unmasked path
    old_ids = index.compact()
    assert old_ids.dtype == torch.int64 and np.array_equal(old_ids.cpu().numpy(), np.nonzero(alive)[0])
    assert len(index) == index.live == int(alive.sum())
    assert torch.equal(index.embeddings, stored[old_ids])
    packed = search(q, k)
    mapped = torch.where(packed[-1] >= 0, old_ids[packed[-1].clamp(min=0)], packed[-1])
    assert _same(tuple(packed[:-1]) + (mapped,), after) is None


def test_masked_index_search_over_a_one_rank_communicator(cuda):
    """The sharded route of tests/test_gpu_retrieval.py on the one rank a single device allows, with tombstones and
    `allow`: bitwise the plain masked search."""
    import socket
    import torch.distributed as dist
    index, Q, k = _index(torch.bfloat16, labels=True), 5, 10
    q = _dev("unit", Q, 64, 1)
    index.remove([3, 64, 699])
    allow = mc.make_mask("random.5", 700, Q, seed=14)
    want = index.search(q, k, id_base=77, allow=allow)
    want_g = index.search_groups(q, k, id_base=77, allow=allow)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        with distributed.Communicator(0) as comm:
            got = index.search(q, k, comm=comm, id_base=77, allow=allow)
            got_g = index.search_groups(q, k, comm=comm, id_base=77, allow=allow)
            torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert _same(got, want) is None and _same(got_g, want_g) is None
