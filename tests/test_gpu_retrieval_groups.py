"""The grouped gallery search on the GPU (vp_op_topk_groups, vp_op_topk_groups_merge,
EmbeddingIndex.search_groups) against the NumPy statement of its rule (tests/grouped_retrieval_restatement.py) and
fp64 scores of the stored gallery.  The exact cases' inputs and the ties they hold: tests/grouped_retrieval_cases.py,
asserted in tests/test_retrieval_groups_cpu.py.

The bar of case 4 is tests/test_gpu_retrieval.py's 2e-5 for the same scores; the measured maxima are written to
profiles/retrieval_groups/gpu_errors.txt."""

import functools
import os

import numpy as np
import pytest
import torch

import grouped_retrieval_restatement as gr
from grouped_retrieval_cases import many_ranges_case, ternary_case
from videoprism import _native, distributed
from videoprism.retrieval import EmbeddingIndex

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
BAR = 2e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _search(q, g, labels, k, **kw):
    s, gg, i = _native.op_topk_groups(q, g, labels, k, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), gg.cpu().numpy(), i.cpu().numpy()


def _dev(x, cuda, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    return t if dtype is None else t.to(dtype)


def _assert_exact(got, want):
    got_s, got_g, got_i = got
    want_s, want_g, want_i = want
    assert got_s.dtype == np.float32 and got_g.dtype == np.int64 and got_i.dtype == np.int64
    assert np.array_equal(got_g, want_g)
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(got_s.astype(np.float64), want_s)


# ---- 1. exact ----
@functools.lru_cache(maxsize=None)
def _ternary_want(labeling, k, id_base):
    _, _, s, lab = ternary_case()
    if labeling == "runs":
        lab = np.repeat(np.arange(47, dtype=np.int64), 11)
    return lab, gr.group_topk(s, lab, k, id_base=id_base)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", [1, 20, 128])
@pytest.mark.parametrize("labeling", ["wide", "runs"])
def test_exact(cuda, labeling, k, dtype):
    q, g, _, _ = ternary_case()
    lab, want = _ternary_want(labeling, k, 1000)
    assert len(lab) == 517
    got = _search(_dev(q, cuda), _dev(g, cuda, dtype), _dev(lab, cuda), k, id_base=1000)
    _assert_exact(got, want)
    if k == 128:  # fewer groups than k: the padded tail
        n = len(np.unique(lab))
        assert (got[1][:, n:] == -1).all() and (got[2][:, n:] == -1).all() and np.isneginf(got[0][:, n:]).all()
        assert (got[1][:, :n] >= 0).all()


# ---- 2. scripted order of events ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", [2, 3])
def test_scripted_order_of_events(cuda, k, dtype):
    """Rows 100 j + 7 arrive in this order (k = 2 in brackets): (1, 10) and (2, 20) fill the list; (3, 30) evicts
    group 10; (4, 10) brings it back and evicts 20; (5, 10) replaces in place; (4.5, 30) replaces the entry in the worst
    slot [k = 3: in place]; (4.5, 20) ties the k-th score with a larger row and must not displace [k = 3: evicts].  All
    other rows score 5 and are blanked.  The seven rows sit in different tiles of 512 and, within a tile, in different
    waves of 64 rows."""
    N, D = 700, 64
    events = [(1.0, 10), (2.0, 20), (3.0, 30), (4.0, 10), (5.0, 10), (4.5, 30), (4.5, 20)]
    g = np.zeros((N, D), np.float32)
    g[:, 0] = 5.0
    lab = np.full(N, -1, np.int64)
    for j, (sc, l) in enumerate(events):
        g[100 * j + 7, 0], lab[100 * j + 7] = sc, l
    q = np.zeros((1, D), np.float32)
    q[0, 0] = 1.0
    s = g.astype(np.float64) @ q.astype(np.float64).T
    want = gr.group_topk(s, lab, k, id_base=3)
    if k == 2:
        assert want[1].tolist() == [[10, 30]] and want[2].tolist() == [[3 + 407, 3 + 507]]
    else:
        assert want[1].tolist() == [[10, 30, 20]] and want[2].tolist() == [[3 + 407, 3 + 507, 3 + 607]]
    got = _search(_dev(q, cuda), _dev(g, cuda, dtype), _dev(lab, cuda), k, id_base=3)
    _assert_exact(got, want)


# ---- 3. degenerate labelings ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_row_its_own_group_is_bitwise_op_topk(cuda, dtype):
    q, g, _, _ = ternary_case()
    qd, gd = _dev(q, cuda), _dev(g, cuda, dtype)
    for k in (1, 20, 128):
        want_s, want_i = _native.op_topk(qd, gd, k, id_base=9)
        got_s, got_g, got_i = _native.op_topk_groups(qd, gd, torch.arange(517, device=cuda), k, id_base=9)
        torch.cuda.synchronize()
        assert torch.equal(got_i, want_i) and torch.equal(got_s.view(torch.int32), want_s.view(torch.int32))
        assert torch.equal(got_g, want_i - 9)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_group_and_blanked_rows(cuda, dtype):
    q, g, s, _ = ternary_case()
    qd, gd = _dev(q, cuda), _dev(g, cuda, dtype)
    one = np.full(517, (1 << 62) + 1, np.int64)
    got = _search(qd, gd, _dev(one, cuda), 5)
    _assert_exact(got, gr.group_topk(s, one, 5))
    assert got[2][:, 0].tolist() == s.argmax(axis=0).tolist() and (got[2][:, 1:] == -1).all()
    third = np.arange(517, dtype=np.int64) // 2
    third[::3] = -7  # every third label negative
    for k in (1, 20, 128):
        got = _search(qd, gd, _dev(third, cuda), k, id_base=50)
        _assert_exact(got, gr.group_topk(s, third, k, id_base=50))
        assert not np.isin(got[2][got[2] >= 0] - 50, np.arange(0, 517, 3)).any()
    got = _search(qd, gd, _dev(np.full(517, -1, np.int64), cuda), 4)  # everything blanked
    assert (got[1] == -1).all() and (got[2] == -1).all() and np.isneginf(got[0]).all()
    got = _search(qd, torch.empty((0, 128), dtype=dtype, device=cuda), torch.empty((0,), dtype=torch.int64, device=cuda), 3)
    assert (got[1] == -1).all() and (got[2] == -1).all() and np.isneginf(got[0]).all()


# ---- 4. against fp64 ----
@functools.lru_cache(maxsize=None)
def _unit(D, N=3001, Q=37, seed=2):
    """tests/test_gpu_retrieval.py's generator."""
    rng = np.random.default_rng(seed + D)
    q = rng.standard_normal((Q, D))
    g = rng.standard_normal((N, D))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return q.astype(np.float32), g.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _unit_ref(D, bf16):
    """(queries, stored gallery, labels row // 7) on the device and the fp64 scores [N, Q] of the stored gallery."""
    q, g = _unit(D)
    gd = torch.from_numpy(g).cuda().to(torch.bfloat16 if bf16 else torch.float32)
    lab = torch.arange(g.shape[0], device="cuda") // 7
    return torch.from_numpy(q).cuda(), gd, lab, gd.double().cpu().numpy() @ q.astype(np.float64).T


_ERRORS = {}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", [768, 1024, 1408])
def test_unit_norm_against_fp64(cuda, D, dtype):
    q, g, lab, s64 = _unit_ref(D, dtype == torch.bfloat16)
    k = 10
    got_s, got_g, got_i = _search(q, g, lab, k)
    N, Q = s64.shape
    labels = lab.cpu().numpy()
    want_s, _, _ = gr.group_topk(s64, labels, k)
    assert (got_i >= 0).all() and (got_i < N).all()
    assert np.array_equal(labels[got_i], got_g)  # each id lies in its group
    for r in range(Q):
        assert len(set(got_g[r].tolist())) == k  # distinct
        d = np.diff(got_s[r])
        assert (d <= 0).all() and (np.diff(got_i[r])[d == 0] > 0).all()  # ordered
    e_own = np.abs(s64[got_i, np.arange(Q)[:, None]] - got_s).max()
    e_top = np.abs(got_s.astype(np.float64) - want_s).max()
    _ERRORS[(D, IDS[DTYPES.index(dtype)])] = (e_own, e_top)
    print(f"topk_groups D={D} {dtype}: |score - fp64 score of its id| max {e_own:.3e}, |score - fp64 k-th group score| "
          f"max {e_top:.3e} (bar {BAR:.0e})")
    if len(_ERRORS) == 6:
        out = os.path.join(ROOT, "profiles", "retrieval_groups", "gpu_errors.txt")
        try:
            os.makedirs(os.path.dirname(out), exist_ok=True)
            with open(out, "w") as f:
                f.write("tests/test_gpu_retrieval_groups.py::test_unit_norm_against_fp64 (N = 3001, Q = 37, k = 10, labels "
                        f"row // 7), {torch.cuda.get_device_name(0)}; bar {BAR:.0e}\n")
                for (d, name), (a, b) in sorted(_ERRORS.items()):
                    f.write(f"  D={d:4d} {name:4s}: |score - fp64 score of its id| max {a:.3e}   |score - fp64 group score "
                            f"of its rank| max {b:.3e}\n")
        except OSError:  # a read-only checkout: the figures are printed above
            pass
    assert e_own <= BAR and e_top <= BAR


# ---- 5. both LDS group sizes ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k, G", [(40, 32), (128, 16)])
def test_both_query_group_sizes(cuda, k, G, dtype):
    """The ternary case widened to D = 1024 with zero columns (the scores stay exact): 33 queries are two workgroups of
    32 at k = 40 and three of 16 at k = 128."""
    assert _native.load().vp_dev_topk_groups_group(1024, k) == G
    q, g, s, lab = ternary_case()
    qw, gw = np.zeros((33, 1024), np.float32), np.zeros((517, 1024), np.float32)
    qw[:, 7::8], gw[:, 7::8] = q, g  # spread over the whole row
    got = _search(_dev(qw, cuda), _dev(gw, cuda, dtype), _dev(lab, cuda), k, id_base=1)
    _assert_exact(got, gr.group_topk(s, lab, k, id_base=1))


# ---- 6. many row ranges ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_many_row_ranges(cuda, dtype):
    """41 ranges of 512 rows, every group in every range, ties across the k boundary and between ranges: the
    deduplicating merge over several rounds."""
    q, g, s, lab = many_ranges_case()
    want = _many_want()
    got = _search(_dev(q, cuda), _dev(g, cuda, dtype), _dev(lab, cuda), 64, id_base=1 << 40)
    _assert_exact(got, want)


@functools.lru_cache(maxsize=None)
def _many_want():
    _, _, s, lab = many_ranges_case()
    return gr.group_topk(s, lab, 64, id_base=1 << 40)


# ---- 7. position independence ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_shards_that_cut_through_groups_merge_to_the_bits_of_the_whole(cuda, dtype):
    q, g, lab, _ = _unit_ref(768, dtype == torch.bfloat16)
    N = g.shape[0]
    whole = _native.op_topk_groups(q, g, lab, 10, id_base=5)
    cuts = ((0, 1000), (1000, 1001), (1001, N))
    assert int(lab[999]) == int(lab[1000]) and N % 7  # the cut at 1000 goes through a group, as does the gallery's end
    lists = [_native.op_topk_groups(q, g[a:b], lab[a:b], 10, id_base=5 + a) for a, b in cuts]
    stacked = [torch.stack([l[j] for l in lists]) for j in range(3)]
    got = _native.op_topk_groups_merge(*stacked, 10)
    head = _native.op_topk_groups_merge(*stacked, 3)
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(torch.int32), whole[0].view(torch.int32))
    assert torch.equal(got[1], whole[1]) and torch.equal(got[2], whole[2])
    # a shorter merge is the head of the longer one
    assert torch.equal(head[0].view(torch.int32), whole[0][:, :3].contiguous().view(torch.int32))
    assert torch.equal(head[1], whole[1][:, :3]) and torch.equal(head[2], whole[2][:, :3])
    # the lists in another order: the result depends on the set of entries alone
    again = _native.op_topk_groups_merge(*(t.flip(0) for t in stacked), 10)
    assert all(torch.equal(a, b) for a, b in zip(again, got))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_strided_gallery_and_repeat_are_bitwise(cuda, dtype):
    q, g, lab, _ = _unit_ref(768, dtype == torch.bfloat16)
    N, D = g.shape
    a = _native.op_topk_groups(q, g, lab, 10)
    wide = torch.full((N, D + 64), 3.0, dtype=dtype, device=cuda)
    wide[:, :D] = g
    b = _native.op_topk_groups(q, wide[:, :D], lab, 10)
    c = _native.op_topk_groups(q, g, lab, 10)
    torch.cuda.synchronize()
    for other in (b, c):
        assert torch.equal(other[0].view(torch.int32), a[0].view(torch.int32))
        assert torch.equal(other[1], a[1]) and torch.equal(other[2], a[2])


# ---- 8. EmbeddingIndex ----
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_index_add_with_groups_in_pieces_equals_the_op(cuda, dtype):
    q, g = _unit(768)
    index = EmbeddingIndex(768, dtype=dtype, device=cuda, capacity=4)
    assert index.groups is None
    with pytest.raises(ValueError):
        index.search_groups(q, 3)  # no labels
    lab = np.concatenate([np.full(3, 1 << 35), np.arange(10) // 4, np.arange(57) // 5 + 100]).astype(np.int64)
    lab[20] = -1
    ids = [index.add(g[:3], group=1 << 35), index.add(torch.from_numpy(g[3:13]).to(cuda), group=lab[3:13]),
           index.add(g[13:70], group=torch.from_numpy(lab[13:70]).to(cuda))]
    assert ids == [range(0, 3), range(3, 13), range(13, 70)]
    assert len(index) == 70 and index.capacity == 128  # grown from 4
    assert index.groups.dtype == torch.int64 and index.groups.shape == (70,)
    assert np.array_equal(index.groups.cpu().numpy(), lab)
    with pytest.raises(ValueError):
        index.add(g[70:71])  # labels held: group is required
    with pytest.raises(ValueError):
        index.add(g[70:72], group=np.zeros(3, np.int64))  # wrong length
    assert len(index) == 70
    plain = EmbeddingIndex(768, dtype=dtype, device=cuda)
    plain.add(g[:2])
    with pytest.raises(ValueError):
        plain.add(g[2:4], group=1)  # rows without labels held
    with pytest.raises(ValueError):
        plain.search_groups(q, 3)

    qd = torch.from_numpy(q).to(cuda)
    want = _native.op_topk_groups(qd, index.embeddings, torch.from_numpy(lab).to(cuda), 10)
    got = index.search_groups(qd, 10)
    assert all(isinstance(t, torch.Tensor) for t in got)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    np_s, np_g, np_i = index.search_groups(q, 10, id_base=1000)
    assert isinstance(np_s, np.ndarray) and np_s.dtype == np.float32 and np_g.dtype == np.int64 and np_i.dtype == np.int64
    assert np.array_equal(np_s, want[0].cpu().numpy()) and np.array_equal(np_g, want[1].cpu().numpy())
    assert np.array_equal(np_i, want[2].cpu().numpy() + 1000)
    # search on the labeled index is the ungrouped search
    want_s, want_i = _native.op_topk(qd, index.embeddings, 10)
    got_s, got_i = index.search(qd, 10)
    assert torch.equal(got_i, want_i) and torch.equal(got_s.view(torch.int32), want_s.view(torch.int32))


def test_index_search_groups_over_a_one_rank_communicator(cuda):
    """The sharded route (search, gather the three lists over RCCL, merge) on the one rank a single device allows:
    bitwise the plain call.  Bootstrapped as tests/test_gpu_retrieval.py's one-rank test."""
    import socket
    import torch.distributed as dist
    q, g = _unit(768)
    index = EmbeddingIndex(768, device=cuda)
    index.add(g[:500], group=np.arange(500, dtype=np.int64) // 6)
    qd = torch.from_numpy(q).to(cuda)
    want = index.search_groups(qd, 10, id_base=77)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        with distributed.Communicator(0) as comm:
            got = index.search_groups(qd, 10, comm=comm, id_base=77)
            torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
