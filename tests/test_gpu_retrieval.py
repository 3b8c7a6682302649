"""The gallery search on the GPU (vp_op_topk, vp_op_topk_merge, videoprism.retrieval.EmbeddingIndex) against the
NumPy statement of its order rule (tests/retrieval_restatement.py) and fp64 scores of the stored gallery.

Measured on MI355X against the 2e-5 bar (the project's fp32 embedding bar), profiles/retrieval/gpu_errors.txt:
test_unit_norm_random fp32 gallery 1.3e-7 - 1.9e-7, bf16 gallery 2.4e-7 - 3.1e-7; test_many_partitions 2.8e-7.  CPU
emulation of these inputs gives 2.8e-4 for a query rounded to one bf16, which the bar refuses."""

import functools
import os

import numpy as np
import pytest
import torch

import retrieval_restatement as rr
from videoprism import _native, distributed
from videoprism.retrieval import EmbeddingIndex

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
BAR = 2e-5


def _stored64(g):
    return g.double().cpu().numpy()


def _search(q, g, k, **kw):
    s, i = _native.op_topk(q, g, k, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


# ---- 1. exact arithmetic ----
@functools.lru_cache(maxsize=None)
def _ternary():
    rng = np.random.default_rng(1)
    q = rng.integers(-1, 2, size=(33, 128)).astype(np.float32)
    g = rng.integers(-1, 2, size=(517, 128)).astype(np.float32)
    return q, g, g.astype(np.float64) @ q.astype(np.float64).T


def test_ternary_inputs_have_the_ties_the_case_is_for():
    _, _, s = _ternary()
    top = np.sort(s, axis=0)[::-1]
    inside = sum(len(np.unique(top[:20, q])) < 20 for q in range(33))
    across = sum(top[19, q] == top[20, q] for q in range(33))
    assert inside == 33 and across == 29, (inside, across)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("k", [1, 20, 128])
def test_exact_arithmetic(cuda, dtype, k):
    q, g, s = _ternary()
    want_s, want_i = rr.topk(s, k)
    got_s, got_i = _search(torch.from_numpy(q).to(cuda), torch.from_numpy(g).to(cuda).to(dtype), k)
    assert got_i.dtype == np.int64 and got_s.dtype == np.float32
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(got_s.astype(np.float64), want_s)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_fewer_rows_than_k_pads_the_tail(cuda, dtype):
    q, g, s = _ternary()
    want_s, want_i = rr.topk(s[:5], 8, id_base=40)
    got_s, got_i = _search(torch.from_numpy(q).to(cuda), torch.from_numpy(g[:5]).to(cuda).to(dtype), 8, id_base=40)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s.astype(np.float64), want_s)
    assert (got_i[:, 5:] == -1).all() and np.isneginf(got_s[:, 5:]).all()
    got_s, got_i = _search(torch.from_numpy(q).to(cuda), torch.empty((0, 128), dtype=dtype, device=cuda), 3)
    assert (got_i == -1).all() and np.isneginf(got_s).all()


# ---- 2. unit-norm random ----
@functools.lru_cache(maxsize=None)
def _unit(D, N=3001, Q=37, seed=2):
    rng = np.random.default_rng(seed + D)
    q = rng.standard_normal((Q, D))
    g = rng.standard_normal((N, D))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return q.astype(np.float32), g.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _unit_ref(D, bf16):
    """(queries, stored gallery) on the device and the fp64 scores [N, Q] of the stored gallery."""
    q, g = _unit(D)
    gd = torch.from_numpy(g).cuda().to(torch.bfloat16 if bf16 else torch.float32)
    return torch.from_numpy(q).cuda(), gd, _stored64(gd) @ q.astype(np.float64).T


def _check_against_f64(got_s, got_i, s64, k, id_base=0):
    """The bar of cases 2 and 4; returns the two measured maxima."""
    want_s, _ = rr.topk(s64, k)
    N, Q = s64.shape
    e_top = np.abs(got_s.astype(np.float64) - want_s).max()
    rows = got_i - id_base
    assert (rows >= 0).all() and (rows < N).all()
    e_own = np.abs(s64[rows, np.arange(Q)[:, None]] - got_s).max()
    for r in range(Q):
        assert len(set(got_i[r].tolist())) == k
        d = np.diff(got_s[r])
        assert (d <= 0).all()
        assert (np.diff(got_i[r])[d == 0] > 0).all()
    return e_top, e_own


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [768, 1024, 1408])
def test_unit_norm_random(cuda, D, dtype):
    q, g, s64 = _unit_ref(D, dtype == torch.bfloat16)
    got_s, got_i = _search(q, g, 10)
    e_top, e_own = _check_against_f64(got_s, got_i, s64, 10)
    print(f"topk D={D} {dtype}: |score - fp64 top-k score| max {e_top:.3e}, |score - fp64 score of its id| max "
          f"{e_own:.3e} (bar {BAR:.0e})")
    assert e_top <= BAR and e_own <= BAR


# ---- 3. position independence ----
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_shards_merge_to_the_bits_of_the_whole(cuda, dtype):
    q, g, _ = _unit_ref(768, dtype == torch.bfloat16)
    N = g.shape[0]
    whole_s, whole_i = _native.op_topk(q, g, 10, id_base=5)
    lists = [_native.op_topk(q, g[a:b], 10, id_base=5 + a) for a, b in ((0, 1000), (1000, 1001), (1001, N))]
    got_s, got_i = _native.op_topk_merge(torch.stack([l[0] for l in lists]), torch.stack([l[1] for l in lists]), 10)
    torch.cuda.synchronize()
    assert torch.equal(got_i, whole_i)
    assert torch.equal(got_s.view(torch.int32), whole_s.view(torch.int32))
    # a shorter merge is the head of the longer one
    s3, i3 = _native.op_topk_merge(torch.stack([l[0] for l in lists]), torch.stack([l[1] for l in lists]), 3)
    assert torch.equal(i3, whole_i[:, :3]) and torch.equal(s3, whole_s[:, :3])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_strided_gallery_and_repeat_are_bitwise(cuda, dtype):
    q, g, _ = _unit_ref(768, dtype == torch.bfloat16)
    N, D = g.shape
    a_s, a_i = _native.op_topk(q, g, 10)
    wide = torch.full((N, D + 64), 3.0, dtype=dtype, device=cuda)
    wide[:, :D] = g
    b_s, b_i = _native.op_topk(q, wide[:, :D], 10)
    c_s, c_i = _native.op_topk(q, g, 10)
    torch.cuda.synchronize()
    for s, i in ((b_s, b_i), (c_s, c_i)):
        assert torch.equal(i, a_i) and torch.equal(s.view(torch.int32), a_s.view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_a_rows_score_does_not_depend_on_its_position(cuda, dtype):
    q, g, _ = _unit_ref(768, dtype == torch.bfloat16)
    N = g.shape[0]
    g = g.clone()
    at = [0, 31, 32, 1000, N - 1]
    g[at] = q[3].to(dtype)  # query 3 itself: its copies score about 1, above every other row
    got_s, got_i = _search(q, g, 10)
    assert got_i[3, :5].tolist() == at
    assert len(set(got_s[3, :5].view(np.int32).tolist())) == 1
    for r in range(q.shape[0]):  # and the same holds wherever the copies rank for the other queries
        sc = {int(got_s[r, j].view(np.int32)) for j in range(10) if got_i[r, j] in at}
        assert len(sc) <= 1


# ---- 4. many partitions ----
def test_many_partitions(cuda):
    N, D, Q, k = 200_003, 768, 5, 128
    gen = torch.Generator(device=cuda).manual_seed(4)
    g = torch.nn.functional.normalize(torch.randn((N, D), device=cuda, generator=gen), dim=1).to(torch.bfloat16)
    q = torch.nn.functional.normalize(torch.randn((Q, D), device=cuda, generator=gen), dim=1)
    s64 = (g.double() @ q.double().T).cpu().numpy()
    got_s, got_i = _search(q, g, k, id_base=1 << 40)
    e_top, e_own = _check_against_f64(got_s, got_i, s64, k, id_base=1 << 40)
    print(f"topk N={N} k={k} bf16: |score - fp64 top-k score| max {e_top:.3e}, own {e_own:.3e} (bar {BAR:.0e})")
    assert e_top <= BAR and e_own <= BAR


# ---- 5. past 4 GiB ----
def test_gallery_past_4_gib(cuda):
    N, D = 1_400_000, 1536
    g = torch.zeros((N, D), dtype=torch.bfloat16, device=cuda)
    assert g.numel() * 2 > 1 << 32
    r_first, r_far, r_last = 7, 1_398_200, N - 1
    assert r_far * D * 2 > 1 << 32
    g[r_first, 0], g[r_far, 0], g[r_last, 0] = 3.0, 1.0, 2.0
    q = torch.zeros((1, D), device=cuda)
    q[0, :4] = 1.0
    got_s, got_i = _search(q, g, 5)
    assert got_i.tolist() == [[r_first, r_last, r_far, 0, 1]]
    assert got_s.tolist() == [[3.0, 2.0, 1.0, 0.0, 0.0]]


# ---- 6. NaN and -inf ----
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_nan_and_neg_inf_rows_are_never_returned(cuda, dtype):
    rng = np.random.default_rng(6)
    N, D, Q = 100, 128, 3
    q = np.abs(rng.integers(-1, 2, size=(Q, D))).astype(np.float32)
    q[:, 0] = 1.0
    g = rng.integers(-1, 2, size=(N, D)).astype(np.float32)
    g[17] = np.nan
    g[60] = 0.0
    g[60, 0] = -np.inf  # scores -inf against every query (their dim 0 is 1, the row's other entries are 0)
    with np.errstate(invalid="ignore"):
        s = g.astype(np.float64) @ q.astype(np.float64).T
    assert np.isnan(s[17]).all() and np.isneginf(s[60]).all()
    want_s, want_i = rr.topk(s, N)
    got_s, got_i = _search(torch.from_numpy(q).to(cuda), torch.from_numpy(g).to(cuda).to(dtype), N)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s.astype(np.float64), want_s)
    assert not np.isin(got_i, [17, 60]).any()
    assert (got_i[:, -2:] == -1).all() and (got_i[:, :-2] >= 0).all()


# ---- 7. EmbeddingIndex ----
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_index_add_in_pieces_equals_the_op(cuda, dtype):
    q, g = _unit(768)
    index = EmbeddingIndex(768, dtype=dtype, device=cuda, capacity=4)
    assert len(index) == 0
    ids = [index.add(g[:3]), index.add(torch.from_numpy(g[3:13]).to(torch.bfloat16)),
           index.add(torch.from_numpy(g[13:70]).to(cuda))]
    assert ids == [range(0, 3), range(3, 13), range(13, 70)]
    assert len(index) == 70 and index.capacity == 128 and index.embeddings.shape == (70, 768)
    stored = torch.cat([torch.from_numpy(g[:3]).to(dtype), torch.from_numpy(g[3:13]).to(torch.bfloat16).to(dtype),
                        torch.from_numpy(g[13:70]).to(dtype)]).to(cuda)
    assert torch.equal(index.embeddings, stored)
    qd = torch.from_numpy(q).to(cuda)
    want_s, want_i = _native.op_topk(qd, stored, 10)
    got_s, got_i = index.search(qd, 10)
    assert isinstance(got_s, torch.Tensor) and torch.equal(got_i, want_i)
    assert torch.equal(got_s.view(torch.int32), want_s.view(torch.int32))
    np_s, np_i = index.search(q, 10, id_base=1000)
    assert isinstance(np_s, np.ndarray) and np_s.dtype == np.float32 and np_i.dtype == np.int64
    assert np.array_equal(np_i, want_i.cpu().numpy() + 1000) and np.array_equal(np_s, want_s.cpu().numpy())


def test_index_search_over_a_one_rank_communicator(cuda):
    """The sharded route (search, gather the lists over RCCL, merge) on the one rank a single device allows: bitwise
    the plain search.  The communicator is bootstrapped as tests/test_gpu_boundary.py does for vp_allgather."""
    import socket
    import torch.distributed as dist
    q, g = _unit(768)
    index = EmbeddingIndex(768, device=cuda)
    index.add(g[:500])
    qd = torch.from_numpy(q).to(cuda)
    want_s, want_i = index.search(qd, 10, id_base=77)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        with distributed.Communicator(0) as comm:
            got_s, got_i = index.search(qd, 10, comm=comm, id_base=77)
            torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert torch.equal(got_i, want_i) and torch.equal(got_s.view(torch.int32), want_s.view(torch.int32))
