"""The fp8 gallery on the GPU (vp_op_quantize_rows_f8, vp_op_topk*_f8, EmbeddingIndex(dtype=torch.float8_e4m3fn))
against the torch restatement of the storage format (tests/retrieval_f8_restatement.py), the NumPy statements of the
order rules (tests/retrieval_restatement.py and its grouped and masked kin) and fp64 scores of the stored gallery.

The bar of the unit-row cases is tests/test_gpu_retrieval.py's 2e-5: a stored row is exactly bf16 and the arithmetic is
the bf16 gallery's, so the error against fp64 scores of the stored values is that path's (measured there 2.4e-7 -
3.1e-7).  Everything else here is equality, of codes by value, of scale bits, of ids and of score bits."""

import functools
import os

import numpy as np
import pytest
import torch

import grouped_retrieval_restatement as gr
import masked_retrieval_cases as mc
import retrieval_f8_restatement as f8
import retrieval_restatement as rr
from videoprism import _native, distributed
from videoprism.retrieval import EmbeddingIndex

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
BAR = 2e-5
NAN_CODE = 0x7F


def _np(*ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    """Two (scores, ids[, ...]) results on the device: the same bits."""
    return all(torch.equal(x if x.dtype != torch.float32 else _bits(x), y if y.dtype != torch.float32 else _bits(y))
               for x, y in zip(a, b)) and len(a) == len(b)


# ---- 1. quantiser parity ----
def _tie_values():
    """Every midpoint of two neighbouring non-negative e4m3 values (the RNE ties, the subnormal ones and the tie with
    zero among them) and a few values close to them, in code units (amax 448 keeps e = 0)."""
    t = np.sort(f8.decode_table()[:0x7F])
    mids = (t[:-1] + t[1:]) / 2
    near = np.concatenate([np.nextafter(mids.astype(np.float32), np.float32(0)),
                           np.nextafter(mids.astype(np.float32), np.float32(1e9))]).astype(np.float64)
    small = np.array([2.0 ** -9, 2.0 ** -10, 2.0 ** -11, 1.5 * 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -20, 0.0])
    return np.concatenate([mids, near, small]).astype(np.float32)


def _quantiser_rows(D):
    rng = np.random.default_rng(D)
    rows = [f8.unit_rows(40, D, D).numpy()]
    unit = rows[0]
    # amax exactly on 448 * 2^j and one ulp either side, the other elements well below
    for j in (-30, -8, -1, 0, 3, 40):
        top = np.float32(448.0 * 2.0 ** j)
        for a in (np.nextafter(top, np.float32(0)), top, np.nextafter(top, np.float32(np.inf))):
            r = unit[len(rows) % 40] * np.float32(0.7) * a
            r[rng.integers(0, D)] = a * np.float32(rng.choice([-1.0, 1.0]))
            rows.append(r[None])
    # ties, in rows whose amax is 448 (e = 0) and, scaled by a power of two, in rows with another e
    ties = _tie_values()
    per = D - 1
    for a in range(0, len(ties), per):
        chunk = np.resize(ties[a:a + per], per) * rng.choice([-1.0, 1.0], per).astype(np.float32)
        for j in (0, -17, 9):
            rows.append((np.concatenate([[448.0], chunk]).astype(np.float32) * np.float32(2.0 ** j))[None])
    special = np.tile(unit[:8], (1, 1)).copy()
    special[0] = 0.0
    special[1, 5] = np.nan
    special[2, 0], special[2, D - 1] = np.inf, -np.inf
    special[3] = np.nan
    special[4] = -np.inf
    special[5, ::2] = -0.0
    special[6] = 0.0
    special[6, 7] = -0.0
    special[7, 1] = np.float32(1e-42)  # a denormal fp32 element in an ordinary row
    rows.append(special)
    rows += [unit[:4] * np.float32(1e30), unit[:4] * np.float32(1e-30), unit[:4] * np.float32(1e-39),
             unit[:2] * np.float32(3e38)]
    return torch.from_numpy(np.concatenate(rows).astype(np.float32))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [64, 192, 768, 1408])
def test_quantiser_parity(cuda, D, bf16):
    x = _quantiser_rows(D)
    if bf16:
        x = x.to(torch.bfloat16)
    want_c, want_s = f8.quantize(x)
    N = x.shape[0]
    got_c, got_s = _native.op_quantize_rows_f8(x.to(cuda))
    torch.cuda.synchronize()
    assert got_c.dtype == F8 and got_s.dtype == torch.float32
    assert torch.equal(_bits(got_s).cpu(), _bits(want_s)), "scales"
    assert f8.same_codes(got_c, want_c), "codes"
    # a strided input, and a code buffer wider and longer than [N, D]: the padding keeps what it held
    wide_x = torch.full((N, D + 64), float("nan"), dtype=x.dtype, device=cuda)
    wide_x[:, :D] = x.to(cuda)
    buf = torch.full((N + 3, D + 48), 0xA5, dtype=torch.uint8, device=cuda)
    sc = torch.full((N + 3,), -7.0, device=cuda)
    _native.op_quantize_rows_f8(wide_x[:, :D], codes=buf[:N, :D], scales=sc[:N])
    torch.cuda.synchronize()
    assert torch.equal(buf[:N, :D], got_c.view(torch.uint8)) and torch.equal(_bits(sc[:N]), _bits(got_s))
    assert bool((buf[:, D:] == 0xA5).all()) and bool((buf[N:] == 0xA5).all()) and bool((sc[N:] == -7.0).all())


# ---- 2. the decode table ----
def test_every_code_decodes_to_its_value(cuda):
    codes = torch.zeros((256, 64), dtype=torch.uint8)
    codes[:, 0] = torch.arange(256, dtype=torch.uint8)
    q = torch.zeros((2, 64))
    q[0, 0], q[1, 0] = 1.0, -1.0
    table = f8.decode_table()
    with np.errstate(invalid="ignore"):
        s64 = np.stack([table, -table], axis=1) + 0.0  # [256, 2]; -0 + 0 = +0, as the accumulators make it
    want_s, want_i = rr.topk(s64, 128)
    got_s, got_i = _np(*_native.op_topk_f8(q.to(cuda), codes.to(cuda), torch.ones(256, device=cuda), 128))
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s.astype(np.float64), want_s)
    assert not np.isin(got_i, [0x7F, 0xFF]).any()
    # the 126 positive values in descending order, then the two zeros; the same of the negative codes for -e0
    assert got_i[0, :126].tolist() == list(range(0x7E, 0, -1)) and got_i[0, 126:].tolist() == [0x00, 0x80]
    assert got_i[1, :126].tolist() == list(range(0xFE, 0x80, -1)) and got_i[1, 126:].tolist() == [0x00, 0x80]
    assert np.array_equal(got_s[0, :126].astype(np.float64), table[0x7E:0:-1]) and got_s[0, 125] == 2.0 ** -9


# ---- 3. exact arithmetic ----
@functools.lru_cache(maxsize=None)
def _ternary():
    rng = np.random.default_rng(1)  # tests/test_gpu_retrieval.py's case
    q = rng.integers(-1, 2, size=(33, 128)).astype(np.float32)
    g = rng.integers(-1, 2, size=(517, 128)).astype(np.float32)
    return q, g, g.astype(np.float64) @ q.astype(np.float64).T


def _index(g, D, cuda, **kw):
    index = EmbeddingIndex(D, dtype=F8, device=cuda)
    if g is not None:
        index.add(g, **kw)
    return index


@pytest.mark.parametrize("k", [1, 20, 128])
def test_exact_arithmetic_ternary(cuda, k):
    q, g, s = _ternary()
    top = np.sort(s, axis=0)[::-1]
    assert sum(top[19, c] == top[20, c] for c in range(33)) == 29  # ties across the k-th place, and inside it
    want_s, want_i = rr.topk(s, k)
    got_s, got_i = _index(g, 128, cuda).search(q, k)
    assert got_i.dtype == np.int64 and got_s.dtype == np.float32
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s.astype(np.float64), want_s)


def test_fewer_rows_than_k_and_an_empty_gallery_pad_the_tail(cuda):
    q, g, s = _ternary()
    want_s, want_i = rr.topk(s[:5], 8, id_base=40)
    got_s, got_i = _index(g[:5], 128, cuda).search(q, 8, id_base=40)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s.astype(np.float64), want_s)
    assert (got_i[:, 5:] == -1).all() and np.isneginf(got_s[:, 5:]).all()
    got_s, got_i = _index(None, 128, cuda).search(q, 3)
    assert (got_i == -1).all() and np.isneginf(got_s).all()
    got_s, got_i = _np(*_native.op_topk_f8(torch.from_numpy(q).to(cuda), torch.empty((0, 128), dtype=F8, device=cuda),
                                           torch.empty((0,), device=cuda), 3))
    assert (got_i == -1).all() and np.isneginf(got_s).all()


@functools.lru_cache(maxsize=None)
def _integers(N=517, Q=33, D=128):
    """Gallery entries n * 2^j, n an integer in [-15, 15] (exact in e4m3 whatever the row's scale) and j per row in
    [-20, 20]; queries integers in [-7, 7] (exact in one bf16 term): every product and partial sum is exact in fp32."""
    rng = np.random.default_rng(8)
    j = rng.integers(-20, 21, size=(N, 1))
    cap = rng.integers(1, 16, size=(N, 1))  # the row's largest magnitude, so that rows differ in their codes' exponents
    g = (np.clip(rng.integers(-15, 16, size=(N, D)), -cap, cap) * 2.0 ** j).astype(np.float32)
    q = rng.integers(-7, 8, size=(Q, D)).astype(np.float32)
    return q, g, g.astype(np.float64) @ q.astype(np.float64).T


def test_exact_arithmetic_over_many_codes_and_scales(cuda):
    q, g, s = _integers()
    index = _index(g, 128, cuda)
    assert np.array_equal(index.embeddings.double().cpu().numpy(), g.astype(np.float64))  # stored exactly
    assert len(set(index.scales.tolist())) > 20 and len(set(index.codes.view(torch.uint8).flatten().tolist())) >= 31
    for k in (1, 20, 128):
        want_s, want_i = rr.topk(s, k)
        got_s, got_i = index.search(q, k)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s.astype(np.float64), want_s)


# ---- 4. unit rows against fp64 scores of the stored gallery ----
@functools.lru_cache(maxsize=None)
def _unit(D, N=3001, Q=37):
    rng = np.random.default_rng(2 + D)
    q = rng.standard_normal((Q, D))
    g = rng.standard_normal((N, D))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return q.astype(np.float32), g.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _unit_dev(D):
    """(queries, codes, scales) on the device, made once and left unchanged."""
    q, g = _unit(D)
    codes, scales = _native.op_quantize_rows_f8(torch.from_numpy(g).cuda())
    return torch.from_numpy(q).cuda(), codes, scales


def _check_against_f64(got_s, got_i, s64, k, id_base=0):
    """tests/test_gpu_retrieval.py's checks; returns the two measured maxima."""
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


@pytest.mark.parametrize("D", [64, 192, 768, 1408, 1536])
def test_unit_norm_random(cuda, D):
    q, g = _unit(D)
    index = _index(g, D, cuda)
    stored = index.embeddings
    assert stored.dtype == torch.bfloat16 and tuple(stored.shape) == (3001, D)
    want_c, want_sc = f8.quantize(torch.from_numpy(g))
    assert torch.equal(stored.double().cpu(), f8.dequantize(want_c, want_sc))  # the copy is the stored values, exactly
    s64 = stored.double().cpu().numpy() @ q.astype(np.float64).T
    got_s, got_i = index.search(q, 10)
    e_top, e_own = _check_against_f64(got_s, got_i, s64, 10)
    exact = g.astype(np.float64) @ q.astype(np.float64).T
    print(f"topk_f8 D={D}: |score - fp64 top-k score of the stored gallery| max {e_top:.3e}, |score - fp64 score of "
          f"its id| max {e_own:.3e} (bar {BAR:.0e}); storage error of the scores max {np.abs(s64 - exact).max():.2e} "
          f"rms {np.sqrt(np.mean((s64 - exact) ** 2)):.2e}")
    assert e_top <= BAR and e_own <= BAR


# ---- 5. a score depends on the two vectors alone ----
def _all_scores(q, codes, scales):
    """fp32 [N, Q]: every row's score as the search returns it, from searches of 128 rows with k = 128 (NaN where a
    row is never returned)."""
    N, Q = codes.shape[0], q.shape[0]
    out = np.full((N, Q), np.nan, dtype=np.float32)
    for a in range(0, N, 128):
        b = min(a + 128, N)
        s, i = _np(*_native.op_topk_f8(q, codes[a:b], scales[a:b], b - a, id_base=a))
        for c in range(Q):
            ok = i[c] >= 0
            out[i[c][ok], c] = s[c][ok]
    return out


@functools.lru_cache(maxsize=None)
def _unit_scores(D):
    return _all_scores(*_unit_dev(D))


def test_shards_merge_to_the_bits_of_the_whole(cuda):
    q, codes, scales = _unit_dev(768)
    N = codes.shape[0]
    whole = _native.op_topk_f8(q, codes, scales, 10, id_base=5)
    lists = [_native.op_topk_f8(q, codes[a:b], scales[a:b], 10, id_base=5 + a)
             for a, b in ((0, 1000), (1000, 1001), (1001, N))]
    got = _native.op_topk_merge(torch.stack([l[0] for l in lists]), torch.stack([l[1] for l in lists]), 10)
    torch.cuda.synchronize()
    assert _same(got, whole)
    s, i = _np(*whole)
    want_s, want_i = rr.topk(_unit_scores(768).astype(np.float64), 10, id_base=5)
    assert np.array_equal(i, want_i) and np.array_equal(s.astype(np.float64), want_s)  # and of 128-row pieces


def test_strided_codes_and_repeat_are_bitwise(cuda):
    q, codes, scales = _unit_dev(768)
    N, D = codes.shape
    a = _native.op_topk_f8(q, codes, scales, 10)
    wide = torch.full((N, D + 64), 0x38, dtype=torch.uint8, device=cuda)  # 1.0 in the padding
    wide[:, :D] = codes.view(torch.uint8)
    b = _native.op_topk_f8(q, wide[:, :D], scales, 10)
    c = _native.op_topk_f8(q, codes, scales, 10)
    torch.cuda.synchronize()
    assert _same(b, a) and _same(c, a)


def test_a_rows_score_does_not_depend_on_its_position(cuda):
    q, g = _unit(768)
    g = g.copy()
    at = [0, 31, 32, 1000, g.shape[0] - 1]
    g[at] = q[3]  # query 3 itself: its copies score about 1, above every other row
    got_s, got_i = _index(g, 768, cuda).search(q, 10)
    assert got_i[3, :5].tolist() == at
    assert len(set(got_s[3, :5].view(np.int32).tolist())) == 1
    for r in range(q.shape[0]):
        sc = {int(got_s[r, j].view(np.int32)) for j in range(10) if got_i[r, j] in at}
        assert len(sc) <= 1


@pytest.mark.parametrize("Q", [1, 31, 32, 33])
def test_a_querys_result_does_not_depend_on_the_other_queries(cuda, Q):
    q, codes, scales = _unit_dev(192)
    whole = _native.op_topk_f8(q, codes, scales, 10)
    part = _native.op_topk_f8(q[:Q].contiguous(), codes, scales, 10)
    torch.cuda.synchronize()
    assert _same(part, tuple(t[:Q] for t in whole))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 511, 512, 513, 3 * 512 + 17])
def test_gallery_sizes_around_the_tiles(cuda, N):
    q, codes, scales = _unit_dev(192)
    want_s, want_i = rr.topk(_unit_scores(192)[:N].astype(np.float64), 10)
    got_s, got_i = _np(*_native.op_topk_f8(q, codes[:N], scales[:N], 10))
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s.astype(np.float64), want_s)


def test_many_row_ranges(cuda):
    N, D, Q, k = 140_003, 128, 5, 128
    gen = torch.Generator(device=cuda).manual_seed(4)
    g = torch.nn.functional.normalize(torch.randn((N, D), device=cuda, generator=gen), dim=1)
    q = torch.nn.functional.normalize(torch.randn((Q, D), device=cuda, generator=gen), dim=1)
    index = _index(g, D, cuda)
    s64 = (index.embeddings.double() @ q.double().T).cpu().numpy()
    got_s, got_i = _np(*index.search(q, k, id_base=1 << 40))
    e_top, e_own = _check_against_f64(got_s, got_i, s64, k, id_base=1 << 40)
    print(f"topk_f8 N={N} k={k}: |score - fp64 top-k score| max {e_top:.3e}, own {e_own:.3e} (bar {BAR:.0e})")
    assert e_top <= BAR and e_own <= BAR


# ---- 6. the scale is applied exactly ----
def test_scales_are_exact(cuda):
    q, codes, _ = _unit_dev(768)
    N = codes.shape[0]
    one = _native.op_topk_f8(q, codes, torch.ones(N, device=cuda), 10)
    small = _native.op_topk_f8(q, codes, torch.full((N,), 2.0 ** -11, device=cuda), 10)
    torch.cuda.synchronize()
    assert torch.equal(small[1], one[1])
    assert torch.equal(_bits(small[0]), _bits(one[0] * 2.0 ** -11)) and bool((one[0].abs() > 1.0).all())


# ---- 7. nothing outside the rows is read ----
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "groups"])
def test_padding_columns_and_rows_past_n_are_not_read(cuda, grouped):
    q, codes, scales = _unit_dev(768)
    N, D = codes.shape
    wide = torch.full((N + 600, D + 64), NAN_CODE, dtype=torch.uint8, device=cuda)
    wide[:N, :D] = codes.view(torch.uint8)
    sc = torch.full((N + 600,), float("nan"), device=cuda)
    sc[:N] = scales
    if grouped:
        labels = torch.arange(N + 600, device=cuda) // 3
        want = _native.op_topk_groups_f8(q, codes, scales, labels[:N], 10)
        got = _native.op_topk_groups_f8(q, wide[:N, :D], sc[:N], labels[:N], 10)
    else:
        want = _native.op_topk_f8(q, codes, scales, 10)
        got = _native.op_topk_f8(q, wide[:N, :D], sc[:N], 10)
    torch.cuda.synchronize()
    assert _same(got, want) and bool(torch.isfinite(want[0]).all())


def test_rows_with_non_finite_elements_are_never_returned(cuda):
    q, g = _unit(192)
    g = g[:100].copy()
    g[17, 3], g[60, 0], g[61, 5] = np.nan, np.inf, -np.inf
    index = _index(g, 192, cuda)
    got_s, got_i = index.search(np.abs(q), 100)
    assert not np.isin(got_i, [17, 60, 61]).any()
    assert (got_i[:, -3:] == -1).all() and (got_i[:, :-3] >= 0).all() and np.isfinite(got_s[:, :-3]).all()


# ---- 8. composition on an fp8 EmbeddingIndex ----
def test_search_groups_is_the_grouped_restatement(cuda):
    q, g, s = _integers()
    N = g.shape[0]
    labels = np.arange(N, dtype=np.int64) // 3 * 7
    labels[5::41] = -1
    index = _index(g, 128, cuda, group=labels)
    for k in (1, 20, 128):
        want = gr.group_topk(s, labels, k, id_base=9)
        got = index.search_groups(q, k, id_base=9)
        assert np.array_equal(got[0].astype(np.float64), want[0])
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_allow_and_remove_search_the_allowed_rows_alone(cuda):
    q, g = _unit(192)
    N, Q = g.shape[0], q.shape[0]
    s = _unit_scores(192).astype(np.float64)  # the unmasked search's score bits
    labels = mc.masked_labels(N)
    index = _index(g, 192, cuda, group=labels)
    rng = np.random.default_rng(3)
    shared, per_query = rng.random(N) < 0.5, rng.random((Q, N)) < 0.3
    for allow in (shared, per_query):
        want_s, want_i = mc.masked_topk(s, allow, 10, id_base=3)
        got_s, got_i = index.search(q, 10, id_base=3, allow=allow)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s.astype(np.float64), want_s)
        want = mc.masked_group_topk(s, labels, allow, 10)
        got = index.search_groups(q, 10, allow=allow)
        assert all(np.array_equal(a.astype(w.dtype), w) for a, w in zip(got, want))
    gone = np.nonzero(rng.random(N) < 0.4)[0]
    index.remove(gone)
    alive = np.ones(N, dtype=bool)
    alive[gone] = False
    for allow, eff in ((None, alive), (shared, alive & shared), (per_query, alive[None] & per_query)):
        want_s, want_i = mc.masked_topk(s, eff, 10)
        got_s, got_i = index.search(q, 10, allow=allow)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s.astype(np.float64), want_s)
        want = mc.masked_group_topk(s, labels, eff, 10)  # a removed row never stands for its group
        got = index.search_groups(q, 10, allow=allow)
        assert all(np.array_equal(a.astype(w.dtype), w) for a, w in zip(got, want))
    # compact keeps codes and scales together: the index is then a fresh index of the survivors, bit for bit
    old = index.compact().cpu().numpy()
    assert np.array_equal(old, np.nonzero(alive)[0]) and len(index) == int(alive.sum())
    fresh = _index(g[alive], 192, cuda, group=labels[alive])
    assert torch.equal(index.codes.view(torch.uint8), fresh.codes.view(torch.uint8))
    assert torch.equal(_bits(index.scales), _bits(fresh.scales))
    qd = torch.from_numpy(q).to(cuda)
    assert _same(index.search(qd, 10), fresh.search(qd, 10))
    assert _same(index.search_groups(qd, 10), fresh.search_groups(qd, 10))
    want_s, want_i = rr.topk(s[alive], 10)
    got_s, got_i = index.search(q, 10)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s.astype(np.float64), want_s)


def test_growth_keeps_earlier_rows(cuda):
    q, g = _unit(768)
    index = EmbeddingIndex(768, dtype=F8, device=cuda, capacity=4)
    ids = [index.add(g[:3]), index.add(torch.from_numpy(g[3:13]).to(cuda))]
    before_c, before_s = index.codes.view(torch.uint8).clone(), index.scales.clone()
    ids.append(index.add(torch.from_numpy(g[13:70]).to(cuda)))  # 13 -> 70 rows: past the capacity of 16
    wide = torch.zeros((30, 800), device=cuda)
    wide[:, :768] = torch.from_numpy(g[70:100]).to(cuda)
    ids.append(index.add(wide[:, :768]))  # rows of a wider tensor
    assert ids == [range(0, 3), range(3, 13), range(13, 70), range(70, 100)]
    assert len(index) == 100 and index.capacity == 128
    assert tuple(index.codes.shape) == (100, 768) and tuple(index.scales.shape) == (100,)
    assert torch.equal(index.codes.view(torch.uint8)[:13], before_c) and torch.equal(_bits(index.scales[:13]), _bits(before_s))
    want_c, want_s = _native.op_quantize_rows_f8(torch.from_numpy(g[:100]).to(cuda))
    assert torch.equal(index.codes.view(torch.uint8), want_c.view(torch.uint8))
    assert torch.equal(_bits(index.scales), _bits(want_s))
    qd = torch.from_numpy(q).to(cuda)
    assert _same(index.search(qd, 10), _native.op_topk_f8(qd, want_c, want_s, 10))
    mixed = EmbeddingIndex(768, dtype=F8, device=cuda)
    mixed.add(torch.from_numpy(g[:100]).to(torch.bfloat16))  # bf16 in: widened, then quantised
    want_c, want_s = f8.quantize(torch.from_numpy(g[:100]).to(torch.bfloat16))
    assert f8.same_codes(mixed.codes, want_c) and torch.equal(_bits(mixed.scales).cpu(), _bits(want_s))


def test_index_search_over_a_one_rank_communicator(cuda):
    """As tests/test_gpu_retrieval.py: search, gather the lists over RCCL, merge, on the one rank a device allows."""
    import socket
    import torch.distributed as dist
    q, g = _unit(768)
    labels = np.arange(500, dtype=np.int64) // 4
    index = _index(g[:500], 768, cuda, group=labels)
    qd = torch.from_numpy(q).to(cuda)
    want = index.search(qd, 10, id_base=77)
    want_g = index.search_groups(qd, 10, id_base=77)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        with distributed.Communicator(0) as comm:
            got = index.search(qd, 10, comm=comm, id_base=77)
            got_g = index.search_groups(qd, 10, comm=comm, id_base=77)
            torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert _same(got, want) and _same(got_g, want_g)
