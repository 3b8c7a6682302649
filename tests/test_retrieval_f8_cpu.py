"""The fp8 gallery without a device: the storage format's restatement (tests/retrieval_f8_restatement.py) against the
properties the format promises, the five new C-ABI symbols, every argument check of vp_op_quantize_rows_f8 and the
four vp_op_topk*_f8 calls (they run before any device call, so fake device addresses are enough), and the refusals the
existing calls keep."""

import ctypes

import numpy as np
import pytest
import torch

import retrieval_f8_restatement as f8
from videoprism import _native
from videoprism.retrieval import EmbeddingIndex

P = 0x10000  # a 16-byte aligned address no check dereferences
VP_OK, VP_EINVAL, VP_ENOTSUP = _native.VP_OK, _native.VP_EINVAL, _native.VP_ENOTSUP
NEW = ("vp_op_quantize_rows_f8", "vp_op_topk_f8", "vp_op_topk_groups_f8", "vp_op_topk_masked_f8",
       "vp_op_topk_groups_masked_f8")


# ---- the restatement's own properties ----
def _row(v, d=64):
    x = torch.zeros((1, d), dtype=torch.float32)
    x[0, 3] = v
    return x


@pytest.mark.parametrize("amax, e, code", [
    (448.0, 0, 448.0), (449.0, -1, 224.0), (0.875, 9, 448.0), (1.0, 8, 256.0), (1e30, -91, None), (1e-30, 100, None),
    (0.0, 0, 0.0), (-448.0, 0, -448.0),
])
def test_boundary_cases(amax, e, code):
    x = _row(amax)
    assert int(f8.exponents(x)[0]) == e
    codes, scales = f8.quantize(x)
    assert float(scales[0]) == 2.0 ** -e
    if code is not None:
        assert float(codes[0, 3].to(torch.float32)) == code
    assert not torch.isnan(codes.to(torch.float32)).any()


def test_rows_without_a_finite_element_and_non_finite_elements():
    x = torch.full((3, 64), float("nan"))
    x[1] = float("inf")
    x[2] = -float("inf")
    codes, scales = f8.quantize(x)
    assert f8.exponents(x).tolist() == [0, 0, 0] and scales.tolist() == [1.0, 1.0, 1.0]
    assert torch.isnan(codes.to(torch.float32)).all()
    y = f8.unit_rows(4, 64, 0)
    y[0, 5], y[1, 6], y[2, 7] = float("nan"), float("inf"), -float("inf")
    codes, scales = f8.quantize(y)
    clean = y.clone()
    clean[0, 5] = clean[1, 6] = clean[2, 7] = 0.0
    want, wscales = f8.quantize(clean)
    assert torch.equal(scales, wscales)  # amax is over the finite elements
    v = codes.to(torch.float32)
    assert torch.isnan(v[0, 5]) and torch.isnan(v[1, 6]) and torch.isnan(v[2, 7]) and int(torch.isnan(v).sum()) == 3
    ok = ~torch.isnan(v)
    assert torch.equal(v[ok], want.to(torch.float32)[ok])


def _varied_rows():
    g = torch.Generator().manual_seed(11)
    x = torch.randn((200, 192), generator=g)
    x = x * torch.exp2(torch.randint(-60, 60, (200, 1), generator=g).float())
    x[:50] *= torch.exp2(torch.randint(-14, 1, (50, 192), generator=g).float())  # elements down into the subnormals
    return x


def test_amax_lands_in_the_top_binade():
    x = torch.cat([_varied_rows(), f8.unit_rows(50, 192, 1)])
    e = f8.exponents(x).to(torch.float64)
    top = x.abs().max(dim=1).values.to(torch.float64) * torch.exp2(e)
    assert (top > 224).all() and (top <= 448).all()


def test_storage_error_per_element():
    """RNE to three mantissa bits: 2^-4 relative; in the subnormal range (below 2^-6 in code units) 2^-10 * scale."""
    x = _varied_rows()
    codes, scales = f8.quantize(x)
    got = f8.dequantize(codes, scales)
    err = (got - x.to(torch.float64)).abs()
    bound = torch.maximum(x.to(torch.float64).abs() * 2.0 ** -4, scales.to(torch.float64)[:, None] * 2.0 ** -10)
    assert (err <= bound).all()
    assert (x.abs() * torch.exp2(f8.exponents(x).float())[:, None] < 2.0 ** -6).any()  # the subnormal range is there


def test_stored_values_are_exactly_bf16():
    x = torch.cat([_varied_rows(), _row(1e30, 192), _row(1e-30, 192), _row(3e-39, 192)])
    codes, scales = f8.quantize(x)
    v = f8.dequantize(codes, scales)
    assert torch.equal(v.to(torch.bfloat16).to(torch.float64), v)
    m, p = torch.frexp(scales)
    assert (m == 0.5).all() and (p >= -99).all() and (p <= 101).all()  # powers of two within 2^+-100


@pytest.mark.parametrize("d", [64, 768, 1408])
def test_unit_rows_have_no_nan_and_use_the_top_binade(d):
    x = f8.unit_rows(300, d, d)
    codes, _ = f8.quantize(x)
    v = codes.to(torch.float32)
    assert not torch.isnan(v).any()
    top = v.abs().max(dim=1).values
    assert (top >= 224).all() and (top <= 448).all()


def test_decode_table_is_torchs():
    t = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    assert np.array_equal(np.isnan(t), np.isnan(f8.decode_table()))
    assert np.array_equal(np.nan_to_num(t), np.nan_to_num(f8.decode_table()))
    assert np.isnan(f8.decode_table()[[0x7f, 0xff]]).all() and np.isnan(f8.decode_table()).sum() == 2


def test_bf16_input_is_widened():
    x = f8.unit_rows(20, 64, 3).to(torch.bfloat16)
    a, sa = f8.quantize(x)
    b, sb = f8.quantize(x.to(torch.float32))
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and torch.equal(sa, sb)


# ---- the C-ABI ----
def test_symbols_exported_and_bound_and_the_abi_version_stays():
    lib = _native.load()
    for name in NEW:
        assert name in _native.exported_symbols()
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
    assert lib.vp_abi_version() == 8
    for name in ("op_quantize_rows_f8", "op_topk_f8", "op_topk_groups_f8", "op_topk_masked_f8",
                 "op_topk_groups_masked_f8"):
        assert callable(getattr(_native, name))


def _err():
    return _native.load().vp_last_error().decode()


def _quant(**kw):
    a = dict(x=P, dtype=_native.VP_F32, N=100, ldx=768, D=768, codes=P, ldc=768, scales=P, stream=None)
    a.update(kw)
    rc = _native.load().vp_op_quantize_rows_f8(a["x"], a["dtype"], a["N"], a["ldx"], a["D"], a["codes"], a["ldc"],
                                               a["scales"], a["stream"])
    return rc, _err()


def _base(grouped, masked):
    a = dict(queries=P, Q=4, codes=P, scales=P, N=100, ld=768, D=768, k=10, id_base=0, scores=P, ids=P, ws=P, stream=None)
    a["ws_bytes"] = (_native.op_topk_groups_workspace_bytes if grouped else _native.op_topk_workspace_bytes)(4, 10)
    if grouped:
        a.update(labels=P, groups=P)
    if masked:
        a.update(mask=P, stride=0)
    return a


def _search(grouped, masked, **kw):
    a = _base(grouped, masked)
    a.update(kw)
    lib = _native.load()
    head = [a["queries"], a["Q"], a["codes"], a["scales"], a["N"], a["ld"], a["D"]]
    mask = [a["mask"], a["stride"]] if masked else []
    tail = [a["ws"], a["ws_bytes"], a["stream"]]
    if grouped:
        fn = lib.vp_op_topk_groups_masked_f8 if masked else lib.vp_op_topk_groups_f8
        rc = fn(*head, a["labels"], a["k"], a["id_base"], *mask, a["scores"], a["groups"], a["ids"], *tail)
    else:
        fn = lib.vp_op_topk_masked_f8 if masked else lib.vp_op_topk_f8
        rc = fn(*head, a["k"], a["id_base"], *mask, a["scores"], a["ids"], *tail)
    return rc, _err()


NAMES = {(False, False): "topk_f8", (True, False): "topk_groups_f8", (False, True): "topk_masked_f8",
         (True, True): "topk_groups_masked_f8"}

COMMON = [
    (dict(queries=None), VP_EINVAL, "queries"),
    (dict(codes=None), VP_EINVAL, "null codes"),
    (dict(scales=None), VP_EINVAL, "null scales"),
    (dict(scores=None), VP_EINVAL, "scores"),
    (dict(ids=None), VP_EINVAL, "ids"),
    (dict(ws=None), VP_EINVAL, "ws"),
    (dict(N=-1), VP_EINVAL, "N"),
    (dict(Q=-1), VP_EINVAL, "Q"),
    (dict(k=0), VP_EINVAL, "k"),
    (dict(k=129, ws_bytes=1 << 40), VP_ENOTSUP, "k"),
    (dict(D=0), VP_ENOTSUP, "D"),
    (dict(D=96, ld=96), VP_ENOTSUP, "D"),
    (dict(D=800, ld=800), VP_ENOTSUP, "D"),
    (dict(D=1600, ld=1600), VP_ENOTSUP, "D"),
    (dict(ld=752), VP_EINVAL, "ld must be >= D"),
    (dict(ld=776), VP_EINVAL, "ld must be a multiple of 16"),
    (dict(queries=P + 4), VP_EINVAL, "queries"),
    (dict(codes=P + 8), VP_EINVAL, "codes must be 16-byte aligned"),
    (dict(scales=P + 2), VP_EINVAL, "scales must be 4-byte aligned"),
    (dict(ws_bytes=1024), VP_EINVAL, "ws_bytes"),
]
GROUPS = [(dict(labels=None), VP_EINVAL, "labels"), (dict(labels=P + 4), VP_EINVAL, "labels"),
          (dict(groups=None), VP_EINVAL, "groups")]
MASKED = [(dict(mask=None), VP_EINVAL, "null mask"), (dict(mask=P + 2), VP_EINVAL, "mask must be 4-byte aligned"),
          (dict(stride=-1), VP_EINVAL, "mask_query_stride_words"), (dict(stride=3), VP_EINVAL, "mask_query_stride_words")]


@pytest.mark.parametrize("grouped, masked", list(NAMES))
def test_search_argument_checks(grouped, masked):
    for kw, code, word in COMMON + (GROUPS if grouped else []) + (MASKED if masked else []):
        rc, msg = _search(grouped, masked, **kw)
        assert rc == code, (kw, rc, msg)
        assert msg.startswith(NAMES[grouped, masked] + ": ") and word in msg, (kw, msg)


@pytest.mark.parametrize("grouped, masked", list(NAMES))
def test_search_calls_that_launch_nothing_need_no_device(grouped, masked):
    assert _search(grouped, masked, Q=0)[0] == VP_OK
    assert _search(grouped, masked, Q=0, ld=784)[0] == VP_OK  # a wider buffer, a multiple of 16 bytes
    nulls = dict(codes=None, scales=None)
    if grouped:
        nulls["labels"] = None
    if masked:
        nulls["mask"] = None
    assert _search(grouped, masked, Q=0, N=0, **nulls)[0] == VP_OK  # N == 0: the gallery's pointers may be null


@pytest.mark.parametrize("grouped, masked", list(NAMES))
def test_the_workspace_is_the_existing_calls(grouped, masked):
    for Q, k in ((1, 1), (4, 10), (33, 128)):
        need = (_native.op_topk_groups_workspace_bytes if grouped else _native.op_topk_workspace_bytes)(Q, k)
        rc, msg = _search(grouped, masked, Q=Q, k=k, ws_bytes=need - 1)
        assert rc == VP_EINVAL and "too small" in msg and f"need {need}" in msg, msg
        assert _search(grouped, masked, Q=Q, k=k, ws_bytes=need, queries=None)[1].endswith("null queries")


@pytest.mark.parametrize("kw, code, word", [
    (dict(x=None), VP_EINVAL, "null x"),
    (dict(codes=None), VP_EINVAL, "null codes"),
    (dict(scales=None), VP_EINVAL, "null scales"),
    (dict(N=-1), VP_EINVAL, "N"),
    (dict(dtype=_native.VP_U8), VP_ENOTSUP, "x_dtype"),
    (dict(dtype=7), VP_ENOTSUP, "x_dtype"),
    (dict(D=0), VP_ENOTSUP, "D"),
    (dict(D=800, ldx=800, ldc=800), VP_ENOTSUP, "D"),
    (dict(D=1600, ldx=1600, ldc=1600), VP_ENOTSUP, "D"),
    (dict(ldx=764), VP_EINVAL, "ldx must be >= D"),
    (dict(ldx=770), VP_EINVAL, "ldx must be a multiple of 16 bytes"),
    (dict(ldx=772, dtype=_native.VP_BF16), VP_EINVAL, "ldx must be a multiple of 16 bytes"),
    (dict(ldc=752), VP_EINVAL, "ldc must be >= D"),
    (dict(ldc=776), VP_EINVAL, "ldc must be a multiple of 16"),
    (dict(x=P + 4), VP_EINVAL, "x must be 16-byte aligned"),
    (dict(codes=P + 8), VP_EINVAL, "codes must be 16-byte aligned"),
    (dict(scales=P + 2), VP_EINVAL, "scales must be 4-byte aligned"),
])
def test_quantize_argument_checks(kw, code, word):
    rc, msg = _quant(**kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("quantize_rows_f8: ") and word in msg, msg


def test_quantize_of_no_rows_needs_no_device():
    assert _quant(N=0)[0] == VP_OK
    assert _quant(N=0, x=None, codes=None, scales=None)[0] == VP_OK
    assert _quant(N=0, ldx=772, ldc=784)[0] == VP_OK  # fp32 rows of 16-byte multiples, a wider code buffer


# ---- what stays as it was ----
@pytest.mark.parametrize("dtype", [2, 3, 7])
def test_the_existing_calls_keep_refusing_other_dtypes(dtype):
    lib = _native.load()
    ws = 1 << 30
    calls = {
        "topk": lambda: lib.vp_op_topk(P, 4, P, dtype, 100, 768, 768, 10, 0, P, P, P, ws, None),
        "topk_groups": lambda: lib.vp_op_topk_groups(P, 4, P, dtype, 100, 768, 768, P, 10, 0, P, P, P, P, ws, None),
        "topk_masked": lambda: lib.vp_op_topk_masked(P, 4, P, dtype, 100, 768, 768, 10, 0, P, 0, P, P, P, ws, None),
        "topk_groups_masked": lambda: lib.vp_op_topk_groups_masked(P, 4, P, dtype, 100, 768, 768, P, 10, 0, P, 0, P, P,
                                                                   P, P, ws, None),
    }
    for name, fn in calls.items():
        assert fn() == VP_ENOTSUP, name
        assert _err() == name + ": gallery_dtype must be VP_F32 or VP_BF16"


# ---- Python ----
def test_index_dtypes():
    index = EmbeddingIndex(64, dtype=torch.float8_e4m3fn, device="cpu", capacity=8)
    assert index.dtype == torch.float8_e4m3fn and len(index) == 0 and index.capacity == 8
    assert index.codes.dtype == torch.float8_e4m3fn and tuple(index.codes.shape) == (0, 64)
    assert index.scales.dtype == torch.float32 and tuple(index.scales.shape) == (0,)
    assert index.embeddings.dtype == torch.bfloat16 and tuple(index.embeddings.shape) == (0, 64)
    for dtype in (torch.float16, torch.float8_e5m2, torch.uint8, torch.float64):
        with pytest.raises(TypeError, match="dtype"):
            EmbeddingIndex(64, dtype=dtype, device="cpu")
    plain = EmbeddingIndex(64, device="cpu")
    with pytest.raises(AttributeError):
        plain.codes
    with pytest.raises(AttributeError):
        plain.scales


def test_native_f8_argument_checks():
    q = torch.zeros((3, 64))
    codes, scales = torch.zeros((40, 64), dtype=torch.uint8), torch.ones(40)
    with pytest.raises(TypeError, match="codes"):
        _native.op_topk_f8(q, torch.zeros((40, 64)), scales, 2)
    with pytest.raises(ValueError, match="codes"):
        _native.op_topk_f8(q, torch.zeros((40, 128), dtype=torch.uint8), scales, 2)
    with pytest.raises(ValueError, match="scales"):
        _native.op_topk_f8(q, codes, torch.ones(39), 2)
    with pytest.raises(ValueError, match="scales"):
        _native.op_topk_groups_f8(q, codes, torch.ones(40, dtype=torch.float64), torch.zeros(40, dtype=torch.int64), 2)
    with pytest.raises(ValueError, match="labels"):
        _native.op_topk_groups_f8(q, codes, scales, torch.zeros(39, dtype=torch.int64), 2)
    with pytest.raises(TypeError, match="mask"):
        _native.op_topk_masked_f8(q, codes, scales, 2, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(TypeError, match="x must be"):
        _native.op_quantize_rows_f8(torch.zeros((4, 64), dtype=torch.float64))
