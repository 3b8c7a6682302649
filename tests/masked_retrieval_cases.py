"""The cases of the masked gallery search (vp_op_topk_masked, vp_op_topk_groups_masked, vp_op_rowmask_pack), shared
by tests/test_retrieval_masked_cpu.py and tests/test_gpu_retrieval_masked.py, and its rule restated in NumPy.

The rule: a masked search is the unmasked search of the gallery that holds the allowed rows alone, ids mapped back.
`masked_topk` / `masked_group_topk` say that with tests/retrieval_restatement.topk and
tests/grouped_retrieval_restatement.group_topk on the fp64 scores of the allowed rows, per query.

The shapes sit on the scan's own boundaries: a mask word is 32 rows, a wave takes 64, a workgroup's tile is 512 and a
row range ("part") is a whole number of tiles; a workgroup takes 32 queries, or 16 where vp_dev_topk_group says so
(D = 1536 always, D = 1024 at k = 128; the grouped search at D = 1024 from k = 64).  The masked scan deals the tiles
to its workgroups in turn.  N = 1025 is three tiles, which a device with at least 3 compute units per group of
queries searches as three parts of one tile each (relied on, not asserted: the result does not depend on it).
Q = 4096 at D = 64 is 128 groups of queries, which leaves a device of 256 compute units two parts, the first of two
tiles (the first and the third): the one case where a clear tile is not a clear part, and where a workgroup steps
over a tile that is not its own.
"""

import collections
import functools

import numpy as np

import grouped_retrieval_restatement as gr
import retrieval_restatement as rr

NS = (1, 31, 32, 33, 63, 65, 511, 512, 513, 1025)


def words(N):
    return (N + 31) // 32


def pack(allow, spare=0):
    """Packed words uint32 [..., words(N)] of allow bool [..., N]: bit r & 31 of word r >> 5 is row r; the spare bits
    of the last word are zeros, or ones with spare=1."""
    allow = np.asarray(allow, dtype=bool)
    N = allow.shape[-1]
    W = words(N)
    bits = np.full(allow.shape[:-1] + (W * 32,), bool(spare))
    bits[..., :N] = allow
    w = bits.reshape(allow.shape[:-1] + (W, 32)).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return w.sum(-1).astype(np.uint32)


def masked_topk(scores_f64, allow, k, id_base=0):
    """scores_f64 [N, Q], allow bool [N] or [Q, N] -> (scores [Q, k] float64, ids [Q, k] int64)."""
    N, Q = scores_f64.shape
    allow = np.broadcast_to(np.asarray(allow, dtype=bool), (Q, N))
    out_s = np.full((Q, k), -np.inf)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        rows = np.nonzero(allow[q])[0]
        s, i = rr.topk(scores_f64[rows, q][:, None], k)
        out_s[q] = s[0]
        out_i[q] = np.where(i[0] >= 0, id_base + rows[np.maximum(i[0], 0)] if len(rows) else -1, -1)
    return out_s, out_i


def masked_group_topk(scores_f64, labels, allow, k, id_base=0):
    """... and labels int64 [N] -> (scores, groups, ids), each [Q, k]."""
    N, Q = scores_f64.shape
    allow = np.broadcast_to(np.asarray(allow, dtype=bool), (Q, N))
    out_s = np.full((Q, k), -np.inf)
    out_g = np.full((Q, k), -1, dtype=np.int64)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        rows = np.nonzero(allow[q])[0]
        s, g, i = gr.group_topk(scores_f64[rows, q][:, None], labels[rows], k)
        out_s[q], out_g[q] = s[0], g[0]
        out_i[q] = np.where(i[0] >= 0, id_base + rows[np.maximum(i[0], 0)] if len(rows) else -1, -1)
    return out_s, out_g, out_i


# ---- masks ----
def make_mask(kind, N, Q, seed=0):
    """allow bool [N] (one mask for all queries) or, for the kinds that start with "pq", [Q, N]."""
    rng = np.random.default_rng(1000 + seed)
    m = np.zeros(N, dtype=bool)
    if kind == "ones":
        m[:] = True
    elif kind == "zeros":
        pass
    elif kind.startswith("one@"):  # exactly one bit
        r = N - 1 if kind == "one@last" else int(kind[4:])
        assert r < N, (kind, N)
        m[r] = True
    elif kind == "alternating":
        m[1::2] = True
    elif kind == "wave_clear":  # the second wave's 64 rows between allowed waves
        m[:] = True
        m[64:128] = False
    elif kind == "tile_clear":  # the first 512-row tile
        m[512:] = True
    elif kind == "part_clear":  # the middle tile: a whole part where a part is one tile
        m[:] = True
        m[512:1024] = False
    elif kind == "few":  # fewer than any k above 3
        m[rng.choice(N, size=min(3, N), replace=False)] = True
    elif kind == "random.5":
        m = rng.random(N) < 0.5
    elif kind == "random.03":
        m = rng.random(N) < 0.03
    elif kind == "pq_random":  # every query its own
        m = rng.random((Q, N)) < 0.5
    elif kind == "pq_mixed":  # nothing beside everything, in the first group of queries and in the last
        m = rng.random((Q, N)) < 0.3
        m[0] = False
        if Q > 1:
            m[1] = True
        if Q > 2:
            m[Q - 1] = False
            m[Q - 2] = True
    else:
        raise KeyError(kind)
    return m


Case = collections.namedtuple("Case", "N D k Q bf16 id_base mask grouped")


def _c(N, D, k, Q, bf16, mask, id_base=0, grouped=False):
    return Case(N, D, k, Q, bool(bf16), id_base, mask, grouped)


# every N, D, k and Q of the axes, both dtypes, every mask kind, and the pairings that share code: 16 queries a
# workgroup with per-query masks, several parts with clear ones, the grouped insert with every kind of skip
CASES = (
    _c(1, 64, 1, 1, 0, "ones"), _c(1, 64, 5, 33, 1, "zeros"), _c(1, 64, 5, 1, 1, "one@0", id_base=9),
    _c(31, 64, 5, 32, 1, "one@0"), _c(31, 64, 1, 33, 0, "one@last"), _c(31, 64, 128, 1, 0, "alternating"),
    _c(32, 64, 5, 1, 0, "one@31"), _c(32, 1024, 128, 33, 1, "pq_mixed"),
    _c(33, 64, 5, 33, 1, "one@32", id_base=1 << 40), _c(33, 64, 1, 32, 0, "one@31"),
    _c(63, 64, 5, 1, 1, "few"), _c(63, 1536, 5, 33, 0, "pq_random"),
    _c(65, 64, 5, 32, 0, "one@63"), _c(65, 64, 128, 1, 1, "one@64"), _c(65, 64, 1, 33, 1, "one@last"),
    _c(511, 64, 5, 33, 0, "wave_clear"), _c(511, 1024, 5, 1, 1, "random.03"), _c(511, 64, 128, 32, 1, "random.5"),
    _c(512, 64, 1, 1, 1, "one@511"), _c(512, 1536, 128, 33, 1, "alternating", id_base=3),
    _c(512, 64, 5, 32, 0, "pq_mixed"),
    _c(513, 64, 5, 1, 0, "one@512"), _c(513, 64, 128, 33, 1, "tile_clear"), _c(513, 1024, 128, 32, 0, "few"),
    _c(513, 64, 1, 33, 1, "one@511"),
    _c(1025, 64, 5, 33, 1, "part_clear"), _c(1025, 64, 128, 1, 0, "tile_clear", id_base=77),
    _c(1025, 1024, 5, 32, 1, "wave_clear"), _c(1025, 1536, 1, 33, 0, "one@last"),
    _c(1025, 64, 5, 32, 0, "random.03"), _c(1025, 1024, 128, 33, 1, "pq_random"), _c(1025, 64, 128, 33, 0, "zeros"),
    _c(1025, 64, 5, 4096, 1, "tile_clear"), _c(1025, 64, 5, 4096, 0, "random.5", id_base=2),
    _c(1025, 64, 1, 4096, 1, "alternating", grouped=True),
    # the grouped search: labels are row // 3 with every 11th row blanked (masked_labels)
    _c(1, 64, 5, 1, 1, "ones", grouped=True), _c(33, 64, 1, 33, 0, "one@32", grouped=True),
    _c(65, 64, 5, 32, 1, "alternating", grouped=True), _c(511, 1024, 64, 33, 1, "pq_mixed", grouped=True),
    _c(513, 64, 128, 1, 0, "wave_clear", grouped=True), _c(1025, 64, 5, 33, 0, "part_clear", grouped=True, id_base=5),
    _c(1025, 1536, 5, 32, 1, "random.5", grouped=True), _c(1025, 64, 128, 33, 1, "few", grouped=True),
    _c(1025, 1024, 1, 1, 0, "tile_clear", grouped=True), _c(512, 64, 5, 33, 1, "zeros", grouped=True),
    _c(1025, 64, 5, 32, 1, "pq_random", grouped=True),
)


def case_id(c):
    return (f"{'groups-' if c.grouped else ''}N{c.N}-D{c.D}-k{c.k}-Q{c.Q}-{'bf16' if c.bf16 else 'f32'}-{c.mask}"
            f"{'-base' if c.id_base else ''}")


@functools.lru_cache(maxsize=None)
def unit_rows(n, D, seed):
    """n unit-norm fp32 rows, the same for every case of one (n, D, seed)."""
    x = np.random.default_rng([seed, n, D]).standard_normal((n, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def masked_labels(N):
    lab = np.arange(N, dtype=np.int64) // 3 + (1 << 33)
    lab[5::11] = -1
    return lab
