"""The order rule of the gallery search (vp_op_topk / vp_op_topk_merge), restated in NumPy.

Score descending, ties by ascending id; a row whose score is NaN or -inf is never returned; with fewer than k
qualifying rows the tail is (-inf, -1); entries with id -1 are padding and sort last.
"""

import numpy as np


def topk(scores_f64, k, id_base=0):
    """scores_f64 [N, Q] (the score of every gallery row for every query) -> (scores [Q, k] float64, ids [Q, k]
    int64 = id_base + row)."""
    s = np.asarray(scores_f64, dtype=np.float64)
    N, Q = s.shape
    out_s = np.full((Q, k), -np.inf)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        col = s[:, q]
        rows = np.nonzero(~np.isnan(col) & (col > -np.inf))[0]
        order = rows[np.argsort(-col[rows], kind="stable")][:k]  # rows ascend, so a stable sort breaks ties by id
        out_s[q, :len(order)] = col[order]
        out_i[q, :len(order)] = id_base + order
    return out_s, out_i


def merge(scores, ids, k):
    """Sorted lists scores / ids [parts, Q, k_in] -> the best k per query, same order."""
    scores = np.asarray(scores, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64)
    parts, Q, k_in = scores.shape
    out_s = np.full((Q, k), -np.inf)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        s, i = scores[:, q].reshape(-1), ids[:, q].reshape(-1)
        keep = (i >= 0) & ~np.isnan(s) & (s > -np.inf)
        s, i = s[keep], i[keep]
        order = np.lexsort((i, -s))[:k]
        out_s[q, :len(order)] = s[order]
        out_i[q, :len(order)] = i[order]
    return out_s, out_i
