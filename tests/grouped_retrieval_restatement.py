"""The order rule of the grouped gallery search (vp_op_topk_groups / vp_op_topk_groups_merge), restated in NumPy.

Each gallery row carries an int64 label, its group.  A group's score is the largest score of its rows and its best row
is the row with that score, of equal scores the one with the smallest id.  The result lists the k best groups: score
descending, equal scores by ascending id of the best row; with fewer than k qualifying groups the tail is
(-inf, -1, -1).  A row whose score is NaN or -inf, or whose label is negative, is never returned and never stands for
a group.  The row rule itself (what qualifies, score descending, ties by id) is tests/retrieval_restatement.py's.
"""

import numpy as np

import retrieval_restatement as rr


def group_topk(scores_f64, labels, k, id_base=0):
    """scores_f64 [N, Q], labels [N] -> (scores [Q, k] float64, groups [Q, k] int64, ids [Q, k] int64 = id_base +
    best row)."""
    s = np.asarray(scores_f64, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    N, Q = s.shape
    assert labels.shape == (N,)
    out_s = np.full((Q, k), -np.inf)
    out_g = np.full((Q, k), -1, dtype=np.int64)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    blank = np.where(labels[:, None] < 0, -np.inf, s)  # a blanked row scores -inf: rr.topk never returns it
    all_s, all_i = rr.topk(blank, N) if N else (np.empty((Q, 0)), np.empty((Q, 0), dtype=np.int64))
    for q in range(Q):
        seen, n = set(), 0
        for sc, row in zip(all_s[q], all_i[q]):  # every qualifying row, best first: a group's first row is its best
            if row < 0 or n == k:
                break
            g = int(labels[row])
            if g in seen:
                continue
            seen.add(g)
            out_s[q, n], out_g[q, n], out_i[q, n] = sc, g, id_base + row
            n += 1
    return out_s, out_g, out_i


def group_merge(scores, groups, ids, k):
    """Lists scores / groups / ids [parts, Q, k_in] -> the best k groups per query: the union of the lists, per group
    the entry that comes first in the order (score descending, id ascending), then the first k."""
    scores = np.asarray(scores, dtype=np.float64)
    groups = np.asarray(groups, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    parts, Q, k_in = scores.shape
    out_s = np.full((Q, k), -np.inf)
    out_g = np.full((Q, k), -1, dtype=np.int64)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        s, g, i = scores[:, q].reshape(-1), groups[:, q].reshape(-1), ids[:, q].reshape(-1)
        keep = (i >= 0) & (g >= 0) & ~np.isnan(s) & (s > -np.inf)
        s, g, i = s[keep], g[keep], i[keep]
        seen, n = set(), 0
        for j in np.lexsort((i, -s)):
            if n == k:
                break
            if int(g[j]) in seen:
                continue
            seen.add(int(g[j]))
            out_s[q, n], out_g[q, n], out_i[q, n] = s[j], g[j], i[j]
            n += 1
    return out_s, out_g, out_i
