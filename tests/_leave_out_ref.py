"""A numpy restatement of the leave-group-out search contract (mirx_index_search_leave_out) for the tests.

It touches no mirx code: the fp64 ranking scores come from oracle.search.scores (oracle/search_ref.c's lane-tree order) and the
rest is numpy.  Row r is eligible for query i when allow[r] != 0 (with a mask), ids[r] != exclude[i] (with excluded ids) and not
(query_codes[i] >= 0 and row_codes[r] == query_codes[i]); the answer is the eligible rows by (score descending, id ascending),
cut at k and padded with (-inf, -1)."""
import numpy as np

from oracle import search as OS


def eligible(row_codes, query_code, ids, exclude_id=None, allow=None):
    """bool [n]: the rows one query may return"""
    row_codes = np.asarray(row_codes)
    ok = np.ones(row_codes.shape[0], dtype=bool) if allow is None else np.asarray(allow) != 0
    if exclude_id is not None:
        ok = ok & (np.asarray(ids) != exclude_id)
    if query_code >= 0:
        ok = ok & (row_codes != query_code)
    return ok


def topk(q, g, k, row_codes, query_codes, metric=0, ids=None, exclude=None, allow=None):
    """-> (fp64 ranking scores [nq, k], ids int64 [nq, k]); q, g: float32 arrays whose width is a multiple of 4"""
    q, g = np.asarray(q, dtype=np.float32), np.asarray(g, dtype=np.float32)
    nq, n = q.shape[0], g.shape[0]
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    out_s = np.full((nq, k), -np.inf, dtype=np.float64)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    if n == 0:
        return out_s, out_i
    for q0 in range(0, nq, 64):
        s = OS.scores(q[q0:q0 + 64], g, metric)
        for j in range(s.shape[0]):
            i = q0 + j
            ok = eligible(row_codes, int(query_codes[i]), ids, None if exclude is None else int(exclude[i]), allow)
            rows = np.nonzero(ok)[0]
            sc = s[j, rows] + 0.0                                   # -0.0 -> +0.0: the two tie, the id decides
            if rows.shape[0] > k:                                   # only the rows at or above the k-th score can rank
                keep = sc >= np.partition(sc, rows.shape[0] - k)[rows.shape[0] - k]
                rows, sc = rows[keep], sc[keep]
            order = np.lexsort((ids[rows], -sc))[:k]
            out_s[i, :order.shape[0]] = s[j, rows[order]]
            out_i[i, :order.shape[0]] = ids[rows[order]]
    return out_s, out_i
