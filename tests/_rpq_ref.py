"""CPU restatement of IVF_PQ with residual coding (include/mirx.h, mirx_ivf_create_pq_ex) on tests/_pq_ref.py and
tests/_ivf_ref.py: residuals, codebooks and codes of the residuals, the per-(query, list) bases, the row norms and the scores
as the two-level sequential float64 sums the header defines.  Test infrastructure only."""
import numpy as np

import _ivf_ref as R
import _pq_ref as P
from oracle import search as OS

F4, F8 = np.float32, np.float64


def residuals(rows, lists, centroids):
    """[n, dim] float32: row - centroid of its list, one rounding per column"""
    rows = np.ascontiguousarray(rows, dtype=F4)
    return np.ascontiguousarray(rows - np.ascontiguousarray(centroids, dtype=F4)[np.asarray(lists)], dtype=F4)


def train_codebooks(rows, centroids, m, iters, metric):
    """_pq_ref.train_codebooks on the residuals of the rows under their own lists"""
    return P.train_codebooks(residuals(rows, R.assign(rows, centroids, metric), centroids), m, iters)


def encode(rows, lists, centroids, cb):
    return P.encode(residuals(rows, lists, centroids), cb)


def reconstruct(codes, lists, centroids, cb):
    """[n, dim] float32: centroid + codewords, one rounding per column"""
    return np.ascontiguousarray(np.ascontiguousarray(centroids, dtype=F4)[np.asarray(lists)] + P.decode(codes, cb), dtype=F4)


def two_level(a, b, m):
    """sum over j ascending of P_j, P_j one sequential float64 accumulator from 0.0 over sub-space j's columns of a * b (the
    product rounded to float64 first); a, b float64 arrays that broadcast to [..., dim]"""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=F8), np.asarray(b, dtype=F8))
    ds = a.shape[-1] // m
    total = np.zeros(a.shape[:-1], dtype=F8)
    for j in range(m):
        part = np.zeros(a.shape[:-1], dtype=F8)
        for e in range(j * ds, (j + 1) * ds):
            part = part + a[..., e] * b[..., e]
        total = total + part
    return total


def bases(q, lists, centroids, m):
    """[nq, nprobe] float64: B[q][s] for the list numbers lists [nq, nprobe]"""
    q = np.ascontiguousarray(q, dtype=F4)
    c = np.ascontiguousarray(centroids, dtype=F4)[np.asarray(lists)]           # [nq, nprobe, dim]
    return two_level(q[:, None, :], c, m)


def qq(q, m):
    q = np.ascontiguousarray(q, dtype=F4)
    return two_level(q, q, m)


def norms(codes, lists, centroids, cb):
    """[n] float64: N2 = the two-level sum of xh * xh, xh = (double)centroid + (double)codeword"""
    xh = np.ascontiguousarray(centroids, dtype=F4)[np.asarray(lists)].astype(F8) + P.decode(codes, cb).astype(F8)
    return two_level(xh, xh, cb.shape[0])


def scores(q, codes, lists, centroids, cb, metric):
    """[nq, n] float64 ranking scores of every row as if its list were probed: ip = B[q][list]; + T[j][code[j]], j ascending, T the
    IP tables of the residual codebooks; IP: ip; L2: -((QQ + N2) - 2.0 * ip)"""
    q = np.ascontiguousarray(q, dtype=F4)
    m, nlist = cb.shape[0], np.asarray(centroids).shape[0]
    every = np.broadcast_to(np.arange(nlist), (q.shape[0], nlist))
    ip = bases(q, every, centroids, m)[:, np.asarray(lists)]
    T = P.tables(q, cb, "IP")
    for j in range(m):
        ip = ip + T[:, j, :][:, codes[:, j]]
    if R.metric_code(metric) == OS.METRIC_IP:
        return ip
    return -((qq(q, m)[:, None] + norms(codes, lists, centroids, cb)[None, :]) - 2.0 * ip)


def search(q, rows, ids, centroids, cb, k, nprobe, metric, exclude=None, codes=None):
    """_pq_ref.search with the residual scores: (fp64 scores [nq, k], ids [nq, k])"""
    q = np.ascontiguousarray(q, dtype=F4)
    rows = np.ascontiguousarray(rows, dtype=F4)
    ids = np.arange(rows.shape[0], dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    lists = R.assign(rows, centroids, metric)
    codes = encode(rows, lists, centroids, cb) if codes is None else codes
    pr = R.probes(q, centroids, nprobe, metric)
    sc = scores(q, codes, lists, centroids, cb, metric)
    out_s = np.full((q.shape[0], k), -np.inf, dtype=F8)
    out_i = np.full((q.shape[0], k), -1, dtype=np.int64)
    for i in range(q.shape[0]):
        keep = np.isin(lists, pr[i])
        if exclude is not None:
            keep &= ids != exclude[i]
        pos = np.flatnonzero(keep)
        order = pos[np.lexsort((ids[pos], -sc[i, pos]))][:k]
        out_s[i, :order.size], out_i[i, :order.size] = sc[i, order], ids[order]
    return out_s, out_i


def shared_codes(codes, lists=None):
    """rows whose whole code row (within their list, if lists are given) repeats an earlier row's: n - the distinct code rows"""
    key = codes if lists is None else np.concatenate([np.asarray(lists)[:, None].astype(np.int64), codes.astype(np.int64)], axis=1)
    return int(key.shape[0] - np.unique(key, axis=0).shape[0])
