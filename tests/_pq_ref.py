"""CPU restatement of IVF_PQ (include/mirx.h, mirx_ivf_create_pq) on tests/_ivf_ref.py and oracle.search: codebooks, codes, the
ADC tables and scores as the sequential float64 sums the header defines, and the answer as a lexsort over the probed lists'
rows.  Test infrastructure only."""
import numpy as np

import _ivf_ref as R
from oracle import search as OS

F4, F8 = np.float32, np.float64


def _sub(a, m, j):
    ds = a.shape[1] // m
    return np.ascontiguousarray(a[:, j * ds:(j + 1) * ds], dtype=F4)


def train_codebooks(rows, m, iters):
    """[m, 256, dim / m]: per sub-space mirx_ivf_train's loop with 256 lists, always L2"""
    return np.stack([R.train(_sub(rows, m, j), 256, iters, "L2") for j in range(m)])


def encode(rows, cb):
    """[n, m] uint8: per sub-space the nearest codeword by the oracle's L2 ranking, ties to the lowest code"""
    m = cb.shape[0]
    return np.stack([R.assign(_sub(rows, m, j), cb[j], "L2") for j in range(m)], axis=1).astype(np.uint8)


def decode(codes, cb):
    return np.ascontiguousarray(np.concatenate([cb[j][codes[:, j]] for j in range(cb.shape[0])], axis=1), dtype=F4)


def tables(q, cb, metric, fused=None):
    """[nq, m, 256] float64: one sequential accumulator over the sub-space's columns; L2 rounds d * d before it is added.
    fused = a float fma(a, b, c): the restatement a fused L2 would match instead (tests show the two differ)."""
    q = np.ascontiguousarray(q, dtype=F4)
    m, _, ds = cb.shape
    ip = R.metric_code(metric) == OS.METRIC_IP
    out = np.empty((q.shape[0], m, 256), dtype=F8)
    for j in range(m):
        acc = np.zeros((q.shape[0], 256), dtype=F8)
        for e in range(ds):
            qe, ce = q[:, j * ds + e].astype(F8)[:, None], cb[j, :, e].astype(F8)[None, :]
            if ip:
                acc = acc + qe * ce
            elif fused is None:
                d = qe - ce
                acc = acc + d * d
            else:
                d = qe - ce
                acc = np.array([[fused(float(x), float(x), float(a)) for x, a in zip(dr, ar)] for dr, ar in zip(d, acc)], dtype=F8)
        out[:, j] = acc
    return out


def scores(q, codes, cb, metric):
    """[nq, n] float64 ranking scores: s = 0.0, then + T[j][code[j]] for j ascending; negated for L2"""
    T = tables(q, cb, metric)
    s = np.zeros((q.shape[0], codes.shape[0]), dtype=F8)
    for j in range(cb.shape[0]):
        s = s + T[:, j, :][:, codes[:, j]]
    return s if R.metric_code(metric) == OS.METRIC_IP else -s


def values(s, metric):
    """the fp32 values the boundary reports for ranking scores s"""
    with np.errstate(invalid="ignore"):
        v = OS.reported_value(np.where(np.isinf(s), 0.0, s), R.metric_code(metric)).astype(F4)
    return np.where(np.isinf(s), F4(-np.inf), v)


def search(q, rows, ids, centroids, cb, k, nprobe, metric, exclude=None, codes=None):
    """(fp64 scores [nq, k], ids [nq, k]): per query the best k ADC scores, (score desc, id asc), over the rows whose list -- chosen
    from the ORIGINAL row -- is probed; the excluded id skipped, (-inf, -1) past the eligible rows"""
    q = np.ascontiguousarray(q, dtype=F4)
    rows = np.ascontiguousarray(rows, dtype=F4)
    ids = np.arange(rows.shape[0], dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    codes = encode(rows, cb) if codes is None else codes
    lists = R.assign(rows, centroids, metric)
    pr = R.probes(q, centroids, nprobe, metric)
    sc = scores(q, codes, cb, metric)
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
