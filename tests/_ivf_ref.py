"""CPU restatement of the IVF_FLAT index (include/mirx.h, mirx_ivf_*) on oracle.search: assignment, one Lloyd update, train,
probes, and the IVF answer as "the oracle's top-k over the rows whose list is probed".  Test infrastructure only."""
import numpy as np

from oracle import search as OS


def metric_code(metric):
    if isinstance(metric, str):
        return OS.METRIC_NEG_L2 if metric.upper() == "L2" else OS.METRIC_IP
    return int(metric)


def assign(rows, centroids, metric):
    """list of every row: its best centroid by the fp64 ranking score, ties to the lowest list"""
    _, ids = OS.topk(rows, centroids, 1, metric_code(metric))
    return ids[:, 0]


def probes(q, centroids, nprobe, metric):
    """[nq, min(nprobe, nlist)] lists, nearest first"""
    _, ids = OS.topk(q, centroids, min(int(nprobe), centroids.shape[0]), metric_code(metric))
    return ids


def update(rows, lists, centroids, metric):
    """One Lloyd update: per list and column one float64 accumulator over the list's rows in ascending row order
    (np.cumsum(...)[-1] is that sequential sum), / count, rounded once to float32; IP: the float32 mean normalised as
    mirx_l2_normalize does; an empty list keeps its centroid."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    out = np.array(centroids, dtype=np.float32, copy=True)
    for l in range(out.shape[0]):
        members = rows[lists == l].astype(np.float64)
        if members.shape[0] == 0:
            continue
        mean = (np.cumsum(members, axis=0)[-1] / np.float64(members.shape[0])).astype(np.float32)
        if metric_code(metric) == OS.METRIC_IP:
            mean = OS.l2_normalize(mean[None])[0]
        out[l] = mean
    return out


def default_positions(n, nlist):
    return (np.arange(nlist, dtype=np.int64) * n) // nlist


def train(rows, nlist, iters, metric, init_positions=None):
    """centroids after mirx_ivf_train's loop: start at rows[init_positions], at most `iters` updates, stop when an
    assignment pass changes nothing"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    pos = default_positions(rows.shape[0], nlist) if init_positions is None else np.asarray(init_positions, dtype=np.int64)
    cent = rows[pos].copy()
    prev = None
    for it in range(iters):
        cur = assign(rows, cent, metric)
        if it > 0 and np.array_equal(cur, prev):
            break
        cent = update(rows, cur, cent, metric)
        prev = cur
    return cent


def search(q, rows, ids, centroids, k, nprobe, metric, exclude=None):
    """(fp64 scores [nq, k], ids [nq, k]): per query the oracle's top-k over the rows whose list is among its probes,
    (-inf, -1) past the eligible rows"""
    q = np.ascontiguousarray(q, dtype=np.float32)
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    ids = np.arange(rows.shape[0], dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    lists = assign(rows, centroids, metric)
    pr = probes(q, centroids, nprobe, metric)
    out_s = np.full((q.shape[0], k), -np.inf, dtype=np.float64)
    out_i = np.full((q.shape[0], k), -1, dtype=np.int64)
    for i in range(q.shape[0]):
        keep = np.isin(lists, pr[i])
        if keep.any():
            ex = None if exclude is None else np.asarray(exclude[i:i + 1], dtype=np.int64)
            s, j = OS.topk(q[i:i + 1], rows[keep], k, metric_code(metric), exclude=ex, ids=ids[keep])
            out_s[i], out_i[i] = s[0], j[0]
    return out_s, out_i


def recall(found, exact):
    """mean over queries of |found ∩ exact| / |exact| (ids >= 0)"""
    return float(np.mean([len(set(f[f >= 0]) & set(e[e >= 0])) / max(1, int((e >= 0).sum())) for f, e in zip(found, exact)]))
