"""CPU restatement of IVF_SQ8's quantiser (include/mirx.h, mirx_ivf_sq8_* / mirx_sq8_*) in numpy, and the IVF_SQ8 answer as
"tests/_ivf_ref.py's answer over the decoded rows, the lists taken from the original rows".  Test infrastructure only."""
import numpy as np

import _ivf_ref as R
from oracle import search as OS

F4, F8 = np.float32, np.float64


def train_range(rows):
    """(vmin [dim], scale [dim]) fp32: the column's minimum (NaN ignored, a zero stored as +0) and
    (float)(((double)vmax - (double)vmin) / 255.0); a column without a number gets vmin = scale = 0"""
    rows = np.ascontiguousarray(rows, dtype=F4)
    nan = np.isnan(rows)
    mn = np.where(nan, F4(np.inf), rows).min(axis=0)
    mx = np.where(nan, F4(-np.inf), rows).max(axis=0)
    some = mn <= mx
    with np.errstate(invalid="ignore"):
        scale = ((mx.astype(F8) - mn.astype(F8)) / F8(255.0)).astype(F4)
    return np.where(some, mn + F4(0.0), F4(0.0)).astype(F4), np.where(some, scale, F4(0.0)).astype(F4)


def encode(rows, vmin, scale):
    """uint8 [n, dim]: min(255, max(0, floor(((double)x - vmin) / scale + 0.5))); a zero scale and NaN give 0"""
    rows = np.ascontiguousarray(rows, dtype=F4)
    with np.errstate(all="ignore"):
        t = (rows.astype(F8) - vmin.astype(F8)) / scale.astype(F8)
        r = np.floor(t + F8(0.5))
    r = np.where(np.isnan(r), 0.0, np.minimum(255.0, np.maximum(0.0, r)))
    return np.where(scale == 0, 0.0, r).astype(np.uint8)


def decode(codes, vmin, scale):
    """fp32 [n, dim]: the issue's literal form"""
    with np.errstate(all="ignore"):
        return (vmin.astype(F8) + codes.astype(F8) * scale.astype(F8)).astype(F4)


def search(q, rows, ids, centroids, vmin, scale, k, nprobe, metric, exclude=None):
    """(fp64 scores, ids): per query the oracle's top-k over the DECODED rows whose list -- assigned from the ORIGINAL rows --
    is among its probes"""
    q = np.ascontiguousarray(q, dtype=F4)
    rows = np.ascontiguousarray(rows, dtype=F4)
    ids = np.arange(rows.shape[0], dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    lists = R.assign(rows, centroids, metric)
    dec = decode(encode(rows, vmin, scale), vmin, scale)
    pr = R.probes(q, centroids, nprobe, metric)
    out_s = np.full((q.shape[0], k), -np.inf, dtype=F8)
    out_i = np.full((q.shape[0], k), -1, dtype=np.int64)
    for i in range(q.shape[0]):
        keep = np.isin(lists, pr[i])
        if keep.any():
            ex = None if exclude is None else np.asarray(exclude[i:i + 1], dtype=np.int64)
            s, j = OS.topk(q[i:i + 1], dec[keep], k, R.metric_code(metric), exclude=ex, ids=ids[keep])
            out_s[i], out_i[i] = s[0], j[0]
    return out_s, out_i
