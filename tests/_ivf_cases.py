"""What the IVF family's GPU tests share (test_ivf_gpu, test_ivf_sq8_gpu, test_ivf_pq_gpu, test_ivf_rpq_gpu, test_ivf_family_gpu):
the small conversions and the generator of rows with forced list sizes.  The per-kind _layout / _check helpers stay in their
files: they assert different things."""
import numpy as np

import _ivf_ref as R
from oracle import search as OS

F4, F8 = np.float32, np.float64
SIZES = [257, 0, 1, 63, 64, 65, 120]          # list 1 is empty: its centroid duplicates list 0's and the tie goes to list 0


def _lib():
    import mirx._lib as L
    return L


def _np(t):
    return t.cpu().numpy()


def _unit(x):
    return OS.l2_normalize(np.ascontiguousarray(x, dtype=F4))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F8 else np.uint32)


def forced(sizes, dim, metric, seed, noise):
    """rows around len(sizes) centroids so that the lists hold `sizes` rows (an empty list's centroid duplicates list 0's), user
    ids descending, two pairs of equal rows in list 0: equal codes, norms and scores, only the ids tell them apart.  `noise` (a
    Python float) is the factor in front of the normal draws around a centroid.  -> (rows, ids, cent, base)"""
    rng = np.random.default_rng(seed)
    base = _unit(rng.standard_normal((len(sizes), dim)))
    cent = base.copy()
    rows, want = [], []
    for l, n in enumerate(sizes):
        if n == 0:
            cent[l] = cent[0]
        r = base[l] + noise * rng.standard_normal((n, dim)).astype(F4)
        rows.append(_unit(r) if metric == "COSINE" else r.astype(F4))
        want += [l] * n
    rows = np.concatenate(rows)
    perm = rng.permutation(rows.shape[0])
    rows, want = np.ascontiguousarray(rows[perm]), np.asarray(want)[perm]
    first = np.flatnonzero(want == 0)
    rows[first[1]] = rows[first[0]]
    rows[first[3]] = rows[first[2]]
    ids = (10 ** 6 - 3 * np.arange(rows.shape[0], dtype=np.int64))
    assert np.bincount(R.assign(rows, cent, metric), minlength=len(sizes)).tolist() == list(sizes)
    return rows, ids, cent, base
