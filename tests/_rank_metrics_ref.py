"""Float64 numpy restatement of the ranked-list metric walk with a group taken out (mirx_rank_metrics_grouped and
mirx_index_rank_metrics): per query it builds the list, deletes the taken-out entries, then applies the reference's
formulas -- the trapezoidal AP of test.py:58-92 as compute_map sums it (test.py:95-146), or the standard AP (mean of the
precision at each relevant rank, test.py:941-985) -- to what is left.  Written from the contract in include/mirx.h, one query at
a time, with none of the kernels' structure (no 64-entry steps, no segments)."""
import numpy as np


def popcount(x):
    return bin(int(x) & 0xFFFFFFFFFFFFFFFF).count("1")


def relevant(glab, qlab, jaccard=None):
    """label equality, or Jaccard of two multi-hot bit masks above the threshold, as test.py:958-961 evaluates it"""
    if jaccard is None:
        return int(glab) == int(qlab)
    inter = float(popcount(int(glab) & int(qlab)))
    union = float(popcount(qlab)) + float(popcount(glab)) - inter
    return inter / (union + 1e-8) > jaccard


def walk(order, gallery_labels, qlab, kappas=(), self_id=None, drop_self=False, gallery_codes=None, qcode=-1, jaccard=None,
         standard_ap=False):
    """One ranked list (ids, best first) -> (ap, cnt [len(kappas)], nrel, maxpos).
    self_id: never relevant; with drop_self also taken out.  An id within [0, len(gallery_labels)) whose code is the query's
    (qcode >= 0) is taken out.  Ids outside that range stay in the list and are never relevant."""
    n_labels = len(gallery_labels)
    rel = []                                                          # relevance of the entries that stay, in order
    for id_ in (int(v) for v in order):
        known = 0 <= id_ < n_labels
        is_self = self_id is not None and id_ == int(self_id)
        if (is_self and drop_self) or (known and gallery_codes is not None and qcode >= 0 and int(gallery_codes[id_]) == int(qcode)):
            continue
        rel.append(known and not is_self and relevant(gallery_labels[id_], qlab, jaccard))
    pos = np.flatnonzero(np.asarray(rel, dtype=bool)).astype(np.float64)      # 0-based positions of the positives left
    nrel = int(pos.size)
    cnt = [int(np.count_nonzero(pos < k)) for k in kappas]
    if nrel == 0:
        return float("nan"), cnt, 0, 0
    j = np.arange(nrel, dtype=np.float64)
    p1 = (j + 1.0) / (pos + 1.0)
    if standard_ap:
        ap = float(np.sum(p1) / nrel)
    else:
        p0 = np.where(pos == 0, 1.0, j / np.where(pos == 0, 1.0, pos))
        ap = float(np.sum((p0 + p1) * 0.5) / nrel)
    return ap, cnt, nrel, int(pos[-1]) + 1


def metrics(ranks, gallery_labels, query_labels, kappas=(), query_ids=None, drop_self=False, gallery_codes=None,
            query_codes=None, jaccard=None, standard_ap=False):
    """rows of `ranks` -> dict of numpy arrays with the keys and dtypes of rank_metrics_device"""
    nq = len(ranks)
    out = {"ap": np.full(nq, np.nan), "cnt": np.zeros((nq, len(kappas)), dtype=np.int64), "nrel": np.zeros(nq, dtype=np.int64),
           "maxpos": np.zeros(nq, dtype=np.int64)}
    for q in range(nq):
        ap, cnt, nrel, maxpos = walk(ranks[q], gallery_labels, query_labels[q], kappas,
                                     None if query_ids is None else query_ids[q], drop_self, gallery_codes,
                                     -1 if query_codes is None else int(query_codes[q]), jaccard, standard_ap)
        out["ap"][q], out["nrel"][q], out["maxpos"][q] = ap, nrel, maxpos
        out["cnt"][q] = cnt
    return out


def map_from(res, kappas):
    """compute_map's (mAP, aps, pr, prs) from walk results: precision@kappa over kq = min(max(pos), kappa) (test.py:139), queries
    without a positive skipped in both means (test.py:122-126)"""
    aps = res["ap"]
    nq, nk = aps.shape[0], len(kappas)
    prs = np.full((nq, nk), np.nan)
    for q in range(nq):
        if res["nrel"][q] == 0:
            continue
        for j, kap in enumerate(kappas):
            kq = min(float(res["maxpos"][q]), float(kap))
            hits = res["cnt"][q, j] if kap <= res["maxpos"][q] else res["nrel"][q]
            prs[q, j] = hits / kq
    ok = ~np.isnan(aps)
    if not ok.any():
        return float("nan"), aps, np.full(nk, np.nan), prs
    return float(aps[ok].sum() / ok.sum()), aps, prs[ok].sum(axis=0) / ok.sum(), prs


def self_ranking(emb, metric="l2", ids=None):
    """[N, N] rows per query: fp64 score descending (negative squared distance, or the dot product), equal scores by ascending
    id, the query itself last (rank_all with exclude_ids = own id).  -> positions (rows of emb), not ids."""
    e = np.asarray(emb, dtype=np.float64)
    n = e.shape[0]
    ids = np.arange(n) if ids is None else np.asarray(ids)
    if metric == "l2":
        s = -((e[:, None, :] - e[None, :, :]) ** 2).sum(-1)
    else:
        s = e @ e.T
    out = np.empty((n, n), dtype=np.int64)
    for q in range(n):
        sq = s[q].copy()
        sq[q] = -np.inf
        out[q] = np.lexsort((ids, -sq))
    return out


def group_sizes_1_to_8(n, seed):
    """group codes for n images: groups of sizes 1, 2, .. 8, 1, 2, .. dealt to a seeded permutation of the images"""
    perm = np.random.default_rng(seed).permutation(n)
    codes = np.empty(n, dtype=np.int32)
    g = i = 0
    while i < n:
        size = g % 8 + 1
        codes[perm[i:i + size]] = g
        i += size
        g += 1
    return codes
