"""Float64 restatement of the ChestMIR two-stage retrieval: what the device path must equal.

Scores are float64 sums of the stored float32 values, base ranking by descending score with ascending id on ties, combined
score w * base + (1 - w) * region in float64, sort key (combined desc, base desc, base position asc).  The dot products that
enter a combined score are summed in the order k_rerank.hip documents (`dot_lane_order`: lane l adds elements l, l + 64, ...
in ascending order, then a butterfly over lane distances 32 .. 1, which is a halving tree), so those keys equal the kernel's
bit for bit.  The base *ranking* comes from plain float64 dot products; rank_all's own summation order is not restated, which
is why the tests first assert `min_base_gap` > 1e-12 on their inputs (a reordering moves such a sum by about d * 2^-53).

Independent of mirx.chestmir: lesion maps come in as {canonical name: [vectors]} and targets as canonical names.
"""
import numpy as np


def dot_lane_order(a, b):
    """Row-wise float64 dot of float32 arrays a, b [m, d] in the kernel's order."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    m, d = a.shape
    k = (d + 63) // 64
    prod = np.zeros((m, k * 64))
    prod[:, :d] = a * b
    prod = prod.reshape(m, k, 64)
    p = np.zeros((m, 64))
    for t in range(k):
        p = p + prod[:, t, :]
    w = 32
    while w >= 1:
        p = p[:, :w] + p[:, w:2 * w]
        w //= 2
    return p[:, 0]


def base_scores(gv):
    g = np.asarray(gv, dtype=np.float32).astype(np.float64)
    s = g @ g.T
    np.fill_diagonal(s, -np.inf)
    return s


def base_ranking(gv):
    """-> (ranks [N, N] column i = query i, float64 scores [N, N])."""
    s = base_scores(gv)
    return np.argsort(-s, axis=0, kind="stable"), s


def min_base_gap(s):
    """Smallest gap between two different float64 scores of one query (exactly equal scores, the planted ties, fall to the id
    rule in every summation order and are exempt)."""
    d = -np.diff(np.sort(s, axis=0)[::-1], axis=0)
    d = d[np.isfinite(d) & (d > 0)]
    return float(d.min())


def plan_specific(lesion_maps, name):
    return [(name, m[name][0]) if m.get(name) else (None, None) for m in lesion_maps]


def plan_adaptive(lesion_maps, targets):
    out = []
    for m in lesion_maps:
        best = (None, None, -1)
        for name in targets:
            if m.get(name) and len(m[name]) > best[2]:
                best = (name, m[name][0], len(m[name]))
        out.append(best[:2])
    return out


def rerank(ranks_base, lesion_maps, plan, rerank_topk, w, gv=None, base_sim=None):
    """-> (ranks [N, N], matched [N], reranked [N], keys): `keys[i]` = (candidate ids, combined, base) of a re-ranked query.
    Base score of a candidate: base_sim[j, i] when given, else the lane-order float64 dot of the global vectors."""
    n = ranks_base.shape[0]
    topk = min(rerank_topk, n - 1)
    out = ranks_base.copy()
    matched = np.zeros(n, dtype=np.int64)
    flags = np.zeros(n, dtype=np.int64)
    keys = {}
    for i in range(n):
        name, q = plan[i]
        if q is None:
            continue
        top = ranks_base[:topk, i]
        if base_sim is not None:
            base = np.asarray([float(base_sim[j, i]) for j in top], dtype=np.float64)
        else:
            base = dot_lane_order(np.repeat(gv[i][None], topk, axis=0), gv[top])
        owner, vecs = [], []
        for c, j in enumerate(top):
            for v in lesion_maps[j].get(name, []):
                owner.append(c)
                vecs.append(v)
        region = np.full(topk, -1.0)
        if vecs:
            d = dot_lane_order(np.repeat(np.asarray(q)[None], len(vecs), axis=0), np.stack(vecs))
            best = np.full(topk, -np.inf)
            np.maximum.at(best, owner, d)
            has = np.zeros(topk, dtype=bool)
            has[owner] = True
            region[has] = best[has]
        matched[i] = int(np.count_nonzero(region >= 0.0))
        if matched[i] == 0:
            continue
        comb = (w * base) + ((1.0 - w) * region)
        order = np.lexsort((np.arange(topk), -base, -comb))
        out[:topk, i] = top[order]
        flags[i] = 1
        keys[i] = (top, comb, base)
    return out, matched, flags, keys


def stats(head, n, topk, matched, flags, rerank_topk, w, usage=None):
    total = int(matched[flags != 0].sum())
    reranked = int(flags.sum())
    out = dict(head)
    out.update({"queries_total": n, "queries_reranked": reranked, "queries_fallback_global": n - reranked,
                "queries_with_candidate_match": reranked, "matched_candidates_in_topk": total,
                "candidate_match_rate_pct": (100.0 * total / (n * topk)) if n * topk > 0 else 0.0, "rerank_topk": rerank_topk,
                "global_weight": w, "region_weight": 1.0 - w})
    if usage is not None:
        out["lesion_usage"] = usage
    return out


def usage(plan, flags):
    out = {}
    for (name, _), f in zip(plan, flags):
        if f:
            out[name] = out.get(name, 0) + 1
    return out


def report(ranks, labels, kappas, cls_k):
    """The metric tail in float64, query by query (compute_map's trapezoidal AP with the query itself a positive at the last
    rank, precision over min(largest positive rank, kappa) ranks, R@K, majority vote with first-met ties)."""
    lab = np.unique(np.asarray(labels).astype(str), return_inverse=True)[1]
    n = lab.shape[0]
    rel = lab[ranks] == lab[None, :]
    aps, prs, acc = np.zeros(n), np.zeros((n, len(kappas))), np.zeros(len(kappas))
    for i in range(n):
        pos = np.flatnonzero(rel[:, i])
        j = np.arange(pos.size, dtype=np.float64)
        p0 = np.where(pos == 0, 1.0, j / np.where(pos == 0, 1.0, pos))
        aps[i] = np.sum((p0 + (j + 1.0) / (pos + 1.0)) * (1.0 / pos.size) / 2.0)
        for t, kap in enumerate(kappas):
            kq = min(int(pos.max()) + 1, int(kap))
            prs[i, t] = np.count_nonzero(pos + 1 <= kq) / kq
            acc[t] += bool(rel[:kap, i].any())
    cls = {}
    for k in cls_k:
        pred = np.zeros(n, dtype=np.int64)
        for i in range(n):
            top = list(lab[ranks[:k, i]])
            pred[i] = max(top, key=lambda v: (top.count(v), -top.index(v)))
        classes = np.unique(np.concatenate([lab, pred]))
        p, r, f, sup = [], [], [], []
        for c in classes:
            tp = np.sum((lab == c) & (pred == c))
            fp = np.sum((lab != c) & (pred == c))
            fn = np.sum((lab == c) & (pred != c))
            pc = tp / (tp + fp) if tp + fp else 0.0
            rc = tp / (tp + fn) if tp + fn else 0.0
            p.append(pc)
            r.append(rc)
            f.append(2 * pc * rc / (pc + rc) if pc + rc else 0.0)
            sup.append(np.sum(lab == c))
        wts = np.asarray(sup, dtype=np.float64) / max(1, sum(sup))
        cls[k] = {"accuracy": float(np.mean(lab == pred)) * 100.0, "precision_macro": float(np.mean(p)) * 100.0,
                  "recall_macro": float(np.mean(r)) * 100.0, "f1_macro": float(np.mean(f)) * 100.0,
                  "precision_weighted": float(np.sum(np.asarray(p) * wts)) * 100.0,
                  "recall_weighted": float(np.sum(np.asarray(r) * wts)) * 100.0,
                  "f1_weighted": float(np.sum(np.asarray(f) * wts)) * 100.0}
    return {"R@K": {k: float(a * 100.0 / n) for k, a in zip(kappas, acc)}, "mAP": float(np.mean(aps) * 100.0),
            "mP@K": {k: float(v * 100.0) for k, v in zip(kappas, prs.mean(axis=0))}, "classification": cls}


def evaluate(gv, labels, lesion_maps, targets, kappas, cls_k, rerank_topk, w):
    """Every stage of evaluate_dataset: -> {"ranks": [S + 1 rank matrices], "matched", "reranked", "stats", "reports"}
    in the order stage 1, adaptive, one per target."""
    n = len(labels)
    topk = min(rerank_topk, n - 1)
    ranks_base, _ = base_ranking(gv)
    plans = [plan_adaptive(lesion_maps, targets)] + [plan_specific(lesion_maps, t) for t in targets]
    out = {"ranks": [ranks_base], "matched": [], "reranked": [], "keys": []}
    for plan in plans:
        r, m, f, keys = rerank(ranks_base, lesion_maps, plan, rerank_topk, w, gv=np.asarray(gv, dtype=np.float32))
        out["ranks"].append(r)
        out["matched"].append(m)
        out["reranked"].append(f)
        out["keys"].append(keys)
    out["plans"] = plans
    out["reports"] = [report(r, labels, kappas, cls_k) for r in out["ranks"]]
    out["topk"] = topk
    return out


def assert_report_close(a, b, tol=1e-12):
    assert set(a) == set(b)
    assert abs(a["mAP"] - b["mAP"]) <= tol, (a["mAP"], b["mAP"])
    for key in ("R@K", "mP@K"):
        assert set(a[key]) == set(b[key])
        for k in a[key]:
            assert abs(a[key][k] - b[key][k]) <= tol, (key, k, a[key][k], b[key][k])
    assert set(a["classification"]) == set(b["classification"])
    for k, m in a["classification"].items():
        assert set(m) == set(b["classification"][k])
        for name, v in m.items():
            assert abs(v - b["classification"][k][name]) <= tol, (k, name, v, b["classification"][k][name])


# ---- seeded synthetic datasets (inputs of the fixture, of the larger GPU case) --------------------------------------------
def synthetic_raw(seed, n, d, dr, classes, spellings, max_regions, signed=()):
    """Raw rows: unnormalised global vectors around class centres, 0..max_regions regions per image with names drawn from
    `spellings` (alias spellings of lesion names) and vectors around a centre per spelling's lesion (`centre_of`), so most
    region dots are positive and some are not.  Lesions in `signed` get the centre with a random sign per region: candidates
    whose only match is a negative dot."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, classes, size=n)
    centres = rng.standard_normal((classes, d))
    gv = (centres[cls] + 1.5 * rng.standard_normal((n, d))).astype(np.float32)
    groups = sorted({g for _, g in spellings})
    lcentre = {g: rng.standard_normal(dr) for g in groups}
    ptr, names, vecs = [0], [], []
    for _ in range(n):
        for _ in range(int(rng.integers(0, max_regions + 1))):
            text, g = spellings[int(rng.integers(0, len(spellings)))]
            sign = -1.0 if g in signed and rng.random() < 0.5 else 1.0
            names.append(text)
            vecs.append(sign * lcentre[g] + (0.3 if g in signed else 1.0) * rng.standard_normal(dr))
        ptr.append(len(names))
    return {"gv_raw": gv, "labels": np.asarray([f"class_{c}" for c in cls]), "image_names": np.asarray([f"img_{i:05d}.png" for i in range(n)]),
            "reg_ptr": np.asarray(ptr, dtype=np.int64), "reg_label": np.asarray(names),
            "reg_vec_raw": np.asarray(vecs, dtype=np.float32).reshape(len(names), dr)}


def rows_from_raw(raw):
    """The five-field row dicts of the collection, region fields as JSON strings (float32 -> repr round-trips exactly)."""
    import json
    rows = []
    for i in range(len(raw["labels"])):
        a, b = int(raw["reg_ptr"][i]), int(raw["reg_ptr"][i + 1])
        rows.append({"id": i, "image_name": str(raw["image_names"][i]), "label": str(raw["labels"][i]),
                     "global_vector": [float(x) for x in raw["gv_raw"][i]],
                     "region_labels_json": json.dumps([str(x) for x in raw["reg_label"][a:b]]),
                     "region_vectors_json": json.dumps([[float(x) for x in v] for v in raw["reg_vec_raw"][a:b]])})
    return rows


def flatten_maps(lesion_maps):
    """Lesion maps -> (ptr [N + 1], names per vector, vectors [R, Dr]) in map order; `unflatten_maps` is the inverse."""
    ptr, names, vecs = [0], [], []
    for m in lesion_maps:
        for name, cands in m.items():
            names.extend([name] * len(cands))
            vecs.extend(cands)
        ptr.append(len(names))
    dr = len(vecs[0]) if vecs else 1
    return np.asarray(ptr, dtype=np.int64), np.asarray(names), np.asarray(vecs, dtype=np.float32).reshape(len(names), dr)


def unflatten_maps(ptr, names, vecs):
    maps = []
    for i in range(len(ptr) - 1):
        m = {}
        for r in range(int(ptr[i]), int(ptr[i + 1])):
            m.setdefault(str(names[r]), []).append(np.asarray(vecs[r], dtype=np.float32))
        maps.append(m)
    return maps
