"""ChestMIR two-stage retrieval: global ranking, lesion-aware re-ranking, evaluation.

Mirrors (paths into the reference tree) ChestMIR/chestmir_eval.py:
  lesion name tables, canonical_lesion_name, parse_json_list, build_lesion_vector_map      :19-125, 276-319
  build_vindr_label_lookup, normalize_rows, EvalDataset, load_eval_dataset                  :127-131, 270-273, 322-431
  similarity_to_ranks, evaluate_rankings                                                    :434-454
  choose_query_lesion_vector, best_candidate_lesion_score, choose_query_adaptive_lesion_vector   :457-514
  rerank_with_specific_lesion, rerank_with_adaptive_lesion, print_stage_report              :517-671
  evaluate_dataset: what main() does between loading the collection and the final summary    :726-829

The reference pages a Milvus collection and then works in numpy with Python loops.  Here the four ranking functions keep
their numpy-in / numpy-out contracts and run on the device when they can: the re-rank on mirx_lesion_rerank (k_rerank.hip),
the mAP / R@K / mP@K tail on mirx_rank_metrics.  `evaluate_dataset` uploads a dataset once, ranks it with
FlatIndex.rank_all and runs every stage (adaptive + one per lesion) in one re-rank launch and one metric launch; only the
first max(classification_k) ranks of each stage come back for the majority vote.  `<function>.last_native` tells which path
the last call took.

Device gate: a GPU is visible, N <= 65 536, all region vectors of one dimension Dr with 1 <= Dr <= 4096,
1 <= min(rerank_topk, N - 1) <= 1024, at most 8 kappas, and the S + 2 [N, N] 8-byte matrices of a call (S re-ranked stages,
the base ranking, the base scores) fit in DEVICE_SHARE of the free device memory.  Everything else runs the reference's formulas in numpy (float32 dot products, Python's stable sort), the same public functions.

Scores on the device are float64 sums of the stored float32 values in the fixed order k_rerank.hip documents; the base
ranking is by float64 score, ties to the lower id.  The reference's float32 path can differ from that only at near-ties
(DESIGN 22 derives the bound); `similarity_to_ranks` itself has no device path (it sorts a host matrix; `last_native` stays
False) and keeps numpy's default sort like the reference.
"""
import csv
import ctypes
import json
from collections import Counter
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import metrics as _metrics

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

RERANK_MAX_N = 65536             # include/mirx.h MIRX_RERANK_MAX_N (the re-rank kernel's own limit)
RERANK_MAX_DR = 4096             # MIRX_RERANK_MAX_DR
RERANK_MAX_TOPK = 1024           # MIRX_RERANK_MAX_TOPK
DEVICE_SHARE = 0.8               # of the free device memory: base ranking, base scores and every re-ranked stage of a call

DEFAULT_COVID_LESIONS = ["Consolidation", "Lung Opacity", "Infiltration", "Atelectasis", "Pleural effusion"]
DEFAULT_VINDR_LESIONS = DEFAULT_COVID_LESIONS + [
    "Nodule/Mass", "Cardiomegaly", "Edema", "Pneumothorax", "Pleural thickening", "Pulmonary fibrosis", "Enlarged PA", "ILD",
    "Calcification", "Lung cavity", "Lung cyst"]

LESION_ALIAS_GROUPS = {
    "consolidation": ["consolidation"],
    "lung opacity": ["lung opacity", "lung_opacity", "opacity", "opacities"],
    "infiltration": ["infiltration", "infiltrate", "infiltrates"],
    "atelectasis": ["atelectasis", "atelectatic"],
    "pleural effusion": ["pleural effusion", "pleural_effusion", "effusion", "plural effusion"],
    "nodule mass": ["nodule mass", "nodule/mass", "nodule_mass", "mass", "nodule"],
    "cardiomegaly": ["cardiomegaly"],
    "edema": ["edema"],
    "pneumothorax": ["pneumothorax"],
    "pleural thickening": ["pleural thickening", "pleural_thickening"],
    "pulmonary fibrosis": ["pulmonary fibrosis", "pulmonary_fibrosis", "fibrosis"],
    "enlarged pa": ["enlarged pa", "enlarged_pa"],
    "ild": ["ild", "interstitial lung disease"],
    "calcification": ["calcification"],
    "lung cavity": ["lung cavity", "lung_cavity", "cavity"],
    "lung cyst": ["lung cyst", "lung_cyst", "cyst"],
}
LESION_ALIAS_TO_CANON = {alias: canon for canon, aliases in LESION_ALIAS_GROUPS.items() for alias in aliases}

EVAL_FIELDS = ["image_name", "label", "global_vector", "region_labels_json", "region_vectors_json"]


@dataclass
class EvalDataset:
    image_names: list
    labels: np.ndarray           # dtype=object, shape [N]
    global_vectors: np.ndarray   # shape [N, D]
    lesion_vectors: list         # per image: canonical lesion name -> list of unit float32 vectors


# ---- host helpers -----------------------------------------------------------------------------------------------------
def normalize_rows(x, eps=1e-12):
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), eps)


def parse_json_list(raw):
    if raw is None or raw == "":
        return []
    try:
        val = json.loads(raw)
    except Exception:
        return []
    return val if isinstance(val, list) else []


def _normalize_lesion_text(name):
    text = str(name).strip().lower()
    for ch in "_-/":
        text = text.replace(ch, " ")
    return " ".join(text.split())


def canonical_lesion_name(name):
    text = _normalize_lesion_text(name)
    return LESION_ALIAS_TO_CANON.get(text, text)


def build_lesion_vector_map(region_labels_json, region_vectors_json):
    labels = parse_json_list(region_labels_json)
    vectors = parse_json_list(region_vectors_json)
    out = {}
    for name, raw in zip(labels, vectors):                 # zip stops at the shorter list
        if not isinstance(raw, list) or len(raw) == 0:
            continue
        vec = np.asarray(raw, dtype=np.float32)
        norm = np.linalg.norm(vec)
        if norm <= 0:
            continue
        out.setdefault(canonical_lesion_name(name), []).append(vec / norm)
    return out


def _is_positive_label(value):
    return str(value).strip().lower() in {"1", "1.0", "true", "yes", "y"}


def build_vindr_label_lookup(labels_csv_path):
    labels_csv_path = Path(labels_csv_path)
    if not labels_csv_path.exists():
        raise FileNotFoundError(f"Missing ViNDR labels file: {labels_csv_path}")
    lookup = {}
    with labels_csv_path.open("r", encoding="utf-8", newline="") as f:
        reader = csv.DictReader(f)
        if not reader.fieldnames or "image_id" not in reader.fieldnames:
            raise ValueError(f"Invalid ViNDR labels CSV (missing image_id): {labels_csv_path}")
        columns = [c for c in reader.fieldnames if c != "image_id"]
        for row in reader:
            image_id = str(row.get("image_id", "")).strip()
            if not image_id:
                continue
            findings = [c for c in columns if _is_positive_label(row.get(c, "")) and c.lower() != "no finding"]
            lookup[image_id] = " | ".join(findings) if findings else "No finding"
    return lookup


def load_eval_dataset(source, fetch_batch_size=2048, label_overrides=None):
    """`source`: an iterable of row dicts with EVAL_FIELDS, or an object with `num_entities` and
    `query(expr=, output_fields=, limit=, offset=)` (a pymilvus Collection, already connected and loaded), paged like the
    reference pages it."""
    if hasattr(source, "query") and hasattr(source, "num_entities"):
        total = int(source.num_entities)
        if total <= 1:
            raise ValueError(f"Collection '{getattr(source, 'name', type(source).__name__)}' has too few entities: {total}")
        rows = []
        while len(rows) < total:
            chunk = source.query(expr="id >= 0", output_fields=list(EVAL_FIELDS), limit=min(fetch_batch_size, total - len(rows)),
                                 offset=len(rows))
            if not chunk:
                break
            rows.extend(chunk)
    else:
        rows = list(source)
        if len(rows) <= 1:
            raise ValueError(f"Collection 'rows' has too few entities: {len(rows)}")
    names, labels, vectors, lesion_maps = [], [], [], []
    for r in rows:
        g = np.asarray(r["global_vector"], dtype=np.float32)
        if g.ndim != 1 or g.size == 0:
            continue
        name = str(r.get("image_name", ""))
        label = str(r.get("label", "unknown"))
        if label_overrides is not None and Path(name).stem in label_overrides:
            label = label_overrides[Path(name).stem]
        names.append(name)
        labels.append(label)
        vectors.append(g)
        lesion_maps.append(build_lesion_vector_map(str(r.get("region_labels_json", "[]")), str(r.get("region_vectors_json", "[]"))))
    if len(vectors) <= 1:
        raise ValueError("Insufficient valid vectors after parsing from Milvus")
    return EvalDataset(image_names=names, labels=np.asarray(labels, dtype=object),
                       global_vectors=normalize_rows(np.stack(vectors, axis=0)), lesion_vectors=lesion_maps)


def choose_query_lesion_vector(lesion_map, lesion_name):
    cands = lesion_map.get(canonical_lesion_name(lesion_name), [])
    return cands[0] if cands else None


def best_candidate_lesion_score(query_vec, candidate_lesions, lesion_name):
    cands = candidate_lesions.get(canonical_lesion_name(lesion_name), [])
    if not cands:
        return -1.0
    return max(float(np.dot(query_vec, c)) for c in cands)


def choose_query_adaptive_lesion_vector(lesion_map, target_lesions):
    """The target lesion the image has most vectors of (strict >, so target order breaks ties) and its first vector."""
    best_name, best_vec, best_count = None, None, -1
    for name in (canonical_lesion_name(x) for x in target_lesions):
        cands = lesion_map.get(name, [])
        if cands and len(cands) > best_count:
            best_name, best_vec, best_count = name, cands[0], len(cands)
    return best_name, best_vec


def print_stage_report(title, report, kappas, cls_k_values):
    print(f"\n=== {title} ===")
    print(", ".join(f"R@{k}: {report['R@K'][k]:.2f}%" for k in kappas))
    print(f"mAP: {report['mAP']:.2f}%")
    print(", ".join(f"P@{k}: {report['mP@K'][k]:.2f}%" for k in kappas))
    for k in cls_k_values:
        m = report["classification"][k]
        print(f"Top-{k}: Acc {m['accuracy']:.2f}% | P_macro {m['precision_macro']:.2f}% | R_macro {m['recall_macro']:.2f}% | "
              f"F1_macro {m['f1_macro']:.2f}%")


# ---- metric tail ------------------------------------------------------------------------------------------------------
def _label_codes(labels):
    return np.unique(np.asarray(labels, dtype=object).astype(str), return_inverse=True)[1].astype(np.int64)


def _classification_from_top(labels, top, k_values):
    """Majority-vote classification metrics (chestmir_eval.py:199-262) from the first ranks `top` [>= max k, N] of every
    query.  A count tie goes to the label met first, as Counter.most_common does.  Same results as
    metrics.compute_classification_metrics(ranks=), whose per-query Python vote takes 54 ms per stage at N = 3000 against 4 ms
    here (array operations); an evaluation has up to 18 stages (tests/test_chestmir_cpu.py compares the two)."""
    codes = _label_codes(labels)
    n = codes.shape[0]
    out = {}
    for k in k_values:
        lab = codes[np.asarray(top)[:k, :]]                                   # [k, N]
        if lab.shape[0] == 0:
            pred = np.full(n, -1, dtype=np.int64)                             # the reference's None
        else:
            counts = (lab[:, None, :] == lab[None, :, :]).sum(axis=0)         # [k, N]: occurrences of the label at each rank
            pred = lab[np.argmax(counts, axis=0), np.arange(n)]               # first maximum = first-met label
        classes = np.unique(np.concatenate([codes, pred]))
        p, r, f, sup = [], [], [], []
        for c in classes:
            tp = int(np.sum((codes == c) & (pred == c)))
            fp = int(np.sum((codes != c) & (pred == c)))
            fn = int(np.sum((codes == c) & (pred != c)))
            pc = tp / (tp + fp) if tp + fp > 0 else 0.0
            rc = tp / (tp + fn) if tp + fn > 0 else 0.0
            p.append(pc)
            r.append(rc)
            f.append(2.0 * pc * rc / (pc + rc) if pc + rc > 0 else 0.0)
            sup.append(int(np.sum(codes == c)))
        sup = np.asarray(sup, dtype=np.float64)
        w = sup / (float(sup.sum()) if sup.sum() > 0 else 1.0)
        out[k] = {
            "accuracy": float(np.mean(codes == pred)) * 100.0,
            "precision_macro": float(np.mean(p)) * 100.0,
            "recall_macro": float(np.mean(r)) * 100.0,
            "f1_macro": float(np.mean(f)) * 100.0,
            "precision_weighted": float(np.sum(np.asarray(p) * w)) * 100.0,
            "recall_weighted": float(np.sum(np.asarray(r) * w)) * 100.0,
            "f1_weighted": float(np.sum(np.asarray(f) * w)) * 100.0,
        }
    return out


def _report(acc, m_ap, pr, cls, kappas):
    return {"R@K": {k: float(v) for k, v in zip(kappas, acc)}, "mAP": float(m_ap * 100.0),
            "mP@K": {k: float(v * 100.0) for k, v in zip(kappas, pr)}, "classification": cls}


def _report_from_device(ap, cnt, nrel, maxpos, kappas, cls):
    """One stage's report from the per-query results of mirx_rank_metrics (host float64 arrays)."""
    n = ap.shape[0]
    acc = [np.count_nonzero(cnt[:, j] > 0) * 100.0 / max(1, n) for j in range(len(kappas))]
    pr = np.zeros(len(kappas))
    for j, kap in enumerate(kappas):                        # precision@kappa over min(largest positive rank, kappa) ranks
        pr[j] = np.sum(np.where(float(kap) <= maxpos, cnt[:, j], nrel) / np.minimum(maxpos, float(kap))) / n
    return _report(acc, float(np.sum(ap) / n), pr, cls, kappas)


def similarity_to_ranks(sim):
    """[N, N], column i = the ranking of query i."""
    similarity_to_ranks.last_native = False
    return np.argsort(-sim, axis=0)


def evaluate_rankings(ranks, labels, kappas, cls_k_values):
    ranks = np.asarray(ranks)
    labels = np.asarray(labels, dtype=object)
    kappas, cls_k_values = list(kappas), list(cls_k_values)
    n = len(labels)
    maxk = max(cls_k_values) if cls_k_values else 0
    cls = _classification_from_top(labels, ranks[:maxk], cls_k_values)
    codes = _label_codes(labels)
    if _gpu() and 2 <= n <= RERANK_MAX_N and ranks.shape == (n, n) and 1 <= len(kappas) <= 8:
        rows = torch.as_tensor(np.ascontiguousarray(ranks.T.astype(np.int64))).cuda()
        res = _metrics.rank_metrics_device(rows, codes, codes, kappas)
        host = [res[k].cpu().numpy().astype(np.float64) for k in ("ap", "cnt", "nrel", "maxpos")]
        evaluate_rankings.last_native = True
        return _report_from_device(*host, kappas, cls)
    evaluate_rankings.last_native = False
    acc = [np.count_nonzero((codes[ranks[:k, :]] == codes[None, :]).any(axis=0)) * 100.0 / max(1, n) for k in kappas]
    m_ap, _aps, pr, _prs = _metrics.compute_map(ranks, codes, kappas)
    return _report(acc, m_ap, pr, cls, kappas)


# ---- region store and stage plans -------------------------------------------------------------------------------------
class RegionStore:
    """CSR over images of the region vectors: row_ptr [N + 1], per region a lesion id (index into `names`) and a unit float32
    vector, the regions of an image in stored order (per lesion, lesions in the order the image's map holds them).
    `vectors` is None when the vectors do not share one dimension (no device path)."""

    def __init__(self, lesion_maps):
        self.names, self._index = [], {}
        row_ptr, ids, vecs = [0], [], []
        self.first, self.count = [], []                    # per image: lesion id -> first region index / number of regions
        for m in lesion_maps:
            first, count = {}, {}
            for name, cands in m.items():
                if not cands:
                    continue
                lid = self.lesion_id(name, add=True)
                first[lid], count[lid] = len(ids), len(cands)
                ids.extend([lid] * len(cands))
                vecs.extend(cands)
            self.first.append(first)
            self.count.append(count)
            row_ptr.append(len(ids))
        self.row_ptr = np.asarray(row_ptr, dtype=np.int64)
        self.lesion = np.asarray(ids, dtype=np.int32)
        dims = {int(np.asarray(v).size) for v in vecs}
        self.dr = dims.pop() if len(dims) == 1 else (1 if not dims else None)
        self.vectors = None
        if self.dr is not None:
            self.vectors = (np.stack([np.asarray(v, dtype=np.float32).reshape(-1) for v in vecs]) if vecs
                            else np.zeros((0, self.dr), dtype=np.float32))

    def lesion_id(self, name, add=False):
        if name not in self._index:
            if not add:
                return -1
            self._index[name] = len(self.names)
            self.names.append(name)
        return self._index[name]

    def plan_specific(self, lesion_name):
        """-> (q_lesion [N] int32, q_region [N] int64): the query vector is the image's first region of that lesion."""
        lid = self.lesion_id(canonical_lesion_name(lesion_name))
        reg = np.asarray([f.get(lid, -1) for f in self.first], dtype=np.int64)
        return np.full(len(self.first), lid, dtype=np.int32), reg

    def plan_adaptive(self, target_lesions):
        lids = [self.lesion_id(canonical_lesion_name(x)) for x in target_lesions]
        les = np.full(len(self.first), -1, dtype=np.int32)
        reg = np.full(len(self.first), -1, dtype=np.int64)
        for i, (first, count) in enumerate(zip(self.first, self.count)):
            best = -1
            for lid in lids:
                if count.get(lid, 0) > best and lid in first:
                    best, les[i], reg[i] = count[lid], lid, first[lid]
        return les, reg


def _gpu():
    return torch is not None and torch.cuda.is_available()


def _fits(n, stages):
    """The base ranking, base scores (or their transposed upload) and `stages` [N, N] int64 outputs, all resident at once."""
    return (stages + 2) * n * n * 8 <= DEVICE_SHARE * torch.cuda.mem_get_info()[0]


def _native_ok(n, store, rerank_topk, stages=1):
    return (_gpu() and 2 <= n <= RERANK_MAX_N and store.dr is not None and 1 <= store.dr <= RERANK_MAX_DR
            and 1 <= min(int(rerank_topk), n - 1) <= RERANK_MAX_TOPK and _fits(n, stages))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


class _DeviceStore:
    def __init__(self, store, dev):
        self.n_regions, self.dr = int(store.lesion.shape[0]), int(store.dr)
        self.row_ptr = torch.as_tensor(store.row_ptr).to(dev)
        self.lesion = torch.as_tensor(store.lesion).to(dev)
        self.vectors = torch.as_tensor(np.ascontiguousarray(store.vectors)).to(dev)


def lesion_rerank_device(base_ids, dstore, q_lesion, q_region, topk, global_weight, base_sim=None, gvec=None):
    """[HIP] mirx_lesion_rerank.  base_ids [N, N] int64 CUDA (row = query), q_lesion / q_region [S, N] CUDA ->
    (ids [S, N, N] int64, matched [S, N] int32, reranked [S, N] int32) on the device."""
    from . import _lib
    lib = _lib.load()
    n = base_ids.shape[0]
    s = q_lesion.shape[0]
    dev = base_ids.device
    for t, dt, shape in ((base_ids, torch.int64, (n, n)), (q_lesion, torch.int32, (s, n)), (q_region, torch.int64, (s, n)),
                         (base_sim, torch.float64, (n, n)), (gvec, torch.float32, None)):
        if t is None:
            continue
        if not (t.is_cuda and t.device == dev and t.dtype == dt and t.is_contiguous()) or (shape and tuple(t.shape) != shape):
            raise ValueError("lesion_rerank_device: contiguous tensors on one device are needed: base_ids int64 [N, N], q_lesion int32 "
                             "and q_region int64 [S, N], base_sim float64 [N, N], gvec float32 [N, D]")
    if gvec is not None and (gvec.dim() != 2 or gvec.shape[0] != n):
        raise ValueError("lesion_rerank_device: gvec must be [N, D]")
    if (base_sim is None) == (gvec is None):
        raise ValueError("lesion_rerank_device: give either base_sim or gvec")
    out = torch.empty((s, n, n), dtype=torch.int64, device=dev)
    matched = torch.empty((s, n), dtype=torch.int32, device=dev)
    flags = torch.empty((s, n), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.mirx_lesion_rerank(_ptr(base_ids), n, _ptr(base_sim), _ptr(gvec), 0 if gvec is None else gvec.shape[1],
                                          _ptr(dstore.row_ptr), _ptr(dstore.lesion), _ptr(dstore.vectors), dstore.n_regions, dstore.dr,
                                          _ptr(q_lesion), _ptr(q_region), s, int(topk), float(global_weight), _ptr(out), _ptr(matched),
                                          _ptr(flags), st), "mirx_lesion_rerank")
    return out, matched, flags


def _stats(head, n, topk, matched, flags, rerank_topk, global_weight, usage=None):
    reranked = int(np.count_nonzero(flags))
    total = int(matched[flags != 0].sum())
    stats = dict(head)
    stats.update({
        "queries_total": n,
        "queries_reranked": reranked,
        "queries_fallback_global": n - reranked,
        "queries_with_candidate_match": reranked,
        "matched_candidates_in_topk": total,
        "candidate_match_rate_pct": (100.0 * total / (n * topk)) if n * topk > 0 else 0.0,
        "rerank_topk": rerank_topk,
        "global_weight": global_weight,
        "region_weight": 1.0 - global_weight,
    })
    if usage is not None:
        stats["lesion_usage"] = usage
    return stats


def _usage(store, q_lesion, flags):
    c = Counter()
    for lid in q_lesion[flags != 0]:
        c[store.names[int(lid)]] += 1
    return dict(c)


def _rerank_host(base_sim, lesion_maps, choose, rerank_topk, global_weight):
    """The reference's loop: `choose(lesion_map)` -> (canonical lesion name or None, query vector or None)."""
    n = base_sim.shape[0]
    ranks_base = similarity_to_ranks(base_sim)
    ranks_new = np.empty_like(ranks_base)
    topk = min(rerank_topk, n - 1)
    matched = np.zeros(n, dtype=np.int64)
    flags = np.zeros(n, dtype=np.int64)
    chosen = [None] * n
    for i in range(n):
        base_rank = ranks_base[:, i]
        ranks_new[:, i] = base_rank
        name, q_vec = choose(lesion_maps[i])
        if q_vec is None or name is None:
            continue
        top = [int(j) for j in base_rank[:topk]]
        base = [float(base_sim[j, i]) for j in top]
        region = [best_candidate_lesion_score(q_vec, lesion_maps[j], name) for j in top]
        matched[i] = sum(1 for v in region if v >= 0.0)
        if matched[i] == 0:
            continue
        comb = [(global_weight * b) + ((1.0 - global_weight) * v) for b, v in zip(base, region)]
        order = sorted(range(len(top)), key=lambda t: (comb[t], base[t]), reverse=True)      # stable: ties keep base order
        new_top = [top[t] for t in order]
        in_top = np.zeros(n, dtype=bool)
        in_top[new_top] = True
        ranks_new[:, i] = np.asarray(new_top + [idx for idx in base_rank if not in_top[idx]], dtype=np.int64)
        flags[i], chosen[i] = 1, name
    return ranks_new, topk, matched, flags, chosen


def _rerank_public(fn, base_sim, lesion_maps, plan, choose, head, rerank_topk, global_weight, adaptive):
    base_sim = np.asarray(base_sim)
    n = base_sim.shape[0]
    store = RegionStore(lesion_maps)
    if _native_ok(n, store, rerank_topk) and 0.0 <= float(global_weight) <= 1.0:
        dev = torch.device("cuda", torch.cuda.current_device())
        topk = min(int(rerank_topk), n - 1)
        ranks_base = np.argsort(-base_sim, axis=0, kind="stable")             # score desc, ties to the lower id
        q_lesion, q_region = plan(store)
        out, matched, flags = lesion_rerank_device(
            torch.as_tensor(np.ascontiguousarray(ranks_base.T.astype(np.int64))).to(dev), _DeviceStore(store, dev),
            torch.as_tensor(q_lesion[None]).to(dev), torch.as_tensor(q_region[None]).to(dev), topk, global_weight,
            base_sim=torch.as_tensor(np.ascontiguousarray(base_sim.T.astype(np.float64))).to(dev))
        ranks_new = np.ascontiguousarray(out[0].t().cpu().numpy())
        matched, flags = matched[0].cpu().numpy().astype(np.int64), flags[0].cpu().numpy()
        usage = _usage(store, q_lesion, flags) if adaptive else None
        fn.last_native = True
    else:
        ranks_new, topk, matched, flags, chosen = _rerank_host(base_sim, lesion_maps, choose, rerank_topk, global_weight)
        usage = dict(Counter(c for c in chosen if c is not None)) if adaptive else None
        fn.last_native = False
    return ranks_new, _stats(head, n, topk, matched, flags, rerank_topk, global_weight, usage)


def rerank_with_specific_lesion(base_sim, lesion_maps, lesion_name, rerank_topk, global_weight):
    key = canonical_lesion_name(lesion_name)
    return _rerank_public(rerank_with_specific_lesion, base_sim, lesion_maps, lambda st: st.plan_specific(lesion_name),
                          lambda m: (key, choose_query_lesion_vector(m, lesion_name)), {"lesion": lesion_name}, rerank_topk,
                          global_weight, False)


def rerank_with_adaptive_lesion(base_sim, lesion_maps, target_lesions, rerank_topk, global_weight):
    return _rerank_public(rerank_with_adaptive_lesion, base_sim, lesion_maps, lambda st: st.plan_adaptive(target_lesions),
                          lambda m: choose_query_adaptive_lesion_vector(m, target_lesions), {"mode": "adaptive"}, rerank_topk,
                          global_weight, True)


def upload_dataset(gv, store, lesions, dev):
    """The one upload of evaluate_dataset: global vectors, the region store, the stage plans (adaptive first, then one per
    lesion) and a FlatIndex over the global vectors.  -> (g, device store, host plans, q_lesion [S, N], q_region [S, N], index)."""
    from .index import FlatIndex
    g = torch.as_tensor(np.ascontiguousarray(gv, dtype=np.float32)).to(dev)
    plans = [store.plan_adaptive(lesions)] + [store.plan_specific(name) for name in lesions]
    q_lesion = torch.as_tensor(np.stack([p[0] for p in plans])).to(dev)
    q_region = torch.as_tensor(np.stack([p[1] for p in plans])).to(dev)
    ix = FlatIndex(g.shape[1], "COSINE", dev.index)
    ix.add(g)
    return g, _DeviceStore(store, dev), plans, q_lesion, q_region, ix


# ---- the whole evaluation ---------------------------------------------------------------------------------------------
def _summary(lesions, reports, stats, kappas):
    rows = [{"lesion": name, "mAP": rep["mAP"], "R@1": rep["R@K"][kappas[0]], "R@5": rep["R@K"][5] if 5 in rep["R@K"] else np.nan,
             "fallback": st["queries_fallback_global"], "reranked": st["queries_reranked"]}
            for name, rep, st in zip(lesions, reports, stats)]
    if not rows:
        return {"mean_mAP": float("nan"), "mean_R@1": float("nan"), "mean_R@5": float("nan"), "per_lesion": rows}
    r5 = [r["R@5"] for r in rows if not np.isnan(r["R@5"])]
    return {"mean_mAP": float(np.mean([r["mAP"] for r in rows])), "mean_R@1": float(np.mean([r["R@1"] for r in rows])),
            "mean_R@5": float(np.mean(r5)) if r5 else float("nan"), "per_lesion": rows}


def evaluate_dataset(dataset, lesions, kappas=(1, 5, 10), classification_k=(1, 5, 10), rerank_topk=50, global_weight=0.5):
    """Stage 1, the adaptive re-rank and one re-rank per lesion, each with its report, as the reference's main() runs them.
    -> {"stage1": report, "adaptive": (report, stats), "lesions": [(name, report, stats), ...], "summary": {...}}.
    After a device call `evaluate_dataset.last_timings` holds event-to-event milliseconds around the ranking, re-rank and metric
    launches (upper bounds on kernel time: the host work between the launches, allocations included, falls inside them)."""
    if not (0.0 <= global_weight <= 1.0):
        raise ValueError("--global-weight must be in [0, 1]")
    lesions, kappas, cls_k = list(lesions), list(kappas), list(classification_k)
    gv = np.asarray(dataset.global_vectors)
    n = gv.shape[0]
    labels = np.asarray(dataset.labels, dtype=object)
    store = RegionStore(dataset.lesion_vectors)
    if not (_native_ok(n, store, rerank_topk, stages=len(lesions) + 1) and 1 <= len(kappas) <= 8):
        evaluate_dataset.last_native = False
        sim = gv @ gv.T
        np.fill_diagonal(sim, -np.inf)
        stage1 = evaluate_rankings(similarity_to_ranks(sim), labels, kappas, cls_k)
        ranks, a_stats = rerank_with_adaptive_lesion(sim, dataset.lesion_vectors, lesions, rerank_topk, global_weight)
        adaptive = (evaluate_rankings(ranks, labels, kappas, cls_k), a_stats)
        per = []
        for name in lesions:
            ranks, st = rerank_with_specific_lesion(sim, dataset.lesion_vectors, name, rerank_topk, global_weight)
            per.append((name, evaluate_rankings(ranks, labels, kappas, cls_k), st))
        return {"stage1": stage1, "adaptive": adaptive, "lesions": per,
                "summary": _summary(lesions, [p[1] for p in per], [p[2] for p in per], kappas)}

    dev = torch.device("cuda", torch.cuda.current_device())
    topk = min(int(rerank_topk), n - 1)
    maxk = min(max(cls_k) if cls_k else 0, n)
    marks = []

    def mark(label):                                        # time between two marks is booked under the later label
        marks.append((label, torch.cuda.Event(enable_timing=True)))
        marks[-1][1].record()

    g, dstore, plans, q_lesion, q_region, ix = upload_dataset(gv, store, lesions, dev)
    codes = torch.as_tensor(_label_codes(labels)).to(dev)
    s_total = len(plans)
    mark("start")
    base_ids = ix.rank_all(g, exclude_ids=torch.arange(n, device=dev))       # [N, N] row = query, the query itself last
    mark("rank_ms")
    out, matched, flags = lesion_rerank_device(base_ids, dstore, q_lesion, q_region, topk, global_weight, gvec=g)   # every stage
    mark("rerank_ms")
    res = [_metrics.rank_metrics_device(base_ids, codes, codes, kappas),
           _metrics.rank_metrics_device(out.view(s_total * n, n), codes, codes.repeat(s_total), kappas)]
    mark("metric_ms")
    # the only copies to the host: per-query metric results, the first max(k) ranks of every stage, the counters
    host = {k: np.concatenate([r[k].cpu().numpy() for r in res]).astype(np.float64) for k in ("ap", "cnt", "nrel", "maxpos")}
    host = {k: v.reshape((s_total + 1, n) + v.shape[1:]) for k, v in host.items()}
    top = np.concatenate([base_ids[None, :, :maxk].cpu().numpy(), out[:, :, :maxk].cpu().numpy()])   # [S + 1, N, maxk]
    matched = matched.cpu().numpy().astype(np.int64)
    flags = flags.cpu().numpy()
    evaluate_dataset.last_timings = {"rank_ms": 0.0, "rerank_ms": 0.0, "metric_ms": 0.0}
    for (_, e0), (label, e1) in zip(marks, marks[1:]):
        evaluate_dataset.last_timings[label] += e0.elapsed_time(e1)
    reports = [_report_from_device(host["ap"][s], host["cnt"][s], host["nrel"][s], host["maxpos"][s], kappas,
                                   _classification_from_top(labels, top[s].T, cls_k)) for s in range(s_total + 1)]
    q_les_h = plans[0][0]
    a_stats = _stats({"mode": "adaptive"}, n, topk, matched[0], flags[0], rerank_topk, global_weight, _usage(store, q_les_h, flags[0]))
    per = [(name, reports[2 + i], _stats({"lesion": name}, n, topk, matched[1 + i], flags[1 + i], rerank_topk, global_weight))
           for i, name in enumerate(lesions)]
    evaluate_dataset.last_native = True
    return {"stage1": reports[0], "adaptive": (reports[1], a_stats), "lesions": per,
            "summary": _summary(lesions, [p[1] for p in per], [p[2] for p in per], kappas)}


for _fn in (similarity_to_ranks, rerank_with_specific_lesion, rerank_with_adaptive_lesion, evaluate_rankings, evaluate_dataset):
    _fn.last_native = False
evaluate_dataset.last_timings = None
del _fn
