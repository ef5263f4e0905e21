"""Loading tests/golden/chestmir_ref.{npz,json} (made by tests/golden/make_golden_chestmir.py) and the near-tie audit of
DESIGN 22, shared by the ChestMIR CPU and GPU tests."""
import json
import os

import numpy as np

import _chestmir_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAP = 0.0005            # at most 0.05 % of the positions of one stage's rank matrix may be excused
CASE_NAMES = ("a", "b0", "b1", "call", "cone", "d")


def _int_keys(rep):
    return {"R@K": {int(k): v for k, v in rep["R@K"].items()}, "mAP": rep["mAP"], "mP@K": {int(k): v for k, v in rep["mP@K"].items()},
            "classification": {int(k): v for k, v in rep["classification"].items()}}


def load_meta():
    with open(os.path.join(GOLD, "chestmir_ref.json")) as fh:
        return json.load(fh)


def load_case(name):
    z = np.load(os.path.join(GOLD, "chestmir_ref.npz"))
    meta = load_meta()["cases"][name]
    c = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
    cfg = meta["config"]
    base = c["base"].astype(np.int64)
    n = base.shape[0]
    topk = min(cfg["topk"], n - 1)
    ranks = [base]
    for head in c["heads"].astype(np.int64):
        r = base.copy()
        r[:topk] = head
        ranks.append(r)
    return {"raw": {k: c[k] for k in ("gv_raw", "labels", "image_names", "reg_ptr", "reg_label", "reg_vec_raw")},
            "gv": c["gv"], "labels": c["labels"].astype(object), "maps": R.unflatten_maps(c["map_ptr"], c["map_name"], c["map_vec"]),
            "cfg": cfg, "targets": cfg["targets"], "targets_canonical": meta["targets_canonical"], "ref_ranks": ranks,
            "ref_stats": meta["stats"], "ref_reports": [_int_keys(r) for r in meta["reports"]],
            "bound": 2 * max(cfg["d"], cfg["dr"]) * 2.0 ** -24}


def audit(ranks, ref_ranks, s64, keys, bound):
    """-> number of positions where `ranks` differs from the reference's float32 ranking.  Every such position must hold
    two ids whose float64 keys (combined score where the query was re-ranked and both ids are candidates, base score
    otherwise) are within `bound` = 2 * max(D, Dr) * 2^-24 of each other, and at most CAP of the positions may differ."""
    ranks, ref_ranks = np.asarray(ranks), np.asarray(ref_ranks)
    assert ranks.shape == ref_ranks.shape
    assert np.array_equal(np.sort(ranks, axis=0), np.sort(ref_ranks, axis=0))      # column by column the same ids
    pos, qq = np.nonzero(ranks != ref_ranks)
    for p, q in zip(pos, qq):
        a, b = int(ranks[p, q]), int(ref_ranks[p, q])
        ka, kb = s64[a, q], s64[b, q]
        if keys is not None and q in keys:
            ids, comb, _ = keys[q]
            where = {int(j): t for t, j in enumerate(ids)}
            if a in where and b in where:
                ka, kb = comb[where[a]], comb[where[b]]
        assert abs(ka - kb) <= bound, f"query {q} position {p}: ids {a} / {b}, float64 keys {ka!r} / {kb!r} are not a near-tie"
    assert pos.size <= CAP * ranks.size, f"{pos.size} of {ranks.size} positions differ: more than {CAP:.2%}"
    return int(pos.size)
