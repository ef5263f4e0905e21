#!/usr/bin/env python3
"""Generate the ChestMIR fixture from the reference's OWN functions.

Run where the reference tree is present (MIRX_REFERENCE, default: `reference` beside the repository):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_chestmir.py

What it does
  * imports the reference's ChestMIR/chestmir_eval.py with `pymilvus` stubbed in sys.modules: `connections.connect` does
    nothing and `Collection(name)` serves the seeded rows of tests/_chestmir_ref.py synthetic_raw through `num_entities`
    and `query(expr=, output_fields=, limit=, offset=)`, so the reference's own load_eval_dataset parses them.  Nothing of the
    reference is copied: only INPUTS and the reference's OUTPUTS are written.
  * per case (CASES below) runs the reference's main() sequence: gv @ gv.T with a -inf diagonal, similarity_to_ranks,
    rerank_with_adaptive_lesion, rerank_with_specific_lesion per target, evaluate_rankings of every stage, and writes
        {case}/gv_raw labels image_names reg_ptr reg_label reg_vec_raw   the raw rows (inputs)
        {case}/gv                          the reference's normalised global vectors (float32)
        {case}/map_ptr map_name map_vec    the reference's lesion maps, flattened in map order
        {case}/base                        stage-1 ranks [N, N] uint16, column i = query i
        {case}/heads                       [S, topk, N] uint16: the first topk rows of the adaptive + per-target rankings
                                           (the generator asserts that every stage's remaining rows equal `base`'s)
    into tests/golden/chestmir_ref.npz, and the configuration, canonical target names, stats dicts and reports of every
    stage, plus the JSON-string cases of build_lesion_vector_map / parse_json_list / canonical_lesion_name, into
    tests/golden/chestmir_ref.json.

Observed with the committed seeds (also written to chestmir_ref.json under "observed"): positions where the reference's
float32 ranking differs from the float64 restatement of tests/_chestmir_ref.py, and the smallest float64 base gap:
    a     2 of 90 000 positions in every one of the 10 stages (0.002 %, one base near-tie); gap 6.5e-9, bound 7.6e-6
    b0 b1 0 of 8 100;  gap 2.5e-6, bound 3.8e-6        call cone 0 of 3 600; gap 2.9e-6        d 0 of 14 400; gap 2.9e-7
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
# the reference tree: MIRX_REFERENCE, or a directory `reference` beside the repository
REF = os.environ.get("MIRX_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(OUT))), "reference"))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(OUT))          # tests/: _chestmir_ref

import _chestmir_ref as R  # noqa: E402

ROWS = {}


class _Collection:
    def __init__(self, name):
        self.name, self.rows = name, ROWS[name]
        self.num_entities = len(self.rows)

    def load(self):
        pass

    def query(self, expr, output_fields, limit, offset):
        return [{k: r[k] for k in ["id"] + list(output_fields)} for r in self.rows[offset:offset + limit]]


pm = types.ModuleType("pymilvus")
pm.Collection = _Collection
pm.connections = types.SimpleNamespace(connect=lambda **kw: None, disconnect=lambda *a, **kw: None)
sys.modules["pymilvus"] = pm
spec = importlib.util.spec_from_file_location("chestmir_eval_ref", os.path.join(REF, "ChestMIR", "chestmir_eval.py"))
C = importlib.util.module_from_spec(spec)
sys.modules[spec.name] = C                         # dataclasses look the module up
spec.loader.exec_module(C)

# alias spellings -> the lesion they belong to (8 lesions)
SPELL = [("Consolidation", "consolidation"), ("consolidation", "consolidation"), ("Lung Opacity", "lung opacity"),
         ("lung_opacity", "lung opacity"), ("opacities", "lung opacity"), ("Infiltrate", "infiltration"),
         ("infiltration", "infiltration"), ("Atelectasis", "atelectasis"), ("atelectatic", "atelectasis"),
         ("Pleural-Effusion", "pleural effusion"), ("plural effusion", "pleural effusion"), ("Nodule/Mass", "nodule mass"),
         ("mass", "nodule mass"), ("Cardiomegaly", "cardiomegaly"), ("EDEMA", "edema")]
T8 = ["Consolidation", "Lung Opacity", "Infiltration", "Atelectasis", "Pleural effusion", "Nodule/Mass", "Cardiomegaly", "Edema"]
KW = dict(kappas=[1, 5, 10], cls_k=[1, 5, 10])
CASES = {
    # (a) the COVID-like shape: adaptive + every lesion
    "a": dict(seed=7, n=300, d=64, dr=32, classes=4, max_regions=4, topk=50, weight=0.5, targets=T8, **KW),
    # (b) the two ends of the weight
    "b0": dict(seed=11, n=90, d=32, dr=16, classes=3, max_regions=3, topk=20, weight=0.0, targets=T8[:3], **KW),
    "b1": dict(seed=11, n=90, d=32, dr=16, classes=3, max_regions=3, topk=20, weight=1.0, targets=T8[:3], **KW),
    # (c) topk >= N - 1 and topk = 1
    "call": dict(seed=13, n=60, d=32, dr=16, classes=3, max_regions=3, topk=500, weight=0.5, targets=T8[:3], **KW),
    "cone": dict(seed=13, n=60, d=32, dr=16, classes=3, max_regions=3, topk=1, weight=0.5, targets=T8[:3], **KW),
    # (d) a lesion no image has ("Lung cyst": every query falls back); "edema" regions with a random sign (candidates whose
    # only match is a negative dot: used in the score, not counted); several regions of one lesion per image (max); the
    # adaptive targets list two lesions many images hold equally often (target order decides)
    "d": dict(seed=17, n=120, d=32, dr=16, classes=3, max_regions=4, topk=30, weight=0.4, signed=("edema",),
              spell=[s for s in SPELL if s[1] in ("edema", "consolidation", "lung opacity")],
              targets=["Edema", "opacity", "Consolidation", "Lung cyst"], **KW),
}

arrays, meta = {}, {"cases": {}, "observed": {}}
for name, cfg in CASES.items():
    raw = R.synthetic_raw(cfg["seed"], cfg["n"], cfg["d"], cfg["dr"], cfg["classes"], cfg.get("spell", SPELL), cfg["max_regions"],
                          signed=cfg.get("signed", ()))
    ROWS[name] = R.rows_from_raw(raw)
    ds = C.load_eval_dataset("host", 0, name, fetch_batch_size=64)
    n, topk = len(ds.labels), min(cfg["topk"], len(ds.labels) - 1)
    sim = ds.global_vectors @ ds.global_vectors.T
    np.fill_diagonal(sim, -np.inf)
    base = C.similarity_to_ranks(sim)
    stages = [("stage1", base, None)]
    r, st = C.rerank_with_adaptive_lesion(sim, ds.lesion_vectors, cfg["targets"], cfg["topk"], cfg["weight"])
    stages.append(("adaptive", r, st))
    for t in cfg["targets"]:
        r, st = C.rerank_with_specific_lesion(sim, ds.lesion_vectors, t, cfg["topk"], cfg["weight"])
        stages.append((t, r, st))
    for _, r, _ in stages[1:]:
        assert np.array_equal(r[topk:], base[topk:])
    reports = [C.evaluate_rankings(r, ds.labels, cfg["kappas"], cfg["cls_k"]) for _, r, _ in stages]
    for k, v in raw.items():
        arrays[f"{name}/{k}"] = v
    ptr, mnames, mvecs = R.flatten_maps(ds.lesion_vectors)
    arrays.update({f"{name}/gv": ds.global_vectors, f"{name}/map_ptr": ptr, f"{name}/map_name": mnames, f"{name}/map_vec": mvecs,
                   f"{name}/base": base.astype(np.uint16),
                   f"{name}/heads": np.stack([r[:topk] for _, r, _ in stages[1:]]).astype(np.uint16)})
    assert ds.global_vectors.dtype == np.float32 and n < 65536
    meta["cases"][name] = {
        "config": {k: v for k, v in cfg.items() if k not in ("spell", "signed")},
        "targets_canonical": [C.canonical_lesion_name(t) for t in cfg["targets"]],
        "stats": [st for _, _, st in stages[1:]],
        "reports": [{"R@K": {str(k): v for k, v in rep["R@K"].items()}, "mAP": rep["mAP"],
                     "mP@K": {str(k): v for k, v in rep["mP@K"].items()},
                     "classification": {str(k): v for k, v in rep["classification"].items()}} for rep in reports],
    }
    # how far the reference's float32 path is from the float64 restatement (recorded, and checked by tests/test_chestmir_cpu.py)
    ref = R.evaluate(ds.global_vectors, ds.labels, ds.lesion_vectors, meta["cases"][name]["targets_canonical"], cfg["kappas"],
                     cfg["cls_k"], cfg["topk"], cfg["weight"])
    diffs = [int(np.count_nonzero(a != b)) for a, (_, b, _) in zip(ref["ranks"], stages)]
    gap = R.min_base_gap(R.base_scores(ds.global_vectors))
    flags = np.asarray(ref["reranked"])
    meta["observed"][name] = {"positions": n * n, "differing_positions_per_stage": diffs, "smallest_fp64_base_gap": gap,
                              "bound": 2 * max(cfg["d"], cfg["dr"]) * 2.0 ** -24,
                              "reranked_per_stage": [int(f.sum()) for f in flags]}
    print(name, meta["observed"][name])

# (e) the JSON-string path
E = [
    ('["Opacity", "EDEMA", "mass", "cyst", "Infiltrates"]', '[[3.0, 4.0], [], [0.0, 0.0], "oops", [1.0, 2.0, 2.0], [9.0]]'),
    ('["consolidation", "Consolidation", "lung_opacity"]', '[[1.0, 0.0], [0.0, 2.0]]'),
    ('not json', '[[1.0]]'), ('{"a": 1}', '[[1.0]]'), ("", ""), ('["Plural  Effusion", "x-ray_thing/other"]', '[[0.5, 0.5], [2, 0]]'),
]
meta["json_cases"] = [{"labels": a, "vectors": b,
                       "map": {k: [[float(x) for x in v] for v in vs] for k, vs in C.build_lesion_vector_map(a, b).items()}}
                      for a, b in E]
NAMES = ["Lung_Opacity", " plural  effusion ", "Nodule/Mass", "nodule-mass", "Interstitial lung disease", "Something Else", "CYST", 7]
meta["canonical"] = [[n if isinstance(n, str) else n, C.canonical_lesion_name(n)] for n in NAMES]
meta["default_covid"] = list(C.DEFAULT_COVID_LESIONS)
meta["default_vindr"] = list(C.DEFAULT_VINDR_LESIONS)
np.savez_compressed(os.path.join(OUT, "chestmir_ref.npz"), **arrays)
with open(os.path.join(OUT, "chestmir_ref.json"), "w") as fh:
    json.dump(meta, fh, indent=1)
for f in ("chestmir_ref.npz", "chestmir_ref.json"):
    print(f, os.path.getsize(os.path.join(OUT, f)))
