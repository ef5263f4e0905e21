#!/usr/bin/env python3
"""Generate tests/golden/anomaly_ref.json from the reference's OWN anomaly/anomaly.py and the installed scikit-learn.

Run where the reference tree is present (MIRX_REFERENCE, default: `reference` beside the repository) and scikit-learn is
installed (both are needed at generation time only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_anomaly.py

"printed" holds what the reference's show_performance, print_measures, print_measures_with_std and show_performance_comparison
write to stdout for fixed arguments.  Per case the inputs (pos, neg) and the reference's get_measures(pos, neg) are written; for two cases also scikit-learn's
roc_curve and precision_recall_curve on (labels, examples) stacked positives first, as test_anomaly.py:51-61 does.  Nothing of
the reference is copied: only INPUTS and OUTPUTS.  "line64_defect" records what test_anomaly.py:64 computes after line 56 has
rebound `labels` to the 0/1 vector -- get_measures(dists[labels == 2], dists[labels != 2]) with no positive left -- as a record
of the defect, not as something to match.
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import warnings

import numpy as np
import sklearn
from sklearn.metrics import precision_recall_curve, roc_curve

OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MIRX_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(OUT))), "reference"))
sys.dont_write_bytecode = True
spec = importlib.util.spec_from_file_location("anomaly_ref", os.path.join(REF, "anomaly", "anomaly.py"))
A = importlib.util.module_from_spec(spec)
spec.loader.exec_module(A)

rng = np.random.default_rng(20260115)
cases = {}


def add(name, pos, neg, curves=False):
    pos, neg = np.asarray(pos, dtype=np.float64), np.asarray(neg, dtype=np.float64)
    auroc, aupr, fpr = A.get_measures(pos, neg)
    c = {"pos": pos.tolist(), "neg": neg.tolist(), "auroc": float(auroc), "aupr": float(aupr), "fpr": float(fpr)}
    if curves:
        examples = np.concatenate((pos, neg))
        labels = np.zeros(examples.size, dtype=np.int32)
        labels[:pos.size] = 1
        f, t, th = roc_curve(labels, examples)
        p, r, th2 = precision_recall_curve(labels, examples)
        c["roc"] = {"fpr": f.tolist(), "tpr": t.tolist(), "thresholds": [float(v) for v in th[1:]]}     # th[0] = inf
        c["pr"] = {"precision": p.tolist(), "recall": r.tolist(), "thresholds": th2.tolist()}
    cases[name] = c


# 300 scores, labels arange(300) % 3, label 2 the anomaly
s300 = rng.random(300)
l300 = np.arange(300) % 3
add("s300", s300[l300 == 2], s300[l300 != 2], curves=True)
# the recall-level tie
for P in (1, 10, 19, 20, 21):
    add(f"tie_p{P}", np.linspace(0.5, 1, P), np.linspace(0, 0.9, 50))
# eight-valued scores, 60 positives and 140 negatives (this seed: AUROC 4071 / 8400 = 0.484642857...)
u = np.random.default_rng(919).random(200)
q = np.round(7 * u) / 7
add("quant8", q[:60], q[60:], curves=True)
add("all_equal", np.full(7, 0.25), np.full(11, 0.25))
add("one_positive", [0.7], rng.random(40))
add("one_negative", rng.random(40), [0.3])
add("n2", [0.9], [0.1])
add("n2_reversed", [0.1], [0.9])

# what the reference's four printers write (stdout captured), for fixed inputs
def printed(fn, *args, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        fn(*args, **kw)
    return buf.getvalue()


pq, nq = cases["quant8"]["pos"], cases["quant8"]["neg"]
pt, nt = cases["tie_p10"]["pos"], cases["tie_p10"]["neg"]
prints = {
    "show_performance": {"args": "quant8", "out": printed(A.show_performance, np.array(pq), np.array(nq))},
    "show_performance_named": {"args": "quant8, method_name='Centroid', recall_level=0.9",
                               "out": printed(A.show_performance, np.array(pq), np.array(nq), method_name="Centroid", recall_level=0.9)},
    "print_measures": {"args": [0.81234, 0.5, 0.04567], "out": printed(A.print_measures, 0.81234, 0.5, 0.04567)},
    "print_measures_named": {"args": [1.0, 0.0, 0.33333, "DenseNet121", 0.8],
                             "out": printed(A.print_measures, 1.0, 0.0, 0.33333, "DenseNet121", 0.8)},
    "print_measures_with_std": {"args": [[0.8, 0.9, 0.85], [0.5, 0.6, 0.7], [0.1, 0.2, 0.15]],
                                "out": printed(A.print_measures_with_std, [0.8, 0.9, 0.85], [0.5, 0.6, 0.7], [0.1, 0.2, 0.15])},
    "show_performance_comparison": {"args": "tie_p10 as the baseline, quant8 as ours",
                                    "out": printed(A.show_performance_comparison, np.array(pt), np.array(nt), np.array(pq),
                                                   np.array(nq))},
}

# the defect of test_anomaly.py:64
dists = s300 / s300.max()
labels01 = np.zeros(300, dtype=np.int32)
labels01[:100] += 1
with warnings.catch_warnings(record=True) as w:
    warnings.simplefilter("always")
    d_auroc, d_aupr, d_fpr = A.get_measures(dists[labels01 == 2], dists[labels01 != 2])
meta = {"sklearn": sklearn.__version__, "numpy": np.__version__, "recall_level": A.recall_level_default, "cases": cases, "printed": prints,
        "line64_defect": {"auroc": None if np.isnan(d_auroc) else float(d_auroc), "aupr": float(d_aupr), "fpr": float(d_fpr),
                          "n": 300, "warnings": len(w)}}
with open(os.path.join(OUT, "anomaly_ref.json"), "w") as fh:
    json.dump(meta, fh, indent=1)
print({k: (v["auroc"], v["aupr"], v["fpr"]) for k, v in cases.items()})
print(meta["line64_defect"], os.path.getsize(os.path.join(OUT, "anomaly_ref.json")))
