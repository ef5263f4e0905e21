#!/usr/bin/env python3
"""Golden vectors for leave-group-out evaluation from the reference's OWN compute_ap / compute_map.

Run where the reference tree is present (MIRX_REFERENCE, as for make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grouped.py

One seeded set: N = 300 images, labels = arange(N) % 3, groups of sizes 1 .. 8, integer embeddings (so that the fixture is
small and every distance is exact).  Per query the full self-ranking loses the entries of the query's own group -- the query
with them -- and the compacted list goes through the reference: AP = compute_ap(positions of the positives left, their number)
(test.py:58-92), precision@kappa = the prs of compute_map (test.py:137-142) on that one list.  Nothing of the reference is
copied: only the inputs and its outputs are written, to tests/golden/grouped_300.json.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

N, DIM, SEED, KAPPAS = 300, 8, 39, [1, 5, 10]


def main():
    from make_golden import import_reference
    import _rank_metrics_ref as R
    ref_test = import_reference()[0]
    rng = np.random.default_rng(SEED)
    labels = np.arange(N) % 3
    centers = rng.integers(-40, 41, (3, DIM))
    emb = (centers[labels] + rng.integers(-60, 61, (N, DIM))).astype(np.int64)     # class structure, far from separable
    codes = R.group_sizes_1_to_8(N, SEED)
    ranks = R.self_ranking(emb, "l2")
    aps, prs = [], []
    for q in range(N):
        kept = ranks[q][codes[ranks[q]] != codes[q]]
        hit = labels[kept] == labels[q]
        pos = np.flatnonzero(hit)
        assert pos.size > 0
        aps.append(float(ref_test.compute_ap(pos, len(pos))))
        # compute_map on the one list: ids 0 = a positive, 1 = not; gnd = [0] makes id 0 the positive set
        col = np.where(hit, 0, 1)[:, None]
        prs.append([float(v) for v in ref_test.compute_map(col, np.array([0]), KAPPAS)[3][0]])
    with open(os.path.join(HERE, "grouped_300.json"), "w") as fh:
        json.dump({"n": N, "dim": DIM, "seed": SEED, "kappas": KAPPAS, "embeds": emb.tolist(), "labels": labels.tolist(),
                   "groups": codes.tolist(), "aps": aps, "prs": prs}, fh)
    print("wrote grouped_300.json: mAP", float(np.mean(aps)))


if __name__ == "__main__":
    main()
