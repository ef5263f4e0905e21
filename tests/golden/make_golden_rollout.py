#!/usr/bin/env python3
"""Generate the attention-rollout fixture from the reference's OWN explainer class.

Run in the build container only (the reference tree is not present on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rollout.py

What it does
  * imports the reference's explanations.py (AttentionRolloutMedSigLIP, explanations.py:979-1147) from the reference tree.
    Nothing of the reference is copied: only INPUTS and the reference's OUTPUTS are written.
  * for each setup of tests/_rollout_ref.py SETUPS builds the stand-in model there (seeded dyadic attentions with ties
    planted at the k-th value, tokens, a query embedding, a float64 projection) and runs every case of CASES in float64:
        {setup}_atts, {setup}_tokens, {setup}_q_feat, {setup}_proj_*   float64 inputs
        {case}_out                                                     float64 output of the reference's class [B, H, W]
    as tests/golden/rollout_ref.npz.
"""
import importlib
import os
import sys

import numpy as np

REF = os.environ.get("MIRX_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(OUT))          # tests/: _rollout_ref


def main():
    import torch

    import _rollout_ref as R

    sys.path.insert(0, REF)
    ref = importlib.import_module("explanations")
    torch.set_default_dtype(torch.float64)
    out = {}
    inputs = {s: R.setup_inputs(s) for s in R.SETUPS}
    for s, inp in inputs.items():
        out.update({f"{s}_{k}": v for k, v in inp.items()})
    for case in R.CASES:
        inp = inputs[case["setup"]]
        explainer = ref.AttentionRolloutMedSigLIP(R.StandIn(inp), head_fusion=case["fusion"], discard_ratio=case["ratio"],
                                                  query_guided=case["qg"])
        res = explainer(R.pixels(1), R.pixels(R.BATCH)).double().numpy()
        out[f"{case['name']}_out"] = res
        # the reference builds its identity in float32: its rollout is float32 arithmetic, the restatement float64
        err = float(np.abs(R.case_expected(case, inp) - res).max() / np.abs(res).max())
        print(f"{case['name']:22s} out {res.shape}  restatement rel. max|diff| {err:.2e}")
    path = os.path.join(OUT, "rollout_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
