#!/usr/bin/env python3
"""Generate the SimCAM fixture from the reference's OWN explainer classes.

Run in the build container only (the reference tree is not present on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_simcam.py

What it does
  * imports the reference's explanations.py (SimCAM_Densenet121, SimCAM, SimCAM_MedSigLIP; explanations.py:664-976) and, through
    it, gradcam.py (ModelOutputs) from the reference tree.  Nothing of the reference is copied: only INPUTS and the reference's
    OUTPUTS are written.
  * runs each case of tests/_simcam_ref.py CASES in float64 (default dtype float64 too: SimCAM_Densenet121 fills a
    default-dtype tensor) on the tiny models there, whose target layer sees 2 x 2 or 3 x 3 block means of the input, and stores
        {name}_xq, {name}_x        float64 inputs [nq, 6, H, W], [nr, 6, H, W]
        {name}_fc_w, {name}_fc_b   float64 fc (embedding dim 5), cases with fc only
        {name}_out                 float64 output of the reference's class
    as tests/golden/simcam_ref.npz.  ModelOutputs' per-call print goes to /dev/null.
"""
import contextlib
import importlib
import io
import os
import sys

import numpy as np

REF = os.environ.get("MIRX_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(OUT))          # tests/: _simcam_ref


def main():
    import torch
    import torch.nn as nn

    import _simcam_ref as R

    sys.path.insert(0, REF)
    ref = importlib.import_module("explanations")
    torch.set_default_dtype(torch.float64)
    g = torch.Generator().manual_seed(2027)
    out = {}
    for case in R.CASES:
        name = case["name"]
        xq, x = R.case_inputs(case, g)
        fc = None
        if case.get("fc"):
            fc = nn.Linear(case["c"], case["fc"]).double()
            with torch.no_grad():
                fc.weight.copy_(torch.randn(case["fc"], case["c"], generator=g, dtype=torch.float64))
                fc.bias.copy_(torch.randn(case["fc"], generator=g, dtype=torch.float64))
            out[f"{name}_fc_w"], out[f"{name}_fc_b"] = fc.weight.detach().numpy(), fc.bias.detach().numpy()
        explainer = R.case_model(case, ref, fc)
        with contextlib.redirect_stdout(io.StringIO()):
            if case["cls"] == "SimCAM_MedSigLIP":
                res = explainer(xq, x)
            else:
                res = explainer(xq, x, point=case.get("point"))
        out[f"{name}_xq"], out[f"{name}_x"], out[f"{name}_out"] = xq.numpy(), x.numpy(), res.double().numpy()
        exp = R.case_expected(case, xq.numpy(), x.numpy(), out.get(f"{name}_fc_w"), out.get(f"{name}_fc_b"))
        err = np.nanmax(np.abs(exp - out[f"{name}_out"])) if not np.isnan(exp).all() else 0.0
        assert np.array_equal(np.isnan(exp), np.isnan(out[f"{name}_out"])), name
        print(f"{name:12s} out {tuple(res.shape)}  restatement max|diff| {err:.2e}")
    path = os.path.join(OUT, "simcam_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
