#!/usr/bin/env python3
"""Generate the SimAtt fixture from the reference's OWN explainer class.

Run in the build container only (the reference tree is not present on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_simatt.py

What it does
  * imports the reference's explanations.py (SimAtt, explanations.py:605-661) and, through it, gradcam.py (ModelOutputs) from the
    reference tree.  Nothing of the reference is copied: only INPUTS and the reference's OUTPUTS are written.
  * runs each case of tests/_simatt_ref.py CASES in float64 on compute_saliency.py's recipe, SimAtt(seq, seq[0], ["relu"]) with
    seq = Sequential(features, avgpool[, fc]), on the tiny model there (a 5 x 7 map of 6 channels, fc to 5), and stores
        {name}_xq, {name}_xp, {name}_xn   float64 inputs (absent when the case has none)
        {name}_fc_w, {name}_fc_b          float64 fc, cases with fc only
        {name}_out                        float64 output of the reference's class, [B, 10, 14]
    Cases with an fc re-draw their seed until no embedding component lies within 1e-3 (relative) of zero, where float32 could
    flip its sign (a discontinuity of the method).
  * runs the driver forms that fail in the reference (_simatt_ref.FAILING) and stores the exception's type name as
    fail_{name}.
  * asserts that the float64 restatement agrees with every output (about 1e-12 relative; printed).
  -> tests/golden/simatt_ref.npz.  ModelOutputs' per-call print goes to /dev/null.
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
sys.path.insert(0, os.path.dirname(OUT))          # tests/: _simatt_ref, _simcam_ref


def main():
    import torch

    import _simatt_ref as R

    sys.path.insert(0, REF)
    ref = importlib.import_module("explanations")
    torch.set_default_dtype(torch.float64)
    out = {}
    worst = 0.0
    for ci, case in enumerate(R.CASES):
        name = case["name"]
        for attempt in range(64):
            g = torch.Generator().manual_seed(2031 + 101 * ci + 10007 * attempt)
            xq, xp, xn = R.case_inputs(case, g)
            fw = fb = None
            if case["fc"]:
                fw = torch.randn(R.FC_DIM, R.CHANNELS, generator=g, dtype=torch.float64).numpy()
                fb = torch.randn(R.FC_DIM, generator=g, dtype=torch.float64).numpy()
                if not R.sign_margin_ok(R.case_rows(xq, xp, xn)[0], fw, fb):
                    continue
            break
        else:
            raise AssertionError(f"{name}: no seed satisfies the sign margin")
        model = R.flat_model(R.make_fc(fw, fb) if case["fc"] else None).double().eval()
        explainer = ref.SimAtt(model, model[0], target_layers=["relu"])
        with contextlib.redirect_stdout(io.StringIO()):          # (the tiny model has no parameter: the query carries the graph)
            res = explainer(xq.clone().requires_grad_(True), xp, xn).detach().double().numpy()
        for key, val in (("xq", xq), ("xp", xp), ("xn", xn)):
            if val is not None:
                out[f"{name}_{key}"] = val.numpy()
        if case["fc"]:
            out[f"{name}_fc_w"], out[f"{name}_fc_b"] = fw, fb
        out[f"{name}_out"] = res
        exp = R.case_expected(xq, xp, xn, fw, fb)
        err = max(R.map_errors(exp, res))
        worst = max(worst, err)
        assert err <= 1e-11, (name, err)
        print(f"{name:22s} out {res.shape}  seed attempt {attempt}  max|map|={np.abs(res).max():.3e}  restatement rel err {err:.2e}")
    for name in R.FAILING:
        fc = R.make_fc(np.zeros((R.FC_DIM, R.CHANNELS)), np.zeros(R.FC_DIM)) if name.endswith("_fc") else None
        model, module, targets = R.failing_form(name, fc)
        model = model.double().eval()
        g = torch.Generator().manual_seed(77)
        xq = torch.randn(1, R.CHANNELS, *R.SIZE, generator=g, dtype=torch.float64)
        xp = torch.randn(1, R.CHANNELS, *R.SIZE, generator=g, dtype=torch.float64)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                ref.SimAtt(model, module, target_layers=targets)(xq.clone().requires_grad_(True), xp)
            raised = "none"
        except Exception as e:                              # noqa: BLE001 (the type is the datum)
            raised = type(e).__name__
        out[f"fail_{name}"] = np.array(raised)
        print(f"fail_{name:18s} {raised}")
    path = os.path.join(OUT, "simatt_ref.npz")
    np.savez_compressed(path, **out)
    print(f"worst restatement rel err {worst:.2e}; wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
