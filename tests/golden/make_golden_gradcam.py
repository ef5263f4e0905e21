#!/usr/bin/env python3
"""Generate the Grad-CAM fixture from the reference's OWN functions.

Run in the build container only (the reference tree is not present on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gradcam.py

What it does
  * imports the reference's medsiglip_saliency.py (compute_gradcam_saliency, _compute_single_gradcam, lines 137-269) with
    cv2, torchvision, model, milvus_setup, path_mapper and tqdm stubbed in sys.modules (its MedSigLIP import is served by
    mirx.model.MedSigLIP).  Nothing of the reference is copied: only INPUTS and the reference's OUTPUTS are written.
  * runs every case of tests/_gradcam_ref.py CASES in float64 on the CPU on the seeded tiny MedSigLIP there:
        w/<name>                 the float32 weights (the model is their float64 image)
        {case}_query, {case}_retrieved (float32 values), {case}_qemb (float64: model(query))
        {case}_out               float64 output [K, H, W] of compute_gradcam_saliency (bq2: _compute_single_gradcam)
    as tests/golden/gradcam_ref.npz.
"""
import importlib
import os
import sys
import types

import numpy as np

REF = os.environ.get("MIRX_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(OUT))          # tests/: _gradcam_ref
sys.path.insert(0, ROOT)                          # mirx


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    return m


def main():
    import torch

    import _gradcam_ref as R
    from mirx.model import MedSigLIP

    for name in ("cv2", "torchvision", "torchvision.transforms", "tqdm"):
        _stub(name, transforms=types.SimpleNamespace(), tqdm=lambda it, *a, **k: it)
    _stub("model", MedSigLIP=MedSigLIP)
    _stub("milvus_setup", MilvusManager=object, MODEL_CONFIGS={})
    _stub("path_mapper", PathMapper=object)
    sys.path.insert(0, REF)
    ref = importlib.import_module("medsiglip_saliency")

    dev = torch.device("cpu")
    base = R.build_model()
    out = {f"w/{k}": v for k, v in R.weights_of(base).items()}
    for case in R.CASES:
        q, r, flat = R.case_inputs(case)
        model = R.build_model({k[2:]: v for k, v in out.items() if k.startswith("w/")})
        if flat:
            with torch.no_grad():
                model.projection[3].weight.zero_()
        with torch.no_grad():
            qemb = model(q)
        if case == "bq2":
            res = np.stack([ref._compute_single_gradcam(model, qemb, r[i:i + 1], dev) for i in range(r.shape[0])])
        else:
            res = ref.compute_gradcam_saliency(model, q, r, dev)
        res = np.asarray(res, np.float64)
        out.update({f"{case}_query": q.float().numpy(), f"{case}_retrieved": r.float().numpy(), f"{case}_qemb": qemb.numpy(),
                    f"{case}_out": res})
        W = {k: v.double().numpy() for k, v in model.state_dict().items()}
        exp = R.expected(W, R.last_tokens(model, r), qemb.numpy(), R.VISION["num_attention_heads"], R.SIZE)
        print(f"{case:6s} out {res.shape} range [{np.nanmin(res):.3f}, {np.nanmax(res):.3f}]  restatement max|diff| "
              f"{float(np.abs(exp - res).max()):.2e}")
    path = os.path.join(OUT, "gradcam_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
