#!/usr/bin/env python3
"""Generate the ATH fixture from the reference's OWN ath_model.py, test_ath.py and train_ath.py.

Run in the build container only (the reference tree is not present on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ath.py

What it does
  * imports the reference's ath_model.py (torch only), test_ath.py and train_ath.py.  The two scripts import torchvision and
    read_data at module import time although the functions used here need neither, so inert placeholder modules are registered
    for those names first (the make_golden.py recipe).  Nothing of the reference is copied: only INPUTS and the reference's OUTPUTS
    are written, to tests/golden/ath_ref.npz.
  * ATHNet in float64 with seeded weights and non-trivial BatchNorm statistics, three models:
        m0: (hash 36, classes 3, S 64), B = 3     m1: (48, 5, 96), B = 3     m2: (36, 3, 256), B = 1
    Stored compactly (tests/_ath_ref.py decodes both): every floating state-dict entry is rounded to a multiple of 2^-12 and
    kept as int16 (the value times 4096); the images have 16 levels v / 15 (float32), two pixels per byte (low nibble first).
    keys  {m}__sd__<state-dict key>, {m}_x4 [B, 3, S, S / 2] uint8, {m}_codes / {m}_logits float64 (the reference's forward),
          {m}_cfg = [hash, classes, S].
    extract_codes_logits_labels(m0, binary) over a loader of m0_x with labels m0_labels -> ext_codes / ext_logits / ext_labels.
  * compute_metrics and compute_retrieval_metrics, topk (1, 5, 10), as JSON strings met_{case}_cm / met_{case}_rm with inputs
    {case}_q, {case}_g, {case}_ql, {case}_gl, {case}_logits:
        l2     real-valued codes (no distance ties), reference unmodified;
        bin    random 0/1 codes, 36 bits, torch.argsort made stable inside the two imported scripts (the lowest-id rule);
        tie    0/1 codes drawn from 6 prototypes of 8 bits: nearly every distance is tied (stable argsort as well).
"""
import importlib
import json
import os
import sys
import types

import numpy as np

REF = os.environ.get("MIRX_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
TOPK = (1, 5, 10)
SD_SCALE = 4096.0


def import_reference():
    import torch  # noqa: F401

    class _Anything:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            return self

        def __getattr__(self, k):
            return _Anything()

    for name in ("torchvision", "torchvision.transforms", "read_data"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []

            def _ga(k, _A=_Anything):
                if k.startswith("__"):
                    raise AttributeError(k)
                return _A()
            m.__getattr__ = _ga  # type: ignore[attr-defined]
            sys.modules[name] = m
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.path.insert(0, REF)
    return (importlib.import_module("ath_model"), importlib.import_module("test_ath"), importlib.import_module("train_ath"))


class _StableTorch:
    """torch, except that argsort is stable: ties go to the lowest index."""

    def __init__(self, torch):
        self._t = torch

    def __getattr__(self, k):
        return getattr(self._t, k)

    def argsort(self, x, dim=-1, descending=False):
        return self._t.argsort(x, dim=dim, descending=descending, stable=True)


def main():
    import torch

    am, ta, tr = import_reference()
    g = torch.Generator().manual_seed(2027)
    out = {}

    def randomize(model):
        sd = model.state_dict()
        for k, v in sd.items():
            if not v.is_floating_point():
                continue
            if k.endswith("running_mean"):
                v.copy_(0.2 * torch.randn(v.shape, generator=g))
            elif k.endswith("running_var"):
                v.copy_(0.5 + 1.5 * torch.rand(v.shape, generator=g))
            elif k.endswith(".weight") and v.dim() == 1:          # BatchNorm gamma
                v.copy_(0.6 + 0.8 * torch.rand(v.shape, generator=g))
            elif k.endswith(".bias") and k.startswith("dense."):      # keep the 1-channel map alive after its relu
                v.copy_(0.5 + 0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith(".bias") and ("net." in k or "downsample" in k):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            else:                                                 # conv / linear weights, linear biases: keep the init, as fp32
                v.copy_(v.float().double())
        for k, v in sd.items():
            if v.is_floating_point():
                v.copy_(torch.round(v * SD_SCALE) / SD_SCALE)
                assert float(v.abs().max()) * SD_SCALE < 32767, k
        return model

    models = {"m0": (36, 3, 64, 3), "m1": (48, 5, 96, 3), "m2": (36, 3, 256, 1)}
    nets = {}
    with torch.no_grad():
        for name, (hs, nc, s, b) in models.items():
            torch.manual_seed({"m0": 11, "m1": 12, "m2": 13}[name])
            net = randomize(am.ATHNet(hs, nc, input_size=s).double()).eval()
            nets[name] = net
            v = torch.randint(0, 16, (b, 3, s, s), generator=g).to(torch.uint8).numpy()
            x = torch.from_numpy(v.astype(np.float32) / np.float32(15))
            codes, logits = net(x.double())
            out[f"{name}_cfg"] = np.array([hs, nc, s], dtype=np.int64)
            out[f"{name}_x4"] = v[..., 0::2] | (v[..., 1::2] << 4)
            out[f"{name}_codes"] = codes.numpy()
            out[f"{name}_logits"] = logits.numpy()
            for k, v in net.state_dict().items():
                out[f"{name}__sd__{k}"] = (torch.round(v * SD_SCALE).to(torch.int16) if v.is_floating_point() else v).numpy()
            # the codes must not be trivially signed, and must depend on the image
            assert (codes > 0).any() and (codes < 0).any(), name
            dense = net.dense(net.net2(net.sa(net.net1(x.double())) * net.net1(x.double())))
            assert float((dense > 0).double().mean()) > 0.5, (name, float((dense > 0).double().mean()))
            if b > 1:
                assert float((codes[0] - codes[1]).abs().max()) > 1e-2, name
        labels = torch.tensor([0, 2, 1])
        v0 = np.empty(out["m0_x4"].shape[:-1] + (2 * out["m0_x4"].shape[-1],), dtype=np.uint8)
        v0[..., 0::2], v0[..., 1::2] = out["m0_x4"] & 15, out["m0_x4"] >> 4
        x0 = torch.from_numpy(v0.astype(np.float32) / np.float32(15)).double()
        loader = [(x0[:2], labels[:2]), (x0[2:], labels[2:])]
        c, lg, lb = ta.extract_codes_logits_labels(nets["m0"], loader, torch.device("cpu"), True)
        out["m0_labels"] = labels.numpy()
        out["ext_codes"], out["ext_logits"], out["ext_labels"] = c.numpy(), lg.numpy(), lb.numpy()

    def case(name, q, gal, ql, gl, logits, binary):
        out[f"{name}_q"], out[f"{name}_g"] = q.numpy(), gal.numpy()
        out[f"{name}_ql"], out[f"{name}_gl"], out[f"{name}_logits"] = ql.numpy(), gl.numpy(), logits.numpy()
        saved = ta.torch, tr.torch
        if binary:
            ta.torch = tr.torch = _StableTorch(torch)
        try:
            cm = ta.compute_metrics(q, ql, gal, gl, logits, list(TOPK), binary)
            rm = tr.compute_retrieval_metrics(q, ql, gal, gl, list(TOPK), binary)
        finally:
            ta.torch, tr.torch = saved
        out[f"met_{name}_cm"] = np.array(json.dumps(cm))
        out[f"met_{name}_rm"] = np.array(json.dumps(rm))

    nq, ng = 40, 300
    ql = torch.randint(0, 4, (nq,), generator=g)
    gl = torch.randint(0, 4, (ng,), generator=g)
    logits = torch.randn((nq, 4), generator=g)
    case("l2", torch.randn((nq, 36), generator=g), torch.randn((ng, 36), generator=g), ql, gl, logits, False)
    case("bin", (torch.rand((nq, 36), generator=g) < 0.5).float(), (torch.rand((ng, 36), generator=g) < 0.5).float(), ql, gl,
         logits, True)
    proto = (torch.rand((6, 8), generator=g) < 0.5).float()
    qt = proto[torch.randint(0, 6, (30,), generator=g)]
    gt = proto[torch.randint(0, 6, (200,), generator=g)]
    case("tie", qt, gt, torch.randint(0, 3, (30,), generator=g), torch.randint(0, 3, (200,), generator=g),
         torch.randn((30, 3), generator=g), True)
    path = os.path.join(OUT, "ath_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
