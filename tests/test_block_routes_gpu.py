"""Route pin of the pre-norm transformer block that DINOv2 (_VitBlock) and the SigLIP towers (_EncoderLayer) run natively:
per geometry and kernel-configuration arm, the literal list of libmirx entry points one block forward calls, in order, and
the block's output against the module path of the same block (the plain PyTorch forward of a float64 CPU copy).

The expected lists were recorded on the commit before the two blocks were folded into one routine; they describe what the
blocks launched there, not how the routine is written.  One case did not pass there: vit / terms_s3_attention raised
UnboundLocalError in _VitBlock.forward (a name used twice) where the SigLIP copy converted the fp32 context with
mirx_rows_to_terms; its list is the SigLIP one.  The bound, 2e-5 of max |want|, is the one
test_linear_gpu.py::test_vit_block_split3_matches_rocblas_path uses (measured maxima: profiles/r17_block_glue.txt)."""
import copy
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

ARMS = {
    "default": {},
    "terms": dict(linear_terms_min_rows=1),
    "terms_s3_attention": dict(linear_terms_min_rows=1, attention_two_fp16=False),
    "three_bf16": dict(linear_two_fp16=False, attention_two_fp16=False),
    "fp32_attention": dict(linear_two_fp16=False, attention_two_fp16=False, attention_three_bf16=False),
}
TERMS_LINEAR = ["mirx_linear_terms_workspace_bytes", "mirx_linear_terms"]


def _h2(attention):
    return ["mirx_layernorm", "mirx_linear_split2h", attention, "mirx_linear_split2h", "mirx_layernorm", "mirx_linear_split2h",
            "mirx_linear_split2h"]


def _s3(attention):
    return ["mirx_layernorm", "mirx_linear_split3", attention, "mirx_linear_split3", "mirx_layernorm", "mirx_linear_split3",
            "mirx_linear_split3"]


def _terms(attention):
    """attention: the launches between the qkv Linear and the projection (the kernel, and the conversion of its fp32
    output to terms rows where it does not write them itself)."""
    return (["mirx_layernorm_terms"] + TERMS_LINEAR + attention + TERMS_LINEAR + ["mirx_layernorm_terms"] + TERMS_LINEAR
            + TERMS_LINEAR)


FLASH = {
    "default": _h2("mirx_attention_qkv_f32_split2h"),
    "terms": _terms(["mirx_attention_qkv_f32_split2h_terms"]),
    "terms_s3_attention": _terms(["mirx_attention_qkv_f32_split3", "mirx_rows_to_terms"]),
    "three_bf16": _s3("mirx_attention_qkv_f32_split3"),
}
SMALL = {
    "default": _h2("mirx_attention_small"),
    "terms": _terms(["mirx_attention_small", "mirx_rows_to_terms"]),
    "terms_s3_attention": _terms(["mirx_attention_small", "mirx_rows_to_terms"]),
    "three_bf16": _s3("mirx_attention_small"),
    "fp32_attention": _s3("mirx_attention_small"),
}
EXPECTED = {
    # DINOv2 honours attention_three_bf16=False (fp32 MFMAs); SigLIP's flash fallback stays on three bf16 terms
    "vit": dict(FLASH, fp32_attention=_s3("mirx_attention_qkv_f32")),
    "siglip_flash": dict(FLASH, fp32_attention=_s3("mirx_attention_qkv_f32_split3")),
    "siglip_short": SMALL,
    "siglip_masked": SMALL,
}


class _Recorder:
    """Every name of _lib.SYMBOLS on the loaded library object replaced by a wrapper that records the name, then calls on."""

    def __enter__(self):
        from mirx import _lib
        self.lib = _lib.load()
        self.calls = []
        self.orig = {name: getattr(self.lib, name) for name in _lib.SYMBOLS}
        for name, fn in self.orig.items():
            setattr(self.lib, name, lambda *a, _fn=fn, _name=name: (self.calls.append(_name), _fn(*a))[1])
        return self

    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(self.lib, name, fn)


def _vit_case():
    import mirx.model as mm
    torch.manual_seed(3)
    blk = mm._VitBlock(128, 2).eval()                            # head_dim 64
    with torch.no_grad():
        blk.ls1.gamma.normal_()
        blk.ls2.gamma.normal_()
        for p in (blk.attn.qkv.bias, blk.attn.proj.bias, blk.mlp.fc1.bias, blk.mlp.fc2.bias):
            p.normal_(std=0.1)
    x = torch.randn(2, 33, 128)                                  # 33 tokens: a partly filled attention tile and a K/V tail
    with torch.no_grad():
        want = copy.deepcopy(blk).double()(x.double())
    blk = blk.cuda()
    at, c = blk.attn, 128
    lins = (at.qkv, at.proj, blk.mlp.fc1, blk.mlp.fc2)
    bounds = dict(b1=mm._layernorm_bound(blk.norm1), b2=mm._layernorm_bound(blk.norm2),
                  bqk=mm._linear_out_bound(blk.norm1, at.qkv, slice(0, 2 * c)),
                  bv=mm._linear_out_bound(blk.norm1, at.qkv, slice(2 * c, 3 * c)), bh=mm._linear_out_bound(blk.norm2, blk.mlp.fc1))
    return dict(block=blk, run=lambda: blk(x.cuda()), x=x, want=want, lins=lins, bounds=bounds, key_mask=None)


def _siglip_cases():
    import mirx.model as mm
    from mirx.siglip import SiglipVisionTower
    torch.manual_seed(4)
    tower = SiglipVisionTower(hidden_size=144, intermediate_size=208, num_hidden_layers=1, num_attention_heads=2, image_size=84,
                              patch_size=14).eval()              # head_dim 72, an MLP width that is no multiple of 128
    layer = tower.encoder.layers[0]
    sa = layer.self_attn
    with torch.no_grad():
        for p in (sa.q_proj.bias, sa.k_proj.bias, sa.v_proj.bias, sa.out_proj.bias, layer.mlp.fc1.bias, layer.mlp.fc2.bias):
            p.normal_(std=0.1)
    ref = copy.deepcopy(layer).double()
    mask = torch.ones(3, 36, dtype=torch.int64)
    for i in range(3):
        mask[i, 36 - 5 * (i + 1):] = 0
    geoms = {"siglip_flash": (torch.randn(3, 36, 144), None),    # 36 tokens, no mask: the flash kernels
             "siglip_short": (torch.randn(3, 16, 144), None),    # fewer than 32 tokens: mirx_attention_small
             "siglip_masked": (torch.randn(3, 36, 144), mask)}   # a key mask: mirx_attention_small
    with torch.no_grad():
        wants = {g: ref(x.double(), km)[0] for g, (x, km) in geoms.items()}
    tower = tower.cuda()
    ln1, ln2 = layer.layer_norm1, layer.layer_norm2
    bounds = dict(b1=mm._layernorm_bound(ln1), b2=mm._layernorm_bound(ln2),
                  bqk=max(mm._linear_out_bound(ln1, sa.q_proj), mm._linear_out_bound(ln1, sa.k_proj)),
                  bv=mm._linear_out_bound(ln1, sa.v_proj), bh=mm._linear_out_bound(ln2, layer.mlp.fc1))
    out = {}
    for g, (x, km) in geoms.items():
        kmc = None if km is None else km.cuda()
        out[g] = dict(block=layer, run=lambda x=x, kmc=kmc: layer(x.cuda(), kmc)[0], x=x, want=wants[g], bounds=bounds, key_mask=km,
                      lins=(sa._packed.refresh(), sa.out_proj, layer.mlp.fc1, layer.mlp.fc2))
    return out


@pytest.fixture(scope="module")
def cases():
    return dict(_siglip_cases(), vit=_vit_case())


def _run_arm(case, arm):
    """One forward of the block under the arm's configuration -> (recorded entry points, output on the CPU)."""
    import mirx.model as mm
    blk = case["block"]
    mm.set_kernel_config(blk, dataclasses.replace(mm.DEFAULT_CONFIG, **ARMS[arm]))
    try:
        with torch.no_grad(), _Recorder() as rec:
            got = case["run"]()
        return rec.calls, got.cpu()
    finally:
        mm.set_kernel_config(blk, mm.DEFAULT_CONFIG)


def _check_preconditions(case, geom, arm):
    """The gate the case means to take is the one it takes."""
    import mirx.model as mm
    blk, x, bd = case["block"], case["x"], case["bounds"]
    cfg = dataclasses.replace(mm.DEFAULT_CONFIG, **ARMS[arm])
    mm.set_kernel_config(blk, cfg)
    try:
        assert not torch.is_grad_enabled()
        assert all(0.0 < v < 3.0e4 for v in bd.values()), bd
        probe = torch.empty(1, device="cuda")
        rows = x.shape[0] * x.shape[1]
        terms = mm._linear_terms_ok(blk, rows, case["lins"], (bd["b1"], bd["b2"], bd["bv"], bd["bh"]))
        assert terms == arm.startswith("terms")
        assert all(mm._linear_s3_ok(lin, probe) for lin in case["lins"])
        assert all(mm._linear_h2_ok(lin, probe, bd["b1"]) == cfg.linear_two_fp16 for lin in case["lins"])
        flash = case["key_mask"] is None and x.shape[1] >= 32
        assert flash == (geom in ("vit", "siglip_flash"))
        assert (geom == "siglip_masked") == (case["key_mask"] is not None)
    finally:
        mm.set_kernel_config(blk, mm.DEFAULT_CONFIG)


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("geom", list(EXPECTED))
def test_block_route_and_output(cases, geom, arm):
    case = cases[geom]
    with torch.no_grad():
        _check_preconditions(case, geom, arm)
    calls, got = _run_arm(case, arm)
    want = case["want"]
    err, bound = float((got.double() - want).abs().max()), 2e-5 * float(want.abs().max())
    print(f"{geom} {arm}: max |got - float64| = {err:.3e}, bound = {bound:.3e}")
    assert calls == EXPECTED[geom][arm]
    assert got.shape == want.shape and err < bound


def test_tap_sees_the_packed_qkv_between_the_projection_and_attention(cases):
    case = cases["siglip_flash"]
    layer, x = case["block"], case["x"].cuda()
    seen = []
    with torch.no_grad(), _Recorder() as rec:
        got = layer._forward_mirx(x, None, tap=lambda qkv: seen.append((tuple(qkv.shape), qkv.dtype, list(rec.calls))))
        plain = layer._forward_mirx(x, None)
    assert seen == [((3, 36, 3 * 144), torch.float32, ["mirx_layernorm", "mirx_linear_split2h"])]
    assert rec.calls == 2 * EXPECTED["siglip_flash"]["default"]
    assert torch.equal(got, plain)                               # the tap changes nothing the layer computes
