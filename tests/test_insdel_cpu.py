"""mirx.insdel without a GPU: the torch path of insdel_curves against the float64 / numpy restatement (tests/_insdel_ref.py) and
against the per-(pair, mode) CausalMetric.evaluate it batches, the stable tie rule, InsDel's return orders, argument validation
and the ABI's new symbols.

Tolerances.  1e-12 against the restatement: both sides embed the same images in the same chunks with the same torch model, so
the embeddings agree bit for bit and only the float64 scoring (a dot product of <= 96 terms, |cos| <= 1) differs in summation
order.  2e-6 against CausalMetric.evaluate: that path takes the cosine in float32 (1.2e-7 per value) and embeds other batch
sizes; it is the bound tests/test_xai_gpu.py sets between two chunkings of that path."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _insdel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, K = 8, 3


class Tiny(torch.nn.Module):
    """conv, pool, flatten, normalize"""

    def __init__(self, dtype=torch.float32):
        super().__init__()
        g = torch.Generator().manual_seed(4)
        self.conv = torch.nn.Conv2d(3, 6, 3, padding=1)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(6, 3, 3, 3, generator=g) * 0.4)
            self.conv.bias.copy_(torch.randn(6, generator=g) * 0.1)
        self.to(dtype)

    def forward(self, x):
        return F.normalize(F.avg_pool2d(self.conv(x), 2).flatten(1), dim=1)


def _inputs(dtype=torch.float32):
    g = torch.Generator().manual_seed(21)
    x_q = torch.randn(1, 3, S, S, generator=g).to(dtype)
    x_r = torch.randn(K, 3, S, S, generator=g).to(dtype)
    x_r[1] = -x_q[0] + 0.3 * x_r[1]                       # a hit that starts with a negative similarity: the counters count
    return x_q, x_r, R.distinct_saliency(K, S * S, 5).reshape(K, S, S)


def _conv_blur(klen, nsig):
    from mirx.xai import gkern
    kern = gkern(klen, nsig)
    return lambda x: F.conv2d(x, kern.to(x.dtype), padding=klen // 2)


@pytest.mark.parametrize("step", [5, 64, 100])
@pytest.mark.parametrize("dtype,max_batch", [(torch.float32, 1024), (torch.float64, 5)])
def test_insdel_curves_matches_the_restatement(step, dtype, max_batch):
    from mirx.xai import GaussianBlur, insdel_curves
    model = Tiny(dtype).eval()
    x_q, x_r, sal = _inputs(dtype)
    blur = GaussianBlur(5, 1.0)
    subs = {"del": torch.zeros_like, "ins": blur}
    res = insdel_curves(model, x_q, x_r, sal, step, substrates=subs, input_size=S, max_batch=max_batch)
    auc, scores, zero = R.insdel_ref(model, x_q, x_r, sal, step, ("del", "ins"), subs, max_batch)
    n_steps = math.ceil(S * S / step)
    assert res.scores.shape == (K, 2, n_steps + 1) and res.auc.shape == (K, 2) and res.zero_counter.shape == (K, 2)
    assert res.scores.dtype == np.float64 and res.auc.dtype == np.float64 and res.zero_counter.dtype == np.int64
    assert not res.last_native and not blur.last_native
    np.testing.assert_allclose(res.scores, scores, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.auc, auc, rtol=0, atol=1e-12)
    assert np.array_equal(res.zero_counter, zero) and zero.sum() > 0
    one = insdel_curves(model, x_q, x_r, sal, step, modes=("ins",), substrates=subs)
    np.testing.assert_allclose(one.scores[:, 0], res.scores[:, 1], rtol=0, atol=1e-6 if dtype == torch.float32 else 1e-12)


@pytest.mark.parametrize("step", [5, 64, 100])
def test_insdel_curves_matches_causal_metric_per_pair(step):
    from mirx.xai import CausalMetric, GaussianBlur, insdel_curves
    model = Tiny().eval()
    x_q, x_r, sal = _inputs()
    assert R.tie_free(sal)
    res = insdel_curves(model, x_q, x_r, sal, step, substrates={"ins": GaussianBlur(5, 1.0)})
    for k in range(K):
        for mi, mode in enumerate(("del", "ins")):
            sub = torch.zeros_like if mode == "del" else _conv_blur(5, 1.0)
            auc, scores, zero = CausalMetric(model, mode, step, sub, input_size=S).evaluate(x_q, x_r[k:k + 1], sal[k])
            np.testing.assert_allclose(res.scores[k, mi], scores, rtol=0, atol=2e-6)
            assert abs(res.auc[k, mi] - auc) <= 2e-6
            assert res.zero_counter[k, mi] == zero


def test_step_map_follows_the_stable_rule_on_ties():
    from mirx.insdel import stable_steps
    g = torch.Generator().manual_seed(8)
    sal = torch.rand(3, 97, generator=g)
    sal[0, ::2] = 0.0                                       # half the map tied at 0, one of them -0.0
    sal[0, 4] = -0.0
    sal[1, 10:20] = sal[1, 3]
    sal[1, 50] = float("nan")
    sal[1, 60] = float("inf")
    sal[1, 61] = -float("inf")
    sal[1, 70] = -float("nan")
    sal[2] = 0.25                                           # all equal
    for step in (1, 7, 97, 102):
        got = stable_steps(sal, step).numpy()
        assert np.array_equal(got, R.steps_ref(sal.numpy(), step)), step
    t1 = stable_steps(sal, 1).numpy()
    assert t1[1, 70] == 0 and t1[1, 50] == 1 and t1[1, 60] == 2 and t1[1, 61] == 96      # NaNs (index descending), +inf, .., -inf
    assert np.array_equal(t1[2], np.arange(97)[::-1])                                    # equal values: descending index
    assert t1[0, 4] > t1[0, 6] and t1[0, 4] < t1[0, 2]                                   # -0.0 ties with its +0.0 neighbours


def test_gaussian_blur_is_the_conv2d_form():
    from mirx.xai import GaussianBlur, gkern
    blur = GaussianBlur(51, math.sqrt(50))
    assert blur.kernel2d.shape == (51, 51) and torch.equal(blur.kernel2d, gkern(51, math.sqrt(50))[0, 0])
    x = torch.randn(2, 3, 9, 11, generator=torch.Generator().manual_seed(2))
    want = F.conv2d(x, gkern(51, math.sqrt(50)), padding=25)
    assert float((blur(x) - want).abs().max()) <= 4 * R.ULP32 * float(want.abs().max())
    assert not blur.last_native


def test_insdel_return_orders():
    """evaluate -> (score_del, score_ins, deletion's counter, insertion's counter); forward -> (ins, del, deletion's counters,
    insertion's counters): the reference's swapped positions."""
    from mirx.xai import InsDel, insdel_curves
    model = Tiny().eval()
    x_q, x_r, sal = _inputs()
    metric = InsDel(model, "cpu", input_size=S)
    res = insdel_curves(model, x_q, x_r, sal, S, substrates=metric.substrates)
    assert (res.zero_counter[:, 0] != res.zero_counter[:, 1]).any()        # the swap is observable
    ins_avg, del_avg, z_ins, z_del = metric.forward(x_q, [x_r[k:k + 1] for k in range(K)], [sal[k] for k in range(K)])
    np.testing.assert_allclose(ins_avg, res.auc[:, 1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(del_avg, res.auc[:, 0], rtol=0, atol=1e-12)
    assert z_ins == [int(v) for v in res.zero_counter[:, 0]] and z_del == [int(v) for v in res.zero_counter[:, 1]]
    assert all(isinstance(v, float) for v in ins_avg + del_avg) and all(isinstance(v, int) for v in z_ins + z_del)
    metric.load_query(x_q)
    for k in range(K):
        s_del, s_ins, third, fourth = metric.evaluate(sal[k], x_r[k])      # a [3, S, S] hit works like a [1, 3, S, S] one
        assert abs(s_del - del_avg[k]) <= 2e-6 and abs(s_ins - ins_avg[k]) <= 2e-6
        assert (third, fourth) == (z_ins[k], z_del[k])
    assert not metric.last_native


def test_argument_validation():
    from mirx.xai import GaussianBlur, insdel_curves
    model = Tiny().eval()
    x_q, x_r, sal = _inputs()
    bad = [
        dict(x_q=x_q[0]), dict(x_q=torch.cat([x_q, x_q])), dict(x_r=x_r[:, :2]), dict(x_r=x_r[:, :, :4, :4]), dict(x_r=x_r.double()),
        dict(saliency=sal[:2]), dict(saliency=sal[:, :4]), dict(step=0), dict(step=2.5), dict(max_batch=0), dict(modes=()),
        dict(modes=("del", "del")), dict(modes=("blur",)), dict(substrates={"ins": 3}), dict(substrates={"both": torch.zeros_like}),
        dict(input_size=S + 1), dict(substrates={"ins": lambda x: x[:, :1]}),
    ]
    for kw in bad:
        args = dict(x_q=x_q, x_r=x_r, saliency=sal, step=5)
        args.update(kw)
        with pytest.raises(ValueError):
            insdel_curves(model, **args)
    with pytest.raises(ValueError):
        GaussianBlur(0, 1.0)
    with pytest.raises(ValueError):
        GaussianBlur(5, 1.0)(torch.zeros(3, 8, 8))


def test_new_symbols_are_declared_and_bound():
    from mirx import _lib
    header = open(os.path.join(ROOT, "include", "mirx.h")).read()
    lib = _lib.load()
    for name in ("mirx_insdel_steps_workspace_bytes", "mirx_insdel_steps", "mirx_blur2d_same", "mirx_insdel_compose",
                 "mirx_insdel_curves"):
        assert name + "(" in header and name in _lib.SYMBOLS and hasattr(lib, name)
    # limits are refused before any HIP call
    assert lib.mirx_insdel_steps_workspace_bytes(1, 0) == -1 and b"hw" in lib.mirx_last_error()
    assert lib.mirx_insdel_steps_workspace_bytes(65536, 16) == -1
    assert lib.mirx_insdel_steps_workspace_bytes(1, (1 << 20) + 1) == -1
    assert lib.mirx_insdel_steps_workspace_bytes(3, 4097) >= 3 * 4097 * 24
    assert lib.mirx_insdel_steps(None, 1, 16, 0, None, 0, None, None) == -1 and b"step" in lib.mirx_last_error()
    assert lib.mirx_blur2d_same(None, 1, 3, 8, 8, None, 50, None, None) == -1 and b"klen" in lib.mirx_last_error()
    assert lib.mirx_blur2d_same(None, 1, 3, 8, 8, None, 65, None, None) == -1
    assert lib.mirx_insdel_compose(None, 1, 16, None, 1, None, None, None, 2, 4, 8, 3, None, None) == -1    # 8 + 3 > 2 * 5
    assert b"g0" in lib.mirx_last_error()
    assert lib.mirx_insdel_curves(None, None, 0, 4, 8, None, None, None, None) == -1
