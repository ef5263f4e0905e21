"""CPU checks of mirx.ath: the module tree against the reference's, the float64 forward against the fixture made from the reference
(tests/golden/make_golden_ath.py), the float64 restatement tests/_ath_ref.py, and the refusal to rank without a GPU."""
import os

import numpy as np
import pytest
import torch

import _ath_ref as R

Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "ath_ref.npz"))
MODELS = ("m0", "m1", "m2")


def _sd(m):
    return R.fixture_state_dict(Z, m)


def _net(m):
    from mirx.ath import ATHNet
    hs, nc, s = (int(v) for v in Z[f"{m}_cfg"])
    net = ATHNet(hs, nc, input_size=s)
    net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in _sd(m).items()}, strict=True)
    return net.eval()


@pytest.mark.parametrize("m", MODELS)
def test_state_dict_keys_and_shapes(m):
    from mirx.ath import ATHNet
    hs, nc, s = (int(v) for v in Z[f"{m}_cfg"])
    mine = ATHNet(hs, nc, input_size=s).state_dict()
    ref = _sd(m)
    assert list(mine) == list(ref)
    assert all(tuple(mine[k].shape) == tuple(ref[k].shape) for k in ref)
    assert {k.split(".")[0] for k in mine} == {"net1", "sa", "net2", "dense", "hashlayer", "typelayer"}
    _net(m)                                               # strict=True load


def test_input_size_must_divide_by_8():
    from mirx.ath import ATHNet
    with pytest.raises(ValueError, match="divisible by 8"):
        ATHNet(36, 3, input_size=100)


def test_init_is_xavier_normal():
    from mirx.ath import ATHNet
    torch.manual_seed(0)
    net = ATHNet(36, 3, input_size=64)
    w = net.net1[0].net[3].weight                          # 16 x 16 x 3 x 3: xavier std = sqrt(2 / (144 + 144))
    assert abs(float(w.detach().std()) - (2.0 / 288) ** 0.5) < 0.02


@pytest.mark.parametrize("m", MODELS)
def test_cpu_float64_forward_matches_fixture(m):
    net = _net(m).double()
    with torch.no_grad():
        c, lg = net(R.fixture_images(Z, m).double())
    np.testing.assert_allclose(c.numpy(), Z[f"{m}_codes"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(lg.numpy(), Z[f"{m}_logits"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("m", MODELS)
def test_restatement_matches_fixture(m):
    c, lg = R.forward(_sd(m), R.fixture_images(Z, m))
    np.testing.assert_allclose(c.numpy(), Z[f"{m}_codes"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(lg.numpy(), Z[f"{m}_logits"], rtol=0, atol=1e-12)


def test_oracle_ties_to_lowest_id():
    g = np.zeros((7, 5), dtype=np.uint8)
    g[3, 0] = 1
    d, i = R.hamming_topk(np.zeros((1, 5)), g, 6, exclude=[1])
    assert i[0].tolist() == [0, 2, 4, 5, 6, 3] and d[0].tolist() == [0, 0, 0, 0, 0, 1]


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a GPU")
def test_ranking_without_gpu_raises_mirx_error():
    from mirx._lib import MirxError
    from mirx.ath import compute_metrics, compute_retrieval_metrics, hamming_topk
    q, g = torch.from_numpy(Z["bin_q"]), torch.from_numpy(Z["bin_g"])
    with pytest.raises(MirxError):
        hamming_topk(q, g, 5)
    with pytest.raises(MirxError):
        compute_metrics(q, torch.from_numpy(Z["bin_ql"]), g, torch.from_numpy(Z["bin_gl"]), torch.from_numpy(Z["bin_logits"]),
                        [1, 5], True)
    with pytest.raises(MirxError):
        compute_retrieval_metrics(torch.from_numpy(Z["l2_q"]), torch.from_numpy(Z["l2_ql"]), torch.from_numpy(Z["l2_g"]),
                                  torch.from_numpy(Z["l2_gl"]), [1, 5], False)


def test_hamming_argument_checks_before_gpu():
    from mirx.ath import hamming_topk
    g = torch.zeros((10, 36))
    with pytest.raises(ValueError, match="k = 11"):
        hamming_topk(g[:2], g, 11)
    with pytest.raises(ValueError, match="bits"):
        hamming_topk(torch.zeros((2, 1025)), torch.zeros((10, 1025)), 5)
    with pytest.raises(ValueError, match="k must be"):
        hamming_topk(g[:2], g, 0)


def test_abi_rejects_bad_hamming_and_ath_arguments():
    import mirx._lib as L
    lib = L.load()
    assert lib.mirx_hamming_words(36) == 2 and lib.mirx_hamming_words(1024) == 32 and lib.mirx_hamming_words(32) == 1
    assert lib.mirx_hamming_topk(None, 1, None, 10, 36, 11, None, None, 0, None, None, None) == -1
    assert b"k must not exceed" in lib.mirx_last_error()
    assert lib.mirx_hamming_topk(None, 1, None, 10, 1025, 5, None, None, 0, None, None, None) == -1
    assert b"bits" in lib.mirx_last_error()
    assert lib.mirx_hamming_pack(None, 0, 4, 0, None, None, None) == -1
    assert lib.mirx_ath_forward(None, 1, 100, None, 36, 3, None, 0, None, None, None) == -1
    assert b"size" in lib.mirx_last_error()
    assert lib.mirx_ath_workspace_floats(2, 256) == 2 * (16 * 128 * 128 * 2 + 2 * 128 * 128)
