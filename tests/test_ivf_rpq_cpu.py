"""IVF_PQ with residual coding without a GPU: the restatement (tests/_rpq_ref.py) against its own definition, the recall and
code-sharing margins that make residual coding worth having on clustered rows, and the argument checks that come before any
device work (mirx_ivf_create_pq_ex, mirx_ivf_pq_train's state rule, Collection's params["by_residual"])."""
import ctypes
import inspect

import numpy as np
import pytest

import _ivf_ref as R
import _pq_ref as P
import _rpq_ref as RP
from oracle import search as OS

F4, F8 = np.float32, np.float64
N, DIM, CENTRES, NLIST, M, SPREAD = 4000, 32, 128, 128, 4, 0.5


def clustered(n, dim, centres, spread, seed):
    """tools/bench_ivf.py::clustered in numpy: unit rows around unit centres"""
    rng = np.random.default_rng(seed)
    c = OS.l2_normalize(rng.standard_normal((centres, dim)).astype(F4))
    which = rng.integers(0, centres, n)
    return OS.l2_normalize((c[which] + spread / dim ** 0.5 * rng.standard_normal((n, dim))).astype(F4))


@pytest.fixture(scope="module")
def gallery():
    rows = clustered(N, DIM, CENTRES, SPREAD, 0)
    rng = np.random.default_rng(1)
    q = OS.l2_normalize((rows[rng.choice(N, 64, replace=False)] + 0.3 * SPREAD / DIM ** 0.5 * rng.standard_normal((64, DIM))).astype(F4))
    raw_cb = P.train_codebooks(rows, M, 10)                       # always L2: one raw quantiser for both metrics
    return rows, q, raw_cb, P.encode(rows, raw_cb)


@pytest.fixture(scope="module", params=["COSINE", "L2"])
def coded(request, gallery):
    metric = request.param
    rows, q, raw_cb, raw_codes = gallery
    cent = R.train(rows, NLIST, 10, metric)
    lists = R.assign(rows, cent, metric)
    cb = RP.train_codebooks(rows, cent, M, 10, metric)
    return metric, cent, lists, cb, RP.encode(rows, lists, cent, cb)


def test_every_list_probed_is_a_lexsort_of_all_scores(gallery, coded):
    rows, q, _, _ = gallery
    metric, cent, lists, cb, codes = coded
    sc = RP.scores(q, codes, lists, cent, cb, metric)
    s, i = RP.search(q, rows, None, cent, cb, 10, NLIST, metric, codes=codes)
    ids = np.arange(N)
    want = np.stack([np.lexsort((ids, -sc[r]))[:10] for r in range(q.shape[0])])
    assert np.array_equal(i, want) and np.array_equal(s.view(np.uint64), np.take_along_axis(sc, want, axis=1).view(np.uint64))
    far_s, far_i = RP.search(q, rows, None, cent, cb, 10, 10 * NLIST, metric, codes=codes)
    assert np.array_equal(far_i, i) and np.array_equal(far_s, s)


def test_zero_centroids_reduce_to_the_raw_scores(gallery):
    rows, q, raw_cb, raw_codes = gallery
    zero = np.zeros((5, DIM), F4)
    lists = np.arange(600) % 5
    assert np.array_equal(RP.residuals(rows[:600], lists, zero).view(np.uint32), rows[:600].view(np.uint32))
    assert np.array_equal(RP.encode(rows[:600], lists, zero, raw_cb), raw_codes[:600])
    got = RP.scores(q, raw_codes[:600], lists, zero, raw_cb, "COSINE")
    assert np.array_equal(got.view(np.uint64), P.scores(q, raw_codes[:600], raw_cb, "COSINE").view(np.uint64))
    assert np.array_equal(RP.reconstruct(raw_codes[:600], lists, zero, raw_cb), P.decode(raw_codes[:600], raw_cb))


def test_l2_score_is_the_distance_to_the_reconstruction(gallery, coded):
    rows, q, _, _ = gallery
    metric, cent, lists, cb, codes = coded
    xh = cent[lists].astype(F8) + P.decode(codes, cb).astype(F8)
    direct = -((q.astype(F8)[:, None, :] - xh[None, :, :]) ** 2).sum(axis=2)
    got = RP.scores(q, codes, lists, cent, cb, "L2")
    err = float(np.abs(got - direct).max())
    print(f"{metric} centroids: largest |expanded - direct| L2 score {err:.3e}")
    assert err <= 1e-12
    ip = RP.scores(q, codes, lists, cent, cb, "COSINE")
    assert float(np.abs(ip - q.astype(F8) @ xh.T).max()) <= 1e-12
    assert np.array_equal(RP.reconstruct(codes, lists, cent, cb), (cent[lists] + P.decode(codes, cb)).astype(F4))


def test_residual_coding_beats_raw_codes_on_clustered_rows(gallery, coded):
    """the reason the feature exists, on the restatement: at nprobe 2 residual recall@10 against IVF_FLAT exceeds raw PQ's by at
    least 0.08, the rows that share a whole code row with another fall from hundreds to a handful, and most queries' id lists
    differ from raw PQ's -- a build that ignored the flag would be seen"""
    rows, q, raw_cb, raw_codes = gallery
    metric, cent, lists, cb, codes = coded
    _, flat = R.search(q, rows, None, cent, 10, 2, metric)
    _, raw = P.search(q, rows, None, cent, raw_cb, 10, 2, metric, codes=raw_codes)
    _, res = RP.search(q, rows, None, cent, cb, 10, 2, metric, codes=codes)
    r_raw, r_res = R.recall(raw, flat), R.recall(res, flat)
    share_raw, share_res = RP.shared_codes(raw_codes), RP.shared_codes(codes, lists)
    differ = sum(not np.array_equal(a, b) for a, b in zip(raw, res))
    print(f"{metric}: recall@10 vs IVF_FLAT at nprobe 2: raw {r_raw:.3f}, residual {r_res:.3f}; rows sharing a code row: raw "
          f"{share_raw}, residual {share_res}; queries whose ids differ {differ} of {q.shape[0]}")
    assert r_res - r_raw >= 0.08, (r_raw, r_res)
    assert share_res < 50 and share_raw > 500, (share_raw, share_res)
    assert differ > q.shape[0] // 2, differ


def _create_ex(lib, dim, metric, nlist, m, nbits, flag):
    h = ctypes.c_void_p()
    rc = lib.mirx_ivf_create_pq_ex(dim, metric, nlist, m, nbits, flag, 0, ctypes.byref(h))
    return rc, h.value, lib.mirx_last_error()


def test_the_new_symbols_exist_and_check_their_arguments_first():
    import mirx._lib as L
    lib = L.load()
    for name in ("mirx_ivf_create_pq_ex", "mirx_ivf_pq_by_residual", "mirx_ivf_get_norms", "mirx_pq_residuals", "mirx_pq_bases"):
        assert hasattr(lib, name), name
    assert lib.mirx_version() == L.ABI_VERSION == 305                               # additions only
    for flag in (2, -1, 255):
        rc, h, msg = _create_ex(lib, 64, 0, 8, 8, 8, flag)
        assert rc == -1 and not h and b"by_residual" in msg, (flag, msg)
    for flag in (0, 1):                                                            # mirx_ivf_create_pq's own checks, behind the flag's
        assert _create_ex(lib, 64, 0, 8, 6, 8, flag)[0] == -1 and b"m must" in lib.mirx_last_error()
        assert _create_ex(lib, 40, 0, 8, 8, 8, flag)[0] == -1 and b"dim" in lib.mirx_last_error()
        assert _create_ex(lib, 64, 0, 8, 8, 4, flag)[0] == -1 and b"nbits" in lib.mirx_last_error()
    assert lib.mirx_ivf_pq_by_residual(None) == -1
    assert lib.mirx_ivf_get_norms(None, None) == -1
    assert lib.mirx_pq_residuals(None, -1, 64, None, None, 4, None, None) == -1
    assert lib.mirx_pq_residuals(None, 5, 0, None, None, 4, None, None) == -1
    assert lib.mirx_pq_residuals(None, 5, 64, None, None, 0, None, None) == -1
    assert lib.mirx_pq_residuals(None, 5, 64, None, None, 4, None, None) == -1 and b"null" in lib.mirx_last_error()
    for bad in ((5, 64, 6), (5, 40, 8), (-1, 64, 8)):
        assert lib.mirx_pq_bases(None, bad[0], bad[1], bad[2], None, 1, None, 4, None, None, None) == -1
    assert lib.mirx_pq_bases(None, 1, 64, 8, None, 0, None, 4, None, None, None) == -1 and b"nprobe" in lib.mirx_last_error()
    assert lib.mirx_pq_bases(None, 1, 64, 8, None, 1, None, 4, None, None, None) == -1 and b"null" in lib.mirx_last_error()


def test_python_argument_errors_come_before_device_work():
    from mirx.index import IvfPqIndex, IvfResidualPqIndex, pq_bases, pq_residuals, residual_flag
    assert issubclass(IvfResidualPqIndex, IvfPqIndex) and IvfResidualPqIndex.KIND == 2
    assert IvfPqIndex.by_residual is False                                         # the raw class does not change
    assert list(inspect.signature(IvfResidualPqIndex.__init__).parameters) == ["self", "dim", "metric", "nlist", "m", "device",
                                                                               "by_residual"]
    assert inspect.signature(IvfResidualPqIndex.__init__).parameters["by_residual"].default is True
    for bad in (0, 1, "yes", None, 2.0):
        with pytest.raises(ValueError, match="by_residual"):
            IvfResidualPqIndex(64, "COSINE", nlist=4, m=8, by_residual=bad)
    with pytest.raises(ValueError, match="m"):
        IvfResidualPqIndex(64, "COSINE", nlist=4, m=6)
    assert residual_flag(True) is True and residual_flag(np.bool_(False)) is False
    for name in ("norms", "bases", "train", "train_codebooks", "set_codebooks", "codebooks", "codes", "reconstruct", "tables"):
        assert hasattr(IvfResidualPqIndex, name), name
    assert callable(pq_bases) and callable(pq_residuals)


def test_collection_takes_by_residual_and_refuses_anything_but_a_bool():
    from mirx.retriever import Collection
    col = Collection("c", 32)
    base = {"index_type": "IVF_PQ", "params": {"nlist": 8, "m": 8}}
    for bad in (1, 0, "true", None, 2.5):
        with pytest.raises(ValueError, match="by_residual"):
            col.create_index("embedding", {"index_type": "IVF_PQ", "params": {"nlist": 8, "m": 8, "by_residual": bad}}, approximate=True)
    assert (col._approx_nlist, col._approx_type, col._approx_m, col._approx_residual) == (None, None, None, False)
    assert col.create_index("embedding", base, approximate=True) is True           # the default stays raw
    assert (col._approx_type, col._approx_m, col._approx_residual) == ("IVF_PQ", 8, False)
    on = {"index_type": "IVF_PQ", "params": {"nlist": 8, "m": 8, "by_residual": True}}
    assert col.create_index("embedding", on, approximate=True) is True
    assert (col._approx_nlist, col._approx_type, col._approx_m, col._approx_residual) == (8, "IVF_PQ", 8, True)
    assert col.search(np.zeros((2, 32), F4), param={"params": {"nprobe": 2}}, limit=3) == [[], []]       # empty: no device
    off = {"index_type": "IVF_PQ", "params": {"nlist": 8, "m": 8, "by_residual": False}}
    assert col.create_index("embedding", off, approximate=True) is True and col._approx_residual is False
    assert col.create_index("embedding", {"index_type": "IVF_FLAT", "params": {"nlist": 8, "by_residual": True}}, approximate=True)
    assert (col._approx_type, col._approx_residual) == ("IVF_FLAT", False)         # the key belongs to IVF_PQ alone
    assert col.create_index("embedding", on) is True and col._approx_type is None  # ignored without the opt-in
