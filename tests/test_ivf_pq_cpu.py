"""IVF_PQ without a GPU: the restatement (tests/_pq_ref.py) against its own definition, the conditions under which
tests/test_ivf_pq_gpu.py cannot pass vacuously, the argument checks of mirx_ivf_create_pq / IvfPqIndex and Collection's surface."""
import ctypes
import inspect

import numpy as np
import pytest

import _ivf_ref as R
import _pq_ref as P
from oracle import search as OS

F4, F8 = np.float32, np.float64
M = 8


@pytest.fixture(scope="module")
def quantiser():
    """tests/test_ivf_cpu.py's rows (3000 unit rows of dimension 32) and 64 perturbed-row queries; m = 8 codebooks after 10
    iterations (always L2: shared by both metrics), the codes and the decoded rows"""
    rows = OS.l2_normalize(np.random.default_rng(0).standard_normal((3000, 32)).astype(F4))
    rng = np.random.default_rng(1)
    q = OS.l2_normalize(rows[rng.choice(3000, 64, replace=False)] + 0.3 * rng.standard_normal((64, 32)).astype(F4))
    cb = P.train_codebooks(rows, M, 10)
    codes = P.encode(rows, cb)
    return rows, q, cb, codes, P.decode(codes, cb)


def test_encode_inverts_decode_and_every_codeword_is_used(quantiser):
    rows, _, cb, codes, dec = quantiser
    assert cb.shape == (M, 256, 4) and cb.dtype == F4 and codes.shape == (3000, M) and codes.dtype == np.uint8
    assert all(np.unique(codes[:, j]).size == 256 for j in range(M))
    assert np.array_equal(P.encode(dec, cb), codes)
    assert np.array_equal(dec[:, 4:8], cb[1][codes[:, 1]])                          # exact fp32 copies of the codewords
    every = np.repeat(np.arange(256, dtype=np.uint8)[:, None], M, axis=1)
    assert np.array_equal(P.encode(P.decode(every, cb), cb), every)


def test_a_duplicated_codeword_is_never_chosen_over_its_lower_twin(quantiser):
    rows, _, cb, codes, _ = quantiser
    twin = cb.copy()
    twin[3, 200] = twin[3, 17]
    got = P.encode(rows[:600], twin)
    assert (got[:, 3] != 200).all() and (got[:, 3] == 17).any()
    assert np.array_equal(got[:, :3], codes[:600, :3])                              # the other sub-spaces do not notice


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_the_recipe_cannot_pass_vacuously(quantiser, metric):
    """what tests/test_ivf_pq_gpu.py relies on, on the restatement first: the ADC answer is neither IVF_FLAT's nor the lane-tree
    search of the decoded rows, so a build that scored the wrong thing would be seen"""
    rows, q, cb, codes, dec = quantiser
    cent = R.train(rows, 24, 10, metric)
    s, i = P.search(q, rows, None, cent, cb, 10, 2, metric, codes=codes)
    _, i_flat = R.search(q, rows, None, cent, 10, 2, metric)
    assert all(not np.array_equal(a, b) for a, b in zip(i, i_flat))                 # every query's id list differs
    rec = R.recall(i, i_flat)
    lane = OS.scores(q, dec, R.metric_code(metric))
    differ = int((np.take_along_axis(lane, i, axis=1).view(np.uint64) != s.view(np.uint64)).sum())
    print(f"{metric}: recall@10 against IVF_FLAT {rec:.3f}; ADC scores whose bits differ from the lane tree's {differ} of 640")
    assert 0.5 < rec < 1.0, rec
    assert differ >= 100, differ
    # nprobe = nlist: the ADC ranking of all rows
    sc = P.scores(q, codes, cb, metric)
    full_s, full_i = P.search(q, rows, None, cent, cb, 10, 24, metric, codes=codes)
    ids = np.arange(3000)
    want = np.stack([np.lexsort((ids, -sc[r]))[:10] for r in range(64)])
    assert np.array_equal(full_i, want) and np.array_equal(full_s, np.take_along_axis(sc, want, axis=1))


def _create_pq(lib, dim, metric, nlist, m, nbits):
    h = ctypes.c_void_p()
    rc = lib.mirx_ivf_create_pq(dim, metric, nlist, m, nbits, 0, ctypes.byref(h))
    return rc, h.value, lib.mirx_last_error()


def test_create_pq_rejects_bad_arguments_before_any_device_call():
    import mirx._lib as L
    lib = L.load()
    for m in (0, 3, 6, 68, -4):
        rc, h, msg = _create_pq(lib, 2176, 0, 8, m, 8)
        assert rc == -1 and not h and b"m must" in msg, (m, msg)
    for dim, m in ((40, 8), (8, 4), (100, 4), (0, 4)):                              # no multiple of 4 m
        rc, h, msg = _create_pq(lib, dim, 0, 8, m, 8)
        assert rc == -1 and not h and b"dim" in msg, (dim, m, msg)
    for nbits in (4, 16, 0):
        rc, h, msg = _create_pq(lib, 64, 0, 8, 8, nbits)
        assert rc == -1 and not h and b"nbits" in msg
    assert _create_pq(lib, 64, 5, 8, 8, 8)[0] == -1 and b"metric" in lib.mirx_last_error()
    assert _create_pq(lib, 64, 0, 0, 8, 8)[0] == -1 and b"nlist" in lib.mirx_last_error()
    assert _create_pq(lib, 4096, 0, 8, 8, 8)[0] == -1 and b"dim" in lib.mirx_last_error()
    h = ctypes.c_void_p()
    assert lib.mirx_ivf_create_typed(64, 0, 8, 2, 0, ctypes.byref(h)) == -1 and not h.value      # a PQ handle needs m
    assert b"kind" in lib.mirx_last_error() and b"mirx_ivf_create_pq" in lib.mirx_last_error()
    assert (L.IVF_FLAT, L.IVF_SQ8, L.IVF_PQ) == (0, 1, 2) and lib.mirx_ivf_pq_m(None) == -1
    assert lib.mirx_ivf_pq_item_rows() >= 64 and lib.mirx_version() == L.ABI_VERSION == 305
    for bad in ((5, 64, 6), (5, 40, 8), (-1, 64, 8)):                               # the quantiser calls check n, dim, m first
        assert lib.mirx_pq_encode(None, bad[0], bad[1], bad[2], None, None, None) == -1
        assert lib.mirx_pq_decode(None, bad[0], bad[1], bad[2], None, None, None) == -1
        assert lib.mirx_pq_tables(None, bad[0], bad[1], bad[2], 0, None, None, None) == -1
    assert lib.mirx_pq_tables(None, 1, 64, 8, 7, None, None, None) == -1 and b"metric" in lib.mirx_last_error()


def test_python_argument_errors_come_before_device_work():
    from mirx.index import IvfPqIndex, IvfFlatIndex, pq_bounds
    assert issubclass(IvfPqIndex, IvfFlatIndex) and IvfPqIndex.KIND == 2
    assert list(inspect.signature(IvfPqIndex.__init__).parameters) == ["self", "dim", "metric", "nlist", "m", "device"]
    for bad in (0, 3, 6, 68, True, 2.5, None, "8"):
        with pytest.raises(ValueError, match="m"):
            IvfPqIndex(2176, "COSINE", nlist=4, m=bad)
    with pytest.raises(ValueError, match="4 m"):
        IvfPqIndex(40, "COSINE", nlist=4, m=8)
    for bad in (0, 65537, True, 2.5):
        with pytest.raises(ValueError, match="nlist"):
            IvfPqIndex(64, "COSINE", nlist=bad, m=8)
    with pytest.raises(ValueError):
        IvfPqIndex(64, "HAMMING", nlist=4, m=8)
    with pytest.raises(ValueError):
        IvfPqIndex(4096, "COSINE", nlist=4, m=8)
    assert pq_bounds(1024, 64) == 64 and pq_bounds(16, np.int64(4)) == 4
    for name in ("train", "train_codebooks", "set_codebooks", "codebooks", "codes", "reconstruct", "tables", "search", "last_stats"):
        assert hasattr(IvfPqIndex, name), name


def test_collection_accepts_ivf_pq_with_m_and_keeps_its_surface():
    from mirx.retriever import Collection, MilvusManager
    from mirx.nih import create_nih_collection, _nih_index_params
    col = Collection("c", 32)
    with pytest.raises(ValueError, match=r"IVF_PQ.*params\['m'\].*IVF_FLAT.*IVF_SQ8"):
        col.create_index("embedding", {"index_type": "IVF_PQ", "params": {"nlist": 8}}, approximate=True)
    with pytest.raises(ValueError, match="IVF_FLAT"):
        col.create_index("embedding", {"index_type": "IVF_PQ"}, approximate=True)
    for bad in (0, 6, 68, 16, True, "8"):                                          # 16: 32 is no multiple of 4 x 16
        with pytest.raises(ValueError, match="m"):
            col.create_index("embedding", {"index_type": "IVF_PQ", "params": {"nlist": 8, "m": bad}}, approximate=True)
    with pytest.raises(ValueError, match="nlist"):
        col.create_index("embedding", {"index_type": "IVF_PQ", "params": {"nlist": 0, "m": 8}}, approximate=True)
    for other in ("HNSW", "FLAT", None):
        with pytest.raises(ValueError, match="'IVF_FLAT', 'IVF_SQ8' or 'IVF_PQ'"):
            col.create_index("embedding", {"index_type": other}, approximate=True)
    assert (col._approx_nlist, col._approx_type, col._approx_m) == (None, None, None)
    assert col.create_index("embedding", {"index_type": "IVF_PQ"}) is True          # ignored without the opt-in, m or not
    assert col._approx_type is None
    assert col.create_index("embedding", {"index_type": "IVF_PQ", "params": {"nlist": 8, "m": 8}}, approximate=True) is True
    assert (col._approx_nlist, col._approx_type, col._approx_m) == (8, "IVF_PQ", 8)
    assert col.create_index("embedding", {"index_type": "IVF_PQ", "params": {"m": 4}}, approximate=True) is True
    assert (col._approx_nlist, col._approx_type, col._approx_m) == (1024, "IVF_PQ", 4)
    assert col.search(np.zeros((2, 32), F4), param={"params": {"nprobe": 2}}, limit=3) == [[], []]       # empty: no device
    assert col.create_index("embedding", {"index_type": "IVF_SQ8", "params": {"nlist": 8}}, approximate=True) is True
    assert (col._approx_nlist, col._approx_type, col._approx_m) == (8, "IVF_SQ8", None)
    sig = inspect.signature(Collection.create_index)
    assert list(sig.parameters) == ["self", "field_name", "index_params", "approximate"]
    sig = inspect.signature(MilvusManager.create_index)
    assert list(sig.parameters) == ["self", "model_type", "index_type", "metric_type", "nlist", "approximate"]
    sig = inspect.signature(create_nih_collection)
    assert list(sig.parameters) == ["collection_name", "drop_old", "metric_type", "index_type", "nlist", "device", "store", "approximate"]
    assert _nih_index_params("COSINE", "IVF_PQ", 16) == {"metric_type": "COSINE", "index_type": "IVF_PQ", "params": {"nlist": 16}}
    with pytest.raises(ValueError, match=r"params\['m'\]"):                         # the reference's call, as real Milvus answers it
        create_nih_collection("nih_pq_cpu", index_type="IVF_PQ", nlist=16, approximate=True)
