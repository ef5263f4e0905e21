"""IVF_FLAT without a GPU: the restatement (tests/_ivf_ref.py) against the oracle, mirx_ivf_create's argument checks, and the
opt-in surface of Collection -- nothing changes without `approximate`."""
import ctypes
import inspect

import numpy as np
import pytest

import _ivf_ref as R
from oracle import search as OS


def _unit(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return OS.l2_normalize(x)


@pytest.fixture(scope="module")
def recipe():
    """the issue's recipe: 3000 unit rows of dimension 32, nlist = 24, strided start, 10 iterations, 64 perturbed-row queries"""
    rows = _unit(3000, 32, 0)
    rng = np.random.default_rng(1)
    q = OS.l2_normalize(rows[rng.choice(3000, 64, replace=False)] + 0.3 * rng.standard_normal((64, 32)).astype(np.float32))
    cent = R.train(rows, 24, 10, "COSINE")
    return rows, q, cent


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_all_lists_probed_is_the_exact_search(metric):
    rows, q = _unit(500, 20, 2), _unit(9, 20, 3)
    ids = np.arange(500, dtype=np.int64)[::-1].copy()                  # descending ids: the tie rule sees ids
    rows[7] = rows[3]                                                  # a duplicated row: equal scores, ids 492 and 496
    cent = R.train(rows, 12, 3, metric)
    ex = np.array([ids[3], -1, 10 ** 9] + [-1] * 6, dtype=np.int64)
    s, i = R.search(q, rows, ids, cent, 10, 12, metric, exclude=ex)
    o_s, o_i = OS.topk(q, rows, 10, R.metric_code(metric), exclude=ex, ids=ids)
    assert np.array_equal(i, o_i) and np.array_equal(s, o_s)


def test_recall_does_not_fall_with_nprobe(recipe):
    rows, q, cent = recipe
    _, exact = OS.topk(q, rows, 10)
    rec = [R.recall(R.search(q, rows, None, cent, 10, p, "COSINE")[1], exact) for p in (1, 2, 4, 8, 16, 24)]
    assert all(b >= a for a, b in zip(rec, rec[1:])), rec
    assert rec[-1] == 1.0 and rec[0] < 1.0, rec


def test_recipe_differs_from_the_exact_answer(recipe):
    """the condition against vacuous passes that tests/test_ivf_gpu.py asserts on the device, checked on the restatement first"""
    rows, q, cent = recipe
    sizes = np.bincount(R.assign(rows, cent, "COSINE"), minlength=24)
    assert sizes.min() > 0
    _, exact = OS.topk(q, rows, 10)
    _, found = R.search(q, rows, None, cent, 10, 2, "COSINE")
    differ = sum(not np.array_equal(a, b) for a, b in zip(found, exact))
    assert differ >= 48, differ


def test_update_keeps_an_empty_list_and_normalises_ip():
    rows = _unit(40, 8, 4)
    cent = rows[[0, 0, 5]].copy()                                      # list 1 duplicates list 0: the tie rule leaves it empty
    lists = R.assign(rows, cent, "COSINE")
    assert not (lists == 1).any()
    new = R.update(rows, lists, cent, "COSINE")
    assert np.array_equal(new[1], cent[1])
    assert np.allclose(np.linalg.norm(new[[0, 2]].astype(np.float64), axis=1), 1.0, atol=1e-6)
    flat = R.update(rows, lists, cent, "L2")
    mean0 = (np.cumsum(rows[lists == 0].astype(np.float64), axis=0)[-1] / (lists == 0).sum()).astype(np.float32)
    assert np.array_equal(flat[0], mean0)


@pytest.mark.parametrize("args, word", [((0, 0, 8), b"dim"), ((16, 0, 0), b"nlist"), ((16, 0, 65537), b"nlist"),
                                        ((16, 7, 8), b"metric"), ((4096, 0, 8), b"dim")])
def test_ivf_create_rejects_bad_arguments_before_any_device_call(args, word):
    import mirx._lib as L
    lib = L.load()
    h = ctypes.c_void_p()
    dim, metric, nlist = args
    rc = lib.mirx_ivf_create(dim, metric, nlist, 0, ctypes.byref(h))
    assert rc == -1 and word in lib.mirx_last_error(), lib.mirx_last_error()
    assert not h.value
    assert lib.mirx_ivf_size(None) == -1
    assert lib.mirx_ivf_row_block() >= 64 and lib.mirx_ivf_query_tile(1024) >= 1 and lib.mirx_ivf_query_tile(0) == -1


def test_ivf_python_argument_errors_come_before_device_work():
    from mirx.index import IvfFlatIndex, ivf_search_bounds
    for bad in (0, 65537, True, 2.5):
        with pytest.raises(ValueError):
            IvfFlatIndex(16, "COSINE", nlist=bad)
    with pytest.raises(ValueError):
        IvfFlatIndex(16, "HAMMING", nlist=4)
    with pytest.raises(ValueError):
        IvfFlatIndex(4096, "COSINE", nlist=4)
    for k, nprobe in ((0, 1), (1025, 1), (10, 0), (10, 1.5), (True, 1)):
        with pytest.raises(ValueError):
            ivf_search_bounds(k, nprobe)
    assert ivf_search_bounds(np.int64(10), 70000) == (10, 70000)


def test_collection_opt_in_surface():
    from mirx.retriever import Collection, MilvusManager
    from mirx.nih import create_nih_collection
    col = Collection("c", 16)
    with pytest.raises(ValueError, match="IVF_FLAT"):
        col.create_index("embedding", {"index_type": "HNSW", "metric_type": "COSINE"}, approximate=True)
    with pytest.raises(ValueError, match="nlist"):
        col.create_index("embedding", {"index_type": "IVF_FLAT", "params": {"nlist": 0}}, approximate=True)
    assert col._approx_nlist is None
    # without `approximate` every index type is accepted and ignored, as before
    assert col.create_index("embedding", {"index_type": "HNSW", "metric_type": "COSINE", "params": {"nlist": 7}}) is True
    assert col._approx_nlist is None
    assert col.create_index("embedding", {"index_type": "IVF_FLAT", "params": {"nlist": 8}}, approximate=True) is True
    assert col._approx_nlist == 8
    assert col.create_index("embedding", {"index_type": "IVF_FLAT"}, approximate=True) is True and col._approx_nlist == 1024
    assert col.search(np.zeros((2, 16), np.float32), param={"params": {"nprobe": 2}}, limit=3) == [[], []]   # empty: no device
    # nprobe is read under "params" or at the top level, integers >= 1 only
    assert Collection._nprobe({"params": {"nprobe": 10}}) == 10 and Collection._nprobe({"nprobe": 3}) == 3
    for p in (None, {}, {"params": {"nprobe": 0}}, {"nprobe": "10"}, {"nprobe": True}, {"params": {"ef": 64}}):
        assert Collection._nprobe(p) is None
    # the parent's signatures and defaults, with the new keyword appended
    sig = inspect.signature(Collection.create_index)
    assert list(sig.parameters) == ["self", "field_name", "index_params", "approximate"]
    assert [sig.parameters[n].default for n in ("field_name", "index_params", "approximate")] == ["embedding", None, False]
    sig = inspect.signature(Collection.search)
    assert list(sig.parameters) == ["self", "data", "anns_field", "param", "limit", "output_fields", "exclude_ids", "expr",
                                    "group_by_field", "group_size", "strict_group_size", "leave_out_field", "leave_out_values"]
    assert sig.parameters["param"].default is None and sig.parameters["limit"].default == 10
    sig = inspect.signature(MilvusManager.create_index)
    assert list(sig.parameters) == ["self", "model_type", "index_type", "metric_type", "nlist", "approximate"]
    assert sig.parameters["approximate"].default is False and sig.parameters["nlist"].default == 1024
    assert inspect.signature(create_nih_collection).parameters["approximate"].default is False
