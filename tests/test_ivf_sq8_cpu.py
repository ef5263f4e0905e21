"""IVF_SQ8 without a GPU: the quantiser's restatement (tests/_sq8_ref.py) against its own definition, the conditions under
which tests/test_ivf_sq8_gpu.py cannot pass vacuously, mirx_ivf_create_typed's argument check and Collection's surface."""
import ctypes
import inspect

import numpy as np
import pytest

import _ivf_ref as R
import _sq8_ref as Q
from oracle import search as OS

F4, F8 = np.float32, np.float64


@pytest.fixture(scope="module", params=["COSINE", "L2"])
def recipe(request):
    """tests/test_ivf_cpu.py's recipe (3000 unit rows of dimension 32, nlist = 24, strided start, 10 iterations, 64
    perturbed-row queries), its range trained on every row, per metric"""
    metric = request.param
    rows = OS.l2_normalize(np.random.default_rng(0).standard_normal((3000, 32)).astype(F4))
    rng = np.random.default_rng(1)
    q = OS.l2_normalize(rows[rng.choice(3000, 64, replace=False)] + 0.3 * rng.standard_normal((64, 32)).astype(F4))
    cent = R.train(rows, 24, 10, metric)
    vmin, scale = Q.train_range(rows)
    codes = Q.encode(rows, vmin, scale)
    return metric, rows, q, cent, vmin, scale, codes, Q.decode(codes, vmin, scale)


def test_range_is_min_and_255th_of_the_span(recipe):
    _, rows, _, _, vmin, scale, codes, _ = recipe
    assert vmin.dtype == scale.dtype == F4 and codes.dtype == np.uint8
    assert np.array_equal(vmin, rows.min(axis=0))
    assert np.array_equal(scale, ((rows.max(axis=0).astype(F8) - rows.min(axis=0).astype(F8)) / 255.0).astype(F4))
    assert (codes.min(axis=0) == 0).all() and (codes.max(axis=0) == 255).all()      # the extremes of every column


def test_encode_inverts_decode_and_the_error_is_half_a_step(recipe):
    _, rows, _, _, vmin, scale, codes, dec = recipe
    assert np.array_equal(Q.encode(dec, vmin, scale), codes)
    every = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 32, axis=1)
    assert np.array_equal(Q.encode(Q.decode(every, vmin, scale), vmin, scale), every)
    # |x - xhat| <= scale / 2 in exact arithmetic; the decoded value is rounded to fp32 once more: one ulp of it on top
    err = np.abs(rows.astype(F8) - dec.astype(F8))
    bound = scale.astype(F8) / 2 + np.spacing(np.abs(dec)).astype(F8)
    assert (err <= bound).all(), float((err - bound).max())
    assert err.max() > scale.min() / 4                                              # and it is not an identity


def test_constant_column_out_of_range_rows_and_specials():
    rows = np.random.default_rng(3).standard_normal((50, 6)).astype(F4)
    rows[:, 2] = F4(0.75)                                                           # a constant column: scale 0
    rows[:, 4] = F4(-0.0)
    rows[7, 4] = F4(0.0)                                                            # both zeros: the minimum is stored as +0
    rows[5, 1] = np.nan                                                             # ignored by the range
    vmin, scale = Q.train_range(rows)
    assert scale[2] == 0 and vmin[2] == F4(0.75) and scale[4] == 0 and not np.signbit(vmin[4])
    assert vmin[1] == np.nanmin(rows[:, 1]) and np.isfinite(scale).all()
    codes = Q.encode(rows, vmin, scale)
    assert (codes[:, 2] == 0).all() and (Q.decode(codes, vmin, scale)[:, 2] == F4(0.75)).all()
    assert codes[5, 1] == 0
    far = np.stack([vmin - 10, vmin + 300 * scale + 10, np.full(6, np.inf, F4), np.full(6, -np.inf, F4), np.full(6, np.nan, F4)])
    got = Q.encode(far.astype(F4), vmin, scale)
    live = scale > 0
    assert (got[0] == 0).all() and (got[1][live] == 255).all() and (got[1][~live] == 0).all()
    assert (got[2][live] == 255).all() and (got[3] == 0).all() and (got[4] == 0).all()
    nothing = np.full((3, 2), np.nan, F4)                                           # a column without a number
    vmin, scale = Q.train_range(nothing)
    assert (vmin == 0).all() and (scale == 0).all() and (Q.encode(nothing, vmin, scale) == 0).all()


def test_ties_round_up_and_boundaries_are_sharp():
    vmin, scale = np.array([1.0], F4), np.array([0.25], F4)                         # exact in binary: t is exact
    x = np.array([[1.0 + 0.25 * c + 0.125] for c in range(4)], F4)                  # t = c + 0.5 exactly
    assert Q.encode(x, vmin, scale)[:, 0].tolist() == [1, 2, 3, 4]
    below, above = np.nextafter(x, F4(-np.inf)), np.nextafter(x, F4(np.inf))
    assert Q.encode(below, vmin, scale)[:, 0].tolist() == [0, 1, 2, 3]
    assert Q.encode(above, vmin, scale)[:, 0].tolist() == [1, 2, 3, 4]


def test_the_recipe_cannot_pass_vacuously(recipe):
    """what tests/test_ivf_sq8_gpu.py relies on, checked on the restatement first: decoding changes every score's bits, many id
    lists and some rows' lists, so an index that scored or assigned the wrong rows would be seen"""
    metric, rows, q, cent, vmin, scale, _, dec = recipe
    code = R.metric_code(metric)
    s_o, i_o = OS.topk(q, rows, 10, code)
    s_d, i_d = OS.topk(q, dec, 10, code)
    assert (s_o != s_d).all(), int((s_o != s_d).sum())                              # 640 of 640
    differ = sum(not np.array_equal(a, b) for a, b in zip(i_o, i_d))
    moved = int((R.assign(rows, cent, metric) != R.assign(dec, cent, metric)).sum())
    print(f"{metric}: id lists that differ {differ} of 64; rows that change list when assigned from the decoded rows {moved}")
    assert differ >= 24, differ
    assert moved >= 1, moved
    # nprobe = nlist over the decoded rows is the flat answer over them
    s, i = Q.search(q, rows, None, cent, vmin, scale, 10, 24, metric)
    assert np.array_equal(i, i_d) and np.array_equal(s, s_d)


@pytest.mark.parametrize("kind", [-1, 2, 7])
def test_create_typed_rejects_a_bad_kind_before_any_device_call(kind):
    import mirx._lib as L
    lib = L.load()
    h = ctypes.c_void_p()
    rc = lib.mirx_ivf_create_typed(16, 0, 8, kind, 0, ctypes.byref(h))
    assert rc == -1 and b"kind" in lib.mirx_last_error(), lib.mirx_last_error()
    assert not h.value
    assert (L.IVF_FLAT, L.IVF_SQ8) == (0, 1) and lib.mirx_ivf_kind(None) == -1


def test_python_argument_errors_come_before_device_work():
    from mirx.index import IvfSq8Index, IvfFlatIndex
    assert issubclass(IvfSq8Index, IvfFlatIndex) and IvfSq8Index.KIND == 1 and IvfFlatIndex.KIND == 0
    for bad in (0, 65537, True, 2.5):
        with pytest.raises(ValueError):
            IvfSq8Index(16, "COSINE", nlist=bad)
    with pytest.raises(ValueError):
        IvfSq8Index(16, "HAMMING", nlist=4)
    with pytest.raises(ValueError):
        IvfSq8Index(4096, "COSINE", nlist=4)
    for name in ("train_range", "set_range", "range", "codes", "reconstruct", "search", "last_stats"):
        assert hasattr(IvfSq8Index, name), name


def test_collection_accepts_ivf_sq8_and_keeps_its_surface():
    from mirx.retriever import Collection, MilvusManager
    from mirx.nih import create_nih_collection
    col = Collection("c", 16)
    for other in ("HNSW", "IVF_PQ", "FLAT", None):
        with pytest.raises(ValueError, match="IVF_FLAT"):
            col.create_index("embedding", {"index_type": other, "metric_type": "COSINE"}, approximate=True)
    with pytest.raises(ValueError, match="nlist"):
        col.create_index("embedding", {"index_type": "IVF_SQ8", "params": {"nlist": 0}}, approximate=True)
    assert col._approx_nlist is None and col._approx_type is None
    assert col.create_index("embedding", {"index_type": "IVF_SQ8", "params": {"nlist": 8}}) is True      # ignored without the opt-in
    assert col._approx_nlist is None
    assert col.create_index("embedding", {"index_type": "IVF_SQ8", "params": {"nlist": 8}}, approximate=True) is True
    assert (col._approx_nlist, col._approx_type) == (8, "IVF_SQ8")
    assert col.create_index("embedding", {"index_type": "IVF_FLAT", "params": {"nlist": 8}}, approximate=True) is True
    assert (col._approx_nlist, col._approx_type) == (8, "IVF_FLAT")
    assert col.create_index("embedding", {"index_type": "IVF_SQ8"}, approximate=True) is True and col._approx_nlist == 1024
    assert col.search(np.zeros((2, 16), F4), param={"params": {"nprobe": 2}}, limit=3) == [[], []]       # empty: no device
    sig = inspect.signature(Collection.create_index)
    assert list(sig.parameters) == ["self", "field_name", "index_params", "approximate"]
    assert [sig.parameters[n].default for n in ("field_name", "index_params", "approximate")] == ["embedding", None, False]
    sig = inspect.signature(Collection.search)
    assert list(sig.parameters) == ["self", "data", "anns_field", "param", "limit", "output_fields", "exclude_ids", "expr",
                                    "group_by_field", "group_size", "strict_group_size", "leave_out_field", "leave_out_values"]
    sig = inspect.signature(MilvusManager.create_index)
    assert list(sig.parameters) == ["self", "model_type", "index_type", "metric_type", "nlist", "approximate"]
    assert sig.parameters["approximate"].default is False and sig.parameters["nlist"].default == 1024
    assert inspect.signature(create_nih_collection).parameters["approximate"].default is False
    # the wrappers hand the type through (create_nih_collection loads its collection: tests/test_ivf_sq8_gpu.py)
    from mirx.nih import _nih_index_params
    assert _nih_index_params("COSINE", "IVF_SQ8", 16) == {"metric_type": "COSINE", "index_type": "IVF_SQ8", "params": {"nlist": 16}}
