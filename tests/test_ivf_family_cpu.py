"""mirx.index.ivf_index_spec, the one table from (dim, index_type, params) to a member of the IVF family and its constructor
keywords: every accepted form gives the expected class and keywords, and every refused form raises the very ValueError that
Collection.create_index(approximate=True) raises for it.  No GPU and no library: nothing is constructed."""
import inspect

import numpy as np
import pytest

DIM = 32

ACCEPTED = [
    ("IVF_FLAT", None, "IvfFlatIndex", {"nlist": 1024}),
    ("IVF_FLAT", {}, "IvfFlatIndex", {"nlist": 1024}),
    ("IVF_FLAT", "no dict", "IvfFlatIndex", {"nlist": 1024}),
    ("IVF_FLAT", {"nlist": 1}, "IvfFlatIndex", {"nlist": 1}),
    ("IVF_FLAT", {"nlist": 65536}, "IvfFlatIndex", {"nlist": 65536}),
    ("IVF_FLAT", {"nlist": np.int64(8)}, "IvfFlatIndex", {"nlist": 8}),
    ("IVF_FLAT", {"nlist": 8, "m": 5, "by_residual": "yes"}, "IvfFlatIndex", {"nlist": 8}),      # the keys belong to IVF_PQ alone
    ("IVF_SQ8", {"nlist": 8}, "IvfSq8Index", {"nlist": 8}),
    ("IVF_SQ8", {"nlist": 8, "m": 8}, "IvfSq8Index", {"nlist": 8}),
    ("IVF_PQ", {"m": 4}, "IvfPqIndex", {"nlist": 1024, "m": 4}),
    ("IVF_PQ", {"nlist": 8, "m": 8}, "IvfPqIndex", {"nlist": 8, "m": 8}),
    ("IVF_PQ", {"nlist": 8, "m": np.int32(8)}, "IvfPqIndex", {"nlist": 8, "m": 8}),
    ("IVF_PQ", {"nlist": 8, "m": 8, "by_residual": False}, "IvfPqIndex", {"nlist": 8, "m": 8}),
    ("IVF_PQ", {"nlist": 8, "m": 8, "by_residual": True}, "IvfResidualPqIndex", {"nlist": 8, "m": 8}),
    ("IVF_PQ", {"nlist": 8, "m": 4, "by_residual": np.bool_(True)}, "IvfResidualPqIndex", {"nlist": 8, "m": 4}),
]

REFUSED = [
    ("HNSW", {"nlist": 8}, "'IVF_FLAT', 'IVF_SQ8' or 'IVF_PQ', got 'HNSW'"),
    ("FLAT", None, "got 'FLAT'"),
    (None, {"nlist": 8}, "got None"),
    ("ivf_flat", {}, "got 'ivf_flat'"),
    ("IVF_PQ", {"nlist": 8}, "needs params['m']"),
    ("IVF_PQ", None, "needs params['m']"),
    ("IVF_PQ", {"nlist": 0}, "needs params['m']"),                                   # m is looked at before nlist
    ("IVF_PQ", {"nlist": 8, "m": 0}, "multiple of 4 in [4, 64], got 0"),
    ("IVF_PQ", {"nlist": 8, "m": 6}, "got 6"),
    ("IVF_PQ", {"nlist": 8, "m": 68}, "got 68"),
    ("IVF_PQ", {"nlist": 8, "m": 16}, "multiple of 4 m = 64, got dim 32"),
    ("IVF_PQ", {"nlist": 8, "m": True}, "m must be an integer, got True"),
    ("IVF_PQ", {"nlist": 8, "m": "8"}, "m must be an integer, got '8'"),
    ("IVF_PQ", {"nlist": 8, "m": 8, "by_residual": 1}, "params['by_residual'] must be True or False, got 1"),
    ("IVF_PQ", {"nlist": 8, "m": 8, "by_residual": "yes"}, "got 'yes'"),
    ("IVF_PQ", {"nlist": 8, "m": 8, "by_residual": None}, "got None"),
    ("IVF_PQ", {"nlist": 0, "m": 8, "by_residual": 1}, "by_residual"),               # ... and by_residual before nlist
    ("IVF_PQ", {"nlist": 0, "m": 8}, "nlist must be an integer in [1, 65536], got 0"),
    ("IVF_FLAT", {"nlist": 0}, "got 0"),
    ("IVF_FLAT", {"nlist": 65537}, "got 65537"),
    ("IVF_SQ8", {"nlist": -1}, "got -1"),
    ("IVF_SQ8", {"nlist": True}, "got True"),
    ("IVF_FLAT", {"nlist": 8.0}, "got 8.0"),
    ("IVF_FLAT", {"nlist": "8"}, "got '8'"),
]


@pytest.mark.parametrize("index_type, params, cls_name, kwargs", ACCEPTED)
def test_accepted_forms_give_the_class_and_its_keywords(index_type, params, cls_name, kwargs):
    import mirx.index as X
    from mirx.retriever import Collection
    cls, got = X.ivf_index_spec(DIM, index_type, params)
    assert cls is getattr(X, cls_name) and got == kwargs
    assert all(type(v) is int for v in got.values())
    accepted = inspect.signature(cls.__init__).parameters
    assert set(got) <= set(accepted) and {"dim", "metric", "device"} <= set(accepted)      # cls(dim, metric, device=, **kwargs)
    col = Collection("c", DIM)
    assert col.create_index("embedding", {"index_type": index_type, "params": params}, approximate=True) is True
    assert (col._approx_nlist, col._approx_type, col._approx_m, col._approx_residual) == \
        (kwargs["nlist"], index_type, kwargs.get("m"), cls is X.IvfResidualPqIndex)
    assert col._ivf is None


@pytest.mark.parametrize("index_type, params, part", REFUSED)
def test_refused_forms_raise_what_create_index_raises(index_type, params, part):
    from mirx.index import ivf_index_spec
    from mirx.retriever import Collection
    with pytest.raises(ValueError) as direct:
        ivf_index_spec(DIM, index_type, params)
    col = Collection("c", DIM)
    with pytest.raises(ValueError) as through:
        col.create_index("embedding", {"index_type": index_type, "params": params}, approximate=True)
    assert str(direct.value) == str(through.value) and part in str(direct.value)
    assert (col._approx_nlist, col._approx_type, col._approx_m, col._approx_residual) == (None, None, None, False)


def test_min_train_rows_and_state_keys_per_class():
    from mirx.index import IVF_INDEX_TYPES, IvfFlatIndex, IvfPqIndex, IvfResidualPqIndex, IvfSq8Index
    assert IVF_INDEX_TYPES == {"IVF_FLAT": IvfFlatIndex, "IVF_SQ8": IvfSq8Index, "IVF_PQ": IvfPqIndex}
    for cls in (IvfFlatIndex, IvfSq8Index):
        assert [cls.min_train_rows(n) for n in (1, 255, 256, 1024)] == [1, 255, 256, 1024]
    for cls in (IvfPqIndex, IvfResidualPqIndex):
        assert [cls.min_train_rows(n) for n in (1, 255, 256, 1024)] == [256, 256, 256, 1024]         # 256 codewords to seed
    assert IvfFlatIndex.STATE_KEYS == ("centroids",) and IvfSq8Index.STATE_KEYS == ("centroids", "vmin", "scale")
    assert IvfPqIndex.STATE_KEYS == IvfResidualPqIndex.STATE_KEYS == ("centroids", "codebooks")


def test_strided_sample_takes_the_rows_floor_i_n_over_limit():
    import torch
    from mirx.index import strided_sample
    rows = torch.arange(1000, dtype=torch.float32).reshape(-1, 1)
    assert strided_sample(rows, 1000) is rows and strided_sample(rows, 5000) is rows
    for limit in (1, 7, 256, 999):
        got = strided_sample(rows, limit)
        assert got.is_contiguous() and got[:, 0].tolist() == [float(i * 1000 // limit) for i in range(limit)]
