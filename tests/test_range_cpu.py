"""Range search, the parts that need no GPU: the pymilvus radius / range_filter mapping (mirx.index.range_bounds), the new
entry points' argument checks, and that Collection.search only reaches the range path when `param` names a radius."""
import ctypes
import math

import numpy as np
import pytest

from mirx.index import range_bounds


@pytest.mark.parametrize("metric", ["COSINE", "IP", "cosine", "ip"])
def test_bounds_similarity_metrics(metric):
    assert range_bounds(metric, 0.25) == (0.25, math.inf)
    assert range_bounds(metric, 0.25, 0.75) == (0.25, 0.75)
    assert range_bounds(metric, -0.5, 0) == (-0.5, 0.0)
    assert range_bounds(metric, np.float32(0.5), np.float64(2.0)) == (0.5, 2.0)
    assert range_bounds(metric, -math.inf) == (-math.inf, math.inf)
    for rf in (0.25, 0.1, -1.0):                         # range_filter <= radius
        with pytest.raises(ValueError):
            range_bounds(metric, 0.25, rf)


def test_bounds_l2_are_negative_squares_in_fp64():
    assert range_bounds("L2", 2.0) == (-4.0, 0.0)
    assert range_bounds("L2", 2.0, 0.5) == (-4.0, -0.25)
    assert range_bounds("l2", 3, 0) == (-9.0, -0.0)
    lo, hi = range_bounds("L2", 0.1)
    assert lo == -(0.1 * 0.1) and hi == 0.0
    # squaring in fp32 gives another number: the bound must come from the fp64 product
    assert lo != -float(np.float32(0.1) * np.float32(0.1))
    assert lo != -float(np.float32(0.1 * 0.1))
    assert isinstance(lo, float) and isinstance(hi, float)


@pytest.mark.parametrize("radius,rf", [(1.0, 1.0), (1.0, 2.0), (-1.0, None), (1.0, -0.5), (0.0, 0.0)])
def test_bounds_l2_errors(radius, rf):
    with pytest.raises(ValueError):
        range_bounds("L2", radius, rf)


@pytest.mark.parametrize("metric", ["COSINE", "IP", "L2"])
def test_bounds_refuse_nan_and_non_numbers(metric):
    for radius, rf in [(math.nan, None), (0.5, math.nan), ("0.5", None), (0.5, "0.9"), (None, None), ([0.5], None),
                       (True, None), (0.5, 1j)]:
        with pytest.raises(ValueError):
            range_bounds(metric, radius, rf)
    with pytest.raises(ValueError):
        range_bounds("HAMMING", 0.5)


def test_entry_points_refuse_a_null_index_without_gpu():
    import mirx._lib as L
    lib = L.load()
    lims = (ctypes.c_int64 * 2)()
    total = ctypes.c_int64(7)
    rc = lib.mirx_index_range_search(None, None, 0, 0.0, 1.0, None, None, 0, ctypes.cast(lims, ctypes.c_void_p),
                                     ctypes.byref(total), None)
    assert rc < 0 and b"range_search" in lib.mirx_last_error() and b"null index" in lib.mirx_last_error()
    rc = lib.mirx_index_range_fetch(None, None, None, None, None)
    assert rc < 0 and b"range_fetch" in lib.mirx_last_error()
    st = L.RangeStats()
    rc = lib.mirx_index_range_last_stats(None, ctypes.byref(st))
    assert rc < 0 and b"range_last_stats" in lib.mirx_last_error()
    assert ctypes.sizeof(L.RangeStats) == 5 * 8
    assert L.OPT_RANGE_MAX_HITS == 8


def test_range_params_are_read_from_both_places():
    from mirx.retriever import Collection
    rp = Collection._range_params
    assert rp(None) is None and rp({}) is None and rp({"metric_type": "COSINE", "params": {"nprobe": 10}}) is None
    assert rp({"params": {"radius": 0.5}}) == (0.5, None)
    assert rp({"params": {"radius": 0.5, "range_filter": 0.9}}) == (0.5, 0.9)
    assert rp({"radius": 0.25, "range_filter": 0.5}) == (0.25, 0.5)
    assert rp({"radius": 0.25, "params": {"nprobe": 4}}) == (0.25, None)


def test_search_without_radius_does_not_reach_the_range_path(monkeypatch):
    """Collection.search(param=...) without a radius ignores param as before: range_search is never called (the empty
    collection answers on the host, so this runs without a GPU), with a radius an empty collection still answers []."""
    from mirx.retriever import Collection

    def boom(*a, **k):
        raise AssertionError("range_search reached without a radius")

    monkeypatch.setattr(Collection, "range_search", boom)
    col = Collection("c", 8)
    q = np.zeros((2, 8), dtype=np.float32)
    for param in (None, {}, {"metric_type": "COSINE", "params": {"nprobe": 10}}, {"params": {"ef": 64}}):
        assert col.search(q, param=param, limit=3) == [[], []]
    assert col.search(q, param={"params": {"radius": 0.5}}, limit=3) == [[], []]
