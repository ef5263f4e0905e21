"""The deep search route (mirx_index_search_deep) as far as a box without a GPU can see it: the entry point's argument
checks, the Python signature, and the host routing bound deep_min_rows against the constants in the sources."""
import ctypes
import inspect
import os
import re

import pytest

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-retrieval---thesis-2026_amd", "csrc")


def _constexpr(fname, name):
    """The value of `constexpr int[64_t] NAME = <int>;` in csrc/FNAME: the test follows the library's capacities."""
    with open(os.path.join(_CSRC, fname)) as f:
        m = re.search(r"constexpr\s+(?:int|int64_t)\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    assert m, (fname, name)
    return int(m.group(1))


def deep_min_rows(k_eff, nq):
    """mirx_index.hip's deep_min_rows restated from the constants: the sampled threshold resolves the route's target candidate
    count only from target * DEEP_GROUP_ROWS / (threshold groups per 256-row tile) rows on"""
    target = _constexpr("mirx_common.h", "DEEP_TARGET_MUL") * k_eff + _constexpr("mirx_common.h", "DEEP_TARGET_ADD")
    tile = 64 if nq <= 64 else (128 if nq <= 128 else 256)
    groups = 8 // (tile // 64)
    return max(_constexpr("mirx_api.hip", "TIER1_MIN_ROWS"), target * _constexpr("mirx_common.h", "DEEP_GROUP_ROWS") // groups)


def test_null_handle_and_k_bounds_are_refused_with_a_message():
    import mirx._lib as L
    lib = L.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.mirx_index_search_deep(None, p, 1, 100, None, None, p, None, p, None) == -1
    assert b"null index" in lib.mirx_last_error()
    for k in (0, 1025):
        assert lib.mirx_index_search_deep(None, p, 1, k, None, None, p, None, p, None) == -1
        assert b"[1, 1024]" in lib.mirx_last_error()


def test_flatindex_search_deep_has_searchs_signature():
    from mirx.index import FlatIndex
    deep, plain = inspect.signature(FlatIndex.search_deep), inspect.signature(FlatIndex.search)
    assert list(deep.parameters) == ["self", "q", "k", "exclude_ids", "return_f64", "allow"]
    assert [(p.name, p.default) for p in deep.parameters.values()] == [(p.name, p.default) for p in plain.parameters.values()]


@pytest.mark.parametrize("nq", [1, 64, 65, 128, 129, 300, 8192, 20000])
@pytest.mark.parametrize("k_eff", [65, 100, 101, 1024, 1025])
def test_deep_min_rows_follows_the_constants(k_eff, nq):
    import mirx._lib as L
    from mirx.index import deep_min_rows as lib_rows, tier1_max_k
    assert tier1_max_k() == _constexpr("mirx_api.hip", "TIER1_MAX_K")
    want = deep_min_rows(k_eff, min(nq, _constexpr("mirx_api.hip", "QUERY_BATCH")))
    assert lib_rows(k_eff, nq) == want
    assert want >= _constexpr("mirx_api.hip", "TIER1_MIN_ROWS")
    assert L.load().mirx_deep_min_rows(0, 1) == -1 and L.load().mirx_deep_min_rows(65, 0) == -1


def test_the_capacities_are_consistent():
    """DEEP_CAP holds the target of the largest k_eff with room, and the deep regions hold a run of consecutive rows"""
    cap = _constexpr("mirx_common.h", "DEEP_CAP")
    assert cap >= _constexpr("mirx_common.h", "DEEP_TARGET_MUL") * 1025 + _constexpr("mirx_common.h", "DEEP_TARGET_ADD")
    assert cap > _constexpr("mirx_common.h", "CAND_CAP") and cap & (cap - 1) == 0
    assert _constexpr("mirx_common.h", "DEEP_MIN_SLOTS") >= 32
