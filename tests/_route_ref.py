"""The route of a top-k search restated in Python from its rules, with the constants read from the sources: what
tests/test_route_cpu.py holds csrc/mirx_route.h against, and what the GPU tests expect of last_stats()."""
import os
import re

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-retrieval---thesis-2026_amd", "csrc")

EXACT, FILTER, DEEP = "EXACT", "FILTER", "DEEP"
INDEX, NEUTRALISED, GATHERED, NONE = "INDEX", "NEUTRALISED", "GATHERED", "NONE"


def constexpr(fname, name):
    """The value of `constexpr int[64_t] NAME = <int>;` in csrc/FNAME."""
    with open(os.path.join(_CSRC, fname)) as f:
        m = re.search(r"constexpr\s+(?:int|int64_t)\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    assert m, (fname, name)
    return int(m.group(1))


TIER1_MIN_ROWS = constexpr("mirx_api.hip", "TIER1_MIN_ROWS")
TIER1_MAX_K = constexpr("mirx_api.hip", "TIER1_MAX_K")
QUERY_BATCH = constexpr("mirx_api.hip", "QUERY_BATCH")
MAX_K = constexpr("mirx_common.h", "MAX_K")
DEEP_TARGET_MUL = constexpr("mirx_common.h", "DEEP_TARGET_MUL")
DEEP_TARGET_ADD = constexpr("mirx_common.h", "DEEP_TARGET_ADD")
DEEP_GROUP_ROWS = constexpr("mirx_common.h", "DEEP_GROUP_ROWS")
# the order tests/route_probe.cpp reads them in
LIMITS = (TIER1_MIN_ROWS, TIER1_MAX_K, MAX_K, DEEP_TARGET_MUL, DEEP_TARGET_ADD, DEEP_GROUP_ROWS)


def query_tile(nq):
    """the filter GEMM's query tile for the widest internal batch of a call of nq queries"""
    nq = min(nq, QUERY_BATCH)
    return 64 if nq <= 64 else (128 if nq <= 128 else 256)


def tile_groups(tile):
    """threshold groups per 256-row gallery tile at that query tile"""
    return 8 // (tile // 64)


def deep_min_rows(k_eff, tile):
    return max(TIER1_MIN_ROWS, (DEEP_TARGET_MUL * k_eff + DEEP_TARGET_ADD) * DEEP_GROUP_ROWS // tile_groups(tile))


def _open(tiers_auto, k, has_exclude, extra, allow_deep, tile):
    k_eff = k + (1 if has_exclude else 0) + extra
    deep_open = allow_deep and tiers_auto and k_eff > TIER1_MAX_K and k + extra <= MAX_K
    return k_eff, deep_open, deep_min_rows(k_eff, tile)


def route(tiers_auto, size, k, has_exclude, extra, allow_deep, masked, n_allowed, tile, row_bytes, gather_max):
    """-> (list, rows)"""
    k_eff, deep_open, deep_rows = _open(tiers_auto, k, has_exclude, extra, allow_deep, tile)
    if not masked or n_allowed == size:
        if deep_open and size >= deep_rows:
            return DEEP, INDEX
        if tiers_auto and size >= TIER1_MIN_ROWS and k_eff <= TIER1_MAX_K:
            return FILTER, INDEX
        return EXACT, INDEX
    if deep_open:
        lists = n_allowed >= deep_rows
    else:
        lists = tiers_auto and n_allowed >= TIER1_MIN_ROWS and k_eff <= TIER1_MAX_K
    if lists:
        return (DEEP if deep_open else FILTER), NEUTRALISED
    if n_allowed > 0 and n_allowed * row_bytes > gather_max:
        return EXACT, NEUTRALISED
    if n_allowed > 0:
        return EXACT, GATHERED
    return EXACT, NONE


def most_rows(tiers_auto, size, k, has_exclude, extra, allow_deep, tile):
    """the most allowed rows a masked call may have to gather, known before the mask is counted"""
    k_eff, deep_open, deep_rows = _open(tiers_auto, k, has_exclude, extra, allow_deep, tile)
    if deep_open:
        return min(size, deep_rows - 1)
    if tiers_auto and k_eff <= TIER1_MAX_K:           # the filter route is open at TIER1_MIN_ROWS rows
        return min(size, TIER1_MIN_ROWS - 1)
    return size
