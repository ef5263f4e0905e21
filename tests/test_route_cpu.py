"""The route planner of the top-k search (csrc/mirx_route.h) without a GPU: tests/route_probe.cpp includes the header,
is compiled by the host side of hipcc alone and answers a grid of calls on stdin; every answer is held against the Python
restatement of the rules in tests/_route_ref.py.  The answer of a search never depends on the route, so nothing else notices a
wrong one but the clock."""
import itertools
import os
import subprocess

import pytest

import _route_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = {R.EXACT: 0, R.FILTER: 1, R.DEEP: 2}
ROWS = {R.INDEX: 0, R.NEUTRALISED: 1, R.GATHERED: 2, R.NONE: 3}
ROW_BYTES = 128 * 4 + 8                                            # a gathered row of the narrowest index: fp32 row + id


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path_factory.mktemp("route") / "route_probe")
    r = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "route_probe.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _grid():
    """(tiers_auto, size, k, has_exclude, extra, allow_deep, masked, n_allowed, tile, row_bytes, gather_max): tiers x k x exclude
    x extra x allow_deep x tile, and for each the sizes and allowed-row counts on either side of every threshold, unmasked and
    masked, with a gather limit on either side of what the allowed rows take"""
    lo = R.TIER1_MIN_ROWS
    gathers = (ROW_BYTES, (lo - 1) * ROW_BYTES - 1, 1 << 40)       # one row fits exactly; lo - 1 rows do not by a byte; all fit
    for auto, k, ex, extra, deep, tile in itertools.product((1, 0), (1, 63, 64, 65, 1023, 1024), (1, 0), (0, 1, 8, 1024), (1, 0),
                                                            (64, 128, 256)):
        deep_rows = R.deep_min_rows(k + ex + extra, tile)
        edges = sorted({0, 1, lo - 1, lo, deep_rows - 1, deep_rows})
        for size in edges + [deep_rows + 1000]:
            yield (auto, size, k, ex, extra, deep, 0, 0, tile, ROW_BYTES, gathers[0])
            for n_allowed in [e for e in edges if e < size] + [size]:
                for gmax in gathers:
                    yield (auto, size, k, ex, extra, deep, 1, n_allowed, tile, ROW_BYTES, gmax)


def test_the_header_answers_every_call_as_the_rules_say(probe):
    calls = list(_grid())
    assert len(calls) >= 2 * 6 * 2 * 4 * 2 * 3 * 7
    lines = [" ".join(map(str, R.LIMITS))]
    lines += ["%d %d %d %d %d %d %d %d %d %d %d" % (c[:8] + (R.tile_groups(c[8]),) + c[9:]) for c in calls]
    r = subprocess.run([probe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-500:])
    got = [tuple(map(int, ln.split())) for ln in r.stdout.splitlines()]
    assert len(got) == len(calls)
    seen = set()
    for c, g in zip(calls, got):
        auto, size, k, ex, extra, deep, masked, n_allowed, tile, row_bytes, gmax = c
        lst, rows = R.route(bool(auto), size, k, bool(ex), extra, bool(deep), bool(masked), n_allowed, tile, row_bytes, gmax)
        want = (LISTS[lst], ROWS[rows], R.most_rows(bool(auto), size, k, bool(ex), extra, bool(deep), tile),
                R.deep_min_rows(k + ex + extra, tile))
        assert g == want, (c, g, want)
        seen.add((lst, rows))
    # the grid reaches every route there is
    assert seen == {(R.EXACT, R.INDEX), (R.FILTER, R.INDEX), (R.DEEP, R.INDEX), (R.FILTER, R.NEUTRALISED), (R.DEEP, R.NEUTRALISED),
                    (R.EXACT, R.NEUTRALISED), (R.EXACT, R.GATHERED), (R.EXACT, R.NONE)}


@pytest.mark.parametrize("nq", [1, 64, 65, 128, 129, 8192, 20000])
@pytest.mark.parametrize("k_eff", [65, 100, 1024, 1025, 2049])
def test_deep_min_rows_is_still_the_restatement_of_the_deep_search_test(k_eff, nq):
    """mirx_deep_min_rows, now computed by the header, against test_search_deep_cpu.py's restatement and this one's"""
    from mirx.index import deep_min_rows as lib_rows
    from test_search_deep_cpu import deep_min_rows as restated
    assert lib_rows(k_eff, nq) == restated(k_eff, min(nq, R.QUERY_BATCH)) == R.deep_min_rows(k_eff, R.query_tile(nq))
