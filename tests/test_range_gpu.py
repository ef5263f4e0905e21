"""FlatIndex.range_search (mirx_index_range_search, k_range.hip) and Collection.range_search against the definition: row r is a
hit of query i when it is live, lo < s(i, r) <= hi on the fp64 ranking score s, its mask entry is non-zero and its id is not the
query's excluded id; hits are ordered by (score descending, id ascending).  GPU only.

No tolerance anywhere.  The expected hits come from oracle.search.scores (the fp64 lane-tree scores, inputs padded with zero
columns to a multiple of 4 as the index pads them) with that definition applied in numpy; ids, the fp64 bits and the reported
fp32 bits are compared.  Ids are 7 + 3 * row.  L2 galleries have row norms in [0.5, 2].  Small galleries take the exact route,
one 45 000 x 64 gallery per metric the filter route (and, forced, the exact one: the answer never depends on the route)."""
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import search as OS

pytestmark = pytest.mark.gpu

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-retrieval---thesis-2026_amd", "csrc")
METRICS = ("COSINE", "L2")
INF = math.inf


def _L():
    from mirx import _lib
    return _lib


def _constexpr(fname, name):
    with open(os.path.join(_CSRC, fname)) as f:
        m = re.search(r"constexpr\s+(?:int|int64_t)\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    assert m, (fname, name)
    return int(m.group(1))


MIN_ROWS = _constexpr("mirx_api.hip", "TIER1_MIN_ROWS")
QUERY_BATCH = _constexpr("mirx_api.hip", "QUERY_BATCH")
RANGE_CAP = _constexpr("mirx_common.h", "CAND_CAP") + _constexpr("mirx_common.h", "CAND_OVF")
DIM_ALIGN = _constexpr("mirx_common.h", "DIM_ALIGN")
BIG_N, BIG_D, BIG_NQ, CLUSTER = 45000, 64, 64, 4000
assert BIG_N >= MIN_ROWS


def _mc(metric):
    return OS.METRIC_IP if metric == "COSINE" else OS.METRIC_NEG_L2


def _unit(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1).contiguous()


def _gallery(n, d, seed, metric):
    """unit rows; for L2 times a norm in [0.5, 2], 0.5 + 1.5 sqrt(u): few rows sit at the small norms where the best L2 scores
    of a unit query are, so the filter's band (4 eps wide in s) around a bound with ~500 hits stays inside its 1280 candidates"""
    x = _unit(n, d, seed)
    if metric == "L2":
        u = torch.rand(n, 1, generator=torch.Generator().manual_seed(seed + 1000))
        x = x * (0.5 + 1.5 * u.sqrt())
    return x.contiguous()


def _ids(n):
    return 7 + 3 * torch.arange(n, dtype=torch.int64)


def _index(g, metric, ids=None):
    from mirx.index import FlatIndex
    ix = FlatIndex(g.shape[1], metric, 0)
    if g.shape[0]:
        ix.add(g, _ids(g.shape[0]) if ids is None else ids)
    return ix


def _pad4(x):
    return torch.nn.functional.pad(x, (0, -x.shape[1] % 4))


def _scores(q, g, metric):
    """[nq, n] float64 oracle ranking scores"""
    return OS.scores(_pad4(q).numpy(), _pad4(g).numpy(), _mc(metric))


def _expected(s, ids, lo, hi, allow=None, exclude=None):
    """the definition, in numpy: -> (lims, fp64 scores, ids) with each query's hits ordered by (-s, id)"""
    ids = np.asarray(ids)
    lims, out_s, out_i = [0], [], []
    for i in range(s.shape[0]):
        m = (s[i] > lo) & (s[i] <= hi)
        if allow is not None:
            m &= np.asarray(allow).astype(bool)
        if exclude is not None:
            m &= ids != int(exclude[i])
        idx = np.nonzero(m)[0]
        idx = idx[np.lexsort((ids[idx], -s[i][idx]))]
        out_s.append(s[i][idx])
        out_i.append(ids[idx])
        lims.append(lims[-1] + idx.shape[0])
    return np.asarray(lims, dtype=np.int64), np.concatenate(out_s), np.concatenate(out_i).astype(np.int64)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _run(ix, q, lo, hi=INF, allow=None, exclude=None):
    """both output forms of one range search -> (lims, fp64, fp32, ids) as numpy, after checking that they agree"""
    l1, s64, i1 = ix.range_search(q, lo, hi, exclude_ids=exclude, allow=allow, return_f64=True)
    l2, s32, i2 = ix.range_search(q, lo, hi, exclude_ids=exclude, allow=allow)
    assert s64.dtype == torch.float64 and s32.dtype == torch.float32 and l1.dtype == i1.dtype == torch.int64
    assert torch.equal(l1, l2) and torch.equal(i1, i2)
    return l1.cpu().numpy(), s64.cpu().numpy(), s32.cpu().numpy(), i1.cpu().numpy()


def _check(ix, q, s, ids, metric, lo, hi=INF, allow=None, exclude=None, tag=""):
    """range_search == the definition applied to the oracle scores `s`: ids, fp64 bits, fp32 bits.  -> per-query counts"""
    lims, s64, s32, got = _run(ix, q, lo, hi, allow=allow, exclude=exclude)
    el, es, ei = _expected(s, ids, lo, hi, None if allow is None else allow.cpu().numpy(), exclude)
    np.testing.assert_array_equal(lims, el, err_msg=tag)
    np.testing.assert_array_equal(got, ei, err_msg=tag)
    np.testing.assert_array_equal(_bits(s64), _bits(es), err_msg=tag)
    np.testing.assert_array_equal(_bits(s32), _bits(OS.reported_value(es, _mc(metric)).astype(np.float32)), err_msg=tag)
    assert lims[0] == 0 and (np.diff(lims) >= 0).all() and lims[-1] == got.shape[0]
    return np.diff(lims)


def _same(a, b, tag=""):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(_bits(x) if x.dtype.kind == "f" else x, _bits(y) if y.dtype.kind == "f" else y, err_msg=tag)


def _mid(srow_desc, r):
    """a bound with exactly r entries of the descending row above it (r >= 1): between entries r - 1 and r"""
    a = srow_desc[r - 1]
    b = srow_desc[r] if r < srow_desc.shape[0] else a - 1.0
    return float(b + (a - b) / 2) if b + (a - b) / 2 < a else float(b)


def _filter_answered_all(ix, nq):
    st = ix.range_last_stats()
    assert st["nq"] == nq and st["filter_answered"] == nq and st["exact_answered"] == 0, st
    return st


# ---- 1. exact route, small galleries ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nq", [1, 5, 257])
@pytest.mark.parametrize("d", [8, 130])
@pytest.mark.parametrize("n", [1, 63, 257, 1000])
def test_exact_route_small(n, d, nq, metric):
    g, q, ids = _gallery(n, d, 11 + n, metric), _unit(nq, d, 12 + n), _ids(n)
    s = _scores(q, g, metric)
    ix = _index(g, metric)
    d0 = np.sort(s[0])[::-1]
    counts = set()
    bounds = [float(s.max()) + 1.0, _mid(d0, 1), _mid(d0, min(10, n)), float(s.min()) - 1.0]
    for lo in bounds:
        counts |= set(_check(ix, q, s, ids, metric, lo, tag="lo=%r" % lo).tolist())
    assert {0, n} <= counts and (1 in counts) and (min(10, n) in counts), counts
    st = ix.range_last_stats()
    assert st["exact_answered"] == nq and st["filter_answered"] == 0 and st["hits"] == nq * n, st
    # lo = -inf: every row, in rank_all's order with its scores
    lims, s64, s32, got = _run(ix, q, -INF)
    assert lims.tolist() == [i * n for i in range(nq + 1)]
    r_ids, r_sc = ix.rank_all(q, with_scores=True)
    np.testing.assert_array_equal(got.reshape(nq, n), r_ids.cpu().numpy())
    np.testing.assert_array_equal(_bits(s32.reshape(nq, n)), _bits(r_sc.cpu().numpy()))
    _check(ix, q, s, ids, metric, -INF)
    # hi <= lo: nothing, whatever the scores
    mid = _mid(d0, 1)
    for lo, hi in ((mid, mid), (mid, mid - 1.0), (INF, INF), (-INF, -INF)):
        lims, s64, s32, got = _run(ix, q, lo, hi)
        assert not lims.any() and got.shape == (0,) and s64.shape == (0,) and s32.shape == (0,)
    # a window: hi between the best and the rest of query 0
    _check(ix, q, s, ids, metric, float(s.min()) - 1.0, _mid(d0, 1), tag="window")


@pytest.mark.parametrize("metric", METRICS)
def test_a_query_with_hits_between_two_without(metric):
    n, d = 257, 8
    g, ids = _gallery(n, d, 21, metric), _ids(n)
    far = -g[5:6] if metric == "COSINE" else g[5:6] + 10.0
    q = torch.cat([far, g[5:6], far])
    s = _scores(q, g, metric)
    lo = 0.99 * float(s[1].max()) if metric == "COSINE" else -1e-3
    counts = _check(_index(g, metric), q, s, ids, metric, lo)
    assert counts[0] == 0 and counts[1] >= 1 and counts[2] == 0, counts


# ---- the 45 000-row galleries: rows [0, CLUSTER) lie around one direction, query 0 of the overflow case -----------------
_big_cache = {}


def _big(metric):
    """(gallery, ids, 64 unit queries, their oracle scores, the cluster's centre), built once per metric and left unchanged"""
    if metric not in _big_cache:
        g = _gallery(BIG_N, BIG_D, 31, metric)
        c = _unit(1, BIG_D, 32)
        norms = g[:CLUSTER].norm(dim=1, keepdim=True)
        g[:CLUSTER] = torch.nn.functional.normalize(c + 0.35 * _unit(CLUSTER, BIG_D, 33), dim=1) * norms
        q = _unit(BIG_NQ, BIG_D, 34)
        q = torch.nn.functional.normalize(q - (q @ c.t()) * c, dim=1).contiguous()     # across the cluster: its rows score low
        _big_cache[metric] = (g.contiguous(), _ids(BIG_N), q, _scores(q, g, metric), c)
    return _big_cache[metric]


_big_index_cache = {}


def _big_index(metric):
    if metric not in _big_index_cache:
        _big_index_cache.clear()                                   # one resident 45 000-row index at a time
        _big_index_cache[metric] = _index(_big(metric)[0], metric)
    ix = _big_index_cache[metric]
    ix.set_option(_L().OPT_TIERS, _L().TIER_AUTO)
    return ix


def _dimp(d):
    return (d + DIM_ALIGN - 1) // DIM_ALIGN * DIM_ALIGN


def _eps(qn, gmax, dimp, metric):
    """k_finalize's bound on |s~ - s'| in the GEMM's units (float64 restatement)"""
    e = qn * gmax * (2.0 ** -8 + 2.0 ** -18 + dimp * 2.0 ** -23)
    if metric == "L2":
        e = e + 2.0 ** -23 * (gmax * gmax + qn * gmax)
    return e


def _most_candidates(q, g, s, lo, metric):
    """per query, an upper bound on the rows the filter can admit for `lo`: s' > lo' - 2.1 eps, in the units of s (x 2 for L2)"""
    eps = _eps(q.double().norm(dim=1).numpy(), float(g.double().norm(dim=1).max()), _dimp(g.shape[1]), metric)
    band = 2.1 * eps * (2.0 if metric == "L2" else 1.0)
    return (s > (lo - band)[:, None]).sum(1)


def _pooled_bound(s, hits_per_query):
    """a bound that about hits_per_query entries of every row of s exceed"""
    flat = np.sort(s.reshape(-1))[::-1]
    r = int(hits_per_query * s.shape[0])
    return float((flat[r - 1] + flat[r]) / 2) if r > 0 else float(flat[0]) + 1.0


def _forced_exact(ix, fn):
    ix.set_option(_L().OPT_TIERS, _L().TIER_EXACT_ONLY)
    try:
        return fn()
    finally:
        ix.set_option(_L().OPT_TIERS, _L().TIER_AUTO)


# ---- 2. boundaries: a bound that IS a row's score; identical rows -----------------------------------------------------
@pytest.mark.parametrize("route", ["exact", "filter"])
@pytest.mark.parametrize("metric", METRICS)
def test_bounds_that_equal_a_score_and_identical_rows(metric, route):
    if route == "exact":
        g, ids = _gallery(1000, 130, 41, metric), _ids(1000)
    else:
        g, ids = _big(metric)[0].clone(), _big(metric)[1]
    # the row the middle query sits next to: for the filter route the shortest row outside the cluster, so that for L2 the
    # bound lies where the two unit queries beside it have no hits at all
    src, twin = (3 if route == "exact" else CLUSTER + int(g[CLUSTER:-300].norm(dim=1).argmin())), g.shape[0] - 300
    g[twin] = g[src]                                               # two rows with one vector
    d = g.shape[1]
    q = torch.cat([_unit(1, d, 42), g[src:src + 1] + 0.02 * _unit(1, d, 43), _unit(1, d, 44)])
    s = _scores(q, g, metric)
    order = np.lexsort((ids.numpy(), -s[1]))
    assert s[1][order[0]] == s[1][order[1]] and order[:2].tolist() == [src, twin]
    lo, hi = float(s[1][order[5]]), float(s[1][order[2]])
    assert s[1][order[6]] < lo < hi < s[1][order[1]]
    if route == "filter":
        assert _most_candidates(q, g, s, np.full(3, lo), metric).max() <= RANGE_CAP
    ix = _index(g, metric)
    # lo is exactly row order[5]'s score: it is out (lo < s), the next better one is the last hit
    _check(ix, q, s, ids, metric, lo)
    if route == "filter":
        _filter_answered_all(ix, 3)
    lims, s64, s32, got = _run(ix, q, lo)
    mine = got[lims[1]:lims[2]].tolist()
    assert mine == ids.numpy()[order[:5]].tolist() and mine[:2] == [int(ids[src]), int(ids[twin])]
    # hi is exactly row order[2]'s score: it is in (s <= hi), the twins above it are out
    _check(ix, q, s, ids, metric, lo, hi)
    lims, s64, s32, got = _run(ix, q, lo, hi)
    assert got[lims[1]:lims[2]].tolist() == ids.numpy()[order[2:5]].tolist()
    if route == "filter":
        _filter_answered_all(ix, 3)
        _same(_forced_exact(ix, lambda: _run(ix, q, lo, hi)), (lims, s64, s32, got))


# ---- 3. filter route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_filter_route(metric):
    g, ids, q, s, _ = _big(metric)
    ix = _big_index(metric)
    for per_query in (0, 10, 500):
        lo = _pooled_bound(s, per_query)
        assert _most_candidates(q, g, s, np.full(BIG_NQ, lo), metric).max() <= RANGE_CAP       # the filter can answer
        counts = _check(ix, q, s, ids, metric, lo, tag="%d per query" % per_query)
        st = _filter_answered_all(ix, BIG_NQ)
        assert st["hits"] == counts.sum() and st["candidates"] >= st["hits"], st
        assert abs(counts.mean() - per_query) <= 0.01 * per_query + 1e-9, counts.mean()
        got = _run(ix, q, lo)
        _same(_forced_exact(ix, lambda: _run(ix, q, lo)), got, tag="forced exact, %d per query" % per_query)
        st = ix.range_last_stats()
        assert st["exact_answered"] == BIG_NQ and st["filter_answered"] == 0, st
    # a mask, the excluded id and an upper bound on the filter route: plain tests at emission
    lo, hi = _pooled_bound(s, 500), _pooled_bound(s, 3)
    allow = torch.rand(BIG_N, generator=torch.Generator().manual_seed(35)) < 0.5
    ex = ids.numpy()[np.argmax(s, axis=1)]                         # each query's best row
    for am in (allow, allow.to("cuda:0")):
        _check(ix, q, s, ids, metric, lo, hi, allow=am, exclude=ex, tag="masked")
        _filter_answered_all(ix, BIG_NQ)


# ---- 4. overflow fallback --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_overflow_falls_back_to_the_exact_route(metric):
    g, ids, q, _, c = _big(metric)
    q = torch.cat([q[:3], c, q[3:8]])                              # query 3 is the cluster's centre
    s = _scores(q, g, metric)
    lo = _mid(np.sort(s[3])[::-1], RANGE_CAP + 220)                # 1500 true hits: more than the candidate lists hold
    most = _most_candidates(q, g, s, np.full(q.shape[0], lo), metric)
    assert (np.delete(most, 3) <= RANGE_CAP // 2).all(), most
    ix = _big_index(metric)
    counts = _check(ix, q, s, ids, metric, lo)
    assert counts[3] == RANGE_CAP + 220
    st = ix.range_last_stats()
    assert st["filter_answered"] == q.shape[0] - 1 and st["exact_answered"] == 1 and st["hits"] == counts.sum(), st
    _same(_forced_exact(ix, lambda: _run(ix, q, lo)), _run(ix, q, lo))


@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("metric", METRICS)
def test_range_cap_hits_and_one_past(metric, over):
    """RANGE_CAP (+ 1) identical rows that equal query 0, lo between their score and every other row's, outside the filter's
    band.  The rows are laid out on k_gemm.hip's plan for one 64-query tile (phase ph walks the gallery tiles ph, ph + nph, ..;
    wave row wm of a tile's 256 rows feeds region ph * 8 + wm) so that no region receives more than its slots: the overflow
    list stays empty and RANGE_CAP hits are exactly what the filter route holds; one more and the exact route answers the
    query, with the full count.  The stats assert which route answered."""
    g, ids = _big(metric)[0].clone(), _big(metric)[1]
    run = RANGE_CAP + over
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nph = min(cus // 8 * 8, (BIG_N + 255) // 256)
    slots = min(64, max(8, 2048 // (nph * 8)))                         # k_gemm.hip: region_slots()
    r = np.arange(BIG_N)
    region = ((r // 256) % nph) * 8 + (r % 256) // 32
    rank_in_region = np.zeros(BIG_N, dtype=np.int64)
    order = np.argsort(region, kind="stable")
    starts = np.r_[0, np.cumsum(np.bincount(region))[:-1]]
    rank_in_region[order] = np.arange(BIG_N) - starts[region[order]]
    rows = np.nonzero(rank_in_region < slots)[0][:run]                 # at most `slots` rows of every region, lowest rows first
    assert rows.shape[0] == run and np.bincount(region[rows]).max() <= slots
    v = _unit(1, BIG_D, 36)
    g[torch.as_tensor(rows)] = v
    q = torch.cat([v, _big(metric)[2][:2]])
    s = _scores(q, g, metric)
    top = np.sort(s[0])[::-1]
    assert top[run - 1] == top[0] and top[run] < top[0]
    lo = _mid(top, run)
    assert _most_candidates(q, g, s, np.full(3, lo), metric).tolist() == [run, 0, 0]      # nothing else inside the band
    ix = _index(g, metric)
    counts = _check(ix, q, s, ids, metric, lo)
    assert counts.tolist() == [run, 0, 0]
    st = ix.range_last_stats()
    if over == 0:
        assert st["filter_answered"] == 3 and st["exact_answered"] == 0 and st["hits"] == st["candidates"] == run, st
    else:
        assert st["filter_answered"] == 2 and st["exact_answered"] == 1 and st["hits"] == run, st


# ---- 5. the eps margin -----------------------------------------------------------------------------------------------
def _bf16(x):
    bits = OS.to_bf16_bits(x.numpy()).astype(np.uint32) << 16
    return torch.from_numpy(bits.view(np.float32).reshape(x.shape).copy())


def _bf16_ulp(v):
    e = (v.numpy().view(np.uint32) >> 23) & 0xFF
    return torch.from_numpy(np.ldexp(1.0, e.astype(np.int64) - 127 - 7).astype(np.float32))


@pytest.mark.parametrize("metric", METRICS)
def test_planted_row_inside_the_eps_margin(metric):
    """Per query a planted row B (row B of tests/test_search_filter_edges_gpu.py's bf16-swap case: the query is bf16-exact,
    v = bf16(c q), B = v + 0.4 ulp towards q, which rounds back to v) whose true score is just above lo while the filter,
    which sees v, scores it 0.2 to 0.6 eps BELOW lo' (lo in the GEMM's units).  It must be returned, by the filter route: that
    takes the threshold eps below lo'.  A zero-width margin (tau = lo') loses it -- verified once on a scratch build with eps
    and the fp64 term set to zero, recorded in DESIGN 33."""
    n, d, nq = 40000, 256, 8
    c = 0.9 if metric == "COSINE" else 1.8                         # |B| ~ c: inside the L2 galleries' norms [0.5, 2]
    gen = torch.Generator().manual_seed(701)
    q = _bf16(torch.randn(nq, d, generator=gen) / d ** 0.5)
    v = _bf16(c * q)
    assert (v != 0).all()
    b = v + 0.4 * torch.sign(q) * _bf16_ulp(v)
    assert torch.equal(_bf16(b), v) and not torch.equal(b, v)
    g = _gallery(n, d, 702, metric)
    pos = (np.arange(nq) * 1237 + 5) % n
    g[torch.as_tensor(pos)] = b
    ids = _ids(n)
    s = _scores(q, g, metric)
    ix = _index(g, metric)
    q64, b64, v64 = q.double(), b.double(), v.double()
    gmax = float(g.double().norm(dim=1).max())
    for i in range(nq):
        s_b = float(s[i, pos[i]])
        lo = float(np.nextafter(s_b, -INF))
        assert s_b > lo                                            # the truth: a hit, by one ulp
        eps = _eps(float(q64[i].norm()), gmax, _dimp(d), metric)
        f_b = float(q64[i] @ v64[i])                               # the filter's view: bf16 operands ...
        lop = lo
        if metric == "L2":
            f_b -= 0.5 * float(b64[i] @ b64[i])                    # ... and the bias of the fp32 row
            lop = 0.5 * (lo + float(q64[i] @ q64[i]))
        assert 0.2 * eps <= lop - f_b <= 0.6 * eps, (lop - f_b) / eps
        counts = _check(ix, q[i:i + 1], s[i:i + 1], ids, metric, lo, tag="query %d" % i)
        lims, s64, s32, got = _run(ix, q[i:i + 1], lo)
        assert int(ids[pos[i]]) in got.tolist() and counts[0] >= 1
        _filter_answered_all(ix, 1)


# ---- 6. mask and exclusion: a self-join -------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_self_join_under_a_mask(metric):
    n, d = 300, 32
    g, ids = _gallery(n, d, 61, metric), _ids(n)
    s = _scores(g, g, metric)
    ix = _index(g, metric)
    lo = _pooled_bound(s, 12)
    own = ids.numpy()
    allow = torch.rand(n, generator=torch.Generator().manual_seed(62)) < 0.5
    plain = _check(ix, g, s, ids, metric, lo, exclude=own, tag="self-join")
    assert plain.sum() > 0 and not (_run(ix, g, lo, exclude=own)[3] == np.repeat(own, plain)).any()    # no row finds itself
    fresh = _index(g[allow], metric, ids[allow])
    want = _run(fresh, g, lo, exclude=own)
    for am in (allow, allow.to("cuda:0"), allow.numpy()):
        _check(ix, g, s, ids, metric, lo, allow=am if torch.is_tensor(am) else torch.from_numpy(am), exclude=own, tag="masked")
        _same(_run(ix, g, lo, allow=am, exclude=own), want, tag="fresh index of the allowed rows")
    ones, zeros = torch.ones(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    _same(_run(ix, g, lo, allow=ones, exclude=own), _run(ix, g, lo, exclude=own))
    lims, s64, s32, got = _run(ix, g, -INF, allow=zeros)
    assert not lims.any() and got.shape == (0,)
    with pytest.raises(ValueError):
        ix.range_search(g, lo, allow=ones[:-1])
    with pytest.raises(ValueError):
        ix.range_search(g, float("nan"))


@pytest.mark.parametrize("metric", METRICS)
def test_exact_route_agrees_with_rank_top(metric):
    """The two callers of the radix ranking, on the shared case of tests/test_search_masked_gpu.py (three sort tiles and a tail,
    ids in no order): with no bounds the exact route's hits of a query are the finite prefix of rank_top(k = n) under the same
    mask and excluded ids -- ids and fp64 scores identical, in order -- and each query has as many as it has eligible rows."""
    from test_search_masked_gpu import rank_top_case
    g, ids, q, own, masks = rank_top_case(metric)
    n = g.shape[0]
    ix = _index(g, metric, ids)
    for name, allow in masks.items():
        for ex in (None, own):
            tag = (metric, name, ex is not None)
            lims, s64, got = _forced_exact(ix, lambda: ix.range_search(q, -INF, INF, exclude_ids=ex, allow=allow, return_f64=True))
            ws, wi = ix.rank_top(q, n, exclude_ids=ex, return_f64=True, allow=allow)
            lims, s64, got, ws, wi = (t.cpu().numpy() for t in (lims, s64, got, ws, wi))
            eligible = [int(allow.sum()) - (int(allow[ids == e].any()) if ex is not None else 0) for e in own]
            np.testing.assert_array_equal(np.diff(lims), eligible, err_msg=str(tag))
            assert lims[0] == 0 and lims[-1] == got.shape[0], tag
            for i in range(q.shape[0]):
                finite = wi[i] != -1
                assert finite[:eligible[i]].all() and not finite[eligible[i]:].any(), tag
                np.testing.assert_array_equal(got[lims[i]:lims[i + 1]], wi[i][finite], err_msg=str(tag))
                np.testing.assert_array_equal(_bits(s64[lims[i]:lims[i + 1]]), _bits(ws[i][finite]), err_msg=str(tag))


# ---- 7. more than one internal batch ----------------------------------------------------------------------------------
def test_more_than_one_internal_batch():
    metric = "COSINE"
    g, ids, q64, s64q, _ = _big(metric)
    nq = QUERY_BATCH + 8
    q = _unit(nq, BIG_D, 71)
    lo = _pooled_bound(s64q, 5)                                    # the 64 cached queries stand for the 8200: same distribution
    ix = _big_index(metric)
    got = _run(ix, q, lo)
    lims = got[0]
    assert lims.shape == (nq + 1,) and lims[0] == 0 and (np.diff(lims) >= 0).all() and lims[-1] == got[3].shape[0]
    st = ix.range_last_stats()
    assert st["nq"] == nq and st["filter_answered"] + st["exact_answered"] == nq and st["hits"] == lims[-1], st
    assert st["filter_answered"] >= 0.99 * nq, st
    assert 2 * nq <= lims[-1] <= 10 * nq                           # about 5 per query
    _same(_forced_exact(ix, lambda: _run(ix, q, lo)), got)
    pick = [0, QUERY_BATCH - 1, QUERY_BATCH, nq - 1]
    el, es, ei = _expected(_scores(q[pick], g, metric), ids, lo, INF)
    for j, qi in enumerate(pick):
        a, b = lims[qi], lims[qi + 1]
        np.testing.assert_array_equal(got[3][a:b], ei[el[j]:el[j + 1]])
        np.testing.assert_array_equal(_bits(got[1][a:b]), _bits(es[el[j]:el[j + 1]]))


# ---- 8. limit and state ------------------------------------------------------------------------------------------------
def test_hit_limit_and_call_order():
    import ctypes
    from mirx._lib import MirxError
    L = _L()
    n, d = 257, 16
    g, ids, q = _gallery(n, d, 81, "COSINE"), _ids(n), _unit(1, d, 82)
    s = _scores(q, g, "COSINE")
    d0 = np.sort(s[0])[::-1]
    ix = _index(g, "COSINE")
    ix.set_option(L.OPT_RANGE_MAX_HITS, 100)
    with pytest.raises(MirxError, match=r"\(-2\).*more hits"):
        ix.range_search(q, _mid(d0, 101))
    sc, got = ix.search(q, 5, return_f64=True)                     # the index is untouched and usable
    np.testing.assert_array_equal(got.cpu().numpy()[0], ids.numpy()[np.lexsort((ids.numpy(), -s[0]))[:5]])
    assert _check(ix, q, s, ids, "COSINE", _mid(d0, 100))[0] == 100
    ix.set_option(L.OPT_RANGE_MAX_HITS, 0)
    assert _check(ix, q, s, ids, "COSINE", _mid(d0, 101))[0] == 101
    # fetch needs the range search right before it
    out = torch.empty(101, dtype=torch.float32, device="cuda:0"), torch.empty(101, dtype=torch.int64, device="cuda:0")
    fetch = lambda: ix._lib.mirx_index_range_fetch(ix._h, ctypes.c_void_p(out[0].data_ptr()), None,
                                                   ctypes.c_void_p(out[1].data_ptr()), None)
    assert fetch() == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[1].cpu().numpy(), _expected(s, ids, _mid(d0, 101), INF)[2])
    ix.search(q, 5)
    assert fetch() == L.ESTATE and b"range_fetch" in ix._lib.mirx_last_error()
    fresh = _index(g, "COSINE")
    assert fresh._lib.mirx_index_range_fetch(fresh._h, ctypes.c_void_p(out[0].data_ptr()), None,
                                             ctypes.c_void_p(out[1].data_ptr()), None) == L.ESTATE
    # not between search_begin and search_end
    h = ix.search_begin(q, 5)
    with pytest.raises(MirxError, match=r"\(-4\)"):
        ix.range_search(q, _mid(d0, 10))
    ix.search_end(h)
    assert _check(ix, q, s, ids, "COSINE", _mid(d0, 10))[0] == 10
    # limits are checked on the host: a mask of the wrong length, a negative query count
    lims, total = torch.zeros(2, dtype=torch.int64, device="cuda:0"), ctypes.c_int64(0)
    qd = q.to("cuda:0")
    bad_mask = torch.ones(n - 1, dtype=torch.uint8, device="cuda:0")
    rc = ix._lib.mirx_index_range_search(ix._h, ctypes.c_void_p(qd.data_ptr()), 1, 0.0, 1.0, None,
                                         ctypes.c_void_p(bad_mask.data_ptr()), n - 1, ctypes.c_void_p(lims.data_ptr()),
                                         ctypes.byref(total), None)
    assert rc == -1 and b"n_allow" in ix._lib.mirx_last_error()
    rc = ix._lib.mirx_index_range_search(ix._h, ctypes.c_void_p(qd.data_ptr()), -1, 0.0, 1.0, None, None, 0,
                                         ctypes.c_void_p(lims.data_ptr()), ctypes.byref(total), None)
    assert rc == -1 and b"nq" in ix._lib.mirx_last_error()


# ---- 9. Collection level -------------------------------------------------------------------------------------------------
def _pairs(hits):
    return [(h.id, h.distance) for h in hits]


def _labels(n):
    return ["COVID-19" if (i * 7 + i // 11) % 3 == 0 else "Normal" for i in range(n)]


def _collection_checks(col, emb, labels, metric):
    """range_search against the oracle (ids = row numbers), search(param=radius) against range_search"""
    from mirx.index import range_bounds
    n = emb.shape[0]
    live = col.live_ids()
    q = emb[[3, 150]] + 0.05 * _unit(2, emb.shape[1], 92)
    s = _scores(q, emb[torch.as_tensor(live)], metric)
    d0 = np.sort(s[0])[::-1]
    s20 = _mid(d0, 20)
    radius = s20 if metric == "COSINE" else math.sqrt(-s20)        # Euclidean units for L2
    lo, hi = range_bounds(metric, radius)
    el, es, ei = _expected(s, live, lo, hi)
    res = col.range_search(q, radius, output_fields=["label", "image_path"])
    assert [[h.id for h in hits] for hits in res] == [ei[el[i]:el[i + 1]].tolist() for i in range(2)]
    assert 15 <= len(res[0]) <= 25
    rep = OS.reported_value(es, _mc(metric)).astype(np.float32)
    want_d = [float(v) if metric == "COSINE" else float(-v) for v in rep]
    assert [h.distance for hits in res for h in hits] == want_d
    assert all(h.entity.get("label") == labels[h.id] and h.entity.get("image_path") == f"img/{h.id}.png" for hits in res for h in hits)
    for param in ({"params": {"radius": radius}}, {"radius": radius}, {"metric_type": metric, "params": {"radius": radius, "nprobe": 10}}):
        top = col.search(q, param=param, limit=5, output_fields=["label"])
        assert [_pairs(h) for h in top] == [_pairs(h[:5]) for h in res], param
        assert all(h.entity.get("label") == labels[h.id] for hits in top for h in hits)
    # a limit above query 0's number of hits: all of them
    assert [_pairs(h) for h in col.search(q, param={"params": {"radius": radius}}, limit=200)] == [_pairs(h[:200]) for h in res]
    # a range_filter that leaves the best hit out
    best = res[0][0]
    second = res[0][1]
    rf = (best.distance + second.distance) / 2
    assert min(best.distance, second.distance) < rf < max(best.distance, second.distance)
    win = col.range_search(q[:1], radius, rf)
    assert _pairs(win[0]) == _pairs(res[0][1:])
    top = col.search(q[:1], param={"params": {"radius": radius, "range_filter": rf}}, limit=5)
    assert _pairs(top[0]) == _pairs(res[0][1:6])
    # the scalar filter and the excluded id
    expr = 'label == "COVID-19"'
    only = col.range_search(q, radius, expr=expr, output_fields=["label"])
    assert [_pairs(h) for h in only] == [[p for p in _pairs(h) if labels[p[0]] == "COVID-19"] for h in res]
    assert [_pairs(h) for h in col.search(q, param={"params": {"radius": radius}}, limit=5, expr=expr)] == [_pairs(h[:5]) for h in only]
    ex = [res[0][0].id, res[1][0].id]
    less = col.range_search(q, radius, exclude_ids=ex)
    assert [_pairs(h) for h in less] == [_pairs(h[1:]) for h in res]
    assert [_pairs(h) for h in col.search(q, param={"params": {"radius": radius}}, limit=5, exclude_ids=ex)] == [_pairs(h[:5]) for h in less]
    # without a radius param is ignored, as before
    assert [_pairs(h) for h in col.search(q, param={"params": {"nprobe": 10}}, limit=5)] == [_pairs(h) for h in col.search(q, limit=5)]
    return q, radius, res


@pytest.mark.parametrize("metric", METRICS)
def test_collection_range_search(metric):
    from mirx.retriever import Collection
    n, dim = 300, 32
    emb, labels = _gallery(n, dim, 91, metric), _labels(n)
    col = Collection("c", dim, metric_type=metric)
    col.insert([[f"img/{i}.png" for i in range(n)], labels, emb])
    q, radius, res = _collection_checks(col, emb, labels, metric)
    gone = res[0][2].id
    col.delete("id in [%d]" % gone)
    after = col.range_search(q, radius)
    assert [_pairs(h) for h in after] == [[p for p in _pairs(h) if p[0] != gone] for h in res]
    _collection_checks(col, emb, labels, metric)
    with pytest.raises(ValueError):
        col.range_search(q, radius, radius)                        # range_filter == radius: refused for both metrics


def test_persistent_collection_range_search(tmp_path):
    from mirx.retriever import MilvusManager
    n, dim = 300, 512
    emb, labels = _gallery(n, dim, 95, "COSINE"), _labels(n)
    uri = str(tmp_path / "db")
    col = MilvusManager(uri=uri).create_collection("dinov2")
    col.insert([[f"img/{i}.png" for i in range(n)], labels, emb])
    col.delete("id in [7, 150]")
    col.flush()
    again = MilvusManager(uri=uri).create_collection("dinov2")
    assert again._index is None                                     # loads on first use
    _collection_checks(again, emb, labels, "COSINE")
