"""The deep search route (FlatIndex.search_deep, mirx_index_search_deep): k (+1 with excluded ids) past TIER1_MAX_K on the
filter GEMM, with candidate lists of DEEP_CAP rows.  GPU only.

Bar of every result case (tests/test_search_filter_edges_gpu.py's `_check`): ids equal oracle.search.topk's, fp64 ranking scores
bit-identical, fp32 values equal to the rounded oracle value for both return forms, and the route asserted from last_stats().
Where a case says "the deep filter must answer", a float64 host precondition comes first, before the GPU is touched: the rows
within 4 eps of the k_eff-th best true score number at most DEEP_CAP (2 eps of guard band around a k-th best that the filter
may have moved by eps, read through scores that are off by eps again).  The gallery sizes follow deep_min_rows, restated here
from the constants in the sources."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import search as OS

pytestmark = pytest.mark.gpu

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-retrieval---thesis-2026_amd", "csrc")


def _constexpr(fname, name):
    """The value of `constexpr int[64_t] NAME = <int>;` in csrc/FNAME: the test follows the library's capacities."""
    with open(os.path.join(_CSRC, fname)) as f:
        m = re.search(r"constexpr\s+(?:int|int64_t)\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    assert m, (fname, name)
    return int(m.group(1))


MIN_ROWS = _constexpr("mirx_api.hip", "TIER1_MIN_ROWS")
MAX_K = _constexpr("mirx_api.hip", "TIER1_MAX_K")
DEEP_CAP = _constexpr("mirx_common.h", "DEEP_CAP")
DIM_ALIGN = _constexpr("mirx_common.h", "DIM_ALIGN")
METRICS = {"COSINE": 0, "IP": 0, "L2": 1}


def deep_min_rows(k_eff, nq):
    target = _constexpr("mirx_common.h", "DEEP_TARGET_MUL") * k_eff + _constexpr("mirx_common.h", "DEEP_TARGET_ADD")
    tile = 64 if nq <= 64 else (128 if nq <= 128 else 256)
    return max(MIN_ROWS, target * _constexpr("mirx_common.h", "DEEP_GROUP_ROWS") // (8 // (tile // 64)))


def _ragged(rows):
    """the smallest multiple of 256 that holds `rows`, plus 257: a ragged last gallery tile"""
    return (rows + 255) // 256 * 256 + 257


def _unit(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)


def _dimp(d):
    return (d + DIM_ALIGN - 1) // DIM_ALIGN * DIM_ALIGN


def _true_scores(q, g, metric):
    """[nq, n] float64: q.g, for L2 q.g - |g|^2 / 2 (what the filter GEMM approximates in bf16 x bf16 + fp32 bias)"""
    q64 = q.double()
    out = torch.empty(q.shape[0], g.shape[0], dtype=torch.float64)
    for c0 in range(0, g.shape[0], 8192):
        gc = g[c0:c0 + 8192].double()
        s = q64 @ gc.t()
        if metric == 1:
            s -= 0.5 * (gc * gc).sum(1)[None]
        out[:, c0:c0 + 8192] = s
    return out


def _norms(x):
    return torch.cat([x[c0:c0 + 8192].double().norm(dim=1) for c0 in range(0, x.shape[0], 8192)])


def _eps(qn, gn, dimp, metric):
    """the finalize kernels' bound on |s~ - s| with `gn` in the place of gnorm_max"""
    e = qn * gn * (2.0 ** -8 + 2.0 ** -18 + dimp * 2.0 ** -23)
    if metric == 1:
        e = e + 2.0 ** -23 * (gn * gn + qn * gn)
    return e


def _admitted(q, g, k_eff, metric, s=None):
    """per query: rows with s >= kth(s) - 4 eps, the most the second-chance filter pass can admit"""
    s = _true_scores(q, g, metric) if s is None else s
    eps = _eps(_norms(q), _norms(g).max(), _dimp(g.shape[1]), metric)
    kth = s.topk(k_eff, dim=1).values[:, -1]
    return (s >= (kth - 4.0 * eps)[:, None]).sum(1)


def _bf16(x):
    bits = OS.to_bf16_bits(x.numpy()).astype(np.uint32) << 16
    return torch.from_numpy(bits.view(np.float32).reshape(x.shape).copy())


def _index(d, metric, g, ids=None):
    from mirx.index import FlatIndex
    ix = FlatIndex(d, metric, 0)
    ix.add(g, ids)
    return ix


def _route(st, nq, deep_must_answer=False):
    assert st["nq"] == nq and st["tier1_answered"] + st["exact_answered"] == nq, st
    if deep_must_answer:
        assert st["tier1_answered"] >= 0.9 * nq, st


def _check(index, q, k, metric, gallery, exclude=None, ids=None, deep_must_answer=False, allow=None):
    """both return forms of search_deep against the oracle; -> (stats of the last call, oracle scores, oracle ids)"""
    nq = q.shape[0]
    sc64, got_ids = index.search_deep(q, k, exclude_ids=exclude, return_f64=True, allow=allow)
    st64 = index.last_stats()
    sc32, got_ids2 = index.search_deep(q, k, exclude_ids=exclude, allow=allow)
    st32 = index.last_stats()
    print("deep k=%d nq=%d %s %s" % (k, nq, st64, st32))
    o_s, o_i = OS.topk(q.numpy(), gallery.numpy(), k, metric=metric, exclude=None if exclude is None else np.asarray(exclude),
                       ids=ids)
    np.testing.assert_array_equal(got_ids.cpu().numpy(), o_i)
    np.testing.assert_array_equal(got_ids2.cpu().numpy(), o_i)
    np.testing.assert_array_equal(sc64.cpu().numpy(), o_s)               # bit-identical fp64
    np.testing.assert_array_equal(sc32.cpu().numpy(), OS.reported_value(o_s, metric).astype(np.float32))
    _route(st64, nq, deep_must_answer)
    _route(st32, nq, deep_must_answer)
    return st32, o_s, o_i


# ---- shared data: one unit gallery of width 64, the perturbed-row queries -------------------------------------------------
_D = 64
_cache = {}


def _gallery(rows):
    """the first `rows` rows of one unit-normal gallery (grown on demand, so every case sees the same leading rows)"""
    have = _cache.get("g")
    if have is None or have.shape[0] < rows:
        _cache["g"] = _unit(max(rows, _ragged(deep_min_rows(101, 300)), _ragged(deep_min_rows(1025, 64))), _D, 3701)
    return _cache["g"][:rows]


def _perturbed(g, nq, seed):
    """nq queries near gallery rows spread over the tile positions -> (queries, the rows)"""
    rows = (np.arange(nq) * 977 + 3) % g.shape[0]
    gen = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(g[rows] + 0.5 / g.shape[1] ** 0.5 * torch.randn(nq, g.shape[1], generator=gen), dim=1)
    return q, rows


# ---- 1. natural threshold: the deep filter must answer --------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("k", [65, 100, 256, 1000, 1024])
def test_natural_threshold_deep_filter_answers(k, metric):
    mc, nq = METRICS[metric], 48
    g = _gallery(_ragged(deep_min_rows(k + 1, nq)))
    q, rows = _perturbed(g, nq, 3702)
    s = _true_scores(q, g, mc)
    worst = max(int(_admitted(q, g, k, mc, s).max()), int(_admitted(q, g, k + 1, mc, s).max()))
    print("rows within 4 eps of the k-th score, at most %d of %d" % (worst, DEEP_CAP))
    assert worst <= DEEP_CAP, worst
    ix = _index(_D, metric, g)
    _check(ix, q, k, mc, g, deep_must_answer=True)
    _, _, o_i = _check(ix, q, k, mc, g, exclude=rows, deep_must_answer=True)
    assert not np.any(o_i == rows[:, None])


# ---- 2. the query tiles and their boundaries -------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("nq", [63, 64, 65, 129, 300])
def test_query_counts_around_the_query_tiles(nq, metric):
    """63 / 64 queries on the 64-query tile, 65 on the 128-query tile, 129 and 300 (one full tile and a ragged one) on the
    256-query tile, each at the smallest gallery its tile's deep_min_rows lets in"""
    mc, k = METRICS[metric], 100
    g = _gallery(_ragged(deep_min_rows(k + 1, nq)))
    q, rows = _perturbed(g, nq, 3703)
    s = _true_scores(q, g, mc)
    worst = max(int(_admitted(q, g, k, mc, s).max()), int(_admitted(q, g, k + 1, mc, s).max()))
    assert worst <= DEEP_CAP, worst
    ix = _index(_D, metric, g)
    _check(ix, q, k, mc, g, deep_must_answer=True)
    if nq <= 65:
        _check(ix, q, k, mc, g, exclude=rows, deep_must_answer=True)


# ---- 3. route boundaries ----------------------------------------------------------------------------------------------------
def test_k_at_the_filter_cap_is_handed_to_search():
    mc, nq = 0, 32
    g = _gallery(_ragged(deep_min_rows(MAX_K + 1, nq)))
    q, rows = _perturbed(g, nq, 3704)
    ix = _index(_D, "COSINE", g)
    for k, ex in ((MAX_K, None), (MAX_K - 1, rows)):
        want = ix.search(q, k, exclude_ids=ex, return_f64=True)
        st_want = ix.last_stats()
        got = ix.search_deep(q, k, exclude_ids=ex, return_f64=True)
        st_got = ix.last_stats()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert st_got == st_want and st_got["tier1_answered"] > 0, (st_got, st_want)


@pytest.mark.parametrize("k,excl", [(MAX_K + 1, False), (MAX_K, True)])
def test_k_eff_one_past_the_filter_cap_is_deep_answered(k, excl):
    mc, nq = 0, 32
    g = _gallery(_ragged(deep_min_rows(MAX_K + 1, nq)))
    q, rows = _perturbed(g, nq, 3705)
    assert int(_admitted(q, g, MAX_K + 1, mc).max()) <= DEEP_CAP
    ix = _index(_D, "COSINE", g)
    st, _, _ = _check(ix, q, k, mc, g, exclude=rows if excl else None, deep_must_answer=True)
    ix.search(q, k, exclude_ids=rows if excl else None)               # the same request through search: the exact scan, as before
    assert ix.last_stats()["tier1_answered"] == 0


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_gallery_size_boundary_and_exact_only(metric):
    from mirx import _lib as L
    mc, nq, k = METRICS[metric], 32, 100
    rows_min = deep_min_rows(k, nq)
    g = _gallery(rows_min)
    q, _ = _perturbed(g, nq, 3706)
    assert int(_admitted(q, g, k, mc).max()) <= DEEP_CAP
    ix = _index(_D, metric, g[:rows_min - 1])
    st, _, _ = _check(ix, q, k, mc, g[:rows_min - 1])
    assert st["tier1_answered"] == 0 and st["exact_answered"] == nq, st
    ix.add(g[rows_min - 1:rows_min])
    st, _, _ = _check(ix, q, k, mc, g)
    assert st["tier1_answered"] > 0, st
    ix.set_option(L.OPT_TIERS, L.TIER_EXACT_ONLY)
    try:
        st, _, _ = _check(ix, q, k, mc, g)
    finally:
        ix.set_option(L.OPT_TIERS, L.TIER_AUTO)
    assert st["tier1_answered"] == 0 and st["exact_answered"] == nq, st


# ---- 4. capacity, with a forced threshold -----------------------------------------------------------------------------------
def _runs(run, k_eff, nq):
    """base unit vectors of width 256, each repeated `run` times, enough of them for deep_min_rows; queries = base vectors"""
    d = 256
    nbase = -(-deep_min_rows(k_eff, nq) // run)
    base = _unit(nbase, d, 3707)
    dots = (base.double() @ base.double().t()).fill_diagonal_(-1)
    eps = 2.0 ** -8 + 2.0 ** -18 + _dimp(d) * 2.0 ** -23
    assert float(dots.max()) < 0.5 - 4 * eps                           # nothing but the query's own run passes 0.5
    qi = (torch.arange(nq) * 5) % nbase
    return d, base.repeat_interleave(run, dim=0), base[qi], qi


@pytest.mark.parametrize("over", [0, 1])
def test_capacity_at_and_one_past_deep_cap(over):
    """tau forced to 0.5: a query equal to a base vector admits exactly its run of identical rows, which tie in the filter and in
    fp64, so the answer is the run's lowest ids.  run = DEEP_CAP fills the candidate list to the last entry and every one is
    re-scored; run = DEEP_CAP + 1 is one past what the route holds (the regions and the overflow list feed the one list of
    DEEP_CAP keys) and goes to the exact scan."""
    from mirx import _lib as L
    nq, k, run = 8, 1024, DEEP_CAP + over
    d, g, q, qi = _runs(run, k, nq)
    ix = _index(d, "COSINE", g)
    ix.set_option(L.OPT_FORCE_TAU, int(np.float32(0.5).view(np.uint32)))
    first = (qi * run).numpy()
    st, _, o_i = _check(ix, q, k, 0, g)
    np.testing.assert_array_equal(o_i, first[:, None] + np.arange(k)[None, :])     # all `run` rows tie: the k lowest ids
    if over == 0:
        assert st["candidates"] == nq * run and st["reranked"] == nq * run, st
        assert st["overflowed"] == 0 and st["incomplete"] == 0 and st["tier1_answered"] == nq, st
    else:
        assert st["overflowed"] == nq and st["exact_answered"] == nq and st["tier1_answered"] == 0, st
    # k = 1023 with the run's first id excluded: k_eff = 1024, the ids start one later
    st, _, o_i = _check(ix, q, k - 1, 0, g, exclude=first)
    np.testing.assert_array_equal(o_i, first[:, None] + 1 + np.arange(k - 1)[None, :])
    assert (st["tier1_answered"] == nq) if over == 0 else (st["exact_answered"] == nq), st


def _lay_out(region, pool, slots, total, surplus):
    """`total` rows out of `pool` of which exactly `surplus` exceed their regions' `slots` and reach the overflow list
    (tests/test_search_filter_edges_gpu.py's layout): regions are saturated one after the other, then filled"""
    by_region = {}
    for r in pool:
        by_region.setdefault(int(region[r]), []).append(int(r))
    rows, left = [], surplus
    for rg in sorted(by_region):
        have = by_region[rg]
        if len(rows) == total:
            break
        if left > 0:
            take = min(len(have), slots + left, total - len(rows))
            left -= max(take - slots, 0)
        else:
            take = min(len(have), slots, total - len(rows))
        rows += have[:take]
    assert len(rows) == total and left == 0, (len(rows), left)
    rows = np.sort(np.asarray(rows))
    assert int(np.maximum(np.bincount(region[rows]) - slots, 0).sum()) == surplus
    return rows


@pytest.mark.parametrize("over", [0, 1])
def test_overflow_list_exactly_full_and_one_past(over):
    """tau forced to 0.5 and runs of identical rows, laid out on k_gemm.hip's plan for one 64-query tile (phase ph walks the
    gallery tiles ph, ph + nph, ..; wave row wm of a tile's 256 rows feeds region ph * 8 + wm) so that saturated regions send
    exactly CAND_OVF (+ 1) rows of every query to the overflow list.  A deep region holds a whole wave row of one tile, so the
    gallery has two tiles per phase.  The full list has lost nothing: the deep filter answers and counts every candidate; one
    row more and the query is `overflowed` and scanned exactly.  The stats assert the premise."""
    from mirx import _lib as L
    ovf = _constexpr("mirx_common.h", "CAND_OVF")
    min_slots = _constexpr("mirx_common.h", "DEEP_MIN_SLOTS")
    nq, k, d, total = 8, 100, 256, 512 + 64 * over
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = max(2 * (cus // 8 * 8) * 256, deep_min_rows(k, nq)) + 257
    nph = min(cus // 8 * 8, (n + 255) // 256)
    r = np.arange(n)
    region, slots = ((r // 256) % nph) * 8 + (r % 256) // 32, max(min_slots, 2 * DEEP_CAP // (nph * 8))   # region_slots_deep()
    g, base, runs = _unit(n, d, 3721), _unit(nq, d, 3722), []
    own = torch.zeros(nq, n, dtype=torch.bool)
    for j in range(nq):
        rows = _lay_out(region, np.nonzero((r % 256) // 32 == j)[0], slots, total, ovf + over)
        g[torch.as_tensor(rows)] = base[j]
        own[j, torch.as_tensor(rows)] = True
        runs.append(rows)
    dots = (base.double() @ g.double().t()).masked_fill_(own, -1.0)
    assert float(dots.max()) < 0.5 - 4 * (2.0 ** -8 + 2.0 ** -18 + _dimp(d) * 2.0 ** -23)   # only the own run passes 0.5
    ix = _index(d, "COSINE", g)
    ix.set_option(L.OPT_FORCE_TAU, int(np.float32(0.5).view(np.uint32)))
    st, _, o_i = _check(ix, base, k, 0, g)
    np.testing.assert_array_equal(o_i, np.stack([rows[:k] for rows in runs]))
    if over == 0:
        assert st["candidates"] == nq * total and st["reranked"] == nq * total, st
        assert st["overflowed"] == 0 and st["incomplete"] == 0 and st["tier1_answered"] == nq, st
    else:
        assert st["overflowed"] == nq and st["exact_answered"] == nq and st["tier1_answered"] == 0, st


# ---- 5. guard and second chance ------------------------------------------------------------------------------------------------
def test_first_threshold_too_high_is_retried():
    """Tight clusters of near-copies (tools/clustered_probe.py's recipe at small scale), larger than the route's candidate
    target: more than rank-j sampled groups hold a member of the query's cluster, so the sampled threshold lands among the
    cluster's scores, which lie within 2 eps of each other -- the guard rejects, and the second pass with tau2 admits the cluster."""
    nq, k, size = 48, 100, 1500
    ncls = -(-_ragged(deep_min_rows(k, nq)) // size)
    d = 64
    gen = torch.Generator().manual_seed(3708)
    centers = torch.nn.functional.normalize(torch.randn(ncls, d, generator=gen), dim=1)
    lab = torch.arange(ncls * size) % ncls
    g = torch.nn.functional.normalize(centers[lab] + 0.01 / d ** 0.5 * torch.randn(ncls * size, d, generator=gen), dim=1)
    rows = (np.arange(nq) * 977 + 3) % g.shape[0]
    q = torch.nn.functional.normalize(g[rows] + 0.01 / d ** 0.5 * torch.randn(nq, d, generator=gen), dim=1)
    assert int(_admitted(q, g, k, 0).max()) <= DEEP_CAP
    ix = _index(d, "COSINE", g)
    st, _, _ = _check(ix, q, k, 0, g)
    assert st["incomplete"] > 0 and st["tier1_answered"] + st["exact_answered"] == nq, st
    assert st["tier1_answered"] >= 0.9 * nq, st                      # the second pass answered them, not the scan


# ---- 6. bf16 misordering at depth ------------------------------------------------------------------------------------------------
def _bf16_ulp(v):
    e = (v.numpy().view(np.uint32) >> 23) & 0xFF
    return torch.from_numpy(np.ldexp(1.0, e.astype(np.int64) - 127 - 7).astype(np.float32))


@pytest.mark.parametrize("metric", ["IP", "L2"])
def test_planted_pair_that_bf16_misorders_at_rank_100(metric):
    """test_search_filter_edges_gpu's planted pair, at the 100th place: per query 99 rows near the query itself, then a row B
    whose true score beats row A's while B's bf16 image scores below A in the filter, then nothing within 4 eps.  The answer
    holds B at rank 100 and not A only because the guard band re-scores every row within 2 eps of the k-th filter score."""
    mc, d, nq, k = METRICS[metric], 256, 8, 100
    n = _ragged(deep_min_rows(k, nq))
    gen = torch.Generator().manual_seed(3709)
    q = _bf16(torch.randn(nq, d, generator=gen) / d ** 0.5)
    v = _bf16((0.9 if mc == 0 else 0.7) * q)           # L2: c - c^2 / 2 must leave the pair 4 eps behind the rows near c = 1
    assert (v != 0).all()
    ulp, sgn = _bf16_ulp(v), torch.sign(q)
    b = v + 0.45 * sgn * ulp                                    # rounds back to v
    a = v.clone()
    a[:, ::4] += (sgn * ulp)[:, ::4]                            # one ulp up on a quarter of the coordinates
    assert torch.equal(_bf16(b), v) and torch.equal(_bf16(a), a) and not torch.equal(a, v)
    g = _unit(n, d, 3710)
    pos = (np.arange(nq * (k + 1)) * 421 + 5) % n
    assert len(set(pos.tolist())) == nq * (k + 1)
    pos = pos.reshape(nq, k + 1)
    near = torch.linspace(0.95, 1.0, k - 1)                     # the 99 rows in front: c q, c in [0.95, 1]
    for i in range(nq):
        g[torch.as_tensor(pos[i, :k - 1])] = near[:, None] * q[i][None, :]
    pa, pb = pos[:, k - 1], pos[:, k]
    tpa, tpb = torch.as_tensor(pa), torch.as_tensor(pb)
    g[tpa], g[tpb] = a, b
    # host precondition, float64
    s = _true_scores(q, g, mc)
    gb = g.clone()
    gb[tpb] = _bf16(g[tpb])
    s_f = _true_scores(q, gb, mc)                                # the filter's view of the planted rows: bf16 operands ...
    if mc == 1:
        s_f += 0.5 * ((gb.double() ** 2).sum(1) - (g.double() ** 2).sum(1))[None]   # ... and the bias of the fp32 row
    eps = _eps(_norms(q), _norms(g).max(), _dimp(d), mc)
    qi = torch.arange(nq)
    sa, sb = s[qi, tpa], s[qi, tpb]
    fa, fb = s_f[qi, tpa], s_f[qi, tpb]
    assert (sb > sa).all()                                         # the truth: B first
    assert (fb < fa).all()                                         # the filter: A first
    assert (fa - fb < 2.0 * eps).all(), ((fa - fb) / eps)          # ... by less than the band
    print("planted gap / eps: %.3f .. %.3f" % (float(((fa - fb) / eps).min()), float(((fa - fb) / eps).max())))
    assert ((s > (torch.maximum(sa, sb) + 4.0 * eps)[:, None]).sum(1) == k - 1).all()      # exactly 99 rows clearly in front
    rest = s.clone()
    rest[qi, tpa] = -np.inf
    rest[qi, tpb] = -np.inf
    rest[s > torch.maximum(sa, sb)[:, None]] = -np.inf
    assert (rest.max(1).values < torch.minimum(sa, sb) - 4.0 * eps).all()                  # and nothing else near the pair
    assert int(_admitted(q, g, k, mc, s).max()) <= DEEP_CAP

    ix = _index(d, metric, g)
    st, _, o_i = _check(ix, q, k, mc, g)
    np.testing.assert_array_equal(o_i[:, k - 1], pb)
    assert not np.any(o_i == pa[:, None])
    assert st["tier1_answered"] == nq, st                          # the deep filter answered, it did not fall back


# ---- 7. masked ------------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    assert torch.equal(got[1], want[1]), what
    assert torch.equal(got[0], want[0]), what


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_masked_deep_search(metric):
    mc, nq, k = METRICS[metric], 32, 100
    rows_min = deep_min_rows(k, nq)
    n = 2 * _ragged(rows_min)
    g = _gallery(n)
    ids = torch.arange(n, dtype=torch.int64) * 3 + 11
    q, _ = _perturbed(g, nq, 3711)
    ix = _index(_D, metric, g, ids)
    order = torch.randperm(n, generator=torch.Generator().manual_seed(3712))
    for count in (n // 2, rows_min - 1, rows_min):
        allow = torch.zeros(n, dtype=torch.bool)
        allow[order[:count]] = True
        assert int(_admitted(q, g[allow], k, mc).max()) <= DEEP_CAP
        fresh = _index(_D, metric, g[allow], ids[allow])
        want = fresh.search(q, k, return_f64=True)                  # the exact scan of the allowed rows alone
        assert fresh.last_stats()["exact_answered"] == nq
        for mask in (allow, allow.to("cuda:0")):
            got = ix.search_deep(q, k, return_f64=True, allow=mask)
            st = ix.last_stats()
            _same(got, want, (metric, count))
            _route(st, nq, deep_must_answer=count >= rows_min)
            if count < rows_min:
                assert st["tier1_answered"] == 0 and st["exact_answered"] == nq, (count, st)
        got32 = ix.search_deep(q, k, allow=allow)
        _same(got32, fresh.search(q, k), (metric, count, "fp32"))
    s, i = ix.search_deep(q, k, return_f64=True, allow=torch.zeros(n, dtype=torch.bool))
    assert bool((i == -1).all()) and bool(torch.isinf(s).all()) and bool((s < 0).all())
    with pytest.raises(ValueError):
        ix.search_deep(q, k, allow=torch.ones(n - 1, dtype=torch.bool))


# ---- 8. determinism and the busy rule ----------------------------------------------------------------------------------------
def test_same_call_twice_and_busy_index():
    from mirx import _lib as L
    mc, nq, k = 0, 32, 100
    g = _gallery(_ragged(deep_min_rows(k, nq)))
    q, _ = _perturbed(g, nq, 3713)
    ix = _index(_D, "COSINE", g)
    a = ix.search_deep(q, k, return_f64=True)
    assert ix.last_stats()["tier1_answered"] > 0
    b = ix.search_deep(q, k, return_f64=True)
    _same(a, b, "twice")
    h = ix.search_begin(q, 10)
    with pytest.raises(L.MirxError, match=r"\(%d\).*mirx_index_search_end" % L.ESTATE):
        ix.search_deep(q, k)
    with pytest.raises(L.MirxError, match=r"\(%d\).*mirx_index_search_end" % L.ESTATE):
        ix.search_deep(q, k, allow=torch.ones(g.shape[0], dtype=torch.bool))
    ix.search_end(h)
    _same(ix.search_deep(q, k, return_f64=True), a, "after search_end")
