"""The search filter route off the unit sphere, at widths its K loop had not seen, and under rows that bf16 misorders.  GPU only.

Bar of every case (tests/test_search_gpu.py's `_check`): ids equal the oracle's, fp64 ranking scores bit-identical to
oracle/search_ref.c, reported fp32 values equal to the rounded oracle value.  Every case also states which route must have
answered (`last_stats()`), and where it says "the filter must answer" a float64 host precondition, asserted before the GPU is
touched, shows that the data leave room for it: at most CAND_CAP rows lie within 4 eps of the k-th best score (2 eps of guard
band around a k-th best that the filter itself may have moved by eps, read through scores that are off by eps again).

`eps` is k_finalize's own bound restated in float64 (`_eps`), and the scores of the preconditions are the true scores in the
filter's space: q.g, and for L2 q.g - |g|^2 / 2 (the ranking score -|q - g|^2 is 2 (q.g - |g|^2 / 2) - |q|^2)."""
import os
import re
import time

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
CAND_CAP = _constexpr("mirx_common.h", "CAND_CAP")
MAX_DIMP = _constexpr("mirx_common.h", "MAX_DIMP")
DIM_ALIGN = _constexpr("mirx_common.h", "DIM_ALIGN")
METRICS = {"COSINE": 0, "IP": 0, "L2": 1}


def _unit(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)


def _dimp(d):
    return (d + DIM_ALIGN - 1) // DIM_ALIGN * DIM_ALIGN


def _pad4(x):
    d = x.shape[1]
    return x if d % 4 == 0 else torch.nn.functional.pad(x, (0, (d + 3) // 4 * 4 - d))


def _route(st, nq, filter_must_answer=False):
    assert st["nq"] == nq and st["tier1_answered"] + st["exact_answered"] == nq, st
    if filter_must_answer:
        assert st["tier1_answered"] >= 0.9 * nq, st


def _check(index, q, k, metric, gallery, exclude=None, ids=None, filter_must_answer=False):
    """tests/test_search_gpu.py's bar, with the oracle's inputs padded with zero columns to a multiple of 4; every call's route
    is checked.  -> (stats of the last call, oracle scores, oracle ids)"""
    nq = q.shape[0]
    sc64, got_ids = index.search(q, k, exclude_ids=exclude, return_f64=True)
    st64 = index.last_stats()
    sc32, got_ids2 = index.search(q, k, exclude_ids=exclude)
    st32 = index.last_stats()
    o_s, o_i = OS.topk(_pad4(q).numpy(), _pad4(gallery).numpy(), k, metric=metric,
                       exclude=None if exclude is None else np.asarray(exclude), ids=ids)
    np.testing.assert_array_equal(got_ids.cpu().numpy(), o_i)
    np.testing.assert_array_equal(got_ids2.cpu().numpy(), o_i)
    np.testing.assert_array_equal(sc64.cpu().numpy(), o_s)               # bit-identical fp64
    np.testing.assert_array_equal(sc32.cpu().numpy(), OS.reported_value(o_s, metric).astype(np.float32))
    _route(st64, nq, filter_must_answer)
    _route(st32, nq, filter_must_answer)
    return st32, o_s, o_i


# ---- the host side: true scores in the filter's space and k_finalize's eps, float64 -------------------------------------
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
    """k_finalize's bound on |s~ - s| with `gn` in the place of gnorm_max; with a row's own norm it bounds that row's error"""
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
    """fp32 tensor rounded to bf16 (the oracle's rounding, round to nearest even), as fp32"""
    bits = OS.to_bf16_bits(x.numpy()).astype(np.uint32) << 16
    return torch.from_numpy(bits.view(np.float32).reshape(x.shape).copy())


def _surely_admitted(q, g, k_eff, metric):
    """per query: rows that EVERY complete filter pass must admit, from the filter's own scores: the bf16 images of both
    operands multiplied exactly (float64), plus the bias of the fp32 row.  What is left to bound is the fp32 accumulation and,
    for L2, the fp32 bias and its add: a_r = |q| |g_r| dimp 2^-23 + 2^-23 (|g_r|^2 + |q| |g_r|), eps's own terms at the row's
    norm.  The band's lower end is at most kth + max a - 2 eps, and row r is seen at s_r - a_r or above.  More than CAND_CAP
    such rows: the candidate list overflows whatever the threshold, and only the exact scan can answer."""
    s = _true_scores(_bf16(q), _bf16(g), metric)
    qn, gn = _norms(q), _norms(g)
    if metric == 1:
        s += 0.5 * ((_bf16(g).double() ** 2).sum(1) - gn ** 2)[None]
    dimp = _dimp(g.shape[1])
    eps = _eps(qn, gn.max(), dimp, metric)
    a_r = _eps(qn[:, None], gn[None, :], dimp, metric) - qn[:, None] * gn[None, :] * (2.0 ** -8 + 2.0 ** -18)
    kth = s.topk(k_eff, dim=1).values[:, -1]
    return (s - a_r > (kth + a_r.max(1).values - 2.0 * eps)[:, None]).sum(1)


def _record(case, st, admitted, t0):
    """one line per case for profiles/r23_search_filter_edges.txt (observations, not thresholds)"""
    print("R23 %s | nq %d tier1 %d exact %d incomplete %d overflowed %d candidates %d reranked %d | admitted<= %s | %.2f s"
          % (case, st["nq"], st["tier1_answered"], st["exact_answered"], st["incomplete"], st["overflowed"],
             st["candidates"], st["reranked"], "-" if admitted is None else int(admitted), time.perf_counter() - t0))


def _index(d, metric, g, ids=None):
    from mirx.index import FlatIndex
    ix = FlatIndex(d, metric, 0)
    ix.add(g, ids)
    return ix


# ---- 1. widths the K loop has not seen -----------------------------------------------------------------------------------
_WIDTH_CASES = [(130, MIN_ROWS - 1, 48), (130, MIN_ROWS, 48), (130, MIN_ROWS + 257, 48),          # nk = 4
                (301, MIN_ROWS + 257, 48),                                                        # nk = 6
                (768, MIN_ROWS + 257, 48),                                                        # nk = 12
                (1152, MIN_ROWS + 257, 48),                                                       # nk = 18
                (2048, MIN_ROWS + 257, 16),                                                       # nk = 32
                (MAX_DIMP, MIN_ROWS, 16),                                                         # nk = 64
                (1, MIN_ROWS, 8)]                                                                 # nk = 2, every score +-1
_width_cache = {}


def _width_data(d):
    """unit gallery (the most rows any case of this width takes) and queries; one width is kept at a time, both metrics and
    every n of the width share it"""
    if d not in _width_cache:
        _width_cache.clear()
        rows = max(n for dd, n, _ in _WIDTH_CASES if dd == d)
        nq = max(q for dd, _, q in _WIDTH_CASES if dd == d)
        _width_cache[d] = (_unit(rows, d, 1000 + d), _unit(nq, d, 2000 + d))
    return _width_cache[d]


@pytest.mark.parametrize("d,n,nq,metric", [(d, n, nq, m) for d, n, nq in _WIDTH_CASES for m in ("COSINE", "L2")])
def test_filter_route_at_untested_widths(d, n, nq, metric):
    t0 = time.perf_counter()
    mc, k = METRICS[metric], 10
    g, q = _width_data(d)
    g, q = g[:n], q[:nq]
    filter_route, must = n >= MIN_ROWS, n >= MIN_ROWS and d > 1
    worst = None
    if must:
        worst = _admitted(q, g, k, mc).max()
        assert worst <= CAND_CAP, worst
    ix = _index(d, metric, g)
    st, o_s, o_i = _check(ix, q, k, mc, g, filter_must_answer=must)
    if not filter_route:
        assert st["tier1_answered"] == 0, st
    if d == 1:
        # every score is +1 or -1: nothing lies strictly above the sampled threshold, the exact scan answers with the k lowest
        # ids among the rows of the query's sign
        assert st["exact_answered"] == nq and st["tier1_answered"] == 0, st
        for i in range(nq):
            same = np.nonzero((g[:, 0] * q[i, 0] > 0).numpy())[0]
            np.testing.assert_array_equal(o_i[i], same[:k])
    _record("widths d=%d n=%d %s" % (d, n, metric), st, worst, t0)
    # self-retrieval over rows spread across the tile positions, the row's own id excluded
    rows = (np.arange(64) * 977) % n
    st2, _, _ = _check(ix, g[rows], k, mc, g, exclude=rows)
    _record("widths d=%d n=%d %s self-excluded" % (d, n, metric), st2, None, t0)
    if d > 1:
        s, i = ix.search(g[rows], 1)
        np.testing.assert_array_equal(i[:, 0].cpu().numpy(), rows)
        st3 = ix.last_stats()
        _route(st3, len(rows))
    else:
        st3, _, _ = _check(ix, g[rows], 1, mc, g)
    _record("widths d=%d n=%d %s self k=1" % (d, n, metric), st3, None, t0)


# ---- 2. off the unit sphere ------------------------------------------------------------------------------------------------
_N, _D, _NQ = 40000, 256, 32
_sphere_cache = {}


def _directions():
    if "dirs" not in _sphere_cache:
        _sphere_cache["dirs"] = (_unit(_N, _D, 501), _unit(_NQ, _D, 502))
    return _sphere_cache["dirs"]


def _scaled(kind):
    """the fixed directions with norms drawn per row and per query from `kind`"""
    if kind not in _sphere_cache:
        g, q = _directions()
        if kind == "uniform":                                      # [0.5, 2]
            gen = torch.Generator().manual_seed(503)
            gn, qn = 0.5 + 1.5 * torch.rand(_N, generator=gen), 0.5 + 1.5 * torch.rand(_NQ, generator=gen)
        else:                                                      # log-uniform in [2^-6, 2^6]
            # Under L2 a query of norm above ~30 spreads its scores so far that its band holds fewer than CAND_CAP rows and
            # the filter answers it, rightly.  511 is the first seed from 503 on with no such query (largest norm 25.8), as the
            # hopeless case's host precondition requires of every query; the precondition is asserted, the seed is not trusted.
            gen = torch.Generator().manual_seed(511)
            gn, qn = 2.0 ** (12 * torch.rand(_N, generator=gen) - 6), 2.0 ** (12 * torch.rand(_NQ, generator=gen) - 6)
        _sphere_cache[kind] = (g * gn[:, None], q * qn[:, None])
    return _sphere_cache[kind]


@pytest.mark.parametrize("metric", ["IP", "L2"])
@pytest.mark.parametrize("kind", ["uniform", "loguniform"])
def test_norms_off_the_unit_sphere(kind, metric):
    """Norms in [0.5, 2] and in [2^-6, 2^6]: the qnorm and gnorm_max factors of eps, the L2 bias and its term of eps decide what
    is re-scored.  Log-uniform norms under L2 leave the band wider than the candidate list for every query: the hopeless eps
    must end in the exact scan, with the oracle's answer."""
    t0 = time.perf_counter()
    mc, k = METRICS[metric], 10
    g, q = _scaled(kind)
    hopeless = kind == "loguniform" and metric == "L2"
    if hopeless:
        worst = _surely_admitted(q, g, k, mc).min()
        assert worst > CAND_CAP, worst
    else:
        worst = _admitted(q, g, k, mc).max()
        assert worst <= CAND_CAP, worst
    ix = _index(_D, metric, g)
    st, _, _ = _check(ix, q, k, mc, g, filter_must_answer=not hopeless)
    if hopeless:
        assert st["exact_answered"] == _NQ and st["incomplete"] + st["overflowed"] >= _NQ, st
    _record("norms %s %s" % (kind, metric), st, worst, t0)


@pytest.mark.parametrize("metric", ["IP", "L2"])
def test_one_outlier_norm_then_removed(metric):
    """One row of norm 1e4 among unit rows makes gnorm_max, and with it eps, 1e4 times what the other rows need: every query
    goes to the exact scan.  Removing the row leaves gnorm_max an upper bound, so the edited index may still scan; a fresh
    index of the survivors answers in the filter, and both give the oracle's answer on the survivors."""
    t0 = time.perf_counter()
    mc, k = METRICS[metric], 10
    dirs, q = _directions()
    out = 12345
    g = dirs.clone()
    g[out] *= 1e4
    worst = _surely_admitted(q, g, k, mc).min()
    assert worst > CAND_CAP, worst
    ix = _index(_D, metric, g)
    st, o_s, o_i = _check(ix, q, k, mc, g)
    assert st["exact_answered"] == _NQ and st["incomplete"] + st["overflowed"] >= _NQ, st
    if mc == 0:
        pos = (q.double() @ g[out].double() > 0).numpy()
        assert pos.any() and (~pos).any()
        assert np.all(o_i[pos, 0] == out) and not np.any(o_i[~pos] == out)
    _record("outlier 1e4 %s" % metric, st, worst, t0)

    assert ix.remove([out]) == 1
    keep = np.delete(np.arange(_N), out)
    gs = g[keep]
    worst = _admitted(q, gs, k, mc).max()
    assert worst <= CAND_CAP, worst
    st_e, _, _ = _check(ix, q, k, mc, gs, ids=keep)                 # the first oracle check of remove at this size
    fresh = _index(_D, metric, gs, keep)
    st_f, _, _ = _check(fresh, q, k, mc, gs, ids=keep, filter_must_answer=True)
    se, ie = ix.search(q, k, return_f64=True)
    sf, jf = fresh.search(q, k, return_f64=True)
    assert torch.equal(ie, jf) and torch.equal(se, sf)
    _record("outlier removed, edited index %s" % metric, st_e, None, t0)
    _record("outlier removed, fresh index %s" % metric, st_f, worst, t0)


_unit_answers = {}


@pytest.mark.parametrize("metric", ["IP", "L2"])
@pytest.mark.parametrize("log2_scale", [40, -40])
def test_uniform_power_of_two_scales(log2_scale, metric):
    """Gallery and queries times 2^40, and times 2^-40: exact in fp32, bf16 and fp64, so every score is the unit-scale score
    times 2^80 (2^-80) to the bit and the ids are the unit-scale ids.  An absolute constant doing a relative one's job (in eps,
    in the norms' upward nudges, in the band's rounding margin) shows here as a route change or a wrong answer."""
    t0 = time.perf_counter()
    mc, k = METRICS[metric], 10
    g, q = _directions()
    if metric not in _unit_answers:
        ix1 = _index(_D, metric, g)
        s1, i1 = ix1.search(q, k, return_f64=True)
        _unit_answers[metric] = (s1.cpu(), i1.cpu())
        del ix1
    s1, i1 = _unit_answers[metric]
    f = 2.0 ** log2_scale
    gs, qs = g * f, q * f
    assert torch.equal((gs / f), g) and torch.equal((qs / f), q)     # the scaling lost nothing
    worst = _admitted(qs, gs, k, mc).max()
    assert worst <= CAND_CAP, worst
    ix = _index(_D, metric, gs)
    st, o_s, o_i = _check(ix, qs, k, mc, gs, filter_must_answer=True)
    np.testing.assert_array_equal(o_i, i1.numpy())
    np.testing.assert_array_equal(o_s, s1.numpy() * (f * f))
    _record("scale 2^%d %s" % (log2_scale, metric), st, worst, t0)


# ---- 3. rows that bf16 is known to misorder --------------------------------------------------------------------------------
def _bf16_ulp(v):
    """the spacing of bf16 at |v| (v bf16-exact, non-zero, normal): 2^(exponent - 7)"""
    e = (v.numpy().view(np.uint32) >> 23) & 0xFF
    return torch.from_numpy(np.ldexp(1.0, e.astype(np.int64) - 127 - 7).astype(np.float32))


_planted_cache = {}


def _planted():
    """unit-scale gallery with the planted pairs, the queries, the positions of rows A and B"""
    if not _planted_cache:
        nq = 16
        gen = torch.Generator().manual_seed(701)
        q = _bf16(torch.randn(nq, _D, generator=gen) / _D ** 0.5)
        v = _bf16(0.9 * q)
        assert (v != 0).all()
        ulp, sgn = _bf16_ulp(v), torch.sign(q)
        b = v + 0.45 * sgn * ulp                                    # rounds back to v
        a = v.clone()
        a[:, ::4] += (sgn * ulp)[:, ::4]                            # one ulp up on a quarter of the coordinates
        assert torch.equal(_bf16(b), v) and torch.equal(_bf16(a), a) and not torch.equal(a, v)
        g = _unit(_N, _D, 702)
        pos = (np.arange(2 * nq) * 1237 + 5) % _N                   # distinct, spread over the positions inside a tile
        assert len(set(pos.tolist())) == 2 * nq and len(set((pos % 256).tolist())) == 2 * nq
        pa = np.where(np.arange(nq) % 2 == 0, pos[0::2], pos[1::2])  # A in front of B for even queries, behind it for odd
        pb = np.where(np.arange(nq) % 2 == 0, pos[1::2], pos[0::2])
        g[torch.as_tensor(pa)], g[torch.as_tensor(pb)] = a, b
        _planted_cache["v"] = (g, q, pa, pb)
    return _planted_cache["v"]


@pytest.mark.parametrize("metric", ["IP", "L2"])
@pytest.mark.parametrize("log2_scale", [0, 40, -40])
def test_planted_pair_that_bf16_misorders(log2_scale, metric):
    """Per query a row B whose true score beats row A's, while B's bf16 image scores BELOW A in the filter: the answer is right
    only because the guard band re-scores every row within 2 eps of the k-th filter score.  With the band at zero width the
    filter's own order (A first) comes out.  The queries are bf16-exact, v = bf16(0.9 q), B = v + 0.45 ulp towards q (rounds
    back to v), A = v + 1 ulp towards q on every fourth coordinate (bf16-exact)."""
    t0 = time.perf_counter()
    mc = METRICS[metric]
    g, q, pa, pb = _planted()
    tpa, tpb = torch.as_tensor(pa), torch.as_tensor(pb)
    f = 2.0 ** log2_scale
    g, q = g * f, q * f
    nq = q.shape[0]
    # host precondition, float64
    s = _true_scores(q, g, mc)
    gb = g.clone()
    gb[tpb] = _bf16(g[tpb])
    s_f = _true_scores(q, gb, mc)                                  # the filter's view of the planted rows: bf16 operands ...
    if mc == 1:
        s_f += 0.5 * ((gb.double() ** 2).sum(1) - (g.double() ** 2).sum(1))[None]   # ... and the bias of the fp32 row
    eps = _eps(_norms(q), _norms(g).max(), _dimp(_D), mc)
    qi = torch.arange(nq)
    sa, sb = s[qi, tpa], s[qi, tpb]
    fa, fb = s_f[qi, tpa], s_f[qi, tpb]
    assert (sb > sa).all()                                         # the truth: B first
    assert (fb < fa).all()                                         # the filter: A first
    assert (fa - fb < 2.0 * eps).all(), ((fa - fb) / eps)          # ... by less than the band
    rest = s.clone()
    rest[qi, tpa] = -np.inf
    rest[qi, tpb] = -np.inf
    assert (rest.max(1).values < torch.minimum(sa, sb) - 4.0 * eps).all()
    worst = max(int(_admitted(q, g, 1, mc, s).max()), int(_admitted(q, g, 2, mc, s).max()))
    assert worst <= CAND_CAP

    ix = _index(_D, metric, g)
    st1, _, i1 = _check(ix, q, 1, mc, g)
    np.testing.assert_array_equal(i1[:, 0], pb)
    assert st1["tier1_answered"] == nq, st1                        # the filter answered, it did not fall back
    st2, _, i2 = _check(ix, q, 2, mc, g)
    np.testing.assert_array_equal(i2, np.stack([pb, pa], 1))
    assert st2["tier1_answered"] == nq, st2
    print("R23 planted gap / eps: %.3f .. %.3f" % (float(((fa - fb) / eps).min()), float(((fa - fb) / eps).max())))
    _record("planted pair 2^%d %s k=1" % (log2_scale, metric), st1, worst, t0)
    _record("planted pair 2^%d %s k=2" % (log2_scale, metric), st2, worst, t0)


# ---- 4. k and query-count edges on the filter route ----------------------------------------------------------------------
def _edge_gallery():
    if "edge" not in _sphere_cache:
        _sphere_cache["edge"] = _unit(_N, _D, 801)
    return _sphere_cache["edge"]


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("k,excl", [(1, False), (MAX_K, False), (MAX_K - 1, True)])
def test_k_up_to_the_filter_cap(k, excl, metric):
    t0 = time.perf_counter()
    mc, nq = METRICS[metric], 32
    g = _edge_gallery()
    rows = (np.arange(nq) * 977) % _N
    gen = torch.Generator().manual_seed(802)
    q = torch.nn.functional.normalize(g[rows] + 0.5 / _D ** 0.5 * torch.randn(nq, _D, generator=gen), dim=1)
    k_eff = k + (1 if excl else 0)
    assert k_eff <= MAX_K
    worst = _admitted(q, g, k_eff, mc).max()
    assert worst <= CAND_CAP, worst
    ix = _index(_D, metric, g)
    st, _, o_i = _check(ix, q, k, mc, g, exclude=rows if excl else None, filter_must_answer=True)
    if excl:
        assert not np.any(o_i == rows[:, None])
    _record("k=%d%s %s" % (k, " excluded" if excl else "", metric), st, worst, t0)


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("k,excl", [(MAX_K, True), (MAX_K + 1, False)])
def test_k_past_the_filter_cap_is_scanned_exactly(k, excl, metric):
    t0 = time.perf_counter()
    mc, nq = METRICS[metric], 16
    g = _edge_gallery()
    rows = (np.arange(nq) * 977) % _N
    ix = _index(_D, metric, g)
    st, _, _ = _check(ix, g[rows], k, mc, g, exclude=rows if excl else None)
    assert st["tier1_answered"] == 0 and st["exact_answered"] == nq, st
    _record("k=%d%s %s" % (k, " excluded" if excl else "", metric), st, None, t0)


def test_ties_at_k_equal_to_the_cap():
    """k = TIER1_MAX_K on the gallery of 200-row runs of identical rows with the forced mid-range threshold: the 200 copies tie
    in the filter and in fp64, and the answer is the 64 lowest ids of the run."""
    from mirx import _lib as L
    t0 = time.perf_counter()
    d, run, nbase, nq = 256, 200, 200, 40
    base = _unit(nbase, d, 21)
    g = base.repeat_interleave(run, dim=0)
    qi = torch.arange(nq) % nbase
    q = base[qi]
    dots = (base.double() @ base.double().t()).fill_diagonal_(-1)
    eps = 2.0 ** -8 + 2.0 ** -18 + _dimp(d) * 2.0 ** -23
    assert float(dots.max()) < 0.5 - 4 * eps and MAX_K <= run <= CAND_CAP   # nothing but the query's own run passes 0.5
    ix = _index(d, "COSINE", g)
    ix.set_option(L.OPT_FORCE_TAU, int(np.float32(0.5).view(np.uint32)))
    st, _, o_i = _check(ix, q, MAX_K, 0, g)
    assert st["candidates"] == nq * run, st
    assert st["overflowed"] == 0 and st["incomplete"] == 0 and st["tier1_answered"] == nq, st
    np.testing.assert_array_equal(o_i, (qi * run).numpy()[:, None] + np.arange(MAX_K)[None, :])
    _record("ties at k=%d" % MAX_K, st, run, t0)


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("nq", [1, 63, 65, 127, 129, 255, 257])
def test_query_counts_around_the_query_tiles(nq, metric):
    t0 = time.perf_counter()
    mc, k = METRICS[metric], 10
    g = _edge_gallery()
    rows = (np.arange(nq) * 977 + 3) % _N
    gen = torch.Generator().manual_seed(803)
    q = torch.nn.functional.normalize(g[rows] + 0.5 / _D ** 0.5 * torch.randn(nq, _D, generator=gen), dim=1)
    s = _true_scores(q, g, mc)
    worst = max(int(_admitted(q, g, k, mc, s).max()), int(_admitted(q, g, k + 1, mc, s).max()))
    assert worst <= CAND_CAP, worst
    ix = _index(_D, metric, g)
    st, _, _ = _check(ix, q, k, mc, g, filter_must_answer=True)
    _record("nq=%d %s" % (nq, metric), st, worst, t0)
    st, _, o_i = _check(ix, q, k, mc, g, exclude=rows, filter_must_answer=True)
    assert not np.any(o_i == rows[:, None])
    _record("nq=%d excluded %s" % (nq, metric), st, worst, t0)


# ---- the candidate lists at their capacities: CAND_CAP, and the overflow list's CAND_OVF ------------------------------------
CAND_OVF = _constexpr("mirx_common.h", "CAND_OVF")


def _region_of_rows(n):
    """k_gemm.hip's plan for ONE 64-query tile over n rows (make_plan, the region index of the filter epilogue): a workgroup
    per phase walks the gallery tiles ph, ph + nph, ..; its wave row wm owns rows 32 wm .. 32 wm + 31 of each 256-row tile and
    the region ph * 8 + wm.  -> (region of every row, regions per query)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ngt = (n + 255) // 256
    nph = max(1, min(cus // 8 * 8, ngt))
    r = np.arange(n)
    return ((r // 256) % nph) * 8 + (r % 256) // 32, nph * 8


def _lay_out(region, pool, slots, total, surplus):
    """`total` rows out of `pool` (row numbers) of which exactly `surplus` exceed their regions' `slots` -- those reach the
    overflow list -- and the others fill regions to at most `slots`: regions are saturated one after the other until the
    surplus is reached, then filled."""
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
    per = np.bincount(region[rows])                                  # the model's own count of what it laid out
    assert int(np.maximum(per - slots, 0).sum()) == surplus
    return rows


def _runs_laid_out(n, nq, slots_of, total, surplus, seed):
    """-> (gallery, queries, rows of each query's run): query j is a unit vector, its run `total` copies of it among the rows
    of wave row j, laid out by _lay_out; every other row is a unit vector that no query scores near 0.5"""
    d = 256
    region, regions = _region_of_rows(n)
    slots = slots_of(regions)
    g = _unit(n, d, seed)
    base = _unit(nq, d, seed + 1)
    runs = []
    for j in range(nq):
        rows = _lay_out(region, np.nonzero((np.arange(n) % 256) // 32 == j)[0], slots, total, surplus)
        g[torch.as_tensor(rows)] = base[j]
        runs.append(rows)
    own = torch.zeros(nq, n, dtype=torch.bool)
    for j in range(nq):
        own[j, torch.as_tensor(runs[j])] = True
    dots = (base.double() @ g.double().t()).masked_fill_(own, -1.0)
    eps = 2.0 ** -8 + 2.0 ** -18 + _dimp(d) * 2.0 ** -23
    assert float(dots.max()) < 0.5 - 4 * eps                          # nothing but the query's own run passes 0.5
    return g, base, runs


def _tier1_slots(regions):                                           # k_gemm.hip: region_slots()
    return min(64, max(8, 2048 // max(regions, 1)))


def _forced_half(g):
    from mirx import _lib as L
    ix = _index(g.shape[1], "COSINE", g)
    ix.set_option(L.OPT_FORCE_TAU, int(np.float32(0.5).view(np.uint32)))
    return ix


@pytest.mark.parametrize("over", [0, 1])
def test_capacity_at_and_one_past_cand_cap(over):
    """tau forced to 0.5: a query admits exactly its run of identical rows, which tie in the filter and in fp64, so the answer
    is the run's lowest ids.  The run is laid out so that no region receives more than its slots (the overflow list stays
    empty): run = CAND_CAP fills the candidate list to the last key and every one is re-scored; CAND_CAP + 1 is one past what
    the list holds and goes to the exact scan.  The stats assert the premise: a lost candidate fails here, it does not pass
    through the fallback."""
    nq, k, run = 8, MAX_K, CAND_CAP + over
    g, q, runs = _runs_laid_out(MIN_ROWS + 4 * 256 + 1, nq, _tier1_slots, run, 0, 811)
    ix = _forced_half(g)
    first = np.stack([r[:k] for r in runs])
    st, _, o_i = _check(ix, q, k, 0, g)
    np.testing.assert_array_equal(o_i, first)                         # all `run` rows tie: the k lowest ids
    if over == 0:
        assert st["candidates"] == nq * run and st["reranked"] == nq * run, st
        assert st["overflowed"] == 0 and st["incomplete"] == 0 and st["tier1_answered"] == nq, st
    else:
        assert st["overflowed"] == nq and st["exact_answered"] == nq and st["tier1_answered"] == 0, st
    # k = 63 with the run's first id excluded: k_eff = 64, the ids start one later
    st, _, o_i = _check(ix, q, k - 1, 0, g, exclude=first[:, 0])
    np.testing.assert_array_equal(o_i, np.stack([r[1:k] for r in runs]))
    if over == 0:
        assert st["candidates"] == nq * run and st["reranked"] == nq * run and st["tier1_answered"] == nq, st
    else:
        assert st["overflowed"] == nq and st["exact_answered"] == nq, st


@pytest.mark.parametrize("over", [0, 1])
def test_overflow_list_exactly_full_and_one_past(over):
    """The same runs, half of CAND_CAP long, laid out so that saturated regions send exactly CAND_OVF (+ 1) rows of every query
    to the overflow list: a full list has lost nothing and tier 1 answers with every candidate counted; one row more and the
    list has lost a row, the query is `overflowed` and the exact scan answers."""
    nq, k, total = 8, MAX_K, CAND_CAP // 2 + over
    g, q, runs = _runs_laid_out(MIN_ROWS + 4 * 256 + 1, nq, _tier1_slots, total, CAND_OVF + over, 821)
    ix = _forced_half(g)
    st, _, o_i = _check(ix, q, k, 0, g)
    np.testing.assert_array_equal(o_i, np.stack([r[:k] for r in runs]))
    if over == 0:
        assert st["candidates"] == nq * total and st["reranked"] == nq * total, st
        assert st["overflowed"] == 0 and st["incomplete"] == 0 and st["tier1_answered"] == nq, st
    else:
        assert st["overflowed"] == nq and st["exact_answered"] == nq and st["tier1_answered"] == 0, st
