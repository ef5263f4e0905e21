"""FlatIndex.search / rank_top under a row mask (mirx_index_search_masked, k_mask.hip) and Collection.search(expr=) against the
contract: the answer is that of a FRESH index holding only the allowed rows, in order, with their ids -- ids, fp64 ranking
scores and reported fp32 values bit for bit -- and the ids are those of oracle.search.topk over the allowed rows.  GPU only.

No tolerance anywhere.  Ids are 7 + 3 * row, so an id is never a row number.  Both metrics; L2 galleries have norms other than
1 because the per-row bias of the filter GEMM moves with the mask.  Small sizes (the tails of 32 / 64 / 256-row units, dims 8
and 130 = padded rows of 128 and 256 floats) take the gathered exact route; one 45 000 x 64 gallery per metric takes the
bf16 filter route, its masked exact fallback, and both sides of the route boundary TIER1_MIN_ROWS."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-retrieval---thesis-2026_amd", "csrc")
METRICS = ("COSINE", "L2")
BIG_N, BIG_D = 45000, 64


def _L():
    from mirx import _lib
    return _lib


def _constexpr(fname, name):
    with open(os.path.join(_CSRC, fname)) as f:
        m = re.search(r"constexpr\s+(?:int|int64_t)\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    assert m, (fname, name)
    return int(m.group(1))


def _gallery(n, d, seed, metric):
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)
    if metric == "L2":
        x = x * (0.5 + 1.5 * torch.rand(n, 1, generator=g))
    return x.contiguous()


def _ids(n):
    return 7 + 3 * torch.arange(n, dtype=torch.int64)


def _index(g, metric, ids):
    from mirx.index import FlatIndex
    ix = FlatIndex(g.shape[1], metric, 0)
    if g.shape[0]:
        ix.add(g, ids)
    return ix


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b, tag):
    (s1, i1), (s2, i2) = a, b
    assert torch.equal(i1, i2), tag
    assert torch.equal(_bits(s1), _bits(s2)), tag


def _empty_tail(s, i, first, tag):
    assert (i[:, first:] == -1).all() and torch.isinf(s[:, first:]).all() and (s[:, first:] < 0).all(), tag
    assert (i[:, :first] >= 0).all(), tag


def _oracle_ids(q, g, ids, allow, k, metric, exclude=None):
    from oracle import search as OS
    sel = allow.numpy().astype(bool)
    pad = -g.shape[1] % 4                                          # the oracle takes dims that are multiples of 4: zero columns
    q, g = torch.nn.functional.pad(q, (0, pad)), torch.nn.functional.pad(g, (0, pad))      # (the index pads the same way)
    _, oi = OS.topk(q.numpy(), g.numpy()[sel], k, OS.METRIC_IP if metric == "COSINE" else OS.METRIC_NEG_L2,
                    None if exclude is None else np.asarray(exclude, dtype=np.int64), ids.numpy()[sel])
    return torch.from_numpy(oi)


def _check_masked(ix, g, ids, allow, metric, q, tag, exclude=None, device_mask=False):
    """masked search on `ix` == plain search on a fresh index of the allowed rows: k = 10 in fp64, k = allowed + 3 in fp32"""
    na = int(allow.sum())
    am = allow.to("cuda:0") if device_mask else allow
    s, i = ix.search(q, 10, exclude_ids=exclude, return_f64=True, allow=am)
    masked_ids = set(ids[~allow].tolist())
    assert not (set(i.cpu().reshape(-1).tolist()) & masked_ids), tag           # a masked row's id appears nowhere
    if na == 0:
        _empty_tail(s, i, 0, tag)
        return
    fresh = _index(g[allow], metric, ids[allow])
    _same((s, i), fresh.search(q, 10, exclude_ids=exclude, return_f64=True), tag)
    ko = min(10, na - (1 if exclude is not None else 0))           # the oracle is asked for no more than every query has
    if ko >= 1:
        assert torch.equal(i.cpu()[:, :ko], _oracle_ids(q, g, ids, allow, ko, metric, exclude)), tag
    if na + 3 <= 1024:
        s, i = ix.search(q, na + 3, exclude_ids=exclude, allow=am)
        _same((s, i), fresh.search(q, na + 3, exclude_ids=exclude), tag)
        if exclude is None:
            _empty_tail(s, i, na, tag)
        assert (i[:, na:] == -1).all(), tag
        assert not (set(i.cpu().reshape(-1).tolist()) & masked_ids), tag


def _masks(n):
    out = {"all": torch.ones(n, dtype=torch.bool), "none": torch.zeros(n, dtype=torch.bool)}
    for name, rows in (("first", [0]), ("last", [n - 1])):
        m = torch.zeros(n, dtype=torch.bool)
        m[rows] = True
        out[name] = m
    m = torch.zeros(n, dtype=torch.bool)
    m[::2] = True
    out["every other"] = m
    m = torch.zeros(n, dtype=torch.bool)
    lo, hi = (250, 262) if n > 256 else (n // 3, max(n // 3 + 1, 2 * n // 3))       # a run crossing row 256 where there is one
    m[lo:min(hi, n)] = True
    out["run"] = m
    return out


# ---- small galleries: the gathered exact route -------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 130])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 256, 257, 1000])
def test_small_galleries_equal_a_fresh_index_of_the_allowed_rows(n, d):
    for metric in METRICS:
        g, ids = _gallery(n, d, 100 + n, metric), _ids(n)
        q = torch.cat([g[: min(n, 3)] + 0.05 * _gallery(min(n, 3), d, 5, "COSINE"), _gallery(3, d, 6, metric)])
        ix = _index(g, metric, ids)
        for j, (name, allow) in enumerate(_masks(n).items()):
            _check_masked(ix, g, ids, allow, metric, q, (n, d, metric, name), device_mask=bool(j & 1))
            st = ix.last_stats()
            assert st["tier1_answered"] == 0 and st["exact_answered"] == st["nq"] == q.shape[0]
        _same(ix.search(q, 10, return_f64=True), _index(g, metric, ids).search(q, 10, return_f64=True), "mask left no state")


@pytest.mark.parametrize("metric", METRICS)
def test_exclude_ids_masked_and_allowed(metric):
    n, d = 257, 8
    g, ids = _gallery(n, d, 11, metric), _ids(n)
    allow = torch.ones(n, dtype=torch.bool)
    allow[1::3] = False
    rows = torch.tensor([0, 2, 255, 1, 4, 250])                    # rows 1, 4, 250 are masked (1 mod 3), the others allowed
    assert allow[rows].tolist() == [True, True, True, False, False, False]
    q = g[rows].clone()
    ix = _index(g, metric, ids)
    _check_masked(ix, g, ids, allow, metric, q, "exclude", exclude=ids[rows])
    s, i = ix.search(q, 5, exclude_ids=ids[rows], return_f64=True, allow=allow)
    assert not (i.cpu() == ids[rows][:, None]).any()               # allowed or not, the excluded id is skipped


@pytest.mark.parametrize("metric", METRICS)
def test_ties_go_to_the_lowest_allowed_id(metric):
    n, d = 300, 8
    g, ids = _gallery(n, d, 12, metric), _ids(n)
    g[40] = g[9]
    g[260] = g[9]                                                  # three copies of one row: ids 34, 127, 787
    allow = torch.ones(n, dtype=torch.bool)
    allow[9] = False                                               # the lowest id of the tie is masked
    ix = _index(g, metric, ids)
    q = g[9:10].clone()
    s, i = ix.search(q, 3, return_f64=True, allow=allow)
    assert i[0, :2].tolist() == [int(ids[40]), int(ids[260])] and float(s[0, 0]) == float(s[0, 1])
    _check_masked(ix, g, ids, allow, metric, q, "ties")


@pytest.mark.parametrize("metric", METRICS)
def test_in_place_exact_scan_when_the_gather_scratch_is_too_small(metric):
    """MIRX_OPT_MASK_GATHER_BYTES = 0: the allowed rows are scanned where they are, masked entries neutralised -- also when
    fewer rows are allowed than k asks for (a masked row must not surface for lack of others)"""
    L = _L()
    for n in (257, 1000):
        g, ids = _gallery(n, 130, 13 + n, metric), _ids(n)
        q = _gallery(4, 130, 3, metric)
        ix = _index(g, metric, ids)
        ix.set_option(L.OPT_MASK_GATHER_BYTES, 0)
        for name, allow in _masks(n).items():
            _check_masked(ix, g, ids, allow, metric, q, (n, metric, name, "in place"))


# ---- 45 000 x 64: the bf16 filter route --------------------------------------------------------------------------------
_BIG = {}


def _big(metric):
    """gallery, ids, index, every-8th-row mask, queries: the first 160 masked rows are 16 centres with 10 near copies each;
    queries = the 16 centres and 16 noisy copies of allowed rows"""
    if metric not in _BIG:
        gen = torch.Generator().manual_seed(77)
        g = _gallery(BIG_N, BIG_D, 21, metric)
        masked_rows = torch.arange(0, BIG_N, 8)
        centres = _gallery(16, BIG_D, 22, metric)
        for c in range(16):
            rows = masked_rows[10 * c: 10 * c + 10]
            g[rows] = centres[c] + 0.01 * centres[c].norm() * torch.randn(10, BIG_D, generator=gen)
        allow = torch.ones(BIG_N, dtype=torch.bool)
        allow[masked_rows] = False
        assert int(allow.sum()) == 39375
        pick = torch.arange(16) * 2504 + 1                         # rows that are 1 mod 8: allowed
        assert allow[pick].all()
        noisy = g[pick] + 0.02 * g[pick].norm(dim=1, keepdim=True) * torch.randn(16, BIG_D, generator=gen)
        q = torch.cat([centres, noisy]).contiguous()
        ids = _ids(BIG_N)
        _BIG[metric] = (g, ids, _index(g, metric, ids), allow, q)
    return _BIG[metric]


_FRESH = {}


def _fresh_big(metric, allow, key):
    if (metric, key) not in _FRESH:
        g, ids, _, _, _ = _big(metric)
        _FRESH[(metric, key)] = _index(g[allow], metric, ids[allow])
    return _FRESH[(metric, key)]


@pytest.mark.parametrize("metric", METRICS)
def test_filter_route_never_returns_a_masked_row(metric):
    g, ids, ix, allow, q = _big(metric)
    _, plain = ix.search(q[:16], 10)
    masked_ids = ids[~allow]
    assert torch.isin(plain.cpu(), masked_ids).all()               # precondition: unmasked, the centres' top 10 are masked rows
    fresh = _fresh_big(metric, allow, "every 8th")
    for dev in (False, True):
        am = allow.to("cuda:0") if dev else allow
        got = ix.search(q, 10, return_f64=True, allow=am)
        st = ix.last_stats()
        assert st["tier1_answered"] > 0 and st["tier1_answered"] + st["exact_answered"] == 32, st
        _same(got, fresh.search(q, 10, return_f64=True), (metric, dev))
        assert not torch.isin(got[1].cpu(), masked_ids).any()
    _same(ix.search(q, 10, allow=allow), fresh.search(q, 10), metric)
    assert torch.equal(ix.search(q, 10, allow=allow)[1].cpu(), _oracle_ids(q, g, ids, allow, 10, metric))
    ex = ids[torch.arange(32) * 8 + 3]                             # allowed rows' ids as exclude ids
    _same(ix.search(q, 10, exclude_ids=ex, return_f64=True, allow=allow), fresh.search(q, 10, exclude_ids=ex, return_f64=True), metric)


@pytest.mark.parametrize("metric", METRICS)
def test_filter_route_masked_exact_fallback(metric):
    """a threshold every allowed row passes: the lists overflow, every query goes to the exact scan, which honours the mask"""
    L = _L()
    g, ids, ix, allow, q = _big(metric)
    fresh = _fresh_big(metric, allow, "every 8th")
    want = fresh.search(q, 10, return_f64=True)
    ix.set_option(L.OPT_FORCE_TAU, int(np.float32(-1e30).view(np.uint32)))
    try:
        got = ix.search(q, 10, return_f64=True, allow=allow)
        st = ix.last_stats()
    finally:
        ix.set_option(L.OPT_FORCE_TAU, L.FORCE_TAU_OFF)
    assert st["exact_answered"] == 32 and st["tier1_answered"] == 0 and st["overflowed"] == 32, st
    _same(got, want, metric)


@pytest.mark.parametrize("metric", METRICS)
def test_filter_route_with_the_last_partial_tile_masked(metric):
    g, ids, ix, allow, q = _big(metric)
    allow = allow.clone()
    allow[BIG_N // 256 * 256:] = False                             # rows 44800 .. 44999
    assert int(allow.sum()) >= _constexpr("mirx_api.hip", "TIER1_MIN_ROWS")
    got = ix.search(q, 10, return_f64=True, allow=allow)
    assert ix.last_stats()["tier1_answered"] > 0
    _same(got, _index(g[allow], metric, ids[allow]).search(q, 10, return_f64=True), metric)


@pytest.mark.parametrize("metric", METRICS)
def test_route_boundary(metric):
    min_rows = _constexpr("mirx_api.hip", "TIER1_MIN_ROWS")
    g, ids, ix, _, q = _big(metric)
    order = torch.randperm(BIG_N, generator=torch.Generator().manual_seed(5))
    for count in (min_rows - 1, min_rows, min_rows + 1):
        allow = torch.zeros(BIG_N, dtype=torch.bool)
        allow[order[:count]] = True
        got = ix.search(q, 10, return_f64=True, allow=allow)
        st = ix.last_stats()
        if count < min_rows:
            assert st["tier1_answered"] == 0 and st["exact_answered"] == 32, (count, st)
        else:
            assert st["tier1_answered"] > 0, (count, st)
        _same(got, _index(g[allow], metric, ids[allow]).search(q, 10, return_f64=True), (metric, count))


@pytest.mark.parametrize("metric", METRICS)
def test_exact_tier_and_large_k_with_many_allowed_rows(metric):
    """forced exact tier, and k above the filter route's limit: the gathered scan of 39 375 rows"""
    L = _L()
    g, ids, ix, allow, q = _big(metric)
    fresh = _fresh_big(metric, allow, "every 8th")
    _same(ix.search(q[:8], 100, return_f64=True, allow=allow), fresh.search(q[:8], 100, return_f64=True), metric)
    assert ix.last_stats()["exact_answered"] == 8
    ix.set_option(L.OPT_TIERS, L.TIER_EXACT_ONLY)
    try:
        got = ix.search(q, 10, return_f64=True, allow=allow)
        st = ix.last_stats()
    finally:
        ix.set_option(L.OPT_TIERS, L.TIER_AUTO)
    assert st["exact_answered"] == 32 and st["tier1_answered"] == 0
    _same(got, fresh.search(q, 10, return_f64=True), metric)


def test_all_ones_wrong_length_and_state():
    L = _L()
    g, ids, ix, allow, q = _big("COSINE")
    ones = torch.ones(BIG_N, dtype=torch.bool)
    plain = ix.search(q, 10, return_f64=True)
    _same(ix.search(q, 10, return_f64=True, allow=ones), plain, "all ones, host")
    _same(ix.search(q, 10, return_f64=True, allow=ones.to("cuda:0")), plain, "all ones, device")
    _same(ix.search(q, 10, return_f64=True, allow=np.ones(BIG_N, dtype=np.uint8) * 5), plain, "non-zero bytes")
    _same(ix.search(q, 10, allow=ones), ix.search(q, 10), "all ones, fp32")
    frozen = np.ones(BIG_N, dtype=bool)
    frozen.setflags(write=False)                                   # what Collection.expr_mask hands out
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _same(ix.search(q, 10, return_f64=True, allow=frozen), plain, "read-only array")
    for bad in (ones[:-1], torch.ones(BIG_N + 1, dtype=torch.bool), torch.ones(0, dtype=torch.bool)):
        with pytest.raises(L.MirxError, match="one byte per row"):
            ix.search(q, 10, allow=bad)
        with pytest.raises(L.MirxError, match="one byte per row"):
            ix.rank_top(q, 2000, allow=bad)
    with pytest.raises(ValueError, match="bool or uint8"):
        ix.search(q, 10, allow=torch.ones(BIG_N))
    h = ix.search_begin(q, 10)
    try:
        with pytest.raises(L.MirxError, match=r"\(%d\)" % L.ESTATE):
            ix.search(q, 10, allow=allow)
        with pytest.raises(L.MirxError, match=r"\(%d\)" % L.ESTATE):
            ix.rank_top(q, 2000, allow=allow)
    finally:
        done = ix.search_end(h, return_f64=True)
    _same(done, plain, "the pending search is unharmed")


@pytest.mark.parametrize("metric", METRICS)
def test_rank_top_masked(metric):
    g, ids, ix, allow, q = _big(metric)
    q = q[:4]
    fresh = _fresh_big(metric, allow, "every 8th")
    for f64 in (True, False):
        _same(ix.rank_top(q, 2000, return_f64=f64, allow=allow), fresh.rank_top(q, 2000, return_f64=f64), (metric, f64))
    _same(ix.search(q, 2000, return_f64=True, allow=allow.to("cuda:0")), fresh.rank_top(q, 2000, return_f64=True), "search forwards")
    ex = ids[torch.tensor([1, 8, 17, 16])]                          # rows 8 and 16 are masked
    _same(ix.rank_top(q, 2000, exclude_ids=ex, return_f64=True, allow=allow),
          fresh.rank_top(q, 2000, exclude_ids=ex, return_f64=True), "exclude")
    few = torch.zeros(BIG_N, dtype=torch.bool)
    few[torch.randperm(BIG_N, generator=torch.Generator().manual_seed(9))[:1500]] = True
    s, i = ix.rank_top(q, 2000, return_f64=True, allow=few)
    s2, i2 = _index(g[few], metric, ids[few]).rank_top(q, 1500, return_f64=True)
    _same((s[:, :1500], i[:, :1500]), (s2, i2), "1500 allowed")
    _empty_tail(s, i, 1500, "1500 allowed")
    s, i = ix.rank_top(q, 2000, allow=few)
    _empty_tail(s, i, 1500, "1500 allowed, fp32")
    _same(ix.rank_top(q, 2000, return_f64=True, allow=torch.ones(BIG_N, dtype=torch.bool)), ix.rank_top(q, 2000, return_f64=True),
          "all ones")


def rank_top_case(metric):
    """The radix path's shared case (tests/test_range_gpu.py runs the range search over it as well): three sort tiles and a tail
    of 5 rows, d = 40 (rows padded to 128 floats), ids a fixed permutation -- not ascending, so the ranking starts from the id
    permutation --, three queries near rows of the first tile, a middle one and the tail, each excluding its own row's id.
    Masks: about half the rows, all, none, and one row of the tail (the only allowed row is the last query's excluded row).
    -> gallery, ids, queries, exclude ids, {name: mask}"""
    n = 3 * _L().load().mirx_rank_sort_tile() + 5
    g = _gallery(n, 40, 61, metric)
    ids = 7 + 3 * torch.randperm(n, generator=torch.Generator().manual_seed(62))
    near = torch.tensor([5, n // 2, n - 1])
    q = g[near] + 0.05 * _gallery(3, 40, 63, metric)
    one = torch.zeros(n, dtype=torch.bool)
    one[n - 1] = True
    masks = {"half": torch.rand(n, generator=torch.Generator().manual_seed(64)) < 0.5, "all": torch.ones(n, dtype=torch.bool),
             "none": torch.zeros(n, dtype=torch.bool), "one": one}
    return g, ids, q, ids[near], masks


@pytest.mark.parametrize("metric", METRICS)
def test_rank_top_masked_on_allow_bytes(metric):
    """k = n under every mask, host and device: the first `allowed` slots are rank_top's on a fresh index of the allowed rows with
    their ids, bit for bit (fp64 and fp32), the slots past them read (-inf, -1); all ones is the unmasked call."""
    g, ids, q, own, masks = rank_top_case(metric)
    n = g.shape[0]
    ix = _index(g, metric, ids)
    for name, allow in masks.items():
        na = int(allow.sum())
        for ex in (None, own):
            for f64 in (True, False):
                tag = (metric, name, ex is not None, f64)
                want = _index(g[allow], metric, ids[allow]).rank_top(q, na, exclude_ids=ex, return_f64=f64) if na else None
                for am in (allow.numpy(), allow.to("cuda:0")):
                    s, i = ix.rank_top(q, n, exclude_ids=ex, return_f64=f64, allow=am)
                    assert s.shape == i.shape == (3, n), tag
                    if na:
                        _same((s[:, :na], i[:, :na]), want, tag)
                    assert (i[:, na:] == -1).all() and (s[:, na:] == float("-inf")).all(), tag
                    if name == "all":
                        _same((s, i), ix.rank_top(q, n, exclude_ids=ex, return_f64=f64), tag)


# ---- Collection.search(expr=) end to end -------------------------------------------------------------------------------
def _hits(res):
    return [[(h.id, h.distance) for h in hits] for hits in res]


def _check_collection(col, emb_of, label_of, q, exprs, dim):
    """every hit satisfies the expression, and the hits equal those of a collection built from the matching rows"""
    from mirx.retriever import Collection
    for expr, pred in exprs:
        match = [i for i in col.live_ids().tolist() if pred(i, label_of[i])]
        res = col.search(q, limit=10, output_fields=["label"], expr=expr)
        assert all(len(h) == min(10, len(match)) for h in res), expr
        assert all(pred(h.id, h.entity.get("label")) and h.id in set(match) for hits in res for h in hits), expr
        if not match:
            continue
        ref = Collection("ref", dim, metric_type=col.metric_type)
        ref.insert([[f"r/{i}.png" for i in match], [label_of[i] for i in match], torch.stack([emb_of[i] for i in match])])
        want = [[(match[i], d) for i, d in hits] for hits in _hits(ref.search(q, limit=10))]
        assert _hits(res) == want, expr
        ex = [match[0]] * q.shape[0]
        want = [[(match[i], d) for i, d in hits] for hits in _hits(ref.search(q, limit=10, exclude_ids=[0] * q.shape[0]))]
        assert _hits(col.search(q, limit=10, exclude_ids=ex, expr=expr)) == want, expr


_EXPRS = [
    ("label == 1", lambda i, lab: lab == 1),
    ("label != 0 and id < 1500", lambda i, lab: lab != 0 and i < 1500),
    ("label in [0, 2] or id == 4", lambda i, lab: lab in (0, 2) or i == 4),
    ("id in [5, 900] and label == 2", lambda i, lab: i in (5, 900) and lab == 2),
    ("label == 7", lambda i, lab: False),
]


def test_collection_search_with_expr():
    from mirx.retriever import Collection
    n, dim = 2000, 32
    emb = _gallery(n, dim, 31, "COSINE")
    labels = [(i * 7 + i // 11) % 3 for i in range(n)]
    col = Collection("c", dim)
    col.insert([[f"img/{i}.png" for i in range(n)], labels, emb])
    q = emb[[3, 700, 1999]] + 0.05 * _gallery(3, dim, 32, "COSINE")
    emb_of, label_of = dict(enumerate(emb)), dict(enumerate(labels))
    _check_collection(col, emb_of, label_of, q, _EXPRS, dim)
    col.search(q, limit=10, expr="label == 1")
    mask = col._expr.device_mask
    col.search(q[:1], limit=5, expr="label == 1")
    assert col._expr.device_mask is mask                            # one constant filter: the device mask is reused
    col.search(q, limit=5, expr="label == 2")
    assert col._expr.device_mask is not mask
    assert col.search(q, limit=3, expr="label == 7") == [[], [], []]
    col.delete("id in [%s]" % ", ".join(str(i) for i in range(1, n, 5)))
    _check_collection(col, emb_of, label_of, q, _EXPRS, dim)
    assert len(col.search(q, limit=2000, expr="label == 1")[0]) == len(col.query("label == 1"))      # limit above 1024: rank_top


def test_persistent_collection_search_with_expr(tmp_path):
    from mirx.retriever import MilvusManager
    n, dim = 2000, 512
    emb = _gallery(n, dim, 41, "COSINE")
    labels = [(i * 5 + i // 13) % 3 for i in range(n)]
    uri = str(tmp_path / "db")
    col = MilvusManager(uri=uri).create_collection("dinov2")
    col.insert([[f"img/{i}.png" for i in range(n)], labels, emb])
    col.delete("id in [0, 7, 1500]")
    col.flush()
    again = MilvusManager(uri=uri).create_collection("dinov2")
    assert again._index is None                                     # loads on first use
    q = emb[[4, 1000]] + 0.05 * _gallery(2, dim, 42, "COSINE")
    _check_collection(again, dict(enumerate(emb)), dict(enumerate(labels)), q, _EXPRS[:2], dim)
