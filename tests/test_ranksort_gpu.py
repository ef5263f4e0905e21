"""The radix ranking (k_ranksort.hip) against the CPU oracle: mirx_index_rank_all past 65536 rows, mirx_index_rank_top, and the
sort's edges under MIRX_OPT_RANK_SORT = radix.  GPU only.

Bar, every case: ids identical to oracle.search.rank_all / topk, fp64 scores bit-identical, reported fp32 values equal to the
rounded oracle value.  No tolerance anywhere.  Shapes are the sort's edges (one element, partial waves, one / two / many tiles of
T = mirx_rank_sort_tile() elements, both sides of the 65536-row switch), not the workload's."""
import numpy as np
import pytest
import torch

from oracle import search as OS

pytestmark = pytest.mark.gpu


def _tile():
    from mirx import _lib
    return _lib.load().mirx_rank_sort_tile()


def _unit(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)


def _index(g, metric, ids=None, sort=None):
    from mirx import _lib
    from mirx.index import FlatIndex
    ix = FlatIndex(g.shape[1], metric, 0)
    ix.add(g, ids)
    if sort is not None:
        ix.set_option(_lib.OPT_RANK_SORT, sort)
    return ix


def _check_rank_all(ix, q, g, metric, exclude):
    """rank_all == the oracle's: ids, and every reported value (the excluded row reads -inf in both)."""
    ranks, sc = ix.rank_all(q, exclude_ids=exclude, with_scores=True)
    o_r, o_s = OS.rank_all(q.numpy(), g.numpy(), metric=metric, exclude=exclude, with_scores=True)
    np.testing.assert_array_equal(ranks.cpu().numpy(), o_r)
    np.testing.assert_array_equal(sc.cpu().numpy(), OS.reported_value(o_s, metric).astype(np.float32))


def _check_rank_top(ix, q, g, k, metric, exclude=None, ids=None):
    """rank_top == the oracle's topk: ids, bit-identical fp64 scores, reported values."""
    s64, got = ix.rank_top(q, k, exclude_ids=exclude, return_f64=True)
    s32, got2 = ix.rank_top(q, k, exclude_ids=exclude)
    o_s, o_i = OS.topk(q.numpy(), g.numpy(), k, metric=metric, exclude=exclude, ids=ids)
    np.testing.assert_array_equal(got.cpu().numpy(), o_i)
    np.testing.assert_array_equal(got2.cpu().numpy(), o_i)
    np.testing.assert_array_equal(s64.cpu().numpy(), o_s)
    np.testing.assert_array_equal(s32.cpu().numpy(), OS.reported_value(o_s, metric).astype(np.float32))
    return o_i


def _self_queries(g, seed):
    """Up to two gallery rows (their own id excluded) and two outside queries (nothing excluded): 3 or 4 queries."""
    m = min(g.shape[0], 2)
    q = torch.cat([g[:m], _unit(2, g.shape[1], seed)])
    return q, np.array(list(range(m)) + [-1, -1], dtype=np.int64)


# ---- 1. forced radix at every tile boundary -----------------------------------------------------------------------------------
_EDGES = [1, 2, 63, 64, 65, "T-1", "T", "T+1", "2T+1", 5000]


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("n", _EDGES)
def test_forced_radix_matches_oracle_at_the_sort_edges(n, metric):
    from mirx import _lib
    from mirx.index import metric_code
    t = _tile()
    n = {"T-1": t - 1, "T": t, "T+1": t + 1, "2T+1": 2 * t + 1}.get(n, n)
    d, m = 16, metric_code(metric)
    g = _unit(n, d, 100 + n)
    q, ex = _self_queries(g, 7)
    ix = _index(g, metric, sort=_lib.RANK_SORT_RADIX)
    _check_rank_all(ix, q, g, m, ex)
    _check_rank_top(ix, q, g, n, m, exclude=ex)


# ---- 2. ties: the id half of the order comes from stability and the cached id permutation ------------------------------------
def _tied_gallery(d=32):
    base = _unit(10, d, 5)
    return torch.cat([_unit(2000, d, 6), base.repeat(100, 1)]), base          # rows 2000.. are 100 copies of 10 rows


def test_exact_ties_rank_by_id_auto_ids():
    from mirx import _lib
    g, base = _tied_gallery()
    q = torch.cat([base[:2], _unit(2, g.shape[1], 8)])
    ex = np.array([2000, 2001, -1, -1], dtype=np.int64)
    for metric, m in (("COSINE", 0), ("L2", 1)):
        ix = _index(g, metric, sort=_lib.RANK_SORT_RADIX)
        _check_rank_all(ix, q, g, m, ex)
        top = _check_rank_top(ix, q, g, g.shape[0], m, exclude=ex)
        assert np.array_equal(top[0, :99], np.arange(2010, 3000, 10))          # the 99 other copies of query 0, by id


def test_exact_ties_rank_by_user_id_and_the_permutation_follows_add():
    from mirx import _lib
    g, base = _tied_gallery()
    n = g.shape[0]
    rng = np.random.default_rng(11)
    ids = ((rng.permutation(n) - n // 2) * 7 + 3).astype(np.int64)             # shuffled, non-contiguous, both signs
    q = torch.cat([base[:2], _unit(2, g.shape[1], 8)])
    ex = np.array([ids[2000], ids[2001], -1, -1], dtype=np.int64)
    ix = _index(g, "COSINE", ids=ids, sort=_lib.RANK_SORT_RADIX)
    _check_rank_top(ix, q, g, n, 0, exclude=ex, ids=ids)
    # rank_all keeps the excluded row (as -inf); without exclusion it is the oracle's topk with k = n
    ranks = ix.rank_all(q)
    np.testing.assert_array_equal(ranks.cpu().numpy(), OS.topk(q.numpy(), g.numpy(), n, ids=ids)[1])
    # a second add whose ids interleave with the first's: a stale permutation would misplace the new copies
    g2 = torch.cat([base.repeat(30, 1), _unit(200, g.shape[1], 9)])
    ids2 = ((rng.permutation(g2.shape[0]) - 250) * 7 + 5).astype(np.int64)
    ix.add(g2, ids2)
    gg, ii = torch.cat([g, g2]), np.concatenate([ids, ids2])
    assert len(np.unique(ii)) == len(ii)
    _check_rank_top(ix, q, gg, gg.shape[0], 0, exclude=ex, ids=ii)
    # auto ids after user ids do not ascend with the row either
    ix.add(g2[:50])
    gg, ii = torch.cat([gg, g2[:50]]), np.concatenate([ii, np.arange(len(ii), len(ii) + 50)])
    _check_rank_top(ix, q, gg, gg.shape[0], 0, ids=ii)


# ---- 3. signed zero ------------------------------------------------------------------------------------------------------------
def test_zero_scores_of_either_sign_tie_by_id():
    """d = 64 (nothing padded), a uniformly negative query, row A all zeros with the LOWER id, rows B with one (+x, -x) pair and
    zeros elsewhere with higher ids: every score is a zero, and hit_before's == makes zeros of either sign a tie, so A ranks first.

    What the host check found: the lane-tree order cannot give A and B zeros of OPPOSITE sign.  Every lane's accumulator starts at
    +0.0, fma(q, 0, +0.0) = +0.0 and x*q - x*q = +0.0 under round-to-nearest, so an inner-product score is never -0.0 (and the L2
    metric's -sum is never +0.0): for each placement of the pair below -- one 16-byte chunk, two chunks, the first and the last
    lane, a denormal x -- OS.scores gives both rows +0.0.  A mixed pair can therefore not reach the device sort through the ABI;
    that -0.0 and +0.0 share a key is pinned by tests/test_ranksort_cpu.py.  The device half of the case stays: whatever the
    signs, A (lower id, LATER row) must come before every B."""
    from mirx import _lib
    d = 64
    q = torch.full((3, d), -0.125)
    rows = []
    for i, j, x in ((0, 1, 0.75), (0, 4, 0.75), (3, 63, 1.5), (8, 9, 1e-40), (2, 34, 3.0)):
        b = torch.zeros(d)
        b[i], b[j] = x, -x
        rows.append(b)
    rows.append(torch.zeros(d))                                                # A: the last row
    g = torch.stack(rows)
    ids = np.array([11, 12, 13, 14, 15, 2], dtype=np.int64)                    # A has the lowest id
    s = OS.scores(q.numpy(), g.numpy(), 0)
    assert np.all(s == 0.0)
    opposite = np.signbit(s[0, :-1]) != np.signbit(s[0, -1])
    print("signbit(A) =", np.signbit(s[0, -1]), " signbit(B) =", np.signbit(s[0, :-1]), " opposite:", opposite)
    for sort in (_lib.RANK_SORT_RADIX, _lib.RANK_SORT_BITONIC):
        ix = _index(g, "COSINE", ids=ids, sort=sort)
        ranks = ix.rank_all(q).cpu().numpy()
        assert np.all(ranks == np.array([2, 11, 12, 13, 14, 15])), ranks
    _check_rank_top(_index(g, "COSINE", ids=ids), q, g, 6, 0, ids=ids)


# ---- 4. past the old wall (fails without the feature: rank_all refused more than 65536 rows, rank_top did not exist) ------------
@pytest.fixture(scope="module", params=[65537, 70001])
def big(request):
    n, d = request.param, 8
    g = _unit(n, d, 40 + n % 7)
    q = torch.cat([g[[n - 1]], _unit(2, d, 41)])                               # query 0 is the last row, its own id excluded
    ex = np.array([n - 1, -1, -1], dtype=np.int64)
    return g, q, ex, _index(g, "COSINE")                                       # sort option on auto


def test_rank_all_past_65536_rows_matches_oracle(big):
    g, q, ex, ix = big
    _check_rank_all(ix, q, g, 0, ex)
    assert int(ix.rank_all(q, exclude_ids=ex)[0, -1]) == g.shape[0] - 1        # excluded row last


def test_rank_top_2000_past_65536_rows_matches_oracle(big):
    g, q, ex, ix = big
    top = _check_rank_top(ix, q, g, 2000, 0, exclude=ex)
    assert g.shape[0] - 1 not in top[0]


def test_forced_bitonic_refuses_more_than_65536_rows(big):
    from mirx import _lib
    from mirx._lib import MirxError
    g, q, ex, ix = big
    ix.set_option(_lib.OPT_RANK_SORT, _lib.RANK_SORT_BITONIC)
    try:
        with pytest.raises(MirxError, match="65536"):
            ix.rank_all(q)
        with pytest.raises(MirxError, match="rank sort"):
            ix.set_option(_lib.OPT_RANK_SORT, 3)
    finally:
        ix.set_option(_lib.OPT_RANK_SORT, _lib.RANK_SORT_AUTO)


# ---- 5. rank_top's conventions are the search's ---------------------------------------------------------------------------------
def test_rank_top_leaves_the_excluded_row_out():
    n, d = 300, 16
    g = _unit(n, d, 50)
    ix = _index(g, "L2")
    ex = np.array([0, 5, -1], dtype=np.int64)
    s, i = ix.rank_top(g[[0, 5, 9]], n, exclude_ids=ex)
    i, s = i.cpu().numpy(), s.cpu().numpy()
    assert i[0, -1] == -1 and i[1, -1] == -1 and np.isneginf(s[0, -1]) and np.isneginf(s[1, -1])
    assert i[2, -1] >= 0 and np.isfinite(s[2, -1]) and 0 not in i[0] and 5 not in i[1]
    _check_rank_top(ix, g[[0, 5, 9]], g, n, 1, exclude=ex)
    from mirx._lib import MirxError
    for k in (0, n + 1):
        with pytest.raises(MirxError, match="rank_top"):
            ix.rank_top(g[:1], k)


def test_search_above_1024_goes_to_rank_top():
    n, d = 1100, 16
    g, q = _unit(n, d, 51), _unit(3, d, 52)
    ix = _index(g, "COSINE")
    s64, i = ix.search(q, 1025, return_f64=True)
    s32, i2 = ix.search(q, 1025)
    o_s, o_i = OS.topk(q.numpy(), g.numpy(), 1025)
    np.testing.assert_array_equal(i.cpu().numpy(), o_i)
    np.testing.assert_array_equal(i2.cpu().numpy(), o_i)
    np.testing.assert_array_equal(s64.cpu().numpy(), o_s)
    np.testing.assert_array_equal(s32.cpu().numpy(), o_s.astype(np.float32))


def test_collection_search_limit_1500_on_70001_rows():
    from mirx.retriever import Collection
    n, d = 70001, 8
    g, q = _unit(n, d, 53), _unit(3, d, 54)
    col = Collection("big", d, metric_type="COSINE", device=0)
    col.insert([[f"img_{i}.png" for i in range(n)], [i % 5 for i in range(n)], g])
    hits = col.search(q.numpy(), limit=1500, output_fields=["image_path"])
    o_s, o_i = OS.topk(q.numpy(), g.numpy(), 1500)
    assert [len(h) for h in hits] == [1500] * 3
    for qi in range(3):
        assert [h.id for h in hits[qi]] == list(o_i[qi])
        assert [h.distance for h in hits[qi]] == [float(v) for v in o_s[qi].astype(np.float32)]
        assert hits[qi][0].entity.get("image_path") == f"img_{o_i[qi, 0]}.png"


# ---- 6. the two sorts agree bit for bit ---------------------------------------------------------------------------------------
def test_forced_radix_equals_forced_bitonic():
    from mirx import _lib
    n, d = 4097, 16
    g = _unit(n, d, 60)
    ids = (np.random.default_rng(61).permutation(n) * 3 - 5000).astype(np.int64)
    q = torch.cat([g[:2], _unit(2, d, 62)])
    ex = np.array([ids[0], ids[1], -1, -1], dtype=np.int64)
    ix = _index(g, "L2", ids=ids)
    out = {}
    for sort in (_lib.RANK_SORT_BITONIC, _lib.RANK_SORT_RADIX):
        ix.set_option(_lib.OPT_RANK_SORT, sort)
        r, s = ix.rank_all(q, exclude_ids=ex, with_scores=True)
        out[sort] = (r.clone(), s.clone())
    a, b = out[_lib.RANK_SORT_BITONIC], out[_lib.RANK_SORT_RADIX]
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
