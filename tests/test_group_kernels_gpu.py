"""The grouping search's three device passes (k_group.hip) on their own, against tests/_group_ref.py and the index's own
searches.  GPU only; no tolerance: ids, codes, counts, flags and fp64 score bits are compared with ==.

mirx_group_walk runs on hand-built ranked lists (no index involved), mirx_group_count on random codes against np.bincount,
mirx_index_group_fill against search(k, allow=groups == g, exclude_ids, return_f64=True) on the same index."""
import ctypes

import numpy as np
import pytest
import torch

import _group_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from mirx import _lib as L
    return L, L.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a, dtype):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _walk(ranks, depth, group_of, group_rows, limit, gs, scores=None, tix=None, excl=None, live=None):
    """mirx_group_walk on numpy inputs (ranks / scores / tix [nq, stride]) -> numpy (ids, scores, codes, kept, state)"""
    L, lib = _lib()
    nq, stride = ranks.shape
    d_ranks, d_tix, d_sc = _dev(ranks, torch.int64), _dev(tix, torch.int64), _dev(scores, torch.float64)
    d_of, d_rows, d_ex = _dev(group_of, torch.int64), _dev(group_rows, torch.int64), _dev(excl, torch.int64)
    ids = torch.full((nq, limit, gs), -7, dtype=torch.int64, device=DEV)
    sc = torch.full((nq, limit, gs), 123.0, dtype=torch.float64, device=DEV)
    codes = torch.full((nq, limit), -7, dtype=torch.int64, device=DEV)
    kept = torch.full((nq, limit), -7, dtype=torch.int32, device=DEV)
    state = torch.full((nq, 2), -7, dtype=torch.int32, device=DEV)
    live = int((np.asarray(group_rows) > 0).sum()) if live is None else live
    rc = lib.mirx_group_walk(_p(d_ranks), _p(d_tix), _p(d_sc), nq, depth, stride, _p(d_of), len(group_of), _p(d_rows),
                             len(group_rows), live, _p(d_ex), limit, gs, _p(ids), _p(sc) if scores is not None else None, _p(codes),
                             _p(kept), _p(state), None)
    assert rc == 0, lib.mirx_last_error()
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), codes.cpu().numpy(), kept.cpu().numpy(), state.cpu().numpy()


def _check(lists, group_of, limit, gs, group_rows=None, excl=None, depth=None, stride=None, with_tix=False, with_scores=True):
    """Run the walk over `lists` (one ranked list of table entries per query, -1 = the ranking's end) and compare every output
    with the reference.  group_rows defaults to the table's own counts (every entry eligible)."""
    group_of = np.asarray(group_of, dtype=np.int64)
    if group_rows is None:
        group_rows = np.bincount(group_of, minlength=int(group_of.max()) + 1)
    nq = len(lists)
    depth = max(len(l) for l in lists) if depth is None else depth
    stride = depth if stride is None else stride
    ent = np.full((nq, stride), -1, dtype=np.int64)
    for i, l in enumerate(lists):
        ent[i, :min(len(l), stride)] = l[:stride]
    ent[:, depth:] = np.where(ent[:, depth:] >= 0, ent[:, depth:], 0)     # what lies past the depth must never be read as a hit
    rng = np.random.default_rng(nq * 1000 + depth)
    scores = -np.sort(rng.standard_normal((nq, stride)), axis=1) if with_scores else None
    ids = np.where(ent >= 0, 7 + 3 * ent, -1) if with_tix else ent
    got = _walk(ids, depth, group_of, group_rows, limit, gs, scores=scores, tix=ent if with_tix else None,
                excl=None if excl is None else np.asarray(excl, dtype=np.int64))
    for i in range(nq):
        prefix = ent[i, :depth].tolist()
        e_ids, e_sc, e_codes, e_kept = R.tensors(prefix, ids[i, :depth], None if scores is None else scores[i, :depth], group_of,
                                                 limit, gs)
        assert np.array_equal(got[0][i], e_ids), (i, got[0][i], e_ids)
        if with_scores:
            assert np.array_equal(got[1][i].view(np.int64), e_sc.view(np.int64)), i
        assert np.array_equal(got[2][i], e_codes), (i, got[2][i], e_codes)
        assert np.array_equal(got[3][i], e_kept), (i, got[3][i], e_kept)
        n_open, complete, final = R.prefix_state(prefix, group_of, group_rows, -1 if excl is None else int(excl[i]), limit, gs)
        assert got[4][i, 0] == n_open, (i, got[4][i], n_open)
        assert bool(got[4][i, 1] & 1) == complete and bool(got[4][i, 1] & 2) == final, (i, got[4][i], complete, final)
    return got


@pytest.mark.parametrize("limit,gs", [(1, 1), (3, 1), (3, 2), (10, 3), (64, 1), (1024, 1), (256, 64)])
@pytest.mark.parametrize("depth", [1, 63, 64, 65, 130])
def test_walk_random_lists(depth, limit, gs):
    """prefixes of random full rankings over a 150-entry table: few groups (every chunk revisits them), many groups (limit
    decides), one group; with and without the id -> entry translation"""
    rng = np.random.default_rng(depth * 7919 + limit * 31 + gs)
    for n_codes, with_tix in ((1, False), (4, True), (40, False), (150, True)):
        group_of = rng.integers(0, n_codes, 150)
        group_of[:n_codes] = np.arange(n_codes)
        lists = [rng.permutation(150)[:depth].tolist() for _ in range(5)]
        _check(lists, group_of, limit, gs, depth=depth, with_tix=with_tix)


def test_walk_deep_lists_fill_the_table():
    """limit 1024 over 1500 groups and (256, 64) over 300 groups, lists deep enough to open every slot: the hash table at its
    design load, completion far from the start, the early stop"""
    rng = np.random.default_rng(5)
    group_of = rng.integers(0, 1500, 6000)
    group_of[:1500] = np.arange(1500)
    _check([rng.permutation(6000).tolist() for _ in range(3)], group_of, 1024, 1)
    _check([rng.permutation(6000)[:3000].tolist() for _ in range(3)], group_of, 1024, 16)
    group_of = rng.integers(0, 300, 30000)
    group_of[:300] = np.arange(300)
    _check([rng.permutation(30000).tolist() for _ in range(2)], group_of, 256, 64)


def test_walk_four_first_rows_of_one_new_group_in_a_chunk():
    group_of = np.array([5] * 6 + [1, 2, 3, 4] * 4)
    lists = [[0, 1, 2, 3, 6, 7, 4, 5, 8, 9], [6, 0, 1, 2, 3, 4, 5, 7], [0, 1, 2, 3, 4, 5]]
    for gs in (1, 3, 5, 8):
        _check(lists, group_of, 3, gs)
        _check(lists, group_of, 1, gs)


def test_walk_group_fills_at_lane_17():
    """group 0 takes its group_size-th row at lane 17 of a chunk; its rows at lanes 20 and 30 and in the next chunk are dropped,
    the other groups go on"""
    group_of = np.array([0] * 10 + list(range(1, 101)))
    order = list(range(10, 110))                      # one row per other group
    lane = {3: 0, 9: 1, 12: 2, 17: 3, 20: 4, 30: 5, 70: 6}
    lst = [lane.get(i, order.pop()) for i in range(100)]
    _check([lst, lst[64:] + lst[:64]], group_of, 100, 4)
    _check([lst], group_of, 20, 4)


def test_walk_last_group_opens_mid_chunk():
    """limit 3: the third group opens at lane 20; the new groups behind it in the same chunk stay closed while later rows of the
    three open groups are still kept"""
    group_of = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2] + list(range(3, 60)))
    body = [0, 3, 1, 4]                              # lanes 0-3: groups 0, 1, 0, 1
    body += [2, 5]                                   # lanes 4-5: third rows of groups 0 and 1 (group_size 3 keeps them)
    body += [0] * 14                                 # lanes 6-19: an entry of a group that is full by now: dropped
    body.append(6)                                   # lane 20: group 2 opens, the last slot
    body += list(range(9, 30))                       # 21 new groups: all stay closed
    body += [7, 8]                                   # rows of group 2 behind them: kept
    body += list(range(30, 50))
    assert len(body) == 64
    for gs in (1, 2, 3):
        _check([body], group_of, 3, gs)
    _check([body], group_of, 4, 3)                    # one more slot: the first new group behind lane 20 takes it


def test_walk_codes_that_all_collide():
    """limit 3 -> 64 table slots; every code a multiple of 64 (and of 2048): each lookup probes past every open group"""
    L, _ = _lib()
    for limit, step in ((3, 64), (20, 64), (3, 2048)):
        codes = np.arange(40) * step
        group_of = np.repeat(codes, 3)
        rng = np.random.default_rng(limit + step)
        lists = [rng.permutation(120).tolist() for _ in range(3)]
        _check(lists, group_of, limit, 2)


def test_walk_padding_before_completion_and_short_groups():
    group_of = np.array([0, 0, 1, 2, 2, 2, 3])
    # the whole eligible ranking is shorter than the depth: -1 ends it, complete although groups are short of group_size
    got = _check([[3, 0, -1, -1, -1, -1], [3, -1, 5, 5, 5, 5], [-1, -1, -1, -1, -1, -1]], group_of, 3, 4,
                 group_rows=np.array([2, 1, 3, 1]))
    assert got[4][:, 1].tolist() == [3, 3, 3]
    # group_rows smaller than group_size: groups 1 and 3 are full with one row, group 0 with two
    got = _check([[2, 6, 0, 1, 3, 4]], group_of, 3, 5)
    assert got[4][0].tolist() == [3, 3] and got[3][0].tolist() == [1, 1, 2]
    got = _check([[2, 6, 0, 3, 4, 5]], group_of, 3, 5)
    assert got[4][0].tolist() == [3, 2]                                        # group 0 still misses a row


def test_walk_excluded_row_takes_its_group_away():
    """query 0 excludes group 1's only row: two groups are left and limit 3 is complete with two open; query 1 excludes a row of
    group 2 (three rows): it needs only two of them; query 2 excludes nothing"""
    group_of = np.array([0, 0, 1, 2, 2, 2])
    lists = [[3, 0, 4, 1, 5], [3, 0, 2, 1, 4], [3, 0, 2, 1, 4]]
    got = _check(lists, group_of, 3, 3, excl=[1, 2, -1])
    assert got[4][:, 0].tolist() == [2, 3, 3]
    assert [bool(v & 1) for v in got[4][:, 1]] == [True, True, False]
    got = _check([l[:2] for l in lists], group_of, 3, 1, excl=[1, 2, -1])
    assert [int(v) for v in got[4][:, 1]] == [3, 0, 0]


@pytest.mark.parametrize("depth,stride", [(5, 9), (64, 100), (70, 128)])
def test_walk_row_stride_larger_than_depth(depth, stride):
    rng = np.random.default_rng(stride)
    group_of = rng.integers(0, 12, 200)
    lists = [rng.permutation(200)[:stride].tolist() for _ in range(6)]
    _check(lists, group_of, 5, 2, depth=depth, stride=stride)
    _check(lists, group_of, 5, 2, depth=depth, stride=stride, with_scores=False, with_tix=True)


def test_walk_skips_entries_outside_the_tables():
    """an entry past the code table and a code past the count table are skipped, not read"""
    group_of = np.array([0, 1, 9, 1, 0])
    got = _walk(np.array([[4, 77, 2, 1, 3, 0]]), 6, group_of, np.array([2, 2]), 2, 2)
    assert got[0][0].tolist() == [[4, 0], [1, 3]] and got[2][0].tolist() == [0, 1] and got[4][0].tolist() == [2, 3]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
@pytest.mark.parametrize("n_codes", [3, 1000])
def test_group_count(n, n_codes):
    L, lib = _lib()
    rng = np.random.default_rng(n + n_codes)
    groups = rng.integers(0, n_codes, n)
    d_groups = _dev(groups, torch.int64)
    for mask in (None, np.ones(n, np.uint8), np.zeros(n, np.uint8), (rng.random(n) < 0.5).astype(np.uint8) * 3):
        out = torch.full((n_codes,), 99, dtype=torch.int64, device=DEV)
        d_mask = _dev(mask, torch.uint8)
        assert lib.mirx_group_count(_p(d_groups), _p(d_mask), n, n_codes, _p(out), None) == 0, lib.mirx_last_error()
        torch.cuda.synchronize()
        keep = groups if mask is None else groups[mask != 0]
        assert np.array_equal(out.cpu().numpy(), np.bincount(keep, minlength=n_codes))
    # codes outside [0, n_groups) are skipped
    out = torch.full((2,), 99, dtype=torch.int64, device=DEV)
    assert lib.mirx_group_count(_p(d_groups), None, n, 2, _p(out), None) == 0
    assert np.array_equal(out.cpu().numpy(), np.bincount(groups[groups < 2], minlength=2))


# ---- the fill ---------------------------------------------------------------------------------------------------------
FILL_N, FILL_GS = 300, 3


def _fill_gallery(d, metric):
    g = torch.Generator().manual_seed(d)
    x = torch.randn(FILL_N, d, generator=g)
    x = torch.nn.functional.normalize(x, dim=1) * (1.0 if metric == "COSINE" else 0.5 + torch.rand(FILL_N, 1, generator=g))
    # groups: 0 = one row, 1 = group_size rows, 2 = group_size + 1 rows, 3 = 200 rows, 4 = the rest
    sizes = [1, FILL_GS, FILL_GS + 1, 200]
    groups = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)] + [np.full(FILL_N - sum(sizes), 4)])
    perm = np.random.default_rng(d).permutation(FILL_N)
    groups = groups[perm]
    big = np.nonzero(groups == 3)[0]
    x[big[10:14]] = x[big[0]].clone()                        # five equal rows in the big group: score ties, decided by id
    x[big[20]] = x[big[1]].clone()
    return x.contiguous(), groups


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("d", [8, 100])
def test_group_fill_equals_the_masked_search(d, metric):
    from mirx.index import FlatIndex
    L, lib = _lib()
    x, groups = _fill_gallery(d, metric)
    ids = 1000 - 3 * torch.arange(FILL_N, dtype=torch.int64)                     # descending ids: id order is not row order
    ix = FlatIndex(d, metric, 0)
    ix.add(x, ids)
    nq, limit = 6, 5
    big = np.nonzero(groups == 3)[0]
    q = torch.cat([x[big[0]][None] + 0.0, x[big[1]][None] * 1.0, torch.randn(nq - 2, d, generator=torch.Generator().manual_seed(9))])
    # query 0 excludes one of the tied rows, query 1 the only row of group 0, query 2 a row of the group_size group
    exclude = torch.tensor([int(ids[big[10]]), int(ids[np.nonzero(groups == 0)[0][0]]), int(ids[np.nonzero(groups == 1)[0][0]]),
                            -1, -1, 5], dtype=torch.int64)
    rng = np.random.default_rng(d + len(metric))
    for mask in (None, rng.random(FILL_N) < 0.6):
        elig = np.arange(FILL_N) if mask is None else np.nonzero(mask)[0]
        # the member lists: eligible rows group after group, shuffled inside a group (the order must not matter)
        members, first, length = [], [], []
        for c in range(5):
            rows = rng.permutation(elig[groups[elig] == c])
            first.append(len(members))
            length.append(len(rows))
            members += rows.tolist()
        pairs = [(qi, c) for qi in range(nq) for c in range(5) if length[c] > 0]
        d_members = _dev(np.asarray(members), torch.int64)
        pq, ps = _dev([p[0] for p in pairs], torch.int64), _dev([p[1] for p in pairs], torch.int64)
        pf, pl = _dev([first[p[1]] for p in pairs], torch.int64), _dev([length[p[1]] for p in pairs], torch.int64)
        for ex in (None, exclude.to(DEV)):
            out_ids = torch.full((nq, limit, FILL_GS), -7, dtype=torch.int64, device=DEV)
            out_sc = torch.full((nq, limit, FILL_GS), 123.0, dtype=torch.float64, device=DEV)
            qd = q.to(DEV).contiguous()
            rc = lib.mirx_index_group_fill(ix._h, _p(qd), nq, _p(ex), limit, FILL_GS, _p(pq), _p(ps), _p(pf), _p(pl), len(pairs),
                                           _p(d_members), len(members), max(length), _p(out_ids), _p(out_sc), None)
            assert rc == 0, lib.mirx_last_error()
            torch.cuda.synchronize()
            for c in range(5):
                allow = torch.from_numpy((groups == c) & (True if mask is None else mask))
                if length[c] == 0:
                    assert (out_ids[:, c] == -7).all()                          # no pair, nothing written
                    continue
                s64, sid = ix.search(q, FILL_GS, exclude_ids=ex, return_f64=True, allow=allow)
                assert torch.equal(out_ids[:, c], sid), (c, out_ids[:, c], sid)
                assert torch.equal(out_sc[:, c].view(torch.int64), s64.view(torch.int64)), c
    # the ties really were decided by id, and the excluded tied row is gone
    s64, sid = ix.search(q[:1], 5, return_f64=True, allow=torch.from_numpy(groups == 3))
    assert (s64[0, :5] == s64[0, 0]).all() and sid[0].tolist() == sorted(sid[0].tolist())


def test_group_fill_refuses_bad_arguments():
    from mirx.index import FlatIndex
    L, lib = _lib()
    ix = FlatIndex(8, "COSINE", 0)
    ix.add(torch.randn(10, 8))
    t = torch.zeros(16, dtype=torch.int64, device=DEV)
    q = torch.zeros(1, 8, device=DEV)
    d = torch.zeros(16, dtype=torch.float64, device=DEV)
    o = torch.zeros(16, dtype=torch.int64, device=DEV)

    def fill(limit=3, gs=1, max_members=8, pq=t, out=o):
        return lib.mirx_index_group_fill(ix._h, _p(q), 1, None, limit, gs, _p(pq), _p(t), _p(t), _p(t), 1, _p(t), 8, max_members,
                                         _p(out), _p(d), None)

    for kw in ({"limit": 0}, {"limit": 1025}, {"gs": 0}, {"gs": 65}, {"limit": 1024, "gs": 17}, {"max_members": 0},
               {"max_members": L.GROUP_FILL_MAX + 1}, {"pq": None}, {"out": None}):
        assert fill(**kw) == -1 and b"group_fill" in lib.mirx_last_error(), kw
    assert fill() == 0
    got = ix.ids()
    assert got.dtype == torch.int64 and got.tolist() == list(range(10))
    out = torch.empty(3, dtype=torch.int64, device=DEV)
    assert lib.mirx_index_get_ids(ix._h, 8, 3, _p(out)) == -1
    assert lib.mirx_index_get_ids(ix._h, 7, 3, _p(out)) == 0 and out.tolist() == [7, 8, 9]
