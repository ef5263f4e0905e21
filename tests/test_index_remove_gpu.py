"""mirx_index_remove_ids (k_compact.hip) against its contract: after a removal the index answers exactly like a FRESH index built
from the survivors in order -- rows and ids bit for bit, search_f64 / rank_all ids and scores -- and goes on doing so after more
rows are added (a tail that was not zeroed again would show there).  GPU only.

No tolerance anywhere.  Sizes are the scan's edges (one row, both sides of a 256-row capacity step and of one and two tiles of
T = mirx_compact_tile() rows), dims 8 and 130 give padded rows of 128 and 256 floats, IP and L2 because the L2 bias moves with
the row.  One case per metric is large enough (>= 32768 survivors) for the bf16 filter pass, which reads the bf16 copy, the
bias and the padded tail of the last GEMM tile."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

NEW_ROWS = 300


def _lib():
    from mirx import _lib
    return _lib


def _tile():
    return _lib().load().mirx_compact_tile()


def _unit(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)


def _index(g, metric, ids, chunk=None):
    from mirx.index import FlatIndex
    ix = FlatIndex(g.shape[1], metric, 0)
    if chunk is not None:
        ix.set_option(_lib().OPT_COMPACT_CHUNK_ROWS, chunk)
    if g.shape[0]:
        ix.add(g, ids)
    return ix


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_answers(ix, fresh, q, tag):
    n = len(fresh)
    assert len(ix) == n, tag
    if n == 0:
        return
    r1, i1 = ix.rows()
    r2, i2 = fresh.rows()
    assert torch.equal(i1, i2) and torch.equal(_bits(r1), _bits(r2)), tag
    s1, h1 = ix.search(q, 10, return_f64=True)
    s2, h2 = fresh.search(q, 10, return_f64=True)
    assert torch.equal(h1, h2) and torch.equal(s1, s2), tag
    a1, v1 = ix.rank_all(q, with_scores=True)
    a2, v2 = fresh.rank_all(q, with_scores=True)
    assert torch.equal(a1, a2) and torch.equal(v1, v2), tag
    if n + 3 <= 1024:                                   # k above the size: the last slots read (-inf, -1)
        s1, h1 = ix.search(q, n + 3)
        s2, h2 = fresh.search(q, n + 3)
        assert torch.equal(h1, h2) and torch.equal(s1, s2), tag
        assert (h1[:, n:] == -1).all() and torch.isinf(s1[:, n:]).all() and (s1[:, n:] < 0).all(), tag
        assert (h1[:, :n] >= 0).all(), tag


def _check_remove(g, ids, request, metric, q, tag, chunk=None, expect=None, request_device="cpu"):
    """remove `request` from an index of (g, ids); compare with a fresh index of the survivors, before and after adding rows"""
    ids_t = torch.as_tensor(ids, dtype=torch.int64)
    req = torch.as_tensor(request, dtype=torch.int64)
    keep = ~torch.isin(ids_t, req)
    ix = _index(g, metric, ids_t, chunk)
    removed = ix.remove(req.to(request_device))
    assert removed == int((~keep).sum()), tag
    if expect is not None:
        assert removed == expect, tag
    fresh = _index(g[keep], metric, ids_t[keep])
    _same_answers(ix, fresh, q, tag)
    more, more_ids = _unit(NEW_ROWS, g.shape[1], 991), torch.arange(NEW_ROWS, dtype=torch.int64) + 10 ** 6
    ix.add(more, more_ids)
    fresh.add(more, more_ids)
    _same_answers(ix, fresh, q, tag + " +300")
    return ix


def _sizes():
    t = _tile()
    return [1, 255, 256, 257, t - 1, t, t + 1, 2 * t + 3]


def _requests(ids):
    """name -> (request, rows removed) for ascending distinct ids"""
    n = len(ids)
    out = {"none": ([], 0), "all": (ids, n), "first": (ids[:1], 1), "last": (ids[-1:], 1), "every other": (ids[::2], (n + 1) // 2),
           "absent": ([ids[-1] + 1, -5, ids[0] - 1, 10 ** 12], 0),
           "duplicates": ([ids[0], ids[n // 2], ids[0], ids[n // 2], ids[0]], len({ids[0], ids[n // 2]}))}
    if n > 250:
        run = ids[250:263]                              # crosses row 256
        out["run over a 256-row boundary"] = (run, len(run))
    return out


@pytest.mark.parametrize("metric", ["IP", "L2"])
@pytest.mark.parametrize("dim", [8, 130])
def test_remove_equals_a_fresh_index_of_the_survivors(dim, metric):
    t = _tile()
    assert t >= 256 and t % 256 == 0
    for n in _sizes():
        g = _unit(n, dim, 10 * n + dim) * (1.0 if metric == "IP" else 3.0)       # L2: norms that matter to the bias
        ids = [7 + 3 * i for i in range(n)]             # an id is not its row number
        q = torch.cat([g[:1], g[n // 2:n // 2 + 1], _unit(2, dim, 5)])
        for name, (request, count) in _requests(ids).items():
            _check_remove(g, ids, request, metric, q, f"n={n} dim={dim} {metric} {name}", expect=count)
        # user ids that repeat: every row of a requested id goes, the others keep their order
        rep = [i // 2 for i in range(n)]
        _check_remove(g, rep, [0, 1, rep[-1], 3], metric, q, f"n={n} dim={dim} {metric} repeated ids")


@pytest.mark.parametrize("metric", ["IP", "L2"])
def test_remove_in_chunks(metric):
    """MIRX_OPT_COMPACT_CHUNK_ROWS = 256 on 1000 rows: four source chunks, the last one partial."""
    n, dim = 1000, 130
    g, ids = _unit(n, dim, 3), list(range(100, 100 + n))
    q = torch.cat([g[300:302], _unit(2, dim, 6)])
    cases = {"every other": ids[::2], "run over a chunk boundary": ids[250:263], "one whole chunk": ids[256:512],
             "a chunk and its neighbours' edges": ids[255:513], "all but the last chunk": ids[:768], "first chunk and tail": ids[:256] + ids[990:]}
    for name, request in cases.items():
        _check_remove(g, ids, request, metric, q, f"chunk 256 {metric} {name}", chunk=256, expect=len(request))
    # chunks that are no multiple of anything, and chunks of one row
    _check_remove(g[:100], ids[:100], ids[:100:3], metric, q, f"chunk 7 {metric}", chunk=7)
    _check_remove(g[:50], ids[:50], ids[1:50:2], metric, q, f"chunk 1 {metric}", chunk=1)


def test_remove_takes_device_and_host_id_lists():
    n, dim = 600, 8
    g, ids = _unit(n, dim, 8), list(range(n))
    q = _unit(3, dim, 9)
    request = ids[5:400:7]
    a = _check_remove(g, ids, request, "IP", q, "host list", request_device="cpu")
    b = _check_remove(g, ids, request, "IP", q, "device list", request_device="cuda:0")
    assert torch.equal(a.rows()[1], b.rows()[1]) and torch.equal(_bits(a.rows()[0]), _bits(b.rows()[0]))
    assert a.remove([]) == 0 and a.remove(torch.empty(0, dtype=torch.int64, device="cuda:0")) == 0
    assert a.remove([[10 ** 6, 10 ** 6 + 1], [10 ** 6 + 2, 5]]) == 3          # any shape: the added rows' ids, 5 was removed


def test_auto_ids_go_on_past_removed_rows():
    """mirx_index_add without ids after a removal: not `size + i`, which a surviving row already carries."""
    from mirx.index import FlatIndex
    g = _unit(10, 8, 1)
    ix = FlatIndex(8, "IP", 0)
    ix.add(g)                                           # ids 0..9
    assert ix.remove([0, 4]) == 2
    ix.add(_unit(2, 8, 2))
    assert ix.rows()[1].tolist() == [1, 2, 3, 5, 6, 7, 8, 9, 10, 11]
    assert ix.remove([11]) == 1
    ix.add(_unit(1, 8, 3))
    assert ix.rows()[1].tolist() == [1, 2, 3, 5, 6, 7, 8, 9, 10, 12]


@pytest.mark.parametrize("n", [700, 40000], ids=["exact scan", "filter pass pending"])
def test_remove_between_search_begin_and_end_is_a_state_error(n):
    L = _lib()
    dim = 8
    g, ids = _unit(n, dim, 4), torch.arange(n, dtype=torch.int64)
    q = _unit(5, dim, 12)
    ix, other = _index(g, "IP", ids), _index(g, "IP", ids)
    handle = ix.search_begin(q, 10)
    req = torch.tensor([1, 2, 3], dtype=torch.int64)
    removed = ctypes.c_int64(-7)
    rc = L.load().mirx_index_remove_ids(ix._h, ctypes.c_void_p(req.data_ptr()), 3, ctypes.byref(removed), None)
    assert rc == L.ESTATE == -4 and b"search_end" in L.load().mirx_last_error()
    with pytest.raises(L.MirxError, match=r"\(-4\)"):
        ix.remove(req)
    s1, h1 = ix.search_end(handle, return_f64=True)
    s2, h2 = other.search(q, 10, return_f64=True)
    assert len(ix) == n and torch.equal(h1, h2) and torch.equal(s1, s2)
    assert ix.remove(req) == 3 and len(ix) == n - 3     # and afterwards it is an ordinary call again


def test_two_identical_removals_leave_identical_buffers():
    n, dim = 2 * _tile() + 3, 130
    g, ids = _unit(n, dim, 21) * 2.0, torch.arange(n, dtype=torch.int64) * 2
    request = ids[torch.randperm(n, generator=torch.Generator().manual_seed(2))[: n // 3]]
    q = _unit(4, dim, 22)
    out = []
    for _ in range(2):
        ix = _index(g, "L2", ids, chunk=512)
        assert ix.remove(request.to("cuda:0")) == n // 3
        rows, rid = ix.rows()
        ranks, vals = ix.rank_all(q, with_scores=True)
        out.append((_bits(rows), rid.cpu(), ranks.cpu(), _bits(vals)))
    assert all(torch.equal(a, b) for a, b in zip(*out))


@pytest.mark.parametrize("metric", ["IP", "L2"])
def test_remove_keeps_the_filter_pass_exact(metric):
    """Enough survivors (>= 32768) that search() runs its bf16 filter GEMM over the bf16 copy, the bias and the last tile's
    zero padding: all three must have moved with the rows.  Several chunks."""
    n, dim = 45000, 64
    g = _unit(n, dim, 31)
    ids = torch.arange(n, dtype=torch.int64) + 5
    request = torch.cat([ids[::16], ids[250:3000], ids[-40:]])
    keep = ~torch.isin(ids, request)
    assert int(keep.sum()) >= 32768 + NEW_ROWS
    q = torch.nn.functional.normalize(g[keep][1000:1016] + 0.05 * _unit(16, dim, 32), dim=1)
    ix = _index(g, metric, ids, chunk=4096)
    assert ix.remove(request) == int((~keep).sum())
    fresh = _index(g[keep], metric, ids[keep])
    for tag in ("removed", "removed +300"):
        s1, h1 = ix.search(q, 10, return_f64=True)
        st = ix.last_stats()
        s2, h2 = fresh.search(q, 10, return_f64=True)
        print(tag, metric, "stats after remove", st, "fresh", fresh.last_stats())
        assert st["tier1_answered"] > 0, st
        assert torch.equal(h1, h2) and torch.equal(s1, s2), tag
        r1, i1 = ix.rows()
        r2, i2 = fresh.rows()
        assert torch.equal(i1, i2) and torch.equal(_bits(r1), _bits(r2)), tag
        more, more_ids = _unit(NEW_ROWS, dim, 33), torch.arange(NEW_ROWS, dtype=torch.int64) + 10 ** 6
        ix.add(more, more_ids)
        fresh.add(more, more_ids)
