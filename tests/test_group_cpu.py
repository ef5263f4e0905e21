"""Grouping search, the parts that need no GPU: the reference walk (tests/_group_ref.py) against a brute-force per-group sort,
Collection.search's argument checks on an empty in-memory collection, MilvusRetriever's result dicts, and the new entry points'
argument checks (MIRX_EINVAL before any HIP call)."""
import ctypes

import numpy as np
import pytest

import _group_ref as R


@pytest.mark.parametrize("seed", range(40))
def test_reference_walk_equals_the_per_group_sort(seed):
    """walk() over the full ranking == sorting every group on its own and ordering the groups by their best member: random
    sizes, scores drawn from a few values (ties everywhere, decided by id), limit above the number of groups, group_size above
    a group's rows."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 120))
    n_codes = int(rng.integers(1, max(2, n)))
    codes = rng.integers(0, n_codes, n)
    ids = rng.permutation(10 * n)[:n].astype(np.int64)
    scores = rng.choice(np.array([-1.5, -0.0, 0.0, 0.25, 0.5, 2.0]), n) if seed % 2 else rng.standard_normal(n)
    limit = int(rng.choice([1, 2, 3, n_codes, n_codes + 5]))
    group_size = int(rng.choice([1, 2, 3, 7, n + 1]))
    order = R.ranking_of(ids, scores)
    got = [(c, [int(order[p]) for p in kept]) for c, kept in R.walk(order, codes, limit, group_size)]
    assert got == R.brute_force(ids, scores, codes, limit, group_size)
    assert len(got) == min(limit, len(set(codes.tolist())))
    for c, rows in got:
        assert len(rows) == min(group_size, int((codes == c).sum()))          # a group is never short while it has rows left


def test_reference_prefix_state():
    group_of = np.array([0, 0, 1, 2, 2, 2])
    rows = np.bincount(group_of)
    # ranking 3 0 2 4 1 5 ; limit 2, group_size 2 -> groups 2 and 0
    full = [3, 0, 2, 4, 1, 5]
    assert R.prefix_state(full[:1], group_of, rows, -1, 2, 2) == (1, False, False)
    assert R.prefix_state(full[:2], group_of, rows, -1, 2, 2) == (2, False, True)          # final, both short
    assert R.prefix_state(full[:4], group_of, rows, -1, 2, 2) == (2, False, True)          # group 0 still short
    assert R.prefix_state(full[:5], group_of, rows, -1, 2, 2) == (2, True, True)
    assert R.prefix_state([3, -1], group_of, rows, -1, 2, 2) == (1, True, True)            # the list ended: nothing is missing
    # the excluded row is group 1's only row: two groups are left, limit 3 is reached with two open
    assert R.prefix_state([3, 0], group_of, rows, 1, 3, 1) == (2, True, True)
    assert R.prefix_state([3, 0], group_of, rows, -1, 3, 1) == (2, False, False)


def _empty_collection():
    from mirx.retriever import Collection
    return Collection("c", 8, extra_fields=("patient",))


def test_collection_search_validates_grouping_arguments_on_an_empty_collection():
    col = _empty_collection()
    q = np.zeros((2, 8), dtype=np.float32)
    assert col.search(q, limit=3, group_by_field="label") == [[], []]
    assert col.search(q, limit=3, group_by_field="patient", group_size=3, strict_group_size=False) == [[], []]
    with pytest.raises(ValueError, match="image_path.*label.*patient"):
        col.search(q, limit=3, group_by_field="diagnosis")
    with pytest.raises(ValueError):
        col.search(q, limit=3, group_by_field="embedding")                    # not a scalar field
    with pytest.raises(ValueError, match="group_size"):
        col.search(q, limit=3, group_by_field="label", group_size=0)
    with pytest.raises(ValueError, match="group_size"):
        col.search(q, limit=3, group_by_field="label", group_size=65)
    with pytest.raises(ValueError, match="16384"):
        col.search(q, limit=1024, group_by_field="label", group_size=17)
    with pytest.raises(ValueError, match="limit"):
        col.search(q, limit=1025, group_by_field="label")
    with pytest.raises(ValueError, match="limit"):
        col.search(q, limit=0, group_by_field="label")
    for param in ({"params": {"radius": 0.5}}, {"radius": 0.5, "range_filter": 0.9}):
        with pytest.raises(ValueError, match="range"):
            col.search(q, limit=3, group_by_field="label", param=param)
    assert col.search(q, limit=3, group_by_field="label", param={"params": {"nprobe": 10}}) == [[], []]
    assert col.search(q, limit=16, group_by_field="label", group_size=64) == [[], []]     # 1024 hits: inside every bound


def test_group_bounds():
    from mirx.index import group_bounds
    assert group_bounds(1, 1) == (1, 1) and group_bounds(1024, 16) == (1024, 16) and group_bounds(np.int64(256), 64) == (256, 64)
    for limit, gs in [(0, 1), (1025, 1), (1, 0), (1, 65), (1024, 17), (257, 64), (True, 1), (2.0, 1), ("3", 1), (3, None)]:
        with pytest.raises(ValueError):
            group_bounds(limit, gs)


def test_retriever_dicts_keep_their_keys_without_group_by():
    from mirx.retriever import Hit, MilvusRetriever
    hit = Hit(5, 0.75, {"image_path": "a.png", "label": "covid", "patient": 17})
    plain = MilvusRetriever._format(hit, "COSINE")
    assert list(plain) == ["id", "image_path", "label", "distance", "similarity"]
    grouped = MilvusRetriever._format(hit, "COSINE", "patient")
    assert list(grouped) == list(plain) + ["group"] and grouped["group"] == 17
    assert {k: grouped[k] for k in plain} == plain


def test_retriever_passes_grouping_only_when_asked(monkeypatch):
    """search() / batch_search() hand Collection.search the grouping keywords only with group_by: every other call is today's."""
    import torch
    from mirx.retriever import Hit, MilvusRetriever

    seen = []

    class _Col:
        metric_type = "COSINE"

        def search(self, **kw):
            seen.append(kw)
            nq = kw["data"].shape[0]
            return [[Hit(1, 0.5, {"image_path": "p", "label": "l"})] for _ in range(nq)]

    class _Model(torch.nn.Module):
        def forward(self, x):
            return x.reshape(x.shape[0], -1)[:, :4] + 1.0

    r = MilvusRetriever(None, "densenet121", _Model(), lambda img: torch.zeros(3, 2, 2))
    r.collection = _Col()
    monkeypatch.setattr(r, "_device", lambda: torch.device("cpu"))
    res, _ = r.search(object(), top_k=3)
    assert "group_by_field" not in seen[-1] and "group_size" not in seen[-1] and set(res[0]) == {"id", "image_path", "label", "distance", "similarity"}
    res, _ = r.search(object(), top_k=3, group_by="label", group_size=2)
    assert seen[-1]["group_by_field"] == "label" and seen[-1]["group_size"] == 2 and res[0]["group"] == "l"
    res = r.batch_search([object(), object()], top_k=3)
    assert "group_by_field" not in seen[-1] and "group" not in res[1][0]
    res = r.batch_search([object()], top_k=3, group_by="label")
    assert seen[-1]["group_by_field"] == "label" and seen[-1]["group_size"] == 1 and res[0][0]["group"] == "l"


def test_entry_points_refuse_bad_arguments_without_gpu():
    import mirx._lib as L
    lib = L.load()
    E = -1                                                                     # MIRX_EINVAL
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def walk(limit, gs, ranks=p, out=p, nq=1, depth=4, stride=4, n_groups=3, live=3):
        return lib.mirx_group_walk(ranks, None, None, nq, depth, stride, p, 8, p, n_groups, live, None, limit, gs, out, None, out,
                                   out, out, None)

    for limit, gs in [(0, 1), (1025, 1), (1, 0), (1, 65), (1024, 17), (-3, 1)]:
        assert walk(limit, gs) == E and b"group_walk" in lib.mirx_last_error()
    assert walk(3, 1, ranks=None) == E and b"null" in lib.mirx_last_error()
    assert walk(3, 1, out=None) == E and b"null" in lib.mirx_last_error()
    assert walk(3, 1, stride=3) == E                                           # row stride below the depth
    assert walk(3, 1, live=4) == E                                             # more live groups than codes
    assert walk(3, 1, nq=-1) == E
    # out_scores without scores
    assert lib.mirx_group_walk(p, None, None, 1, 4, 4, p, 8, p, 3, 3, None, 3, 1, p, p, p, p, p, None) == E

    assert lib.mirx_group_count(None, None, 5, 3, p, None) == E and b"group_count" in lib.mirx_last_error()
    assert lib.mirx_group_count(p, None, 5, 3, None, None) == E
    assert lib.mirx_group_count(p, None, -1, 3, p, None) == E
    assert lib.mirx_group_count(p, None, 5, -1, p, None) == E
    assert lib.mirx_group_count(p, None, 5, 2 ** 31, p, None) == E

    def fill(ix=None, limit=3, gs=1, max_members=8):
        return lib.mirx_index_group_fill(ix, p, 1, None, limit, gs, p, p, p, p, 1, p, 8, max_members, p, p, None)

    assert fill() == E and b"null index" in lib.mirx_last_error()
    assert lib.mirx_index_get_ids(None, 0, 0, None) == E and b"get_ids" in lib.mirx_last_error()
    assert (L.GROUP_MAX_LIMIT, L.GROUP_MAX_SIZE, L.GROUP_MAX_HITS, L.GROUP_FILL_MAX) == (1024, 64, 16384, 4096)
