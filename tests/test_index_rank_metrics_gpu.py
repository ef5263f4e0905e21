"""mirx_index_rank_metrics (FlatIndex.rank_metrics) on the MI355X: the fused, streaming call against the composition it
stands for -- FlatIndex.rank_all followed by the grouped walk over that ranking, labels and codes mapped from row order to ids.
Integer outputs equal, AP within 1e-12, NaN in the same places.  Shapes: more queries than one batch of the radix ranking (1024),
more rows than one segment of the walk (4096) and than the bitonic sort's reach (65536), and the sizes around a segment."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
K3 = (1, 5, 10)
K8 = (1, 2, 5, 10, 64, 100, 4096, 5000)


def _index(g, metric, ids=None):
    from mirx.index import FlatIndex
    ix = FlatIndex(g.shape[1], metric, 0)
    ix.add(g, ids)
    return ix


def _compose(ix, q, ex, self_kind, row_labels, qlabels, row_codes, qcodes, kappas, jaccard=None, standard_ap=False):
    """rank_all, then the walk over the [nq, size] ranking with labels and codes indexed by id"""
    from mirx.metrics import rank_metrics_device
    ids = ix.ids().to(DEV)
    table = int(ids.max()) + 1 if ids.numel() else 0
    gl = torch.zeros(table, dtype=torch.int64, device=DEV)
    gl[ids] = row_labels
    gc = None
    if row_codes is not None:
        gc = torch.full((table,), -1, dtype=torch.int32, device=DEV)
        gc[ids] = row_codes
    ranks = ix.rank_all(q, exclude_ids=ex)
    res = rank_metrics_device(ranks, gl, qlabels, kappas, query_ids=None if self_kind == 0 else ex, drop_self=self_kind == 2,
                              jaccard_threshold=jaccard, standard_ap=standard_ap, gallery_codes=gc,
                              query_codes=None if gc is None else qcodes)
    return res, ranks


def _same(got, want, what=""):
    for k in ("cnt", "nrel", "maxpos"):
        assert torch.equal(got[k], want[k]), (what, k)
    a, b = got["ap"], want["ap"]
    assert torch.equal(torch.isnan(a), torch.isnan(b)), what
    ok = ~torch.isnan(a)
    assert ok.sum() == 0 or float((a[ok] - b[ok]).abs().max()) <= 1e-12, (what, float((a[ok] - b[ok]).abs().max()))


def _bits(res):
    return torch.cat([res["ap"].view(torch.int64), res["nrel"], res["maxpos"], res["cnt"].reshape(-1)])


def _check(ix, q, ex, self_kind, rl, ql, rc, qc, kappas=K3, jaccard=None, standard_ap=False, what=""):
    got = ix.rank_metrics(q, rl, ql, kappas, exclude_ids=ex, self_kind=self_kind, row_codes=rc, query_codes=qc,
                          jaccard_threshold=jaccard, standard_ap=standard_ap)
    want, ranks = _compose(ix, q, ex, self_kind, rl, ql, rc, qc, kappas, jaccard, standard_ap)
    _same(got, want, what)
    return got, ranks


def _world(n, d, seed, n_out=0, classes=3, group=5):
    g = torch.Generator().manual_seed(seed)
    rows = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)
    q = torch.cat([rows, torch.nn.functional.normalize(torch.randn(n_out, d, generator=g), dim=1)])
    rl = torch.randint(0, classes, (n,), generator=g)
    ql = torch.cat([rl, torch.randint(0, classes, (n_out,), generator=g)])
    rc = (torch.randperm(n, generator=g) // group).to(torch.int32)    # groups of `group` rows, dealt at random
    rc[torch.rand(n, generator=g) < 0.05] = -1                        # rows without a code
    qc = torch.cat([rc, torch.randint(-1, max(n // group, 1), (n_out,), generator=g).to(torch.int32)])
    ex = torch.cat([torch.arange(n), torch.full((n_out,), -1, dtype=torch.int64)])
    return rows, q, rl.to(DEV), ql, rc.to(DEV), qc, ex


@pytest.fixture(scope="module")
def w1000():
    return _world(1000, 100, 1, n_out=30)


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("self_kind", [0, 1, 2])
@pytest.mark.parametrize("codes", [False, True], ids=["plain", "codes"])
def test_more_queries_than_one_batch(w1000, metric, self_kind, codes):
    rows, q, rl, ql, rc, qc, ex = w1000
    assert q.shape[0] == 1030                                         # radix_plan batches 1024 queries
    ix = _index(rows, metric)
    got, _ = _check(ix, q, ex, self_kind, rl, ql, rc if codes else None, qc if codes else None)
    assert int(torch.isnan(got["ap"]).sum()) == 0 and int(got["nrel"].min()) > 100


def test_bit_masks_standard_ap_and_eight_kappas(w1000):
    rows, q, _, _, rc, qc, ex = w1000
    g = torch.Generator().manual_seed(2)
    bits = (torch.rand(1000, 14, generator=g) < 0.12).to(torch.int64)
    masks = (bits << torch.arange(14)).sum(dim=1)
    qm = torch.cat([masks, masks[:30]])
    ix = _index(rows, "IP")
    for kind in (0, 1):
        got, _ = _check(ix, q, ex, kind, masks.to(DEV), qm, rc, qc, K8, jaccard=0.4, standard_ap=True, what=f"kind {kind}")
    assert int(torch.isnan(got["ap"]).sum()) > 0                      # images without a label: no relevant row, NaN on both sides
    _check(ix, q[:7], ex[:7], 2, masks.to(DEV), qm[:7], None, None, (), jaccard=0.25)       # no kappa at all


def test_a_query_alone_and_among_1030_and_twice(w1000):
    rows, q, rl, ql, rc, qc, ex = w1000
    ix = _index(rows, "L2")
    call = lambda s: ix.rank_metrics(q[s], rl, ql[s], K3, exclude_ids=ex[s], self_kind=0, row_codes=rc, query_codes=qc[s])
    whole = call(slice(0, 1030))
    again = call(slice(0, 1030))
    assert torch.equal(_bits(whole), _bits(again))
    for i in (0, 517, 1023, 1024, 1029):
        one = call(slice(i, i + 1))
        assert one["ap"].view(torch.int64)[0] == whole["ap"].view(torch.int64)[i], i    # the bits, not a tolerance
        assert one["nrel"][0] == whole["nrel"][i] and torch.equal(one["cnt"][0], whole["cnt"][i])
    part = call(slice(500, 700))
    assert torch.equal(part["ap"].view(torch.int64), whole["ap"].view(torch.int64)[500:700])


def test_past_the_bitonic_reach_group_in_first_middle_and_last_segment():
    n, d, nq = 70001, 32, 5
    g = torch.Generator().manual_seed(3)
    rows = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)
    src = torch.tensor([0, 1234, 35000, 69999, 70000])
    q, ex = rows[src], src.clone()
    rl = torch.randint(0, 4, (n,), generator=g).to(DEV)
    ix = _index(rows, "COSINE")
    ranks = ix.rank_all(q, exclude_ids=ex).cpu()
    # query i's group: the rows its own ranking holds at these positions (first, a middle and the last segment of 4096), and
    # the query's row; every other row in a group of eight
    where = torch.tensor([0, 1, 4095, 4096, 40000, 40001, 69990, 69999])
    rc = (torch.randperm(n, generator=g) // 8 + 10).to(torch.int32)
    for i in range(nq):
        rc[ranks[i][where]] = i
        rc[src[i]] = i
    rc = rc.to(DEV)
    qc = torch.arange(nq, dtype=torch.int32)
    assert all(int((rc[ranks[i].to(DEV)][where.to(DEV)] == i).sum()) >= 6 for i in range(nq))   # (another query may have claimed a row)
    kappas = (1, 5, 10, 4090, 4096, 40000, 69000, 70001)
    for kind in (0, 1, 2):
        got, _ = _check(ix, q, ex, kind, rl, rl[src.to(DEV)].cpu(), rc, qc, kappas, what=f"kind {kind}")
        plain, _ = _check(ix, q, ex, kind, rl, rl[src.to(DEV)].cpu(), None, None, kappas, what=f"plain kind {kind}")
    assert int(got["nrel"].min()) > 15000 and not torch.equal(got["maxpos"], plain["maxpos"])
    one = ix.rank_metrics(q[3:4], rl, rl[src[3:4].to(DEV)].cpu(), kappas, exclude_ids=ex[3:4], self_kind=2, row_codes=rc,
                          query_codes=qc[3:4])
    assert torch.equal(_bits(one), torch.cat([got["ap"].view(torch.int64)[3:4], got["nrel"][3:4], got["maxpos"][3:4], got["cnt"][3]]))


@pytest.mark.parametrize("n", [1, 63, 4096, 4097])
def test_sizes_around_a_segment(n):
    rows, q, rl, ql, rc, qc, ex = _world(n, 16, 40 + n, n_out=3, classes=2, group=3)
    sel = torch.cat([torch.arange(min(n, 4)), torch.arange(n, n + 3)])                      # a few rows as queries, and outside ones
    for metric in ("COSINE", "L2"):
        ix = _index(rows, metric)
        for kind in (0, 1, 2):
            _check(ix, q[sel], ex[sel], kind, rl, ql[sel], rc, qc[sel], K8, what=f"{metric} kind {kind}")
        _check(ix, q[sel], None, 0, rl, ql[sel], rc, qc[sel], K3, standard_ap=True, what="no exclude")
    # the whole gallery is one group: nothing is left
    ix = _index(rows, "COSINE")
    res = ix.rank_metrics(q[:1], rl, ql[:1], K3, row_codes=torch.zeros(n, dtype=torch.int32, device=DEV), query_codes=[0])
    assert torch.isnan(res["ap"]).all() and int(res["nrel"][0]) == 0 and int(res["maxpos"][0]) == 0 and int(res["cnt"].sum()) == 0


def test_ids_out_of_row_order_after_remove_and_identical_rows():
    n, d = 500, 24
    rows, q, rl, ql, rc, qc, ex = _world(n, d, 7, n_out=4)
    rows = rows.clone()
    rows[100:140] = rows[60:100]                                      # exact ties, decided by id
    rows[300:] = rows[299]                                            # 201 identical rows
    g = torch.Generator().manual_seed(8)
    ids = torch.randperm(n, generator=g) * 3 + 5                      # ids do not ascend with the row: the idperm path
    q = torch.cat([rows, q[n:]])
    ex = torch.cat([ids, torch.full((4,), -1, dtype=torch.int64)])
    ix = _index(rows, "COSINE", ids)
    for kind in (0, 1, 2):
        _, ranks = _check(ix, q, ex, kind, rl, ql, rc, qc, what=f"idperm kind {kind}")
    tied = ranks[0].cpu()                                             # the ties really are in id order in what was compared
    pos = {int(v): p for p, v in enumerate(tied.tolist())}
    order = sorted(ids[300:].tolist())
    assert [pos[v] for v in order] == sorted(pos[v] for v in order)
    gone = ids[torch.randperm(n, generator=g)[:77]]
    assert ix.remove(gone) == 77
    keep = ~torch.isin(ids, gone)
    keep_q = torch.cat([keep, torch.ones(4, dtype=torch.bool)])
    rl2, rc2 = rl[keep.to(DEV)], rc[keep.to(DEV)]
    got, _ = _check(ix, q[keep_q], ex[keep_q], 2, rl2, ql[keep_q], rc2, qc[keep_q], what="after remove")
    fresh = _index(rows[keep], "COSINE", ids[keep])
    again = fresh.rank_metrics(q[keep_q], rl2, ql[keep_q], K3, exclude_ids=ex[keep_q], self_kind=2, row_codes=rc2, query_codes=qc[keep_q])
    assert torch.equal(_bits(got), _bits(again))


def test_busy_index_and_refusals(w1000):
    from mirx import _lib as L
    from mirx.index import FlatIndex
    rows, q, rl, ql, rc, qc, ex = w1000
    ix = _index(rows, "COSINE")
    q, ql, qc, ex = q[:6], ql[:6], qc[:6], ex[:6]
    ok = ix.rank_metrics(q, rl, ql, K3, exclude_ids=ex, row_codes=rc, query_codes=qc)
    h = ix.search_begin(q, 10)
    with pytest.raises(L.MirxError, match=r"\(%d\).*mirx_index_search_end" % L.ESTATE):
        ix.rank_metrics(q, rl, ql, K3, exclude_ids=ex, row_codes=rc, query_codes=qc)
    ix.search_end(h)
    assert torch.equal(_bits(ix.rank_metrics(q, rl, ql, K3, exclude_ids=ex, row_codes=rc, query_codes=qc)), _bits(ok))
    for bad in (rl.cpu(), rl.to(torch.int32), rl[:-1], rl.cpu().numpy(), rl.reshape(1, -1)):
        with pytest.raises(ValueError, match="row_labels"):
            ix.rank_metrics(q, bad, ql)
    for bad in (rc.cpu(), rc.to(torch.int64), rc[:-1], rc.reshape(-1, 1)):
        with pytest.raises(ValueError, match="row_codes"):
            ix.rank_metrics(q, rl, ql, row_codes=bad, query_codes=qc)
    with pytest.raises(ValueError, match="come together"):
        ix.rank_metrics(q, rl, ql, row_codes=rc)
    with pytest.raises(ValueError, match="come together"):
        ix.rank_metrics(q, rl, ql, query_codes=qc)
    with pytest.raises(ValueError, match="query_labels"):
        ix.rank_metrics(q, rl, ql[:-1])
    with pytest.raises(ValueError, match="query_codes"):
        ix.rank_metrics(q, rl, ql, row_codes=rc, query_codes=qc[:-1])
    with pytest.raises(ValueError, match="integers"):
        ix.rank_metrics(q, rl, ql.to(torch.float32))
    with pytest.raises(ValueError, match="self_kind"):
        ix.rank_metrics(q, rl, ql, self_kind=3)
    for kind in (1, 2):
        with pytest.raises(ValueError, match="needs exclude_ids"):
            ix.rank_metrics(q, rl, ql, self_kind=kind)
    with pytest.raises(ValueError, match="kappas"):
        ix.rank_metrics(q, rl, ql, kappas=range(1, 10))
    with pytest.raises(ValueError, match="kappas"):
        ix.rank_metrics(q, rl, ql, kappas=(0,))
    with pytest.raises(ValueError, match="queries"):
        ix.rank_metrics(q[:, :50], rl, ql)
    # no query: empty results; no row: nothing is relevant
    none = ix.rank_metrics(q[:0], rl, ql[:0], K3)
    assert none["ap"].shape == (0,) and none["cnt"].shape == (0, 3)
    empty = FlatIndex(100, "COSINE", 0)
    res = empty.rank_metrics(q, rl[:0], ql, K3, row_codes=rc[:0], query_codes=qc)
    assert torch.isnan(res["ap"]).all() and int(res["nrel"].sum()) == 0 and int(res["cnt"].sum()) == 0 and int(res["maxpos"].sum()) == 0
