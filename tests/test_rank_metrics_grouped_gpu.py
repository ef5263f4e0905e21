"""mirx_rank_metrics_grouped (metrics.rank_metrics_device(gallery_codes=, query_codes=)) on the MI355X against the
float64 restatement (tests/_rank_metrics_ref.py): integer outputs equal, AP within 1e-12 (the bar of the metric goldens, DESIGN
10), NaN in the same places.  One wavefront walks a list 64 entries at a time, so the lists are sized and the taken-out entries
placed around that step."""
import numpy as np
import pytest
import torch

import _rank_metrics_ref as R

pytestmark = pytest.mark.gpu

K3 = (1, 5, 10)
K8 = (1, 2, 5, 10, 63, 64, 65, 200)


def _device(ranks, gl, ql, kappas, **kw):
    from mirx.metrics import rank_metrics_device
    r = ranks if torch.is_tensor(ranks) else torch.as_tensor(np.asarray(ranks, dtype=np.int64)).cuda()
    return rank_metrics_device(r, np.asarray(gl, dtype=np.int64), np.asarray(ql, dtype=np.int64), kappas, **kw)


def _check(ranks, gl, ql, kappas=K3, query_ids=None, drop_self=False, gc=None, qc=None, jaccard=None, standard_ap=False):
    got = _device(ranks, gl, ql, kappas, query_ids=query_ids, drop_self=drop_self, gallery_codes=gc, query_codes=qc,
                  jaccard_threshold=jaccard, standard_ap=standard_ap)
    want = R.metrics(np.asarray(ranks), gl, ql, kappas, query_ids, drop_self and query_ids is not None, gc, qc, jaccard, standard_ap)
    for k in ("cnt", "nrel", "maxpos"):
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k], err_msg=k)
    ap = got["ap"].cpu().numpy()
    np.testing.assert_array_equal(np.isnan(ap), np.isnan(want["ap"]))
    np.testing.assert_allclose(ap, want["ap"], rtol=0, atol=1e-12)
    return want


def _lists(rng, nq, n, n_ids=None):
    n_ids = n if n_ids is None else n_ids
    return np.stack([rng.permutation(n_ids)[:n] for _ in range(nq)]).astype(np.int64)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1000])
@pytest.mark.parametrize("standard_ap", [False, True])
def test_list_lengths_around_the_step(n, standard_ap):
    rng = np.random.default_rng(n)
    nq = 9                                                            # more than one block of four lists
    ranks = _lists(rng, nq, n)
    gl = rng.integers(0, 3, n)
    gc = rng.integers(-1, max(2, n // 6), n).astype(np.int32)         # -1: a row without a code is never left out
    src = rng.integers(0, n, nq)                                      # the query is image src[q]: its label, its code
    qc = gc[src].copy()
    qc[-1] = -1                                                       # a query without a code leaves nothing out
    want = _check(ranks, gl, gl[src], K3, gc=gc, qc=qc, standard_ap=standard_ap)
    assert n < 64 or (want["nrel"] > 0).any()


def _placed(n, where, rng):
    """a list of ids 0 .. n-1 in which the ids < len(where) sit at the positions `where` and the rest fill the gaps at random"""
    order = np.full(n, -1, dtype=np.int64)
    order[np.asarray(where)] = np.arange(len(where))
    order[order < 0] = rng.permutation(np.arange(len(where), n))
    return order


@pytest.mark.parametrize("where", [[0], [63], [62, 63, 64, 65, 66], list(range(64, 128)), [0, 63, 64, 127, 128, 199],
                                   list(range(200))], ids=["lane0", "lane63", "straddle", "whole-step", "edges", "everything"])
def test_where_the_taken_out_entries_sit(where):
    rng = np.random.default_rng(len(where))
    n = 200
    gc = np.where(np.arange(n) < len(where), 5, rng.integers(0, 4, n)).astype(np.int32)      # ids < len(where) are group 5
    gl = rng.integers(0, 2, n)
    gl[:len(where)] = 1                                               # the taken-out entries would all be hits
    ranks = np.stack([_placed(n, where, rng) for _ in range(5)])
    for standard_ap in (False, True):
        want = _check(ranks, gl, np.ones(5, dtype=np.int64), K8, gc=gc, qc=np.full(5, 5, dtype=np.int32), standard_ap=standard_ap)
    if len(where) == n:
        assert np.isnan(want["ap"]).all() and (want["nrel"] == 0).all() and (want["cnt"] == 0).all()
    else:
        assert (want["nrel"] == int(gl[len(where):].sum())).all()


@pytest.mark.parametrize("kappas", [(5,), K3, K8], ids=["1-kappa", "3-kappas", "8-kappas"])
def test_taken_out_positives_on_both_sides_of_every_kappa(kappas):
    """a positive that leaves sits just before and just after each kappa (raw and compacted), in turn and together; and 400 random
    short lists, where two labels and three groups reach every pattern around kappa = 1, 2, 5, 10"""
    n = 260
    gl = np.zeros(n, dtype=np.int64)
    gc = np.zeros(n, dtype=np.int32)
    ids = np.arange(n)                                                # the list is the identity: position = id
    lab = 1
    for kap in kappas:
        for gone in ([kap - 1], [kap], [kap - 1, kap], [max(kap - 2, 0), kap - 1], [0, kap]):
            pos = [p for p in {0, kap - 1, kap, kap + 1, n - 1} | set(gone) if 0 <= p < n]
            gl_q, gc_q = gl.copy(), gc.copy()
            gl_q[pos] = lab
            gc_q[[g for g in gone if g < n]] = lab
            _check(ids[None], gl_q, [lab], kappas, gc=gc_q, qc=np.array([lab], dtype=np.int32))
            _check(ids[None], gl_q, [lab], kappas, gc=gc_q, qc=np.array([lab], dtype=np.int32), standard_ap=True)
    rng = np.random.default_rng(7)
    m = 16
    _check(_lists(rng, 400, m), rng.integers(0, 2, m), rng.integers(0, 2, 400), kappas, gc=rng.integers(0, 3, m).astype(np.int32),
           qc=rng.integers(0, 3, 400).astype(np.int32))


@pytest.mark.parametrize("classes", [14, 63])
@pytest.mark.parametrize("standard_ap", [False, True])
def test_bit_mask_labels(classes, standard_ap):
    rng = np.random.default_rng(classes)
    n, nq = 300, 8
    bits = rng.random((n, classes)) < (0.2 if classes == 14 else 0.05)
    bits[:, classes - 1] |= rng.random(n) < 0.3                       # the top bit is in use (bit 62: the sign stays clear)
    masks = (bits.astype(np.int64) << np.arange(classes, dtype=np.int64)[None, :]).sum(axis=1)
    gc = rng.integers(-1, 40, n).astype(np.int32)
    src = rng.integers(0, n, nq)
    ranks = _lists(rng, nq, n)
    for thr in (0.25, 0.4):
        _check(ranks, masks, masks[src], K3, query_ids=src, gc=gc, qc=gc[src], jaccard=thr, standard_ap=standard_ap)


@pytest.mark.parametrize("drop_self", [False, True])
@pytest.mark.parametrize("with_ids", [False, True])
def test_self_entry_inside_and_outside_the_group(drop_self, with_ids):
    rng = np.random.default_rng(11)
    n, nq = 150, 12
    gl = rng.integers(0, 3, n)
    gc = rng.integers(0, 25, n).astype(np.int32)
    src = rng.integers(0, n, nq)
    qc = gc[src].copy()                                               # the self entry carries the query's code: inside the group
    qc[::3] = (qc[::3] + 1) % 25                                      # every third query leaves out ANOTHER group: self stays
    qc[1] = -1
    ranks = _lists(rng, nq, n)
    for standard_ap in (False, True):
        _check(ranks, gl, gl[src], K3, query_ids=src if with_ids else None, drop_self=drop_self, gc=gc, qc=qc, standard_ap=standard_ap)


def test_negative_query_codes_give_the_ungrouped_bits():
    rng = np.random.default_rng(3)
    n, nq = 333, 37
    gl = rng.integers(0, 4, n)
    src = rng.integers(0, n, nq)
    ranks = torch.as_tensor(_lists(rng, nq, n)).cuda()
    gc = rng.integers(-1, 9, n).astype(np.int32)
    for kw in ({}, {"query_ids": src}, {"query_ids": src, "drop_self": True}, {"standard_ap": True}):
        a = _device(ranks, gl, gl[src], K8, **kw)
        b = _device(ranks, gl, gl[src], K8, gallery_codes=gc, query_codes=np.full(nq, -1, dtype=np.int32), **kw)
        for k in ("cnt", "nrel", "maxpos"):
            assert torch.equal(a[k], b[k]), k
        assert torch.equal(a["ap"].view(torch.int64), b["ap"].view(torch.int64))         # the bits, NaN included
    masks = rng.integers(0, 1 << 14, n)
    a = _device(ranks, masks, masks[src], K3, jaccard_threshold=0.3)
    b = _device(ranks, masks, masks[src], K3, jaccard_threshold=0.3, gallery_codes=gc, query_codes=np.full(nq, -7, dtype=np.int32))
    assert all(torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) for k in a)


def test_ids_outside_the_label_table_and_null_row_codes():
    rng = np.random.default_rng(5)
    n_labels, n, nq = 100, 140, 6
    ranks = _lists(rng, nq, n, n_ids=n) - 20                          # ids -20 .. 119: below and above [0, 100)
    gl = rng.integers(0, 2, n_labels)
    gc = rng.integers(-1, 3, n_labels).astype(np.int32)
    gc[:10] = -1
    qc = np.array([0, 1, 2, -1, 0, 1], dtype=np.int32)
    want = _check(ranks, gl, np.ones(nq, dtype=np.int64), K3, gc=gc, qc=qc)
    # entries without a label stay in the list: the positions count them
    assert (want["maxpos"] > want["nrel"]).all()
    _check(ranks, gl, np.ones(nq, dtype=np.int64), K3, query_ids=np.full(nq, -1), drop_self=True, gc=gc, qc=qc, standard_ap=True)


def test_strided_view_of_the_ranks():
    rng = np.random.default_rng(9)
    n, nq = 130, 7
    wide = torch.full((nq, n + 9), -5, dtype=torch.int64, device="cuda")
    lists = _lists(rng, nq, n)
    wide[:, :n] = torch.as_tensor(lists).cuda()
    view = wide[:, :n]
    assert view.stride(0) == n + 9 and not view.is_contiguous()
    gl = rng.integers(0, 3, n)
    gc = rng.integers(0, 20, n).astype(np.int32)
    src = rng.integers(0, n, nq)
    got = _device(view, gl, gl[src], K3, gallery_codes=gc, query_codes=gc[src])
    want = R.metrics(lists, gl, gl[src], K3, gallery_codes=gc, query_codes=gc[src])
    np.testing.assert_array_equal(got["cnt"].cpu().numpy(), want["cnt"])
    np.testing.assert_array_equal(got["nrel"].cpu().numpy(), want["nrel"])
    np.testing.assert_allclose(got["ap"].cpu().numpy(), want["ap"], rtol=0, atol=1e-12)


def test_compute_map_and_multilabel_cuda_paths_take_groups(golden_dir):
    import json
    import os
    from mirx.metrics import compute_map, compute_map_multilabel
    with open(os.path.join(golden_dir, "grouped_300.json")) as fh:
        g = json.load(fh)
    labels, groups = np.asarray(g["labels"]), np.asarray(g["groups"])
    ranks = R.self_ranking(np.asarray(g["embeds"]), "l2")
    mAP, aps, pr, prs = compute_map(torch.as_tensor(ranks).cuda().t(), labels, g["kappas"], groups=groups)
    np.testing.assert_allclose(aps, np.asarray(g["aps"]), rtol=0, atol=1e-12)           # the reference's recorded outputs
    np.testing.assert_allclose(prs, np.asarray(g["prs"]), rtol=0, atol=1e-12)
    assert mAP == pytest.approx(float(np.mean(g["aps"])), abs=1e-12)
    multi = np.eye(3, dtype=np.float32)[labels]
    host = compute_map_multilabel(None, multi, 0.5, ranks=ranks.T, groups=groups)
    dev = compute_map_multilabel(None, multi, 0.5, ranks=torch.as_tensor(ranks).cuda().t(), groups=groups)
    assert dev == pytest.approx(host, abs=1e-12)


def test_python_refusals():
    from mirx.metrics import rank_metrics_device
    r = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="come together"):
        rank_metrics_device(r, [0, 0, 0, 0], [0, 0], gallery_codes=[0, 0, 0, 0])
    with pytest.raises(ValueError, match="come together"):
        rank_metrics_device(r, [0, 0, 0, 0], [0, 0], query_codes=[0, 0])
    with pytest.raises(ValueError, match="one gallery code"):
        rank_metrics_device(r, [0, 0, 0, 0], [0, 0], gallery_codes=[0, 0, 0], query_codes=[0, 0])
    with pytest.raises(ValueError, match="one gallery code"):
        rank_metrics_device(r, [0, 0, 0, 0], [0, 0], gallery_codes=[0, 0, 0, 0], query_codes=[0])
