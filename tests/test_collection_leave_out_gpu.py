"""Collection.search(leave_out_field=, leave_out_values=) and MilvusRetriever.search / batch_search(leave_out=)
against what a caller could do before: one Collection.search(expr='<field> != <value>') per query.  Hit for hit: ids, distances
(fp32 bits) and entities.  GPU only."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_D, _N, _NQ = 64, 32768 + 300, 8
_FIELDS = ["image_path", "label", "patient", "site"]


def _rows(rng, n, dim):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.fixture(scope="module")
def world():
    """one COSINE collection: `patient` (int) groups of 8 rows scattered over the gallery, each group a tight cluster, so a query
    near one study finds its patient's other studies first; `site` (str) five values"""
    from mirx.retriever import Collection
    rng = np.random.default_rng(38)
    patient = rng.permutation(_N) // 8
    centers = _rows(rng, int(patient.max()) + 1, _D)
    emb = centers[patient] + 0.02 * rng.standard_normal((_N, _D)).astype(np.float32)
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(np.float32)
    col = Collection("leave_out", _D, extra_fields=("patient", "site"))
    col.insert([[f"img/{i}.png" for i in range(_N)], [i % 3 for i in range(_N)], emb, [int(p) for p in patient],
                [f"s{i % 5}" for i in range(_N)]])
    rows = (np.arange(_NQ) * 4099 + 17) % _N
    q = emb[rows] + 0.01 * rng.standard_normal((_NQ, _D)).astype(np.float32)
    return col, q.astype(np.float32), rows, patient


def _flat(hits):
    return [(h.id, np.float32(h.distance).tobytes(), tuple(h.entity.get(f) for f in _FIELDS)) for h in hits]


def _literal(v):
    return json.dumps(v)


def _compare(col, q, field, values, limit, expr=None, exclude_ids=None):
    got = col.search(q, limit=limit, output_fields=_FIELDS, leave_out_field=field, leave_out_values=values, expr=expr,
                     exclude_ids=exclude_ids)
    assert len(got) == q.shape[0]
    for i, v in enumerate(values):
        parts = ([] if v is None else [f"{field} != {_literal(v)}"]) + ([] if expr is None else [f"({expr})"])
        want = col.search(q[i:i + 1], limit=limit, output_fields=_FIELDS, expr=" and ".join(parts) or None,
                          exclude_ids=None if exclude_ids is None else exclude_ids[i:i + 1])[0]
        assert _flat(got[i]) == _flat(want), (field, i, v)
        if v is not None:
            assert all(h.entity.get(field) != v for h in got[i])
    return got


@pytest.mark.parametrize("limit", [10, 100])
def test_leave_out_equals_one_filtered_search_per_query(world, limit):
    col, q, rows, patient = world
    own = [int(patient[r]) for r in rows]
    plain = col.search(q, limit=limit, output_fields=_FIELDS)
    assert all(plain[i][0].entity.get("patient") == own[i] for i in range(_NQ))       # the leak: the query's own patient first
    got = _compare(col, q, "patient", own, limit)
    assert all(len(h) == limit for h in got)
    _compare(col, q, "patient", own, limit, expr='label != 1 and site in ["s0", "s1", "s3"]')
    ex = col.live_ids()[rows]
    _compare(col, q, "patient", own, limit, exclude_ids=ex)
    _compare(col, q, "patient", own, limit, expr="label == 2", exclude_ids=ex)
    # None and a value the collection does not hold leave nothing out
    mixed = own[:3] + [None, 10 ** 7, None] + own[6:]
    got = _compare(col, q, "patient", mixed, limit)
    for i in (3, 4, 5):
        assert _flat(got[i]) == _flat(plain[i])
    # a string field: a fifth of the gallery per value
    _compare(col, q, "site", [f"s{i % 5}" for i in range(_NQ)], limit)
    _compare(col, q, "site", ["s1", None, "nowhere", "s4", "s0", "s0", None, "s2"], limit, expr="label != 0", exclude_ids=ex)
    _compare(col, q, "image_path", [f"img/{r}.png" for r in rows], limit)              # the reference's own field: one row each


def test_after_delete_and_compact(world):
    from mirx.retriever import Collection
    col0, q, rows, patient = world
    rng = np.random.default_rng(39)
    emb, _ = col0.index.rows()
    col = Collection("leave_out_2", _D, extra_fields=("patient", "site"))
    col.insert([col0.field("image_path"), col0.field("label"), emb.cpu(), col0.field("patient"), col0.field("site")])
    own = [int(patient[r]) for r in rows]
    before = _compare(col, q, "patient", own, 10)
    gone = sorted({int(h.id) for hits in before for h in hits[:3]} | {int(i) for i in rng.integers(0, _N, 200)})
    assert col.delete(f"id in {gone}").delete_count == len(gone)
    after = _compare(col, q, "patient", own, 10)
    assert not {h.id for hits in after for h in hits} & set(gone)
    col.compact()
    assert [_flat(h) for h in _compare(col, q, "patient", own, 10)] == [_flat(h) for h in after]
    _compare(col, q, "site", ["s0"] * _NQ, 100, exclude_ids=col.live_ids()[:_NQ])


def test_retriever_search_and_batch_search(world):
    from mirx.retriever import MilvusRetriever
    col, q, rows, patient = world
    table = torch.from_numpy(q)

    class _Model(torch.nn.Module):
        def forward(self, x):
            return x.reshape(x.shape[0], -1)

    r = MilvusRetriever(None, "stub", _Model(), lambda img: table[img].reshape(1, 8, 8))
    r.collection = col
    own = [int(patient[x]) for x in rows]
    keys = ["id", "image_path", "label", "distance", "similarity"]
    singles = []
    for i in range(_NQ):
        got, _ = r.search(i, top_k=10, leave_out=("patient", own[i]))
        want, _ = r.search(i, top_k=10, expr=f"patient != {own[i]}")
        assert got == want and len(got) == 10 and list(got[0]) == keys
        singles.append(got)
    assert r.batch_search(list(range(_NQ)), top_k=10, leave_out=("patient", own)) == singles
    got = r.batch_search(list(range(_NQ)), top_k=10, leave_out=("site", ["s2"] * _NQ), expr="label == 1")
    assert got == r.batch_search(list(range(_NQ)), top_k=10, expr='label == 1 and site != "s2"')
    assert r.batch_search(list(range(_NQ)), top_k=10, leave_out=("patient", [None] * _NQ)) == r.batch_search(list(range(_NQ)), top_k=10)
    with pytest.raises(ValueError):
        r.batch_search(list(range(_NQ)), top_k=10, leave_out=("patient", own[:-1]))


def test_file_backed_collection_reloaded(world, tmp_path):
    """a stored NIH-schema collection, flushed, dropped from the process and opened again from its files: the same hits as the
    collection that wrote them, with the string field `image_name` standing for the patient"""
    from mirx import nih
    col0, _, rows, patient = world
    n = 4000
    rng = np.random.default_rng(40)
    emb = _rows(rng, n, nih.EMBEDDING_DIM)
    names = [f"patient{int(p) % 400:04d}" for p in patient[:n]]
    col = nih.create_nih_collection("lo_store", store=tmp_path)
    col.insert([[f"img/{i}.png" for i in range(n)], names, ["a|b"] * n, ["[]"] * n, emb])
    col.flush()
    q = emb[[5, 1234, 3999]] + 0.01 * rng.standard_normal((3, nih.EMBEDDING_DIM)).astype(np.float32)
    vals = [names[5], names[1234], None]
    fields = ["image_path", "image_name"]
    want = col.search(q, limit=20, output_fields=fields, leave_out_field="image_name", leave_out_values=vals)
    mine = [key for key in nih._STORED if key[1] == "lo_store"]
    assert len(mine) == 1
    nih._STORED.pop(mine[0])                                        # forget it: the next open reads the files
    back = nih.get_nih_collection("lo_store", store=tmp_path)
    assert back is not col and back.num_entities == n
    got = back.search(q, limit=20, output_fields=fields, leave_out_field="image_name", leave_out_values=vals)
    flat = lambda hits: [(h.id, np.float32(h.distance).tobytes(), h.entity.get("image_path"), h.entity.get("image_name")) for h in hits]
    assert [flat(h) for h in got] == [flat(h) for h in want]
    for i, v in enumerate(vals[:2]):
        ref = back.search(q[i:i + 1], limit=20, output_fields=fields, expr=f'image_name != "{v}"')[0]
        assert flat(got[i]) == flat(ref) and all(h.entity.get("image_name") != v for h in got[i])
    for key in [key for key in nih._STORED if key[1] == "lo_store"]:
        nih._STORED.pop(key)
