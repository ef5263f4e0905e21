"""The reference's two-script flow on a persistent MilvusManager: one process fills a collection and flushes
(ingest_embeddings.py:399-411,532-534), ANOTHER process opens it by name and searches (evaluate_test_dataset_milvus.py:339-364).
Each script runs as a fresh child process (subprocess.run, one at a time); the parent holds the same gallery in memory and is
the yardstick: ids and fp64 ranking scores must be equal, bit for bit.  GPU only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DIM, BATCH, TOP_K = 1000, 64, 100, 10

_COMMON = '''
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from mirx import retriever as R

R.MODEL_CONFIGS["tiny"] = {"embedding_dim": %d, "description": "tiny test gallery",
                           "collection_names": {"default": "tiny_gallery"}}


def unit(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, %d, generator=g), dim=1)
''' % (DIM, DIM)

# ingest_embeddings.py: create_collection, insert in batches of 100, one flush at the end
_INGEST = _COMMON + '''
mgr = R.MilvusManager(uri=sys.argv[2])
assert mgr.connect()
col = mgr.create_collection("tiny", drop_old=True)
mgr.create_index("tiny", metric_type="COSINE")
rows = unit(%d, 1)
for s in range(0, %d, %d):
    col.insert([[f"img/{i}.png" for i in range(s, s + %d)], [i %% 5 for i in range(s, s + %d)], rows[s:s + %d].tolist()])
col.flush()
print("ingested", col.num_entities)
''' % (N, N, BATCH, BATCH, BATCH, BATCH)

# evaluate_test_dataset_milvus.py:339-364: a manager on the same uri, MilvusRetriever.load_collection(), searches
_EVALUATE = _COMMON + '''
mgr = R.MilvusManager(uri=sys.argv[2])
assert mgr.connect()
info = mgr.get_collection_info("tiny")                  # before anything is loaded
retriever = R.MilvusRetriever(mgr, "tiny", None, None)
col = retriever.load_collection()
q = unit(7, 2)
hits = retriever.search_ids(q, top_k=%d)
s64, ids = col.index.search(q, %d, return_f64=True)
np.savez(sys.argv[3], ids=ids.cpu().numpy(), s64=s64.cpu().numpy(),
         hits=np.array(json.dumps([[[h["id"], h["image_path"], h["label"], h["distance"]] for h in hs] for hs in hits])),
         num_entities=info["num_entities"], loaded=len(col.index))
''' % (TOP_K, TOP_K)


def _run(tmp_path, name, source, *args):
    script = tmp_path / name
    script.write_text(source)
    r = subprocess.run([sys.executable, str(script), ROOT, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def _unit(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, DIM, generator=g), dim=1)


def _tiny_config():
    from mirx import retriever as R
    R.MODEL_CONFIGS["tiny"] = {"embedding_dim": DIM, "description": "tiny test gallery",
                               "collection_names": {"default": "tiny_gallery"}}
    return R


@pytest.fixture(scope="module")
def ingested(tmp_path_factory):
    """the database child 1 wrote, and the same gallery in an in-memory collection of this process"""
    R = _tiny_config()
    tmp = tmp_path_factory.mktemp("flow")
    db = tmp / "db"
    out = _run(tmp, "ingest.py", _INGEST, db)
    assert f"ingested {N}" in out.stdout
    mem = R.MilvusManager(uri=None).create_collection("tiny")
    rows = _unit(N, 1)
    for s in range(0, N, BATCH):
        mem.insert([[f"img/{i}.png" for i in range(s, s + BATCH)], [i % 5 for i in range(s, s + BATCH)], rows[s:s + BATCH].tolist()])
    yield R, tmp, db, mem
    R.MODEL_CONFIGS.pop("tiny", None)


def _expected(R, mem):
    q = _unit(7, 2)
    retriever = R.MilvusRetriever(R.MilvusManager(uri=None), "tiny", None, None)
    retriever.collection = mem
    hits = retriever.search_ids(q, top_k=TOP_K)
    s64, ids = mem.index.search(q, TOP_K, return_f64=True)
    return ids.cpu().numpy(), s64.cpu().numpy(), [[[h["id"], h["image_path"], h["label"], h["distance"]] for h in hs] for hs in hits]


def _evaluate_in_a_child(tmp, db, tag):
    out = tmp / f"result_{tag}.npz"
    _run(tmp, "evaluate.py", _EVALUATE, db, out)
    return np.load(out)


def _assert_child_equals_parent(got, R, mem):
    ids, s64, hits = _expected(R, mem)
    assert int(got["num_entities"]) == int(got["loaded"]) == mem.num_entities
    np.testing.assert_array_equal(got["ids"], ids)
    np.testing.assert_array_equal(got["s64"], s64)                      # fp64 ranking scores, bit for bit
    assert json.loads(str(got["hits"])) == hits
    return hits


def test_flow_and_persistent_delete_across_processes(ingested):
    R, tmp, db, mem = ingested
    # 1. ingest in child 1 (the fixture), evaluate in child 2
    _assert_child_equals_parent(_evaluate_in_a_child(tmp, db, "flow"), R, mem)

    # 2. delete 37 rows by image_path in this process (nothing is loaded for it), flush; a child sees 963 rows and none of them
    gone = [f"img/{i}.png" for i in range(3, 1000, 27)]
    assert len(gone) == 37
    expr = "image_path in " + json.dumps(gone)
    col = R.MilvusManager(uri=str(db)).create_collection("tiny")
    assert col.num_entities == N and col.delete(expr).delete_count == 37 and col.num_entities == N - 37
    col.flush()
    assert mem.delete(expr).delete_count == 37                          # the resident yardstick: FlatIndex.remove
    for step in ("deleted", "compacted"):
        if step == "compacted":
            col.compact()
            assert os.path.getsize(db / "tiny_gallery" / "rows.1.f32") == (N - 37) * DIM * 4
        got = _evaluate_in_a_child(tmp, db, step)
        assert int(got["num_entities"]) == N - 37 == 963
        hits = _assert_child_equals_parent(got, R, mem)
        assert not {h[1] for hs in hits for h in hs} & set(gone), step

    # 3. the persistent collection made resident here, after the deletes: the same index as the yardstick's
    col.load()
    r1, i1 = col.index.rows()
    r2, i2 = mem.index.rows()
    assert torch.equal(i1, i2) and torch.equal(r1.view(torch.int32), r2.view(torch.int32))
    # resident and persistent at once: a delete reaches the index now, an insert gets a fresh id
    assert col.delete("id == 0").delete_count == 1 and len(col.index) == 962
    assert col.insert([["late.png"], [1], _unit(1, 5)]) == [N] and len(col.index) == 963
    assert col.search(_unit(1, 5), limit=1, output_fields=["image_path"])[0][0].entity.get("image_path") == "late.png"


def test_bounded_load_equals_the_default_load(ingested, monkeypatch):
    """Rows reach the index in pieces of at most mirx.store.LOAD_CHUNK_BYTES: with 4 KiB pieces (16 rows each) the index is the
    one the default piece size loads."""
    import mirx.store as S
    R, tmp, db, mem = ingested
    whole = R.MilvusManager(uri=str(db)).load_collection("tiny")
    calls = []
    from mirx.index import FlatIndex
    real_add = FlatIndex.add
    monkeypatch.setattr(FlatIndex, "add", lambda self, rows, ids=None: (calls.append(len(rows)), real_add(self, rows, ids))[1])
    monkeypatch.setattr(S, "LOAD_CHUNK_BYTES", 4096)
    pieces = R.MilvusManager(uri=str(db)).load_collection("tiny")
    assert calls and max(calls) <= 4096 // (DIM * 4) and len(calls) >= pieces.num_entities // 16
    r1, i1 = whole.index.rows()
    r2, i2 = pieces.index.rows()
    assert len(i1) == whole.num_entities and torch.equal(i1, i2) and torch.equal(r1.view(torch.int32), r2.view(torch.int32))
    q = _unit(5, 3)
    a, b = whole.index.search(q, TOP_K, return_f64=True), pieces.index.search(q, TOP_K, return_f64=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_nih_helpers_with_a_store(tmp_path):
    from mirx import nih
    rng = np.random.default_rng(4)
    emb = rng.standard_normal((40, nih.EMBEDDING_DIM)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    rows = [{"image_path": f"/d/{i}.npy", "image_name": f"{i}.npy", "label_names": ["Mass"] if i % 2 else [],
             "multi_hot": [i % 2] * 14, "embedding": emb[i]} for i in range(40)]
    mem = nih.create_nih_collection("nih_mem_for_store_test", drop_old=True)
    nih.insert_rows(mem, rows)
    col = nih.create_nih_collection("nih_t", store=tmp_path / "nih")
    assert col.is_persistent and nih.create_nih_collection("nih_t", store=tmp_path / "nih") is col
    nih.insert_rows(col, rows[:25])                                     # the drivers flush per batch
    nih.insert_rows(col, rows[25:])
    nih._STORED.clear()                                                 # what a new process starts with
    with pytest.raises(ValueError, match="does not exist"):
        nih.get_nih_collection("nih_other", store=tmp_path / "nih")
    with pytest.raises(ValueError, match="does not exist"):
        nih.get_nih_collection("nih_t")                                 # not in this process' memory: store= is needed
    back = nih.get_nih_collection("nih_t", store=str(tmp_path / "nih"))
    assert back is not col and back.num_entities == 40 and back.schema == mem.schema         # before anything is loaded
    for k in (5, 0):
        assert nih.query_gallery(back, rows[:6], top_k=k) == nih.query_gallery(mem, rows[:6], top_k=k)
    assert nih.search_collection(back, emb[3], 4) == nih.search_collection(mem, emb[3], 4)
    fresh = nih.create_nih_collection("nih_t", drop_old=True, store=tmp_path / "nih")
    assert fresh.num_entities == 0 and nih.get_nih_collection("nih_t", store=tmp_path / "nih") is fresh
    nih._COLLECTIONS.pop("nih_mem_for_store_test", None)
