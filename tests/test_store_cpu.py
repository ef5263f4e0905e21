"""mirx.store (the collection catalogue on disk) and what is wired to it on the host: Collection.flush / delete / compact on a
persistent collection that was never made resident, MilvusManager's uri handling, the delete expression parser.  No GPU: a
persistent collection touches no device until load()."""
import json
import os
import shutil

import numpy as np
import pytest

from mirx import store as S
from mirx.store import Store

NIH_SCHEMA = ["id", "image_path", "image_name", "label_text", "label_vector_json", "embedding"]
DEFAULT_SCHEMA = ["id", "image_path", "label", "embedding"]


def _rows(n, dim, seed=0):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


def _columns(schema, ids):
    cols = {}
    for f in schema:
        if f == "label":
            cols[f] = [int(i) % 7 for i in ids]                     # the default schema's label is an integer
        elif f == "label_vector_json":
            cols[f] = [json.dumps([int(i) % 2, 1]) for i in ids]
        elif f not in ("id", "embedding"):
            cols[f] = [f"{f}/é\n{int(i)}" for i in ids]         # non-ASCII and a newline: both must survive a JSON line
    return cols


def _files(path):
    return sorted(os.listdir(path))


def _read_all(col, chunk_bytes=None):
    parts = list(col.chunks(chunk_bytes))
    if not parts:
        return np.zeros((0,), np.int64), np.zeros((0, col.dim), np.float32)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


# ---- round trips ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schema", [DEFAULT_SCHEMA, NIH_SCHEMA], ids=["default", "nih"])
@pytest.mark.parametrize("dim", [1, 8, 130])
def test_round_trip_over_flushes(tmp_path, schema, dim):
    """1, 3 and 40 flushes (one of them with nothing new) give back every bit of the rows, the ids and the columns; the
    number of files does not grow with the number of flushes."""
    st = Store(tmp_path / "root")
    nfiles = {}
    for flushes in (1, 3, 40):
        name = f"c{flushes}"
        col = st.create(name, dim, "L2", schema, "a description")
        all_rows, at = _rows(5 * flushes, dim, seed=flushes), 0
        for k in range(flushes):
            m = 0 if (flushes > 1 and k == 1) else 5                # the second flush has nothing new
            ids = np.arange(at, at + m)
            col.append(ids, all_rows[at:at + m], _columns(schema, ids))
            at += m
            col.flush()
        nfiles[flushes] = len(_files(tmp_path / "root" / name))
        back = st.open(name, dim=dim, metric_type="L2", schema=schema)
        ids, rows = _read_all(back)
        assert back.rows == at and back.description == "a description" and back.next_id == at
        assert np.array_equal(ids, np.arange(at)) and ids.dtype == np.int64
        assert rows.dtype == np.float32 and np.array_equal(rows.view(np.uint32), all_rows[:at].view(np.uint32))
        assert back.read_columns() == _columns(schema, np.arange(at))
        assert os.path.getsize(tmp_path / "root" / name / "rows.0.f32") == at * dim * 4       # unpadded fp32
    assert nfiles[3] == nfiles[40] == nfiles[1]
    assert st.names() == ["c1", "c3", "c40"] and st.has("c3") and not st.has("c2")


def test_empty_collection_round_trip(tmp_path):
    st = Store(tmp_path / "root")
    st.create("empty", 8, "COSINE", DEFAULT_SCHEMA, "")
    back = st.open("empty", dim=8, schema=DEFAULT_SCHEMA)
    ids, rows = _read_all(back)
    assert back.rows == 0 and ids.shape == (0,) and rows.shape == (0, 8)
    assert back.read_columns() == {"image_path": [], "label": []} and back.read_deleted().shape == (0,)
    back.flush()                                                     # nothing to commit
    assert Store(tmp_path / "root").open("empty").rows == 0
    with pytest.raises(ValueError, match="exists already"):
        st.create("empty", 8)


def test_chunks_are_bounded(tmp_path):
    """Rows come back in pieces of at most the requested bytes (one row when a row is larger), equal to one whole read."""
    st = Store(tmp_path)
    col = st.create("c", 130, "COSINE", DEFAULT_SCHEMA)
    rows = _rows(50, 130)
    col.append(np.arange(50), rows, _columns(DEFAULT_SCHEMA, np.arange(50)))
    col.flush()
    back = st.open("c")
    parts = list(back.chunks(4096))
    assert all(p[1].nbytes <= 4096 for p in parts) and len(parts) == -(-50 // (4096 // 520))
    assert np.array_equal(np.concatenate([p[1] for p in parts]), rows)
    assert [p[1].shape[0] for p in back.chunks(100)] == [1] * 50     # a row is 520 bytes: one row per piece
    assert S.LOAD_CHUNK_BYTES <= 256 << 20


# ---- crash forms, each made by hand on a copy of a good store -----------------------------------------------------------------
@pytest.fixture()
def good(tmp_path):
    st = Store(tmp_path / "good")
    col = st.create("c", 8, "COSINE", DEFAULT_SCHEMA, "good")
    for k in range(3):
        ids = np.arange(4 * k, 4 * k + 4)
        col.append(ids, _rows(12, 8)[4 * k:4 * k + 4], _columns(DEFAULT_SCHEMA, ids))
        col.flush()
    col.delete([5])
    col.flush()

    def copy(name):
        shutil.copytree(tmp_path / "good", tmp_path / name)
        return Store(tmp_path / name), tmp_path / name / "c"
    return copy


def _expect_good(col, n=12):
    ids, rows = _read_all(col)
    assert np.array_equal(ids, np.arange(n)) and np.array_equal(rows[:12], _rows(12, 8))
    assert col.read_columns() == _columns(DEFAULT_SCHEMA, np.arange(n)) and col.read_deleted().tolist() == [5]


def test_leftover_temporary_manifest_is_ignored(good):
    st, path = good("tmp")
    (path / "manifest.json.tmp").write_text('{"format": "mirx-store", "version": 1, "rows": 99')       # cut off mid-write
    col = st.open("c")
    _expect_good(col)
    col.append([12], _rows(1, 8, 9), _columns(DEFAULT_SCHEMA, [12]))
    col.flush()
    assert not (path / "manifest.json.tmp").exists() and st.open("c").rows == 13


def test_uncommitted_tail_is_ignored_then_overwritten(good):
    """Data files longer than the manifest says: an unfinished flush.  The tail is not read, and the next flush writes over it."""
    st, path = good("tail")
    for f in _files(path):
        if f != "manifest.json":
            with open(path / f, "ab") as fh:
                fh.write(b"\xde\xad\xbe\xef" * 11)                   # not even a whole record
    col = st.open("c", dim=8, schema=DEFAULT_SCHEMA)
    _expect_good(col)
    new = _rows(3, 8, 5)
    col.append([12, 13, 14], new, _columns(DEFAULT_SCHEMA, [12, 13, 14]))
    col.delete([0])
    col.flush()
    back = st.open("c")
    ids, rows = _read_all(back)
    assert np.array_equal(ids, np.arange(15)) and np.array_equal(rows, np.concatenate([_rows(12, 8), new]))
    assert back.read_columns() == _columns(DEFAULT_SCHEMA, np.arange(15)) and back.read_deleted().tolist() == [5, 0]
    assert os.path.getsize(path / "rows.0.f32") == 15 * 8 * 4


@pytest.mark.parametrize("victim", ["rows.0.f32", "ids.0.i64", "col0.0.jsonl", "col1.0.jsonl", "deleted.0.i64"])
def test_data_file_one_byte_short_is_rejected(good, victim):
    st, path = good("short")
    with open(path / victim, "r+b") as fh:
        fh.truncate(os.path.getsize(path / victim) - 1)
    with pytest.raises(ValueError, match=victim.replace(".", r"\.")):
        st.open("c")


def test_future_version_wrong_dim_schema_metric_are_rejected(good):
    st, path = good("ver")
    with pytest.raises(ValueError, match=r"manifest\.json.*stored dim 8.*expects 16"):
        st.open("c", dim=16)
    with pytest.raises(ValueError, match=r"manifest\.json.*stored schema"):
        st.open("c", schema=NIH_SCHEMA)
    with pytest.raises(ValueError, match=r"manifest\.json.*stored metric_type COSINE.*expects L2"):
        st.open("c", metric_type="L2")
    man = json.loads((path / "manifest.json").read_text())
    man["version"] = 2
    (path / "manifest.json").write_text(json.dumps(man))
    with pytest.raises(ValueError, match=r"manifest\.json.*format version 2"):
        st.open("c")
    with pytest.raises(ValueError, match="does not exist"):
        st.open("absent")


def test_store_stays_inside_its_root(tmp_path):
    st = Store(tmp_path / "root")
    for bad in ("../x", "a/b", "", ".", "..", ".hidden", "a\\b"):
        with pytest.raises(ValueError, match="plain directory name"):
            st.create(bad, 8)
        with pytest.raises(ValueError, match="plain directory name"):
            st.has(bad)
    assert _files(tmp_path) == []                                    # not even the root: only create() makes it
    assert st.names() == [] and st.drop("nothing") is False
    st.create("c", 8)
    assert _files(tmp_path) == ["root"] and _files(tmp_path / "root") == ["c"]


# ---- the format is pinned: a store written by version 1 of this code -------------------------------------------------------
def test_golden_store_v1_opens_to_known_rows(golden_dir, tmp_path):
    """tests/golden/store_v1 (tests/golden/make_golden_store_v1.py): three rows of dim 8, ids 0..2, id 1 deleted.  A change of
    the format that cannot read it orphans users' stores."""
    shutil.copytree(os.path.join(golden_dir, "store_v1"), tmp_path / "s")
    st = Store(tmp_path / "s")
    assert st.names() == ["pinned"]
    col = st.open("pinned", dim=8, metric_type="COSINE", schema=DEFAULT_SCHEMA)
    ids, rows = _read_all(col)
    assert ids.tolist() == [0, 1, 2] and col.read_deleted().tolist() == [1] and col.next_id == 3
    assert np.array_equal(rows, (np.arange(24, dtype=np.float32).reshape(3, 8) - 7) / 4)
    assert col.read_columns() == {"image_path": ["a.png", "b.png", "c é.png"], "label": [0, 1, None]}
    assert col.description == "format pin" and col.generation == 0
    from mirx.retriever import Collection
    c = Collection.from_stored(col)
    assert c.num_entities == 2 and c.live_ids().tolist() == [0, 2] and c.entity(1) is None
    assert c.entity(2) == {"image_path": "c é.png", "label": None}
    assert sum(os.path.getsize(os.path.join(golden_dir, "store_v1", "pinned", f))
               for f in os.listdir(os.path.join(golden_dir, "store_v1", "pinned"))) < 1024


# ---- delete expressions ----------------------------------------------------------------------------------------------------
def test_delete_expression_forms():
    from mirx.retriever import parse_delete_expr as p
    assert p("id in [3, 1, 3]") == ("id", [3, 1, 3])
    assert p(" id == 7 ") == ("id", [7])
    assert p("id in []") == ("id", [])
    assert p("id in [-2]") == ("id", [-2])
    assert p('image_path in ["a.png", \'b c.png\']') == ("image_path", ["a.png", "b c.png"])
    assert p('image_path == "x in [1].png"') == ("image_path", ["x in [1].png"])
    assert p("image_path=='q'") == ("image_path", ["q"])


@pytest.mark.parametrize("expr, message", [
    ("", "empty expression"),
    (None, "must be a string"),
    ("id > 3", "cannot parse"),
    ("label == 3", "cannot delete by field 'label'"),
    ("id in [1, 2.5]", "id takes integers, got 2.5"),
    ("id == True", "id takes integers, got True"),
    ('image_path in ["a", 4]', "image_path takes strings, got 4"),
    ("id in (1, 2)", "needs a \\[..\\] list"),
    ("id == [1]", "needs one value"),
    ("id in [1] and id in [2]", "not a literal"),
    ("id in [__import__('os')]", "not a literal"),
])
def test_delete_expression_rejects(expr, message):
    from mirx.retriever import parse_delete_expr
    with pytest.raises(ValueError, match=message):
        parse_delete_expr(expr)


# ---- Collection on a store, never resident ---------------------------------------------------------------------------------
def _manager(tmp_path, uri=None):
    from mirx.retriever import MilvusManager
    return MilvusManager(uri=str(tmp_path / "db") if uri is None else uri)


def _fill(col, n, dim, start=0):
    emb = _rows(n, dim, seed=start + 1)
    ids = col.insert([[f"img/{start + i}.png" for i in range(n)], [(start + i) % 3 for i in range(n)], emb])
    return ids, emb


def test_persistent_collection_delete_compact_and_auto_ids(tmp_path):
    mgr = _manager(tmp_path)
    col = mgr.create_collection("dinov2")
    assert col.is_persistent and mgr.is_persistent and col.num_entities == 0
    ids, emb = _fill(col, 10, 512)
    assert ids == list(range(10))
    assert col.delete("id in [2, 2, 99]").delete_count == 1          # a duplicate and an unknown id
    assert col.delete('image_path in ["img/9.png", "img/4.png", "nope"]').delete_count == 2
    assert col.delete("id == 2").delete_count == 0                   # already gone
    assert col.delete('image_path == "img/0.png"').delete_count == 1
    with pytest.raises(ValueError, match="cannot parse"):
        col.delete("id >= 0")
    live = [1, 3, 5, 6, 7, 8]
    assert col.num_entities == 6 and col.live_ids().tolist() == live
    assert col.field("image_path") == [f"img/{i}.png" for i in live] and col.entity(4) is None and col.position(5) == 2
    assert [r["id"] for r in col.query("id >= 0", ["image_path"], limit=4, offset=1)] == [3, 5, 6, 7]
    ids2, emb2 = _fill(col, 2, 512, start=10)
    assert ids2 == [10, 11]                                          # not "previous size + i" = 6, 7: those are live rows
    col.flush()

    def reopened():
        return _manager(tmp_path).create_collection("dinov2")        # create_collection opens what exists

    for step in ("flushed", "compacted", "compacted twice"):
        if step != "flushed":
            col.compact()
            assert sorted(os.listdir(tmp_path / "db" / col.name)) == sorted(
                ["manifest.json"] + [f"{s}.{1 if step == 'compacted' else 2}.{e}" for s, e in
                                     (("rows", "f32"), ("ids", "i64"), ("col0", "jsonl"), ("col1", "jsonl"), ("deleted", "i64"))])
        for c in (col, reopened()):
            assert c.num_entities == 8 and c.live_ids().tolist() == live + [10, 11], step
            assert c.field("image_path") == [f"img/{i}.png" for i in live + [10, 11]]
            assert c.field("label") == [i % 3 for i in live + [10, 11]]
            assert all(c.entity(i) is None for i in (0, 2, 4, 9, 12)) and c.entity(10) == {"image_path": "img/10.png", "label": 1}
            assert c.position(10) == 6 and c.position(0) is None
        got_ids, got_rows = _read_all(mgr._disk.open(col.name))
        keep = np.isin(got_ids, live + [10, 11])
        assert np.array_equal(got_rows[keep], np.concatenate([emb[live], emb2]))           # live rows bit for bit
    again = reopened()
    assert again.insert([["late.png"], [0], _rows(1, 512)]) == [12]  # never 8 (the row count) nor a deleted id
    assert again.delete("id in [12]").delete_count == 1 and again.insert([["later.png"], [0], _rows(1, 512)]) == [13]


def test_drop_and_drop_old(tmp_path):
    mgr = _manager(tmp_path)
    col = mgr.create_collection("dinov2")
    _fill(col, 3, 512)
    col.flush()
    name = col.name
    assert mgr.has_collection(name) and mgr.list_collections() == [name] and os.path.isdir(tmp_path / "db" / name)
    assert _manager(tmp_path).get_collection_info("dinov2")["num_entities"] == 3           # metadata without load()
    fresh = _manager(tmp_path).create_collection("dinov2", drop_old=True)
    assert fresh.num_entities == 0 and Store(tmp_path / "db").open(name).rows == 0
    mgr2 = _manager(tmp_path)
    mgr2.drop_collection(name)
    assert not mgr2.has_collection(name) and mgr2.list_collections() == [] and not os.path.exists(tmp_path / "db" / name)
    with pytest.raises(ValueError, match="does not exist"):
        mgr2.load_collection("dinov2")
    mgr2.drop_collection(name)                                       # dropping what is not there is no error
    assert Store(tmp_path / "db").drop(name) is False


def test_file_uri_names_the_same_store(tmp_path):
    from mirx.retriever import store_root_of
    assert store_root_of(f"file://{tmp_path}/db") == f"{tmp_path}/db" == store_root_of(f"{tmp_path}/db")
    assert store_root_of(None) is None and store_root_of("grpc://h:1") is None and store_root_of("tcp://h:1") is None
    with pytest.raises(ValueError, match="file:// uri"):
        store_root_of("ftp://h/x")
    col = _manager(tmp_path, f"file://{tmp_path}/db").create_collection("dinov2")
    _fill(col, 2, 512)
    col.flush()
    assert _manager(tmp_path).create_collection("dinov2").num_entities == 2


@pytest.mark.parametrize("uri", [None, "https://x", "http://localhost:19530"])
def test_network_and_absent_uris_write_nothing(tmp_path, monkeypatch, uri):
    """uri=None or a network uri: in memory, as before.  Nothing appears under tmp_path or the working directory (and such
    a uri is never contacted: there is no socket code to reach)."""
    from mirx.retriever import MilvusManager
    cwd = os.getcwd()
    before_cwd = sorted(os.listdir(cwd))
    work = tmp_path / "work"
    work.mkdir()
    monkeypatch.chdir(work)
    mgr = MilvusManager(uri=uri)
    assert not mgr.is_persistent
    col = mgr.create_collection("dinov2")
    assert not col.is_persistent and col.flush() is None and col.num_entities == 0
    assert mgr.has_collection(col.name) and mgr.list_collections() == [col.name]
    assert mgr.get_collection_info("dinov2")["schema"] == DEFAULT_SCHEMA
    mgr.drop_collection(col.name)
    assert not mgr.has_collection(col.name)
    assert _files(work) == [] and _files(tmp_path) == ["work"] and sorted(os.listdir(cwd)) == before_cwd
