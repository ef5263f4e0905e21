"""A collection catalogue on disk: what the reference leaves to the Milvus server between its two scripts.

ingest_embeddings.py:399-411,532-534 fills a collection and ends with collection.flush() ("Flush to persist data"); another
process later opens it by name (evaluate_test_dataset_milvus.py:339-364, query_nih_zilliz.py:30, ChestMIR/chestmir_eval.py:
366-368).  `Store(root)` is that catalogue as a directory; mirx.retriever.Collection writes to it on flush() and reads it
back on load().  Host code only: numpy and the standard library, no GPU, no socket.

Layout: one directory per collection under `root`, holding only what cannot be derived

    manifest.json        format version, dim, metric, schema, description, generation, committed counts, next auto id
    rows.<g>.f32         [rows, dim] float32, little-endian, unpadded, append-only
    ids.<g>.i64          [rows] int64, append-only
    col<i>.<g>.jsonl     one file per scalar column of the schema, one JSON value per line, append-only
    deleted.<g>.i64      [deleted] int64, append-only

flush() appends what is new at the committed offsets, then writes the manifest through manifest.json.tmp and os.replace: the
manifest is the commit.  Bytes past the committed counts are an unfinished flush; they are ignored and overwritten.  compact()
writes generation g + 1 without the deleted rows, commits, and removes generation g.
"""
import json
import os
import shutil

import numpy as np

FORMAT = "mirx-store"
VERSION = 1
MANIFEST = "manifest.json"
LOAD_CHUNK_BYTES = 64 << 20       # most row bytes one read of chunks() holds (at most 256 MiB: DESIGN.md 31); tests lower it
_SCALAR_SKIP = ("id", "embedding")
_METRICS = ("COSINE", "IP", "L2")


def _check_name(name):
    if (not isinstance(name, str) or not name or name in (".", "..") or name.startswith(".")
            or any(c in name for c in "/\\\0") or os.path.basename(name) != name):
        raise ValueError(f"collection name {name!r} is not a plain directory name")
    return name


def _fsync_write(path, offset, data):
    """data at `offset` of `path` (created when absent), whatever lay behind `offset` cut off; durable on return."""
    with open(path, "r+b" if os.path.exists(path) else "w+b") as fh:
        fh.seek(offset)
        fh.write(data)
        fh.truncate()
        fh.flush()
        os.fsync(fh.fileno())


class StoredCollection:
    """One collection of a Store: the committed state of its files plus what was added or deleted since the last flush().

    ids / deleted ids / scalar columns live in host memory (a few bytes per row); the rows are only ever read in chunks."""

    def __init__(self, path, manifest):
        self.path = path
        self.name = manifest["name"]
        self.dim = int(manifest["dim"])
        self.metric_type = manifest["metric_type"]
        self.schema = list(manifest["schema"])
        self.description = manifest["description"]
        self.generation = int(manifest["generation"])
        self.rows = int(manifest["rows"])                      # committed
        self.ndeleted = int(manifest["deleted"])               # committed
        self.col_bytes = [int(b) for b in manifest["column_bytes"]]
        self.next_id = int(manifest["next_id"])
        self.fields = [f for f in self.schema if f not in _SCALAR_SKIP]
        if len(self.col_bytes) != len(self.fields):
            raise ValueError(f"{self._file(MANIFEST)}: {len(self.col_bytes)} column sizes for {len(self.fields)} scalar columns")
        self._new_rows, self._new_ids, self._new_cols, self._new_deleted = [], [], [[] for _ in self.fields], []
        self._dirty = False

    # -- files ---------------------------------------------------------------------------------------------------------
    def _file(self, base, gen=None):
        if base == MANIFEST:
            return os.path.join(self.path, MANIFEST)
        stem, ext = base.rsplit(".", 1)
        return os.path.join(self.path, f"{stem}.{self.generation if gen is None else gen}.{ext}")

    def _data_files(self, gen=None):
        """(path, committed bytes) of every data file"""
        out = [(self._file("rows.f32", gen), self.rows * self.dim * 4), (self._file("ids.i64", gen), self.rows * 8)]
        out += [(self._file(f"col{i}.jsonl", gen), b) for i, b in enumerate(self.col_bytes)]
        out.append((self._file("deleted.i64", gen), self.ndeleted * 8))
        return out

    def _check_files(self):
        for path, need in self._data_files():
            have = os.path.getsize(path) if os.path.exists(path) else 0
            if have < need:
                raise ValueError(f"{path}: {have} bytes on disk, the manifest commits {need}: the store is truncated")

    def _read(self, path, nbytes):
        if nbytes == 0:
            return b""
        with open(path, "rb") as fh:
            data = fh.read(nbytes)
        if len(data) != nbytes:
            raise ValueError(f"{path}: {len(data)} bytes read, the manifest commits {nbytes}")
        return data

    def _manifest(self):
        return {"format": FORMAT, "version": VERSION, "name": self.name, "dim": self.dim, "metric_type": self.metric_type,
                "schema": self.schema, "description": self.description, "generation": self.generation, "rows": self.rows,
                "deleted": self.ndeleted, "column_bytes": self.col_bytes, "next_id": self.next_id}

    def _commit(self):
        """the manifest last, through a temporary file and os.replace"""
        tmp = self._file(MANIFEST) + ".tmp"
        with open(tmp, "w") as fh:
            json.dump(self._manifest(), fh, indent=1)
            fh.write("\n")
            fh.flush()
            os.fsync(fh.fileno())
        os.replace(tmp, self._file(MANIFEST))
        self._dirty = False

    # -- committed state -----------------------------------------------------------------------------------------------
    def read_ids(self):
        return np.frombuffer(self._read(self._file("ids.i64"), self.rows * 8), dtype="<i8").astype(np.int64)

    def read_deleted(self):
        return np.frombuffer(self._read(self._file("deleted.i64"), self.ndeleted * 8), dtype="<i8").astype(np.int64)

    def read_columns(self):
        """{field: list of the committed values}"""
        out = {}
        for i, f in enumerate(self.fields):
            text = self._read(self._file(f"col{i}.jsonl"), self.col_bytes[i]).decode("utf-8")
            vals = [json.loads(line) for line in text.split("\n")[:-1]] if text else []
            if len(vals) != self.rows:
                raise ValueError(f"{self._file(f'col{i}.jsonl')}: {len(vals)} values for {self.rows} committed rows")
            out[f] = vals
        return out

    def chunks(self, chunk_bytes=None):
        """The committed rows in file order as (ids [m] int64, rows [m, dim] float32) pieces of at most chunk_bytes of rows
        (LOAD_CHUNK_BYTES; one row when a row is larger), then the rows added since the last flush.  Each piece is a fresh
        buffer: the gallery is never read or mapped whole."""
        chunk_bytes = min(int(chunk_bytes or LOAD_CHUNK_BYTES), 256 << 20)
        per = max(1, chunk_bytes // (self.dim * 4))
        ids = self.read_ids()
        if self.rows:
            with open(self._file("rows.f32"), "rb") as fh:
                for s in range(0, self.rows, per):
                    m = min(per, self.rows - s)
                    buf = np.empty((m, self.dim), dtype="<f4")
                    got = fh.readinto(memoryview(buf).cast("B"))
                    if got != m * self.dim * 4:
                        raise ValueError(f"{self._file('rows.f32')}: short read at row {s}")
                    yield ids[s:s + m], buf.astype(np.float32, copy=False)
        for new_ids, new_rows in zip(self._new_ids, self._new_rows):
            yield new_ids, new_rows

    # -- changes -------------------------------------------------------------------------------------------------------
    @property
    def pending(self):
        return bool(self._new_ids or self._new_deleted or self._dirty)

    def append(self, ids, rows, columns):
        """ids [m], rows [m, dim] float32, columns = {field: m values}: held in memory until flush()"""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape != (ids.shape[0], self.dim):
            raise ValueError(f"expected [{ids.shape[0]}, {self.dim}] rows, got {rows.shape}")
        if sorted(columns) != sorted(self.fields) or any(len(columns[f]) != ids.shape[0] for f in self.fields):
            raise ValueError(f"columns must be {self.fields} with {ids.shape[0]} values each")
        if ids.shape[0] == 0:
            return
        self._new_ids.append(ids.copy())
        self._new_rows.append(rows.copy())
        for i, f in enumerate(self.fields):
            self._new_cols[i].extend(columns[f])
        self.next_id = max(self.next_id, int(ids.max()) + 1)

    def delete(self, ids):
        self._new_deleted.extend(int(i) for i in ids)

    def set_metric(self, metric_type):
        if metric_type != self.metric_type:
            self.metric_type = metric_type
            self._dirty = True

    def flush(self):
        """Append what is new behind the committed bytes of each file, then commit.  Cost: the new rows."""
        if not self.pending:
            return
        if self._new_ids:
            ids = np.concatenate(self._new_ids)
            _fsync_write(self._file("rows.f32"), self.rows * self.dim * 4,
                         b"".join(r.astype("<f4", copy=False).tobytes() for r in self._new_rows))
            _fsync_write(self._file("ids.i64"), self.rows * 8, ids.astype("<i8", copy=False).tobytes())
            for i in range(len(self.fields)):
                data = "".join(json.dumps(_plain(v)) + "\n" for v in self._new_cols[i]).encode("utf-8")
                _fsync_write(self._file(f"col{i}.jsonl"), self.col_bytes[i], data)
                self.col_bytes[i] += len(data)
            self.rows += ids.shape[0]
        if self._new_deleted:
            gone = np.asarray(self._new_deleted, dtype="<i8")
            _fsync_write(self._file("deleted.i64"), self.ndeleted * 8, gone.tobytes())
            self.ndeleted += gone.shape[0]
        self._new_rows, self._new_ids, self._new_cols, self._new_deleted = [], [], [[] for _ in self.fields], []
        self._commit()

    def compact(self, chunk_bytes=None):
        """Rewrite the files without the deleted rows: generation g + 1 beside g, commit, remove g.  Includes a flush."""
        self.flush()
        dead = set(self.read_deleted().tolist())
        new = self.generation + 1
        ids, cols = self.read_ids(), self.read_columns()
        keep = np.fromiter((int(i) not in dead for i in ids), dtype=bool, count=ids.shape[0])
        for path, _ in self._data_files(new):
            if os.path.exists(path):
                os.remove(path)                                 # what a compaction that never committed left behind
        at = 0
        with open(self._file("rows.f32", new), "wb") as fh:
            for _, rows in self.chunks(chunk_bytes):
                live = rows[keep[at:at + rows.shape[0]]]
                at += rows.shape[0]
                fh.write(live.astype("<f4", copy=False).tobytes())
            fh.flush()
            os.fsync(fh.fileno())
        _fsync_write(self._file("ids.i64", new), 0, ids[keep].astype("<i8").tobytes())
        col_bytes = []
        for i, f in enumerate(self.fields):
            data = "".join(json.dumps(v) + "\n" for v, k in zip(cols[f], keep) if k).encode("utf-8")
            _fsync_write(self._file(f"col{i}.jsonl", new), 0, data)
            col_bytes.append(len(data))
        _fsync_write(self._file("deleted.i64", new), 0, b"")
        self.generation, self.rows, self.ndeleted, self.col_bytes = new, int(keep.sum()), 0, col_bytes
        self._commit()
        current = {os.path.basename(p) for p, _ in self._data_files()}
        for n in os.listdir(self.path):                         # generation `old`, and whatever an interrupted compaction left
            if n not in current and n != MANIFEST and n.rsplit(".", 1)[-1] in ("f32", "i64", "jsonl"):
                os.remove(os.path.join(self.path, n))


def _plain(v):
    """a scalar column's value as JSON can hold it (numpy scalars -> Python's)"""
    if isinstance(v, np.generic):
        return v.item()
    return v


class Store:
    """Collections under one directory.  Nothing is created outside `root`, and `root` itself only by create()."""

    def __init__(self, root):
        self.root = os.path.abspath(os.fspath(root))

    def _dir(self, name):
        return os.path.join(self.root, _check_name(name))

    def has(self, name):
        return os.path.isfile(os.path.join(self._dir(name), MANIFEST))

    def names(self):
        if not os.path.isdir(self.root):
            return []
        return sorted(n for n in os.listdir(self.root) if os.path.isfile(os.path.join(self.root, n, MANIFEST)))

    def create(self, name, dim, metric_type="COSINE", schema=("id", "image_path", "label", "embedding"), description=""):
        """A new, empty, committed collection.  ValueError when `name` exists."""
        path = self._dir(name)
        if self.has(name):
            raise ValueError(f"{os.path.join(path, MANIFEST)}: collection {name} exists already")
        if int(dim) < 1:
            raise ValueError(f"dim must be >= 1, got {dim}")
        if metric_type not in _METRICS:
            raise ValueError(f"Unknown metric type: {metric_type}")
        schema = [str(f) for f in schema]
        if "id" not in schema or "embedding" not in schema or len(set(schema)) != len(schema):
            raise ValueError(f"schema {schema} needs distinct fields with an id and an embedding")
        os.makedirs(path, exist_ok=True)
        col = StoredCollection(path, {"name": name, "dim": int(dim), "metric_type": metric_type, "schema": schema,
                                      "description": str(description), "generation": 0, "rows": 0, "deleted": 0,
                                      "column_bytes": [0] * (len(schema) - 2), "next_id": 0})
        for data_file, _ in col._data_files():                  # every file from the start: their number never changes
            open(data_file, "ab").close()
        col._commit()
        return col

    def open(self, name, dim=None, metric_type=None, schema=None):
        """The committed state of `name`.  ValueError naming the file for a missing or unreadable manifest, another format
        version, a data file shorter than committed, or a dim / metric_type / schema other than the caller's (None = any)."""
        path = self._dir(name)
        mpath = os.path.join(path, MANIFEST)
        if not os.path.isfile(mpath):
            raise ValueError(f"{mpath}: collection {name} does not exist")
        try:
            with open(mpath) as fh:
                man = json.load(fh)
        except (OSError, json.JSONDecodeError) as e:
            raise ValueError(f"{mpath}: unreadable manifest ({e})") from None
        if not isinstance(man, dict) or man.get("format") != FORMAT:
            raise ValueError(f"{mpath}: not a {FORMAT} manifest")
        if man.get("version") != VERSION:
            raise ValueError(f"{mpath}: format version {man.get('version')!r}, this build reads version {VERSION}")
        missing = [k for k in ("name", "dim", "metric_type", "schema", "description", "generation", "rows", "deleted",
                               "column_bytes", "next_id") if k not in man]
        if missing:
            raise ValueError(f"{mpath}: manifest lacks {missing}")
        if dim is not None and int(dim) != man["dim"]:
            raise ValueError(f"{mpath}: stored dim {man['dim']}, the caller expects {dim}")
        if metric_type is not None and metric_type != man["metric_type"]:
            raise ValueError(f"{mpath}: stored metric_type {man['metric_type']}, the caller expects {metric_type}")
        if schema is not None and [str(f) for f in schema] != man["schema"]:
            raise ValueError(f"{mpath}: stored schema {man['schema']}, the caller expects {list(schema)}")
        col = StoredCollection(path, man)
        col._check_files()
        return col

    def drop(self, name):
        """Remove `name` from disk (its own directory only).  -> whether it existed."""
        path = self._dir(name)
        if not self.has(name):
            return False
        shutil.rmtree(path)
        return True
