"""In-process replacement for the reference's Milvus layer, same object protocol.

Mirrors (paths into /root/reference):
  MODEL_CONFIGS, MilvusManager                      milvus/milvus_setup.py:19-252
  MilvusRetriever.search / batch_search             milvus/milvus_retrieval.py:15-140
  get_model_and_transform                           milvus/milvus_retrieval.py:143-200
  collection.insert([paths, labels, embeddings])    ingest_embeddings.py:399-411
  search_by_embeddings                              retrieval_analysis/milvus_adapter.py:218-275 (mirx.adapter)
  NIH helpers                                       mirx.nih (nih_zilliz_utils.py)
  hybrid_search / AnnSearchRequest / rankers        pymilvus' hybrid search over the per-model collections the reference joins
                                                    on image_path (fusion_eval/, retrieval_analysis/); DESIGN 35
The "server" is a device-resident FlatIndex (libmirx); searches are EXACT (the reference's
IVF_FLAT nlist=1024 / nprobe=10 index is approximate, milvus_setup.py:191-213) and
`search_params` / `nprobe` are accepted and ignored, except `radius` / `range_filter` (a range search) and, on a collection
whose index was created with `create_index(..., approximate=True)`, `nprobe`: the opt-in IVF_FLAT index (mirx.index.IvfFlatIndex,
DESIGN 41) that reproduces the reference's own search, or IVF_SQ8 (mirx.index.IvfSq8Index), the same over 8-bit codes, or IVF_PQ (mirx.index.IvfPqIndex), the ADC
ranking over product-quantised codes.  Metadata (image_path, label) stays on
the host, keyed by the int64 ids the index returns.

Errors follow the reference: unknown model type -> ValueError; connect() swallows failures
and returns False; everything else raises ordinary exceptions (callers wrap each query in
try/except, evaluate_test_dataset_milvus.py:586-590).
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from .index import FlatIndex, IvfResidualPqIndex, group_bounds, ivf_index_spec, range_bounds, tier1_max_k

MODEL_CONFIGS = {
    "densenet121": {"embedding_dim": 1024, "description": "DenseNet121 image embeddings"},
    "resnet50": {"embedding_dim": 2048, "description": "ResNet50 image embeddings"},
    "convnextv2": {"embedding_dim": 1024, "description": "ConvNeXtV2 image embeddings"},
    "convnextv2_sra": {"embedding_dim": 1024, "description": "ConvNeXtV2_SRA image embeddings"},
    "dinov2": {"embedding_dim": 512, "description": "DINOv2 image embeddings"},
    "medsiglip": {"embedding_dim": 512, "description": "MedSigLIP image embeddings"},
}
for _name, _cfg in MODEL_CONFIGS.items():
    _suffix = "isic_image_retrieval_medsiglip" if _name == "medsiglip" else f"image_retrieval_{_name}"
    _cfg["collection_names"] = {"default": _suffix, "isic": f"isic_image_retrieval_{_name}",
                                "covid": f"covid_image_retrieval_{_name}"}


class _Entity:
    def __init__(self, fields):
        self._f = fields

    def get(self, name, default=None):
        return self._f.get(name, default)


class Hit:
    """pymilvus-like hit: .id, .distance, .entity.get(field)."""

    def __init__(self, id_, distance, fields):
        self.id = id_
        self.distance = distance
        self.entity = _Entity(fields)


class MutationResult:
    """pymilvus' MutationResult as far as delete() is concerned: .delete_count."""

    def __init__(self, delete_count):
        self.delete_count = int(delete_count)

    def __repr__(self):
        return f"(delete count: {self.delete_count})"


_DELETE_FORMS = 'id in [..], id == n, image_path in ["..", ..], image_path == ".."'


def parse_delete_expr(expr):
    """-> ("id", [int, ..]) or ("image_path", [str, ..]) for the pymilvus forms `id in [..]`, `id == n`,
    `image_path in ["..", ..]` and `image_path == ".."`; ValueError for anything else."""
    import ast
    import re
    if not isinstance(expr, str):
        raise ValueError(f"delete: the expression must be a string, got {type(expr).__name__}")
    text = expr.strip()
    if not text:
        raise ValueError("delete: empty expression")
    m = re.match(r"^([A-Za-z_][A-Za-z0-9_]*)\s*(==|\bin\b)\s*(.+)$", text, flags=re.S)
    if not m:
        raise ValueError(f"delete: cannot parse {expr!r}: the supported forms are {_DELETE_FORMS}")
    field, op, rhs = m.group(1), m.group(2), m.group(3).strip()
    if field not in ("id", "image_path"):
        raise ValueError(f"delete: cannot delete by field {field!r}: only id and image_path")
    try:
        value = ast.literal_eval(rhs)
    except (ValueError, SyntaxError, MemoryError, RecursionError):
        raise ValueError(f"delete: the right-hand side of {expr!r} is not a literal: the supported forms are {_DELETE_FORMS}") from None
    if op == "in":
        if not isinstance(value, list):
            raise ValueError(f"delete: `{field} in` needs a [..] list, got {rhs!r}")
        values = value
    else:
        if isinstance(value, (list, tuple, set, dict)):
            raise ValueError(f"delete: `{field} ==` needs one value, got {rhs!r}")
        values = [value]
    want = int if field == "id" else str
    for v in values:
        if type(v) is not want:
            raise ValueError(f"delete: {field} takes {'integers' if want is int else 'strings'}, got {v!r}")
    return field, values


class Collection:
    """The slice of pymilvus.Collection the reference uses: insert / flush / load / search / delete / compact /
    num_entities / name / description, backed by a FlatIndex.

    In memory (stored=None) the index is the only copy of the rows.  With `stored` (a mirx.store.StoredCollection) the
    collection is persistent: flush() commits inserts and deletions to disk, load() makes the rows resident, and metadata
    (num_entities, schema, entity(), field()) is served from the host without a GPU.  Until load(), insert() and delete()
    of a persistent collection touch no device either.

    Rows are known by their int64 id.  Ids are assigned by insert(), ascending, and never reused: a deleted row's id stays
    retired.  Metadata is read through entity() / field() / live_ids() / position(), which hide deleted rows."""

    def __init__(self, name, dim, description="", metric_type="COSINE", device=None, extra_fields=(), has_label=True, stored=None):
        self.name = name
        self.description = description
        self.dim = dim
        self.metric_type = metric_type
        # column order of insert(): the default schema is id, image_path, label, embedding (milvus_setup.py:169-176)
        # followed by any extra scalar fields; the NIH schema (nih_zilliz_utils.py:149-156, has_label=False) is id,
        # image_path, <extra fields>, embedding
        if has_label:
            self.schema = ["id", "image_path", "label", "embedding"] + list(extra_fields)
        else:
            self.schema = ["id", "image_path"] + list(extra_fields) + ["embedding"]
        self._device = device
        self._index = None
        # one slot per row ever inserted and not yet compacted away: _ids[slot] (ascending), _meta[field][slot]; _dead = the
        # ids of deleted slots.  While nothing was compacted away a row's id IS its slot (_slot_of is None).
        self._meta = {f: [] for f in self.schema if f not in ("id", "embedding")}
        self._ids = []
        self._dead = set()
        self._slot_of = None
        self._next_id = 0
        self._live = None                                   # cache: ids of the live slots in order (numpy int64)
        self._expr = None                                   # cache: mirx.expr.ExprCache of the current rows (see _changed)
        self._version = 0                                   # counts _changed(): what a hybrid search's join table was built from
        self._joins = {}                                    # cache: the join tables of hybrid searches this collection leads
        self._stored = stored
        self._resident = stored is None                     # whether _index mirrors the live rows
        # the opt-in approximate index (create_index(..., approximate=True)): process state, never stored
        self._approx_nlist = None                           # nlist while the approximate index is on
        self._approx_type = None                            # "IVF_FLAT", "IVF_SQ8" or "IVF_PQ" while it is on
        self._approx_m = None                               # IVF_PQ: its number of sub-quantisers
        self._approx_residual = False                       # IVF_PQ: params["by_residual"], residual coding (IvfResidualPqIndex)
        self._approx_spec = None                            # (class, constructor keywords) of it: mirx.index.ivf_index_spec
        self._ivf = None                                    # the index of that class over the live rows; None = to be (re)built
        self._ivf_state = None                              # its state(): trained once, set_state() across rebuilds

    @classmethod
    def from_stored(cls, stored, device=None):
        """The committed state of a mirx.store.StoredCollection; no row is read and no device touched before load()."""
        col = cls(stored.name, stored.dim, stored.description, stored.metric_type, device, stored=stored)
        col.schema = list(stored.schema)
        col._meta = stored.read_columns()
        col._ids = [int(i) for i in stored.read_ids()]
        present = set(col._ids)
        col._dead = {int(i) for i in stored.read_deleted()} & present
        col._next_id = max(stored.next_id, col._ids[-1] + 1 if col._ids else 0)
        if col._ids != list(range(len(col._ids))):
            col._slot_of = {i: s for s, i in enumerate(col._ids)}
        return col

    # -- the one way to a row's metadata ---------------------------------------------------------------------------------
    def _slot(self, id_):
        """slot of a live id, else None"""
        if id_ in self._dead:
            return None
        if self._slot_of is None:
            return id_ if 0 <= id_ < len(self._ids) else None
        return self._slot_of.get(id_)

    def entity(self, id_, fields=None):
        """{field: value} of the live row `id_` (every scalar field, or those of `fields` the schema has); None when the id
        is unknown or deleted."""
        s = self._slot(int(id_))
        if s is None:
            return None
        return {f: self._meta[f][s] for f in (self._meta if fields is None else fields) if f in self._meta}

    def live_ids(self):
        """ids of the live rows in index order (numpy int64)"""
        if self._live is None:
            ids = np.asarray(self._ids, dtype=np.int64)
            if self._dead:
                ids = ids[~np.isin(ids, np.fromiter(self._dead, dtype=np.int64, count=len(self._dead)))]
            self._live = ids
        return self._live

    def field(self, name):
        """values of one scalar field for the live rows, in index order (aligned with live_ids())"""
        col = self._meta[name]
        if not self._dead:
            return col
        return [v for v, i in zip(col, self._ids) if i not in self._dead]

    def has_field(self, name):
        return name in self._meta

    def position(self, id_):
        """row number of the live row `id_` in the resident index (the p of index.rows(p, 1)), else None"""
        if self._slot(int(id_)) is None:
            return None
        live = self.live_ids()
        p = int(np.searchsorted(live, int(id_)))
        return p if p < live.shape[0] and live[p] == int(id_) else None

    def _changed(self):
        """the live rows changed (insert / delete / compact): drop what was derived from them"""
        self._live = None
        self._expr = None
        self._version += 1
        self._joins = {}
        self._ivf = None                                    # rebuilt lazily, with the kept centroids

    def expr_mask(self, expr):
        """The rows a filter expression (mirx.expr: comparisons of id and the scalar fields with literals, in / not in,
        and / or / not) selects: a read-only bool array aligned with live_ids(), the resident index's row order.  Column
        codes are built once per state of the collection and the last expression's mask is kept until the rows change."""
        from .expr import ExprCache
        if self._expr is None:
            self._expr = ExprCache(self.live_ids(), self.field)
        return self._expr.evaluate(expr, ["id"] + list(self._meta))

    def _device_mask(self, expr):
        """expr_mask(expr) as a uint8 tensor on the index's device, uploaded once per expression and collection state"""
        index = self._ensure()
        mask = self.expr_mask(expr)
        cache = self._expr
        if cache.device_mask is None or cache.device_mask.device != index.device:
            cache.device_mask = torch.from_numpy(mask.astype(np.uint8)).to(index.device)
        return cache.device_mask

    def query(self, expr="id >= 0", output_fields=None, limit=None, offset=0):
        """pymilvus' collection.query: "id >= 0" (every live row, the paging loop of ChestMIR/chestmir_eval.py:380-395) takes
        a short cut, any other filter expression (mirx.expr; the forms of delete() are among them) is evaluated on the host
        columns.  -> row dicts with id and the output fields, ascending by id."""
        if isinstance(expr, str) and expr.replace(" ", "") == "id>=0":
            ids = self.live_ids()
        else:
            ids = self.live_ids()[self.expr_mask(expr)]
        ids = ids[int(offset):] if limit is None else ids[int(offset):int(offset) + int(limit)]
        fields = [f for f in (output_fields or []) if f != "id"]
        return [dict(self.entity(int(i), fields), id=int(i)) for i in ids]

    def _match(self, expr):
        """live ids an expression of delete() names, ascending"""
        field, values = parse_delete_expr(expr)
        if field == "id":
            return sorted({v for v in values if self._slot(v) is not None})
        wanted = set(values)
        return [int(i) for i, p in zip(self._ids, self._meta["image_path"]) if p in wanted and i not in self._dead]

    # -- pymilvus surface ------------------------------------------------------------------------------------------------
    def _ensure(self):
        if not self._resident:
            self.load()
        if self._index is None:
            self._index = FlatIndex(self.dim, self.metric_type, self._device)
        return self._index

    @property
    def num_entities(self):
        return len(self._ids) - len(self._dead)

    @property
    def index(self):
        return self._ensure()

    @property
    def is_persistent(self):
        return self._stored is not None

    def create_index(self, field_name="embedding", index_params=None, approximate=False):
        """pymilvus' create_index.  Without `approximate` only the metric is kept: index_type and nlist are accepted and
        ignored, every search is exact.  approximate=True with index_params["index_type"] "IVF_FLAT", "IVF_SQ8" or "IVF_PQ" (any
        other type: ValueError) turns the collection's approximate index on: an IvfFlatIndex / IvfSq8Index / IvfPqIndex of
        index_params["params"]["nlist"] lists (default 1024) beside the flat index, built from the resident rows at load() or at
        the first approximate search and trained once; after insert / delete / compact the lists are rebuilt lazily with the
        kept centroids (IVF_SQ8: and the kept range, so rows inserted later clamp to the trained range; IVF_PQ: and the kept
        codebooks).  IVF_PQ needs index_params["params"]["m"], as Milvus does (ValueError without it or with an m that
        mirx.index.pq_bounds refuses), and stays exact below max(nlist, 256) rows; index_params["params"]["by_residual"] (default
        False; anything but a bool: ValueError) = True encodes every row minus the centroid of its list, Milvus' own IVF_PQ form
        (IvfResidualPqIndex).  The type and its parameters are checked by mirx.index.ivf_index_spec, which also names
        the class.  It is process state: a
        stored collection opened again is exact until this call is made again.  See search() for the calls it serves."""
        params = index_params or {}
        nlist, kind, m, residual, spec = None, None, None, False, None
        if approximate:
            kind = params.get("index_type")
            spec = ivf_index_spec(self.dim, kind, params.get("params"))
            nlist, m, residual = spec[1]["nlist"], spec[1].get("m"), spec[0] is IvfResidualPqIndex
        metric = params.get("metric_type", self.metric_type)
        if self._ids and metric != self.metric_type:
            raise ValueError("metric_type cannot change after rows were inserted")
        self.metric_type = metric
        if self._stored is not None:
            self._stored.set_metric(metric)
        if (nlist, kind, m, residual) != (self._approx_nlist, self._approx_type, self._approx_m, self._approx_residual):
            self._approx_nlist, self._approx_type, self._approx_m, self._approx_residual = nlist, kind, m, residual
            self._approx_spec, self._ivf, self._ivf_state = spec, None, None
        return True

    def _ensure_ivf(self):
        """The approximate index over the live rows, or None while there are fewer rows than lists (nothing to train on: the
        exact routes answer; IVF_PQ: than max(nlist, 256) -- the class's min_train_rows).  A build copies the flat index's rows
        on the device (both indexes stay resident), trains on the first build and keeps the index's state(); later builds
        set_state() it: the same centroids, range and codebooks."""
        if self._approx_nlist is None:
            return None
        cls, kwargs = self._approx_spec
        if self.num_entities < cls.min_train_rows(self._approx_nlist):
            return None
        if self._ivf is None:
            index = self._ensure()
            rows, ids = index.rows()
            ivf = cls(self.dim, self.metric_type, device=index.device, **kwargs)
            if self._ivf_state is None:
                ivf.train(rows)
                self._ivf_state = ivf.state()
            else:
                ivf.set_state(self._ivf_state)
            ivf.add(rows, ids)
            self._ivf = ivf
        return self._ivf

    @staticmethod
    def _nprobe(param):
        """nprobe of pymilvus' search `param` -- under param["params"] or at its top level, as _range_params reads its keys --
        when it is an integer >= 1, else None"""
        if not isinstance(param, dict):
            return None
        inner = param.get("params") if isinstance(param.get("params"), dict) else {}
        v = inner["nprobe"] if "nprobe" in inner else param.get("nprobe")
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            return None
        return int(v)

    def load(self):
        """Make the rows resident.  A collection opened from disk streams its file in bounded pieces (mirx.store.
        LOAD_CHUNK_BYTES) into FlatIndex.add(rows, ids) with the stored ids, deleted rows dropped on the host."""
        if self._resident:
            if self._index is None:
                self._index = FlatIndex(self.dim, self.metric_type, self._device)
            self._ensure_ivf()
            return
        index = FlatIndex(self.dim, self.metric_type, self._device)
        index.reserve(self.num_entities)
        dead = np.fromiter(self._dead, dtype=np.int64, count=len(self._dead)) if self._dead else None
        for ids, rows in self._stored.chunks():
            if dead is not None:
                keep = ~np.isin(ids, dead)
                ids, rows = ids[keep], rows[keep]
            if ids.shape[0]:
                index.add(torch.from_numpy(np.ascontiguousarray(rows)), torch.from_numpy(np.ascontiguousarray(ids)))
        if len(index) != self.num_entities:
            raise RuntimeError(f"{self.name}: {len(index)} rows loaded, {self.num_entities} live rows expected")
        self._index, self._resident = index, True
        if self._expr is not None:
            self._expr.device_mask = None
            self._expr.device_codes = {}
        self._ensure_ivf()

    def release(self):
        """pymilvus' collection.release(): a persistent collection gives its device memory back (load() reads it again);
        in memory the index is the only copy and stays."""
        if self._stored is not None:
            self._index, self._resident, self._ivf = None, False, None
            if self._expr is not None:
                self._expr.device_mask = None
                self._expr.device_codes = {}

    def flush(self):
        """Commit inserts and deletions to disk (ingest_embeddings.py:532-534, "Flush to persist data"); in memory there is
        nothing to commit.  Costs the rows added since the last flush; never rewrites old data (compact() does)."""
        if self._stored is not None:
            self._stored.flush()
        return None

    def insert(self, columns):
        """columns = one list per schema field after `id`, in schema order: [image_paths, labels, embeddings]
        (ingest_embeddings.py:402-408) for the default schema.  Returns the assigned ids (auto_id: one past the largest id
        ever assigned, so the row number while nothing was deleted)."""
        fields = self.schema[1:]
        if len(columns) != len(fields):
            raise ValueError(f"expected {len(fields)} columns ({', '.join(fields)}), got {len(columns)}")
        cols = dict(zip(fields, columns))
        emb = cols.pop("embedding")
        emb = torch.as_tensor(np.asarray(emb, dtype=np.float32) if not torch.is_tensor(emb) else emb)
        if emb.dim() != 2 or emb.shape[1] != self.dim:
            raise ValueError(f"embedding dimension mismatch: expected {self.dim}, got {tuple(emb.shape)}")
        if any(len(c) != emb.shape[0] for c in cols.values()):
            raise ValueError("column lengths differ")
        cols = {f: ([str(p) for p in col] if f == "image_path" else list(col)) for f, col in cols.items()}
        ids = list(range(self._next_id, self._next_id + emb.shape[0]))
        if self._resident:
            self._ensure().add(emb, torch.tensor(ids, dtype=torch.int64))
        if self._stored is not None:
            self._stored.append(ids, emb.detach().to(torch.float32).cpu().numpy(), cols)
        for f, col in cols.items():
            self._meta[f].extend(col)
        if self._slot_of is not None:
            self._slot_of.update((i, len(self._ids) + k) for k, i in enumerate(ids))
        self._ids.extend(ids)
        self._next_id += emb.shape[0]
        self._changed()
        return ids

    def delete(self, expr):
        """pymilvus' collection.delete(expr) for `id in [..]`, `id == n`, `image_path in ["..", ..]` and
        `image_path == ".."` (anything else: ValueError).  The rows leave the resident index at once (FlatIndex.remove) and
        every metadata reader; a persistent collection commits the deletion with the next flush().  -> .delete_count = the
        live rows removed."""
        ids = self._match(expr)
        if ids:
            if self._resident and self._index is not None:
                removed = self._index.remove(torch.tensor(ids, dtype=torch.int64))
                if removed != len(ids):
                    raise RuntimeError(f"{self.name}: the index removed {removed} rows for {len(ids)} live ids")
            self._dead.update(ids)
            self._changed()
            if self._stored is not None:
                self._stored.delete(ids)
        return MutationResult(len(ids))

    def compact(self):
        """pymilvus' collection.compact(): forget the deleted rows' metadata and, for a persistent collection, rewrite its
        files without them (includes a flush).  Deleted ids stay retired; the resident index is compact already."""
        if self._stored is not None:
            self._stored.compact()
        if self._dead:
            keep = [i not in self._dead for i in self._ids]
            for f, col in self._meta.items():
                self._meta[f] = [v for v, k in zip(col, keep) if k]
            self._ids = [i for i, k in zip(self._ids, keep) if k]
            self._dead = set()
            self._slot_of = {i: s for s, i in enumerate(self._ids)}
            self._changed()
        return None

    def _queries(self, data):
        q = torch.as_tensor(np.asarray(data, dtype=np.float32) if not torch.is_tensor(data) else data)
        return q[None] if q.dim() == 1 else q

    def _hits(self, ids, sc, fields):
        """Hits of one query from its ids and fp32 reported values (numpy), empty slots skipped"""
        hits = []
        for i, v in zip(ids.tolist(), sc.tolist()):
            if i < 0 or not np.isfinite(v):
                continue
            hits.append(Hit(i, v if self.metric_type in ("COSINE", "IP") else -v, self.entity(i, fields)))
        return hits

    @staticmethod
    def _range_params(param):
        """(radius, range_filter) of pymilvus' search `param` -- under param["params"] or at its top level -- or None when it
        names no radius"""
        if not isinstance(param, dict):
            return None
        inner = param.get("params") if isinstance(param.get("params"), dict) else {}
        if "radius" not in inner and "radius" not in param:
            return None
        get = lambda k: inner[k] if k in inner else param.get(k)
        return get("radius"), get("range_filter")

    def range_search(self, data, radius, range_filter=None, expr=None, exclude_ids=None, output_fields=None):
        """pymilvus' range search (search param {"radius": .., "range_filter": ..}) without a limit: -> one list of Hit per
        query, best first, holding EVERY live row within the range -- COSINE / IP: radius < similarity <= range_filter; L2:
        range_filter <= distance < radius in the Euclidean units of Hit.distance (mirx.index.range_bounds; decided on the fp64
        ranking score, not on the rounded `distance`).  expr and exclude_ids as in search()."""
        lo, hi = range_bounds(self.metric_type, radius, range_filter)
        q = self._queries(data)
        if self.num_entities == 0:
            return [[] for _ in range(q.shape[0])]
        allow = None if expr is None else self._device_mask(expr)
        lims, sc, ids = self._ensure().range_search(q, lo, hi, exclude_ids=exclude_ids, allow=allow)
        lims, sc, ids = lims.cpu().numpy(), sc.cpu().numpy(), ids.cpu().numpy()
        fields = output_fields or []
        return [self._hits(ids[lims[i]:lims[i + 1]], sc[lims[i]:lims[i + 1]], fields) for i in range(q.shape[0])]

    def _device_codes(self, name):
        """The dictionary codes of scalar field `name` (mirx.expr.ExprCache.codes: one int64 per live row, aligned with
        live_ids()) as a tensor on the index's device, and the distinct values they stand for; built and uploaded once per
        collection state, like _device_mask."""
        from .expr import ExprCache
        index = self._ensure()
        if self._expr is None:
            self._expr = ExprCache(self.live_ids(), self.field)
        cache = self._expr
        distinct, codes = cache._coded(name)
        dev = cache.device_codes.get(name)
        if dev is None or dev.device != index.device:
            dev = cache.device_codes[name] = torch.from_numpy(codes).to(index.device)
        return distinct, dev

    def _leave_out_check(self, field, values, nq, limit, group_by_field, param):
        """The argument checks of search(leave_out_field=, leave_out_values=): host only, no device touched."""
        from .expr import _kind
        if field is None or values is None:
            raise ValueError("leave_out_field and leave_out_values come together: the field, and one value (or None) per query")
        if not isinstance(field, str) or not self.has_field(field):
            raise ValueError(f"leave_out_field {field!r} is not a scalar field of {self.name} (fields: {', '.join(self._meta)})")
        if group_by_field is not None:
            raise ValueError("leave_out_field does not combine with group_by_field (grouping search has no leave-out form)")
        if self._range_params(param) is not None:
            raise ValueError("leave_out_field does not combine with a radius / range_filter (range search has no leave-out form)")
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 1 <= int(limit) <= 1024:
            raise ValueError(f"leave_out_field: limit must be an integer in [1, 1024], got {limit!r}")
        if isinstance(values, (str, bytes)) or not hasattr(values, "__len__"):
            raise ValueError("leave_out_values must be a sequence with one value (or None) per query")
        if len(values) != nq:
            raise ValueError(f"leave_out_values needs one value (or None) per query ({nq}), got {len(values)}")
        column = self._meta[field]
        want = "str" if field == "image_path" else (_kind(column[0]) if column else None)
        for v in values:
            if v is None:
                continue
            kind = _kind(v)
            if kind is None or (want is not None and kind != want):
                held = f"{type(column[0]).__name__} values such as {column[0]!r}" if column else "strings"
                raise ValueError(f"leave_out_values: type mismatch: {field} holds {held}, got {v!r}")

    def _leave_out_codes(self, field, values):
        """-> (row codes: int32 on the index's device, cast once per collection state; one int32 code per query on the host, -1
        for None and for a value no live row holds; the most rows one of the named values has)"""
        _, codes = self._device_codes(field)
        cache = self._expr
        dev = cache.device_codes.get((field, "int32"))
        if dev is None or dev.device != codes.device:
            dev = cache.device_codes[(field, "int32")] = codes.to(torch.int32)
        table, counts = cache.table(field)
        qcodes = np.fromiter((-1 if v is None else table.get(v, -1) for v in values), dtype=np.int32, count=len(values))
        named = qcodes[qcodes >= 0]
        return dev, qcodes, int(counts[named].max()) if named.size else 0

    def self_metrics(self, label_field="label", kappas=(1, 5, 10), leave_out_field=None, standard_ap=False, chunk_rows=4096):
        """Self-retrieval metrics of the collection's live rows from field names, without re-embedding anything: every row
        queries the collection with its own vector and is excluded from its own list; relevance is equality of
        `label_field`.  The full rankings are walked on the device (FlatIndex.rank_metrics), `chunk_rows` queries per call, and
        never exist as arrays.  leave_out_field (e.g. the patient of a study): a row's list also loses every row that shares
        its value of that field -- leave-group-out.
        Default: evaluate()'s numbers (mirx.evaluate.evaluate_embeddings) -- the trapezoidal AP, precision@kappa over
        min(largest positive rank, kappa), and without leave_out_field the row itself as the positive at the last rank.
        standard_ap=True: the mean of precision at each relevant rank with the row itself taken out of its list and
        precision@kappa = hits / kappa (fusion_eval/metrics.py).
        -> {"mAP", "pr": mean precision@kappa [len(kappas)], "acc": R@kappa in percent float32 [len(kappas)], "n_queries",
        "n_skipped": rows without a relevant row left (skipped in mAP and pr)}.  Unknown fields: ValueError."""
        from .metrics import map_from_device_result
        for what, f in (("label_field", label_field), ("leave_out_field", leave_out_field)):
            if f is not None and (not isinstance(f, str) or not self.has_field(f)):
                raise ValueError(f"{what} {f!r} is not a scalar field of {self.name} (fields: {', '.join(self._meta)})")
        if label_field is None:
            raise ValueError("self_metrics: label_field names the field that decides relevance")
        ks = [int(k) for k in kappas]
        if len(ks) > 8 or any(k < 1 for k in ks):
            raise ValueError(f"self_metrics: at most 8 kappas, each at least 1, got {list(kappas)}")
        n = self.num_entities
        if n == 0:
            return {"mAP": float("nan"), "pr": np.full(len(ks), np.nan), "acc": np.zeros(len(ks), dtype=np.float32),
                    "n_queries": 0, "n_skipped": 0}
        index = self._ensure()
        _, labels = self._device_codes(label_field)
        codes = None if leave_out_field is None else self._leave_out_codes(leave_out_field, [])[0]
        parts = []
        for s in range(0, n, int(chunk_rows)):
            q, ids = index.rows(s, min(int(chunk_rows), n - s))
            e = s + q.shape[0]
            parts.append(index.rank_metrics(q, labels, labels[s:e], ks, exclude_ids=ids, self_kind=2 if standard_ap else 0,
                                            row_codes=codes, query_codes=None if codes is None else codes[s:e],
                                            standard_ap=standard_ap))
        res = {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]}
        hit = (res["cnt"] > 0).sum(dim=0).cpu().numpy()
        acc = np.array([np.float32(np.float32(h) * np.float32(100.0 / n)) for h in hit], dtype=np.float32)
        if standard_ap:
            aps = res["ap"].cpu().numpy()
            ok = ~np.isnan(aps)
            cnt = res["cnt"].cpu().numpy().astype(np.float64)
            m_ap = float(aps[ok].mean()) if ok.any() else float("nan")
            pr = (cnt[ok] / np.asarray(ks, dtype=np.float64)[None, :]).mean(axis=0) if ok.any() else np.full(len(ks), np.nan)
        else:
            m_ap, aps, pr, _ = map_from_device_result(res, ks)
        return {"mAP": m_ap, "pr": pr, "acc": acc, "n_queries": n, "n_skipped": int(np.isnan(aps).sum())}

    def _search_grouped(self, q, limit, group_by_field, group_size, fields, exclude_ids, expr):
        distinct, codes = self._device_codes(group_by_field)
        allow = None if expr is None else self._device_mask(expr)
        ids, sc, _ = self._ensure().search_grouped(q, codes, limit, group_size, exclude_ids=exclude_ids, allow=allow)
        ids, sc = ids.cpu().numpy().reshape(q.shape[0], -1), sc.cpu().numpy().reshape(q.shape[0], -1)
        fields = list(fields) + ([] if group_by_field in fields else [group_by_field])
        return [self._hits(ids[qi], sc[qi], fields) for qi in range(q.shape[0])]

    def search(self, data, anns_field="embedding", param=None, limit=10, output_fields=None, exclude_ids=None, expr=None,
               group_by_field=None, group_size=1, strict_group_size=True, leave_out_field=None, leave_out_values=None):
        """-> list (one per query) of lists of Hit, best first.  `distance` follows Milvus:
        COSINE/IP -> similarity, L2 -> Euclidean distance (>= 0).  expr (pymilvus' scalar filter, mirx.expr) restricts the
        search to the rows it selects -- exactly, on the device (FlatIndex.search(allow=)) -- so there are fewer than `limit`
        hits when fewer rows are eligible; the mask of the last expression is reused until the collection changes.
        param: {"params": {"radius": r, "range_filter": f}} (or the two keys at the top level) makes it pymilvus' range search:
        the first `limit` hits of range_search(data, r, f, ...).  Every other key of param (nprobe, ef, metric_type) is ignored,
        with one exception: on a collection whose index was created with approximate=True (IVF_FLAT, IVF_SQ8 or IVF_PQ), a plain top-k call --
        no expr, no grouping, no leave-out, no radius, limit <= 1024; exclude_ids allowed -- whose param carries an integer
        nprobe >= 1 (under "params" or at the top level) is answered by that index: the exact top `limit` of the rows
        in the nprobe lists nearest to the query (IvfFlatIndex.search; IVF_SQ8: of their decoded rows, IvfSq8Index.search; IVF_PQ: by the ADC score of their codes,
        IvfPqIndex.search).  Every other call stays on the exact routes below, and
        so do hybrid_search's lists and self_metrics; so does every call while the collection holds fewer rows than nlist (IVF_PQ:
        than max(nlist, 256)).
        group_by_field (a scalar field of the schema) makes it pymilvus' grouping search: `limit` counts GROUPS (at most 1024),
        the result per query is one flat list of Hit, group after group, best group first and rank order inside a group, each
        group holding its best min(group_size, its eligible rows) rows (group_size <= 64, limit * group_size <= 16384); a
        hit's entity always carries the group field.  Exact (FlatIndex.search_grouped): strict_group_size=True is the only
        deterministic reading, so False is accepted and returns the same.  expr and exclude_ids work as without grouping; a
        radius does not combine with grouping (ValueError: range_search is the other call).
        leave_out_field (a scalar field of the schema) with leave_out_values (one literal per query, or None) makes it the
        leave-group-out search: query i skips every row whose field equals leave_out_values[i] -- the reference's
        `r.image_path != query.image_path` (fusion_eval/metrics.py:65, milvus_adapter.py:204-207) for any field, e.g. the patient
        of a study -- exactly, on the device (FlatIndex.search_leave_out), as one `expr='field != value'` search per query would.
        None, or a value no row holds, leaves nothing out.  expr and exclude_ids combine with it; limit <= 1024; grouping and a
        radius do not combine with it (ValueError, like an unknown field, a wrong length or a literal of the wrong type)."""
        q = self._queries(data)
        fields = output_fields or []
        if leave_out_field is not None or leave_out_values is not None:
            self._leave_out_check(leave_out_field, leave_out_values, q.shape[0], limit, group_by_field, param)
            if self.num_entities == 0:
                return [[] for _ in range(q.shape[0])]
            limit = min(int(limit), self.num_entities)
            codes, qcodes, most = self._leave_out_codes(leave_out_field, leave_out_values)
            allow = None if expr is None else self._device_mask(expr)
            sc, ids = self._ensure().search_leave_out(q, limit, codes, qcodes, exclude_ids=exclude_ids, allow=allow,
                                                      max_left_out=most)
            ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
            return [self._hits(ids[qi], sc[qi], fields) for qi in range(q.shape[0])]
        if group_by_field is not None:
            if not self.has_field(group_by_field):
                raise ValueError(f"group_by_field {group_by_field!r} is not a scalar field of {self.name} "
                                 f"(fields: {', '.join(self._meta)})")
            limit, group_size = group_bounds(limit, group_size)
            if self._range_params(param) is not None:
                raise ValueError("group_by_field does not combine with a radius / range_filter: range search "
                                 "(Collection.range_search) is the other call")
            if self.num_entities == 0:
                return [[] for _ in range(q.shape[0])]
            return self._search_grouped(q, limit, group_by_field, group_size, fields, exclude_ids, expr)
        if self.num_entities == 0:
            return [[] for _ in range(q.shape[0])]
        limit = min(int(limit), self.num_entities)
        rng = self._range_params(param)
        if rng is not None and rng[1] is not None:
            return [hits[:limit] for hits in self.range_search(q, rng[0], rng[1], expr=expr, exclude_ids=exclude_ids,
                                                               output_fields=output_fields)]
        lo = None if rng is None else range_bounds(self.metric_type, rng[0])[0]
        nprobe = self._nprobe(param) if self._approx_nlist is not None and rng is None and expr is None and limit <= 1024 else None
        ivf = None if nprobe is None else self._ensure_ivf()
        if ivf is not None:
            sc, ids = ivf.search(q, limit, nprobe, exclude_ids=exclude_ids)
            ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
            return [self._hits(ids[qi], sc[qi], fields) for qi in range(q.shape[0])]
        allow = None if expr is None else self._device_mask(expr)
        find = self._finder(limit, exclude_ids)
        if lo is None:
            sc, ids = find(q, limit, exclude_ids=exclude_ids, allow=allow)
            ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
        else:
            # a radius alone: the best `limit` rows, then those outside the radius dropped by their fp64 ranking scores -- the
            # first `limit` hits of range_search without collecting the rest
            s64, ids = find(q, limit, exclude_ids=exclude_ids, allow=allow, return_f64=True)
            ids, s64 = ids.cpu().numpy(), s64.cpu().numpy()
            ids = np.where(s64 > lo, ids, -1)
            sc = (s64 if self.metric_type in ("COSINE", "IP") else -np.sqrt(np.maximum(-s64, 0.0))).astype(np.float32)
        return [self._hits(ids[qi], sc[qi], fields) for qi in range(q.shape[0])]

    def _finder(self, limit, exclude_ids):
        """the index call that answers `limit` hits per query: search up to the filter lists' k, search_deep up to 1024 (the
        filter GEMM with deep candidate lists where the gallery is large enough), rank_top beyond"""
        index = self._ensure()
        if limit > 1024:
            return index.rank_top
        return index.search_deep if limit + (0 if exclude_ids is None else 1) > tier1_max_k() else index.search

    def _ranked(self, q, limit, exclude_ids=None, expr=None, param=None):
        """The lists of search(q, limit=limit, exclude_ids=.., expr=.., param=..) as tensors on the index's device, for a
        collection with rows: (ids [nq, w] int64, distance [nq, w] float32 in the units of Hit.distance), w = min(limit,
        rows); a slot past a list's hits holds id -1 or a distance that is not finite.  The plain top-k never leaves the
        device; a radius / range_filter request goes through search() itself and is copied back (rare, and exact by
        construction)."""
        limit = min(int(limit), self.num_entities)
        index = self._ensure()
        if self._range_params(param) is not None:
            lists = self.search(q, param=param, limit=limit, exclude_ids=exclude_ids, expr=expr)
            ids = np.full((len(lists), limit), -1, dtype=np.int64)
            dist = np.zeros((len(lists), limit), dtype=np.float32)
            for qi, hits in enumerate(lists):
                ids[qi, :len(hits)] = [h.id for h in hits]
                dist[qi, :len(hits)] = [h.distance for h in hits]
            return torch.from_numpy(ids).to(index.device), torch.from_numpy(dist).to(index.device)
        allow = None if expr is None else self._device_mask(expr)
        find = self._finder(limit, exclude_ids)
        sc, ids = find(q, limit, exclude_ids=exclude_ids, allow=allow)
        return ids, (sc if self.metric_type in ("COSINE", "IP") else -sc)


# -- hybrid search: several requests, one fused ranking ---------------------------------------------------------
class AnnSearchRequest:
    """pymilvus' AnnSearchRequest: one search of a hybrid search.  `anns_field` names the collection the request searches
    (a model type for MilvusManager.hybrid_search, a key of the mapping for hybrid_search); data, param, limit and expr are
    those of Collection.search."""

    def __init__(self, data, anns_field, param=None, limit=10, expr=None):
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)):
            raise ValueError(f"AnnSearchRequest: limit must be an integer, got {type(limit).__name__}")
        if int(limit) < 1:
            raise ValueError(f"AnnSearchRequest: limit must be at least 1, got {limit}")
        if param is not None and not isinstance(param, dict):
            raise ValueError(f"AnnSearchRequest: param must be a dict or None, got {type(param).__name__}")
        if expr is not None and not isinstance(expr, str):
            raise ValueError(f"AnnSearchRequest: expr must be a string or None, got {type(expr).__name__}")
        self.data, self.anns_field, self.param, self.limit, self.expr = data, anns_field, param, int(limit), expr


class RRFRanker:
    """pymilvus' RRFRanker: reciprocal rank fusion, score = sum over the requests whose list holds the document of
    1 / (k + rank), rank counted from 1.  0 < k < 16384."""

    def __init__(self, k=60):
        if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)):
            raise ValueError(f"RRFRanker: k must be a number, got {type(k).__name__}")
        if not 0 < float(k) < 16384:
            raise ValueError(f"RRFRanker: k must be in (0, 16384), got {k}")
        self.k = float(k)

    def kernel_form(self, metric_types):
        """the ranker as mirx.index.fuse_ranked takes it, for requests on collections of these metric types"""
        return ("rrf", self.k)


class WeightedRanker:
    """pymilvus' WeightedRanker: score = sum of weight_r * n_r(distance_r), one weight in [0, 1] per request.  With
    norm_score=True every distance is first mapped into [0, 1] by its collection's metric -- COSINE (1 + d) / 2, IP
    0.5 + atan(d) / pi, L2 1 - 2 atan(d) / pi; norm_score=False adds the raw similarities, which only COSINE and IP
    collections allow (an L2 distance grows as the match gets worse)."""

    def __init__(self, *weights, norm_score=True):
        if not weights:
            raise ValueError("WeightedRanker: one weight per request is needed")
        for w in weights:
            if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)):
                raise ValueError(f"WeightedRanker: a weight must be a number, got {type(w).__name__}")
            if not 0.0 <= float(w) <= 1.0:
                raise ValueError(f"WeightedRanker: a weight must be in [0, 1], got {w}")
        self.weights = [float(w) for w in weights]
        self.norm_score = bool(norm_score)

    def kernel_form(self, metric_types):
        metric_types = list(metric_types)
        if len(metric_types) != len(self.weights):
            raise ValueError(f"WeightedRanker: {len(self.weights)} weights for {len(metric_types)} requests")
        for m in metric_types:
            if m not in ("COSINE", "IP", "L2"):
                raise ValueError(f"WeightedRanker: unknown metric type {m!r}")
        if not self.norm_score:
            if "L2" in metric_types:
                raise ValueError("WeightedRanker: norm_score=False adds raw similarities and does not combine with an L2 collection")
            return ("weighted", self.weights, ["RAW"] * len(metric_types))
        return ("weighted", self.weights, metric_types)


def join_codes(columns, join_field="image_path"):
    """Document codes of a hybrid search.  columns: one (name, keys, ids) per collection in request order, keys / ids those of
    its live rows in index order.  Rows whose keys are equal are one document; a document's code is the index of its key's
    first appearance, collection after collection, row after row.
    -> (codes: one int64 array per collection aligned with its rows, owners: per code the (collection number, id) of the row
    that introduced it, id_of: per collection {key: id}).  A key that repeats inside one collection: ValueError."""
    code_of, owners, codes, id_of = {}, [], [], []
    for ci, (name, keys, ids) in enumerate(columns):
        own = {}
        arr = np.empty((len(keys),), dtype=np.int64)
        for p, (key, id_) in enumerate(zip(keys, ids)):
            if key in own:
                raise ValueError(f"hybrid search: {join_field} {key!r} repeats among the live rows of {name}; "
                                 f"joining needs one row per {join_field} and collection")
            own[key] = int(id_)
            code = code_of.get(key)
            if code is None:
                code = code_of[key] = len(owners)
                owners.append((ci, int(id_)))
            arr[p] = code
        codes.append(arr)
        id_of.append(own)
    return codes, owners, id_of


class _JoinTable:
    """join_codes of some collections in their current state, and its per-collection code arrays on the device"""

    def __init__(self, cols, join_field):
        for c in cols:
            if not c.has_field(join_field):
                raise ValueError(f"join_field {join_field!r} is not a scalar field of {c.name} (fields: {', '.join(c._meta)})")
        self.cols = cols
        self.versions = tuple(c._version for c in cols)
        self.codes, self.owners, self.id_of = join_codes([(c.name, c.field(join_field), c.live_ids().tolist()) for c in cols],
                                                         join_field)
        self._device = {}

    def device_codes(self, ci, device):
        dev = self._device.get(ci)
        if dev is None or dev.device != device:
            dev = self._device[ci] = torch.from_numpy(self.codes[ci]).to(device)
        return dev


def _join_table(cols, join_field):
    """the join table of these collections (distinct, in request order), built once per state of all of them: it is kept by
    the first one and dropped when any of them changes"""
    key = (join_field,) + tuple(id(c) for c in cols[1:])
    table = cols[0]._joins.get(key)
    if table is None or table.versions != tuple(c._version for c in cols):
        table = cols[0]._joins[key] = _JoinTable(cols, join_field)
    return table


def _request_collections(collections, reqs):
    if isinstance(collections, dict):
        cols = []
        for r in reqs:
            if r.anns_field not in collections:
                raise ValueError(f"Collection for {r.anns_field} not loaded")
            cols.append(collections[r.anns_field])
        return cols
    cols = list(collections)
    if len(cols) != len(reqs):
        raise ValueError(f"hybrid search: {len(cols)} collections for {len(reqs)} requests (one per request, or a mapping that the "
                         f"requests' anns_field names)")
    return cols


def hybrid_search(collections, reqs, rerank, limit, join_field="image_path", output_fields=None, exclude_keys=None,
                  group_by_field=None):
    """pymilvus' hybrid_search across collections: run every request, fuse the ranked lists on the device, -> one list of Hit
    per query, best first.

    collections: {name: Collection} that each request's anns_field names, or one Collection per request; the same collection
    may serve several requests (several query vectors, one gallery).  reqs: 1 to 8 AnnSearchRequest with equally many
    queries, their limits at most 4096 together.  rerank: RRFRanker or WeightedRanker.  limit: 1 to 1024 documents.
    Rows of different collections are one DOCUMENT when their `join_field` values are equal (join_codes).  Request r's list
    is exactly what its collection's search(data, limit=, expr=, param=, exclude_ids=) returns; a document's fp64 score is
    the sum of its lists' contributions in request order (the ranker's docstring; include/mirx.h for the arithmetic).
    The result holds the min(limit, distinct documents) best documents, equal scores by first appearance of the key.  A Hit's
    id and entity are those of the document's row in the first requested collection that holds it, its `distance` is the
    fused score, its entity always carries the join field.
    exclude_keys: one join-field value per query (or None): that document leaves every list before the fusion -- the
    reference's exclude_self by image_path; a key a collection does not hold excludes nothing there.
    Grouping does not combine with hybrid search (ValueError)."""
    from .index import fuse_bounds, fuse_ranked
    reqs = list(reqs)
    for r in reqs:
        if not isinstance(r, AnnSearchRequest):
            raise ValueError(f"hybrid search: the requests must be AnnSearchRequest, got {type(r).__name__}")
    segments, limit = fuse_bounds([r.limit for r in reqs], limit)
    if group_by_field is not None or any("group_by_field" in (r.param or {}) for r in reqs):
        raise ValueError("hybrid search does not combine with group_by_field: grouping search (Collection.search) is the other call")
    if not isinstance(rerank, (RRFRanker, WeightedRanker)):
        raise ValueError(f"hybrid search: rerank must be an RRFRanker or a WeightedRanker, got {type(rerank).__name__}")
    cols = _request_collections(collections, reqs)
    form = rerank.kernel_form([c.metric_type for c in cols])
    queries = [c._queries(r.data) for c, r in zip(cols, reqs)]
    nq = queries[0].shape[0]
    if any(q.shape[0] != nq for q in queries):
        raise ValueError(f"hybrid search: every request needs the same number of queries, got {[q.shape[0] for q in queries]}")
    if exclude_keys is not None:
        exclude_keys = list(exclude_keys)
        if len(exclude_keys) != nq:
            raise ValueError("exclude_keys needs one key per query")
    distinct = []
    for c in cols:
        if not any(c is d for d in distinct):
            distinct.append(c)
    which = [next(i for i, d in enumerate(distinct) if d is c) for c in cols]
    table = _join_table(distinct, join_field)
    if not table.owners:
        return [[] for _ in range(nq)]
    device = next(c for c in distinct if c.num_entities).index.device
    codes = torch.full((nq, sum(segments)), -1, dtype=torch.int64, device=device)
    dist = torch.zeros((nq, sum(segments)), dtype=torch.float32, device=device)
    off = 0
    for c, ci, r, q, width in zip(cols, which, reqs, queries, segments):
        if c.num_entities:
            ex = None
            if exclude_keys is not None:
                ex = torch.tensor([table.id_of[ci].get(k, -1) for k in exclude_keys], dtype=torch.int64)
            ids, d = c._ranked(q, r.limit, ex, r.expr, r.param)
            pos = c.index._positions(ids)
            code = table.device_codes(ci, ids.device)[pos.clamp(min=0)]
            code = torch.where((pos >= 0) & torch.isfinite(d), code, torch.full_like(code, -1))
            codes[:, off:off + ids.shape[1]] = code.to(device)
            dist[:, off:off + ids.shape[1]] = torch.where(code >= 0, d, torch.zeros_like(d)).to(device)
        off += width
    out_codes, out_scores, _, _, count = fuse_ranked(codes, dist, segments, form, limit, n_codes=len(table.owners))
    out_codes, out_scores, count = out_codes.cpu().tolist(), out_scores.cpu().tolist(), count.cpu().tolist()
    fields = list(output_fields or [])
    fields += [] if join_field in fields else [join_field]
    results = []
    for qi in range(nq):
        hits = []
        for code, score in zip(out_codes[qi][:count[qi]], out_scores[qi][:count[qi]]):
            ci, id_ = table.owners[code]
            hits.append(Hit(id_, score, distinct[ci].entity(id_, fields)))
        results.append(hits)
    return results


_NETWORK_SCHEMES = ("http", "https", "tcp", "grpc")


def store_root_of(uri):
    """The directory a MilvusManager uri names, or None for "in memory": None and every uri with a network scheme (http,
    https, tcp, grpc -- never contacted, this package opens no socket) keep the gallery in the process; a filesystem path
    or a file:// uri names a mirx.store.Store."""
    if uri is None or uri == "":
        return None
    uri = os.fspath(uri)
    if "://" in uri:
        from urllib.parse import unquote, urlparse
        parts = urlparse(uri)
        if parts.scheme.lower() in _NETWORK_SCHEMES:
            return None
        if parts.scheme.lower() != "file":
            raise ValueError(f"uri {uri!r}: a filesystem path, a file:// uri or a {'/'.join(_NETWORK_SCHEMES)} uri is expected")
        if parts.netloc not in ("", "localhost"):
            raise ValueError(f"uri {uri!r}: a file:// uri names a local path")
        return unquote(parts.path)
    return uri


class MilvusManager:
    """Same surface as milvus_setup.MilvusManager; "connecting" binds a GPU instead of a server.  With a filesystem path or
    a file:// uri the collections persist in a mirx.store.Store under it; with uri=None or a network uri they live in this
    object, as before, and nothing is written anywhere."""

    def __init__(self, uri=None, token=None, user="", password="", dataset="default", device=None):
        self.uri, self.token, self.user, self.password = uri, token, user, password
        self.dataset = dataset
        self.collections = {}
        self.device = device
        self._store = {}
        root = store_root_of(uri)
        self._disk = None
        if root is not None:
            from .store import Store
            self._disk = Store(root)
        self.connected = False

    @property
    def is_persistent(self):
        return self._disk is not None

    def get_model_config(self, model_type):
        if model_type not in MODEL_CONFIGS:
            raise ValueError(f"Unknown model type: {model_type}")
        config = dict(MODEL_CONFIGS[model_type])
        names = config.pop("collection_names", {})
        config["collection_name"] = names.get(self.dataset, names.get("default"))
        if not config["collection_name"]:
            raise ValueError(f"No collection name configured for model '{model_type}' and dataset '{self.dataset}'")
        return config

    def connect(self):
        try:
            from . import _lib
            _lib.load()
            if not torch.cuda.is_available():
                raise RuntimeError("no GPU visible")
            self.connected = True
            return True
        except Exception as e:  # reference behaviour: report and return False (milvus_setup.py:135-137)
            print(f"Connection failed: {e}")
            return False

    def disconnect(self):
        self.connected = False

    # -- pymilvus.utility analogues (milvus_setup.py:150-158 uses has_collection / drop_collection) ------------------------
    def has_collection(self, name):
        return name in self._store or (self._disk is not None and self._disk.has(name))

    def list_collections(self):
        return sorted(set(self._store) | set(self._disk.names() if self._disk is not None else ()))

    def drop_collection(self, name):
        """Forget `name` (and remove it from disk for a persistent manager); a name that does not exist is no error."""
        col = self._store.pop(name, None)
        for model_type in [m for m, c in self.collections.items() if c is col or c.name == name]:
            del self.collections[model_type]
        if self._disk is not None:
            self._disk.drop(name)

    def _open(self, name):
        """the collection `name` from this manager's catalogue (memory first, then disk), or None"""
        if name not in self._store and self._disk is not None and self._disk.has(name):
            self._store[name] = Collection.from_stored(self._disk.open(name), device=self.device)
        return self._store.get(name)

    def create_collection(self, model_type, drop_old=False):
        config = self.get_model_config(model_type)
        name = config["collection_name"]
        if drop_old:
            self.drop_collection(name)
        col = self._open(name)
        if col is None:
            stored = None
            if self._disk is not None:
                stored = self._disk.create(name, config["embedding_dim"], "COSINE", ["id", "image_path", "label", "embedding"],
                                           config["description"])
            col = Collection(name, config["embedding_dim"], config["description"], device=self.device, stored=stored)
            self._store[name] = col
        elif col.dim != config["embedding_dim"]:
            raise ValueError(f"Collection {name} holds {col.dim}-dimensional rows, {model_type} embeds {config['embedding_dim']}")
        self.collections[model_type] = col
        return col

    def create_index(self, model_type, index_type="IVF_FLAT", metric_type="COSINE", nlist=1024, approximate=False):
        if model_type not in self.collections:
            raise ValueError(f"Collection for {model_type} not loaded")
        # index_type / nlist are accepted for compatibility: the search is exhaustive unless approximate=True asks for the
        # reference's IVF_FLAT (Collection.create_index).  "IVF_PQ" is handed through and raises there: this signature, the
        # reference's, carries no m, and Milvus refuses the type without one too
        self.collections[model_type].create_index(
            "embedding", {"metric_type": metric_type, "index_type": index_type, "params": {"nlist": nlist}}, approximate=approximate)
        return True

    def load_collection(self, model_type):
        if model_type not in self.collections:
            name = self.get_model_config(model_type)["collection_name"]
            col = self._open(name)
            if col is None:
                raise ValueError(f"Collection {name} does not exist")
            self.collections[model_type] = col
        self.collections[model_type].load()
        return self.collections[model_type]

    def get_collection_info(self, model_type):
        if model_type not in self.collections:
            name = self.get_model_config(model_type)["collection_name"]
            col = self._open(name)
            if col is None:
                raise ValueError(f"Collection {name} does not exist")
            self.collections[model_type] = col               # metadata only: nothing is loaded for it
        c = self.collections[model_type]
        return {"name": c.name, "num_entities": c.num_entities, "description": c.description, "schema": c.schema}

    def setup_all_collections(self, drop_old=False, metric_type="COSINE"):
        for model_type in MODEL_CONFIGS:
            self.create_collection(model_type, drop_old=drop_old)
            self.create_index(model_type, metric_type=metric_type)
            self.load_collection(model_type)

    def hybrid_search(self, reqs, rerank, limit, join_field="image_path", output_fields=None, exclude_keys=None,
                      group_by_field=None):
        """hybrid_search (above) over this manager's collections: a request's anns_field names the model type whose
        collection it searches ("convnextv2", "dinov2", ..; created or loaded before, else ValueError)."""
        return hybrid_search(self.collections, reqs, rerank, limit, join_field=join_field, output_fields=output_fields,
                             exclude_keys=exclude_keys, group_by_field=group_by_field)


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SIGLIP_MEAN, SIGLIP_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)


def default_transform(img_size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, resize=None, interpolation="bilinear"):
    """convert('RGB') -> Resize(shorter side) -> CenterCrop -> ToTensor -> Normalize(mean, std): the pipeline of
    milvus_retrieval.py:176-198 without torchvision (PIL + torch only).  Resize defaults follow the reference
    (448 -> 512, 384 -> 432, otherwise 256); MedSigLIP normalises with mean = std = 0.5 (milvus_retrieval.py:177-178),
    every other model with the ImageNet statistics.

    resize = (img_size, img_size) is the drivers' square stretch instead, Resize((S, S)) without a crop (test.py:1323,
    evaluate_saliency.py:249, test_ath.py:18, ...); any other pair raises ValueError.  interpolation is "bilinear" or
    "bicubic" (PIL's Image.BILINEAR / Image.BICUBIC are accepted): Resize(S + 32, BICUBIC) + CenterCrop(S) is
    get_transforms_medsiglip (compute_saliency.py:131-148), Resize((384, 384), BICUBIC) compute_saliency_convnextv2.py:154."""
    from .preprocess import attach, filter_name
    interpolation = filter_name(interpolation)
    if resize is None:
        resize = {448: 512, 384: 432}.get(img_size, 256)
    stretch = isinstance(resize, (tuple, list))
    if stretch:
        if tuple(resize) != (img_size, img_size):
            raise ValueError(f"resize must be an int or the pair (img_size, img_size) = ({img_size}, {img_size}), got {resize!r}")
        resize = (img_size, img_size)
    # numpy float32 arithmetic (the same IEEE operations as ToTensor + Normalize, bit for bit): torch's CPU operators cost
    # 10+ ms per call on a 150 k-element image when the intra-op thread pool is larger than the cores the process may use
    mean = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    std = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)

    def pixels(img):
        """convert -> Resize -> CenterCrop: the 8-bit pixels [3, S, S] that ToTensor + Normalize would then turn into floats"""
        from PIL import Image
        flt = Image.BICUBIC if interpolation == "bicubic" else Image.BILINEAR
        img = img.convert("RGB")
        if stretch:
            return np.ascontiguousarray(np.asarray(img.resize(resize, flt), dtype=np.uint8).transpose(2, 0, 1))
        w, h = img.size
        if w <= h:
            nw, nh = resize, int(resize * h / w)
        else:
            nw, nh = int(resize * w / h), resize
        img = img.resize((nw, nh), flt)
        left, top = int(round((nw - img_size) / 2.0)), int(round((nh - img_size) / 2.0))
        img = img.crop((left, top, left + img_size, top + img_size))
        return np.ascontiguousarray(np.asarray(img, dtype=np.uint8).transpose(2, 0, 1))

    def tf(img):
        x = pixels(img).astype(np.float32) / np.float32(255.0)
        return torch.from_numpy(np.ascontiguousarray((x - mean) / std))

    # MilvusRetriever.search hands the 8-bit pixels to a model that normalises them itself with the same constants (DenseNet121:
    # inside the stem kernel, bit-identical to the float path -- tests/test_model_gpu.py): a quarter of the bytes to the device
    # and no float pass over the image on the host
    tf.pixels = pixels
    tf.mean, tf.std = tuple(float(v) for v in mean.ravel()), tuple(float(v) for v in std.ravel())
    # tf.batch_pixels(images, device) / tf.batch(images, device): the same two results for a list of images, resized on the
    # device in one launch and bit-equal to the above; tf.last_preprocess counts the images per path (mirx.preprocess, DESIGN 28,
    # 30)
    return attach(tf, img_size, resize, interpolation)


class MilvusRetriever:
    """milvus_retrieval.MilvusRetriever with an exact in-process search."""

    def __init__(self, manager, model_type, model, transform):
        self.manager = manager
        self.model_type = model_type
        self.model = model
        self.transform = transform
        self.collection = None

    def load_collection(self):
        if self.collection is None:
            self.manager.load_collection(self.model_type)
            self.collection = self.manager.collections[self.model_type]
        return self.collection

    def _device(self):
        if hasattr(self.model, "device"):
            return self.model.device
        try:
            return next(self.model.parameters()).device
        except StopIteration:
            return torch.device("cuda")

    def _query_tensor(self, img):
        """transform(img)[None] -- or, when the transform is default_transform and the model normalises 8-bit input itself with
        the transform's constants, the 8-bit pixels (same embedding bit for bit, a quarter of the bytes, no host float pass)."""
        tf, m = self.transform, self.model
        px = getattr(tf, "pixels", None)
        if px is not None and getattr(m, "accepts_uint8", False) and self._device().type == "cuda" and not m.training:
            mean, std = getattr(m, "input_mean", None), getattr(m, "input_std", None)
            if mean is not None and tuple(float(v) for v in mean) == tf.mean and tuple(float(v) for v in std) == tf.std:
                if hasattr(tf, "batch_pixels"):              # resized on the device (mirx.preprocess): the same bytes
                    return tf.batch_pixels([img], self._device())
                return torch.from_numpy(px(img)).unsqueeze(0)
        if hasattr(tf, "batch"):
            return tf.batch([img], self._device())
        return tf(img).unsqueeze(0)

    @property
    def last_preprocess(self):
        """{"device": n, "host": m}: how many images of the last query batch were resized on the device / on the host (None for
        a transform without the batch attributes)."""
        return getattr(self.transform, "last_preprocess", None)

    def embed(self, images):
        """Batched F.normalize(model(x)) for a [B,3,H,W] tensor (milvus_retrieval.py:60-63)."""
        with torch.no_grad():
            out = self.model(images.to(self._device()))
            if isinstance(out, dict):
                out = out["embedding"]
            return F.normalize(out, p=2, dim=1)

    def _embed_rows(self, images):
        """embed() with every row normalised as the [1, D] tensor a single search() normalises: torch reduces a [B, D] and a
        [1, D] tensor in different orders, so F.normalize of a batch can put a row's norm one ulp from the single query's and
        with it every distance of that query.  One small reduction per row, then F.normalize's own clamp and division: each
        row equals embed(images[i:i + 1]) bit for bit (the model's rows do not depend on the batch)."""
        with torch.no_grad():
            out = self.model(images.to(self._device()))
            if isinstance(out, dict):
                out = out["embedding"]
            norms = torch.cat([out[i:i + 1].norm(2, 1, True) for i in range(out.shape[0])])
            return out / norms.clamp_min(1e-12).expand_as(out)

    def search(self, query_image_path, top_k=10, search_params=None, metric_type="COSINE", expr=None, group_by=None, group_size=1,
               leave_out=None):
        """-> (results, query_embedding).  results: best-first dicts {id, image_path, label,
        distance, similarity}; similarity = distance for COSINE/IP, 1 - d^2/2 for L2.  expr: Collection.search's filter.
        group_by (a scalar field) / group_size: Collection.search's grouping search -- top_k counts groups, the dicts come group
        after group and gain a "group" key with the field's value (without group_by the dicts keep the reference's keys).
        leave_out: (field, value) -- Collection.search's leave-group-out search: rows whose field equals value are skipped (the
        dicts are unchanged)."""
        if isinstance(query_image_path, str):
            from PIL import Image
            img = Image.open(query_image_path).convert("RGB")
        else:
            img = query_image_path
        query_embedding = self.embed(self._query_tensor(img))
        if self.collection is None:
            self.load_collection()
        if metric_type not in ("COSINE", "IP", "L2"):
            raise ValueError(f"Unknown metric type: {metric_type}")
        if metric_type != self.collection.metric_type and {metric_type, self.collection.metric_type} != {"COSINE", "IP"}:
            # Milvus rejects a search whose metric differs from the index's (milvus_retrieval.py:75-86)
            raise ValueError(f"metric type not match: index has {self.collection.metric_type}, search asked {metric_type}")
        hits = self.collection.search(data=query_embedding, anns_field="embedding", param=search_params,
                                      limit=top_k, output_fields=["image_path", "label"], expr=expr,
                                      **self._grouping(group_by, group_size), **self._leaving_out(leave_out, 1))[0]
        return [self._format(h, metric_type, group_by) for h in hits], query_embedding

    @staticmethod
    def _grouping(group_by, group_size):
        """Collection.search's grouping keywords, none when no grouping is asked for"""
        return {} if group_by is None else {"group_by_field": group_by, "group_size": group_size}

    @staticmethod
    def _leaving_out(leave_out, nq):
        """Collection.search's leave-out keywords from search()'s (field, value) (nq = 1) or batch_search()'s (field, [values])"""
        if leave_out is None:
            return {}
        if not isinstance(leave_out, (tuple, list)) or len(leave_out) != 2:
            raise ValueError("leave_out is a pair: (field, value) for search, (field, [one value per query]) for batch_search")
        field, values = leave_out
        return {"leave_out_field": field, "leave_out_values": [values] if nq == 1 else values}

    @staticmethod
    def _format(hit, metric_type, group_by=None):
        d = hit.distance
        sim = d if metric_type in ("COSINE", "IP") else 1.0 - (d * d) / 2.0
        out = {"id": hit.id, "image_path": hit.entity.get("image_path"), "label": hit.entity.get("label"),
               "distance": d, "similarity": sim}
        if group_by is not None:
            out["group"] = hit.entity.get(group_by)
        return out

    def batch_search(self, query_image_paths, top_k=10, search_params=None, expr=None, group_by=None, group_size=1, leave_out=None):
        """One batched embed + one batched search (the reference loops search(); results equal, to the bit: _embed_rows).
        expr: Collection.search's filter, one for the whole batch.  group_by / group_size: as in search().  leave_out:
        (field, [one value or None per query]) -- search()'s leave-group-out, each query with its own value."""
        if len(query_image_paths) == 0:
            return []
        from PIL import Image
        imgs = [Image.open(p).convert("RGB") if isinstance(p, str) else p for p in query_image_paths]
        if hasattr(self.transform, "batch"):                 # one device-side resize of the whole batch: the same floats
            emb = self._embed_rows(self.transform.batch(imgs, self._device()))
        else:
            emb = self._embed_rows(torch.stack([self.transform(i) for i in imgs]))
        if self.collection is None:
            self.load_collection()
        all_hits = self.collection.search(data=emb, param=search_params, limit=top_k, output_fields=["image_path", "label"],
                                          expr=expr, **self._grouping(group_by, group_size),
                                          **self._leaving_out(leave_out, None))
        return [[self._format(h, self.collection.metric_type, group_by) for h in hits] for hits in all_hits]

    def adapter(self, name=None):
        """This retriever's collection seen through retrieval_analysis' MilvusCollectionAdapter (mirx.adapter)."""
        from .adapter import MilvusCollectionAdapter, MilvusCollectionConfig
        if self.collection is None:
            self.load_collection()
        return MilvusCollectionAdapter(MilvusCollectionConfig(name=name or self.model_type,
                                                              collection_name=self.collection.name),
                                       collection=self.collection)

    def search_by_embeddings(self, queries, query_embeddings, top_k, search_params=None, reranker=None,
                             exclude_self=True, metadata_fields=None, batch_size=None):
        """retrieval_analysis/milvus_adapter.py:218-275, same arguments and return type (list[SearchResult]): one
        batched exact search; self dropped by image_path after fetching top_k + 1; `reranker.rerank(query, results)`
        applied before the cut to top_k."""
        return self.adapter().search_by_embeddings(queries, query_embeddings, top_k, search_params, reranker,
                                                   exclude_self, metadata_fields, batch_size)

    def search_ids(self, query_embeddings, top_k=10, exclude_ids=None):
        """Device-side batch form (no reference counterpart): -> best-first dicts per query, self excluded by id."""
        if self.collection is None:
            self.load_collection()
        hits = self.collection.search(data=query_embeddings, limit=top_k, output_fields=["image_path", "label"],
                                      exclude_ids=exclude_ids)
        return [[self._format(h, self.collection.metric_type) for h in hs] for hs in hits]


def search_collection(collection, query_vector, top_k, nprobe=10):
    """nih_zilliz_utils.search_collection (lives in mirx.nih with the other NIH helpers)."""
    from .nih import search_collection as _sc
    return _sc(collection, query_vector, top_k, nprobe)


def get_model_and_transform(model_type, model_weights, embedding_dim, device):
    """milvus_retrieval.get_model_and_transform for the model families built so far."""
    from .model import build_model
    model, img_size = build_model(model_type, embedding_dim=embedding_dim)
    if model_weights:
        checkpoint = torch.load(model_weights, map_location=device)
        for key in ("state-dict", "state_dict"):
            if isinstance(checkpoint, dict) and key in checkpoint:
                checkpoint = checkpoint[key]
        model.load_state_dict(checkpoint, strict=False)
    model.eval()
    model.to(device)
    if model_type == "medsiglip":                  # SigLIP normalisation (milvus_retrieval.py:176-181)
        return model, default_transform(img_size, SIGLIP_MEAN, SIGLIP_STD)
    return model, default_transform(img_size)
