"""FlatIndex -- device-resident exhaustive index over the C ABI (include/mirx.h).

Stands where the reference uses a Milvus collection (milvus/milvus_setup.py:139-222,
milvus/milvus_retrieval.py:80-86) or the inline torch brute force (test.py:1080-1090).
Torch is plumbing only: tensors own the query/result memory, `data_ptr()` crosses the ABI.
"""
import ctypes
import types

import numpy as np
import torch

from . import _lib
from ._lib import METRIC_IP, METRIC_NEG_L2, MirxError

_METRICS = {"COSINE": METRIC_IP, "IP": METRIC_IP, "L2": METRIC_NEG_L2,
            "cosine": METRIC_IP, "ip": METRIC_IP, "l2": METRIC_NEG_L2, "cdist": METRIC_NEG_L2}


def metric_code(metric):
    if isinstance(metric, int):
        return metric
    try:
        return _METRICS[metric]
    except KeyError:
        raise ValueError(f"Unknown metric type: {metric}") from None


def _bound(value, name):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {type(value).__name__}")
    value = float(value)
    if value != value:
        raise ValueError(f"{name} is NaN")
    return value


def range_bounds(metric_type, radius, range_filter=None):
    """pymilvus' `radius` / `range_filter` search parameters as the bounds (lo, hi) of FlatIndex.range_search, in fp64.

    COSINE / IP keep radius < similarity <= range_filter: lo = radius, hi = range_filter (+inf when absent).
    L2 keeps range_filter <= distance < radius in the Euclidean units of Hit.distance; the index ranks by the NEGATIVE SQUARED
    distance, so lo = -(radius ** 2) and hi = -(range_filter ** 2) (0.0 when absent).
    Membership is decided on the fp64 ranking score (what search(return_f64=True) returns), not on the rounded fp32 `distance`
    a hit reports: a row whose fp32 distance rounds onto the radius can fall on either side of it.
    ValueError as pymilvus: range_filter <= radius for COSINE / IP; range_filter >= radius or a negative value for L2; a NaN;
    a value that is not a number."""
    metric = metric_code(metric_type)
    radius = _bound(radius, "radius")
    rf = None if range_filter is None else _bound(range_filter, "range_filter")
    if metric == METRIC_NEG_L2:
        if radius < 0 or (rf is not None and rf < 0):
            raise ValueError("L2 radius / range_filter are distances: they must not be negative")
        if rf is not None and rf >= radius:
            raise ValueError(f"L2 range_filter ({rf}) must be less than radius ({radius})")
        return -(radius * radius), (0.0 if rf is None else -(rf * rf))
    if rf is not None and rf <= radius:
        raise ValueError(f"COSINE / IP range_filter ({rf}) must be greater than radius ({radius})")
    return radius, (float("inf") if rf is None else rf)


# Routing of FlatIndex.search_grouped: these only affect speed, never the answer.
GROUP_DIRECT_MAX = 16                      # at most this many groups with eligible rows: one masked search per group
GROUP_FILL_MAX = _lib.GROUP_FILL_MAX       # largest group mirx_index_group_fill completes; a larger one is reached by deepening
GROUP_FIRST_DEPTH = 64                     # the first walked prefix (k + excluded id <= 64 keeps search() on the filter-GEMM tier)
GROUP_DEEPEN_FACTOR = 8                    # each deeper prefix is this many times the previous one
GROUP_DEEPEN_BYTES = 256 << 20             # most ids + fp64 scores one rank_top call of the deepening returns
_GROUP_ROUTES = ("auto", "direct", "walk", "deepen")


def group_bounds(limit, group_size):
    """limit / group_size of a grouping search as ints, ValueError outside the contract's bounds"""
    for name, v in (("limit", limit), ("group_size", group_size)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {type(v).__name__}")
    limit, group_size = int(limit), int(group_size)
    if not 1 <= limit <= _lib.GROUP_MAX_LIMIT:
        raise ValueError(f"grouping search: limit (the number of groups) must be in [1, {_lib.GROUP_MAX_LIMIT}], got {limit}")
    if not 1 <= group_size <= _lib.GROUP_MAX_SIZE:
        raise ValueError(f"grouping search: group_size must be in [1, {_lib.GROUP_MAX_SIZE}], got {group_size}")
    if limit * group_size > _lib.GROUP_MAX_HITS:
        raise ValueError(f"grouping search: limit * group_size must not exceed {_lib.GROUP_MAX_HITS}, got {limit * group_size}")
    return limit, group_size


def tier1_max_k():
    """the most k (+1 with excluded ids) FlatIndex.search answers on the filter route; past it search_deep is the faster call"""
    return int(_lib.load().mirx_tier1_max_k())


def deep_min_rows(k_eff, nq):
    """rows (the index's, or a mask's allowed rows) from which search_deep's filter route answers nq queries at this k_eff"""
    return int(_lib.load().mirx_deep_min_rows(int(k_eff), int(nq)))


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ptr_or_null(t):
    """_ptr, with a null for an empty tensor too"""
    return None if t is None or not t.numel() else ctypes.c_void_p(t.data_ptr())


def _score_ptrs(sc, return_f64):
    """(fp32 reported values, fp64 ranking scores): the score outputs of a call that fills `sc` as one of the two"""
    return (None, _ptr_or_null(sc)) if return_f64 else (_ptr_or_null(sc), None)


class FlatIndex:
    """Exact top-k over fp32 rows resident on one GPU.

    Ranking semantics (pinned by oracle/search_ref.c): fp64 score, ties -> lower id.
    `metric`: 'COSINE'/'IP' (dot product; cosine for unit rows) or 'L2' (ranks by distance,
    reports -||q-g||_2 like the reference's `-torch.cdist`).
    """

    def __init__(self, dim, metric="COSINE", device=None):
        if not torch.cuda.is_available():
            raise MirxError("FlatIndex needs a GPU: libmirx has no CPU path")
        self._lib = _lib.load()
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        self.dim = int(dim)
        self.metric = metric_code(metric)
        h = ctypes.c_void_p()
        _lib.check(self._lib.mirx_index_create(self.dim, self.metric, self.device.index, ctypes.byref(h)),
                   "mirx_index_create")
        self._h = h
        self._ids = self._id_table = None                    # ids() and what search_grouped derives from them, until the rows change
        self._group_stats = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.mirx_index_destroy(h)
            self._h = None

    def __len__(self):
        return int(self._lib.mirx_index_size(self._h))

    @property
    def ntotal(self):
        return len(self)

    def set_option(self, option, value):
        _lib.check(self._lib.mirx_index_set_option(self._h, option, int(value)), "mirx_index_set_option")

    def reserve(self, rows):
        _lib.check(self._lib.mirx_index_reserve(self._h, int(rows)), "mirx_index_reserve")

    def add(self, rows, ids=None):
        """Append rows: torch tensor (cpu or this GPU) or anything `torch.as_tensor` accepts."""
        rows = torch.as_tensor(rows)
        if rows.dim() != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"expected [n, {self.dim}] rows, got {tuple(rows.shape)}")
        rows = rows.detach().to(torch.float32).contiguous()
        if rows.is_cuda and rows.device != self.device:
            rows = rows.to(self.device)
        idp = None
        if ids is not None:
            ids = torch.as_tensor(ids).detach().to(torch.int64).contiguous()
            if ids.numel() != rows.shape[0]:
                raise ValueError("ids and rows disagree in length")
            if ids.is_cuda and ids.device != self.device:
                ids = ids.to(self.device)
            idp = ctypes.c_void_p(ids.data_ptr())
        if rows.is_cuda:
            torch.cuda.current_stream(self.device).synchronize()
        self._ids = self._id_table = None
        _lib.check(self._lib.mirx_index_add(self._h, ctypes.c_void_p(rows.data_ptr()), rows.shape[0], idp),
                   "mirx_index_add")

    def remove(self, ids):
        """Remove every row whose id occurs in `ids` (tensor on the cpu or this GPU, or anything `torch.as_tensor` accepts);
        ids that are absent are ignored, duplicates count once.  The survivors keep their order: searches afterwards equal
        those of a fresh index built from them.  -> the number of rows removed."""
        ids = torch.as_tensor(ids).detach().to(torch.int64).reshape(-1).contiguous()
        if ids.is_cuda and ids.device != self.device:
            ids = ids.to(self.device)
        removed = ctypes.c_int64(0)
        self._ids = self._id_table = None
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mirx_index_remove_ids(self._h, ctypes.c_void_p(ids.data_ptr()) if ids.numel() else None,
                                                       ids.numel(), ctypes.byref(removed), _stream_ptr(self.device)),
                       "mirx_index_remove_ids")
        return int(removed.value)

    def _prep_queries(self, q, exclude_ids):
        q = torch.as_tensor(q)
        if q.dim() == 1:
            q = q[None]
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] queries, got {tuple(q.shape)}")
        q = q.detach().to(device=self.device, dtype=torch.float32).contiguous()
        ex = None
        if exclude_ids is not None:
            ex = torch.as_tensor(exclude_ids).detach().to(device=self.device, dtype=torch.int64).contiguous()
            if ex.numel() != q.shape[0]:
                raise ValueError("exclude_ids needs one id per query")
        return q, ex

    def _prep_allow(self, allow):
        """a row mask as contiguous bytes (bool / uint8 tensor or array, on the cpu or this GPU; non-zero = eligible)"""
        if isinstance(allow, np.ndarray) and not allow.flags.writeable:
            allow = allow.copy()                                   # (torch warns about tensors over read-only arrays)
        a = torch.as_tensor(allow).detach()
        if a.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"allow must be a bool or uint8 mask, got {a.dtype}")
        a = a.reshape(-1).contiguous()
        if a.dtype == torch.bool:
            a = a.view(torch.uint8)
        if a.is_cuda and a.device != self.device:
            a = a.to(self.device)
        return a

    def _topk_call(self, q, k, exclude_ids, allow, return_f64, mask_who=None):
        """What search / search_deep / search_leave_out / rank_top / range_search hand the library: the queries and exclude ids
        on the device, the row mask as bytes (None without one) and, unless k is None (range_search), the [nq, k] outputs with
        the arguments every top-k entry point shares -- `head` = queries, nq, k, exclude ids; `outs` = the fp32 values or the
        fp64 ranking scores (the other one null), ids.  mask_who: the method's name where a mask of the wrong length is its ValueError,
        before any device work (an empty index's empty mask then counts as none); None leaves the length to the library."""
        c = types.SimpleNamespace()
        c.q, c.ex = self._prep_queries(q, exclude_ids)
        c.am = None if allow is None else self._prep_allow(allow)
        if mask_who is not None and c.am is not None:
            if c.am.numel() != len(self):
                raise ValueError(f"{mask_who}: allow needs one entry per row of the index ({len(self)}), got {c.am.numel()}")
            if c.am.numel() == 0:
                c.am = None
        c.nq = c.q.shape[0]
        if k is not None:
            c.head = (_ptr(c.q), c.nq, int(k), _ptr(c.ex))
            c.ids = torch.empty((c.nq, max(k, 0)), dtype=torch.int64, device=self.device)
            c.sc = torch.empty((c.nq, max(k, 0)), dtype=torch.float64 if return_f64 else torch.float32, device=self.device)
            c.outs = _score_ptrs(c.sc, return_f64) + (_ptr(c.ids),)
        return c

    def _call(self, name, *args):
        """the library's index entry point `name` on this index, its device current, the current stream as the last argument"""
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._lib, name)(self._h, *args, _stream_ptr(self.device)), name)

    def _per_row(self, t, dtype, who, name):
        """`t` checked as a tensor of `dtype` on the index's device with one entry per row (in the order of ids()), contiguous"""
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError(f"{who}: {name} must be an {str(dtype).split('.')[-1]} tensor")
        if t.device != self.device:
            raise ValueError(f"{who}: {name} must be on the index's device ({self.device}), got {t.device}")
        if t.dim() != 1 or t.numel() != len(self):
            raise ValueError(f"{who}: {name} needs one entry per row of the index ({len(self)}), got shape {tuple(t.shape)}")
        return t.detach().contiguous()

    def _per_query(self, v, nq, dtype, who, name):
        """`v` (tensor or sequence of nq integers) as a contiguous `dtype` tensor on the index's device"""
        t = torch.as_tensor(v).detach().reshape(-1)
        if t.numel() != nq:
            raise ValueError(f"{who}: {name} needs one entry per query ({nq}), got {t.numel()}")
        if t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError(f"{who}: {name} must be integers, got {t.dtype}")
        return t.to(device=self.device, dtype=dtype).contiguous()

    def search(self, q, k, exclude_ids=None, return_f64=False, allow=None):
        """-> (scores [nq,k] float32 reported values, ids [nq,k] int64) on the index device.

        With return_f64=True the first tensor holds the fp64 ranking scores instead
        (dot product, or NEGATIVE SQUARED distance for the L2 metric).  k above 1024 goes to rank_top.
        allow: a bool / uint8 mask with one entry per row of the index, in row order (cpu or this GPU): only rows whose entry
        is non-zero can be returned, and the answer is that of a fresh index holding just those rows (ids and scores to the
        bit); slots past the eligible rows read (-inf, -1).  The mask belongs to this call alone."""
        if int(k) > _lib.MAX_SEARCH_K:
            return self.rank_top(q, k, exclude_ids=exclude_ids, return_f64=return_f64, allow=allow)
        c = self._topk_call(q, k, exclude_ids, allow, return_f64)
        if c.am is not None:
            self._call("mirx_index_search_masked", *c.head, _ptr_or_null(c.am), c.am.numel(), *c.outs)
        elif return_f64:
            self._call("mirx_index_search_f64", *c.head, *c.outs[1:])
        else:
            self._call("mirx_index_search", *c.head, c.outs[0], c.outs[2])
        return c.sc, c.ids

    def search_deep(self, q, k, exclude_ids=None, return_f64=False, allow=None):
        """search()'s arguments and results, for 64 < k (+1 with exclude_ids) <= 1024 on galleries of at least
        deep_min_rows(k_eff, nq) rows: the filter GEMM with candidate lists of 4096 rows per query (mirx_index_search_deep)
        instead of search()'s scan of every row.  The answer is search()'s to the bit; every other call is handed to search()'s
        own route inside the library, and k above 1024 goes to rank_top as in search().  last_stats() tells which route answered."""
        if int(k) > _lib.MAX_SEARCH_K:
            return self.rank_top(q, k, exclude_ids=exclude_ids, return_f64=return_f64, allow=allow)
        c = self._topk_call(q, k, exclude_ids, allow, return_f64, mask_who="search_deep")
        self._call("mirx_index_search_deep", *c.head, _ptr(c.am), *c.outs)
        return c.sc, c.ids

    def search_leave_out(self, q, k, row_codes, query_codes, exclude_ids=None, allow=None, return_f64=False, max_left_out=-1):
        """Leave-group-out search (mirx_index_search_leave_out): search_deep()'s results over the rows that do not share the
        query's code -- row r is skipped for query i when query_codes[i] >= 0 and row_codes[r] == query_codes[i].  Negative
        codes are nulls: such a query leaves nothing out, such a row is never left out.
        row_codes: an int32 tensor on the index's device with one code per row, in the order of ids() (any other dtype, device
        or length: ValueError).  query_codes: a tensor or sequence of nq ints.  exclude_ids / allow combine with it as in
        search().  max_left_out: an upper bound on the rows one query leaves out, or -1 when unknown; it only picks the route
        (speed), never the answer.  1 <= k <= 1024.  last_stats()["left_out"] counts the candidates the predicate dropped."""
        k = int(k)
        if not 1 <= k <= _lib.MAX_SEARCH_K:
            raise ValueError(f"search_leave_out: k must be in [1, {_lib.MAX_SEARCH_K}], got {k}")
        rc_t = self._per_row(row_codes, torch.int32, "search_leave_out", "row_codes")
        c = self._topk_call(q, k, exclude_ids, allow, return_f64, mask_who="search_leave_out")
        qc = self._per_query(query_codes, c.nq, torch.int32, "search_leave_out", "query_codes")
        if c.nq == 0:
            return c.sc, c.ids
        if len(self) == 0:
            rc_t = torch.full((1,), -1, dtype=torch.int32, device=self.device)   # no code to read (the ABI refuses a null)
        self._call("mirx_index_search_leave_out", *c.head, _ptr(c.am), _ptr(rc_t), _ptr(qc), int(max_left_out), *c.outs)
        return c.sc, c.ids

    def search_begin(self, q, k, exclude_ids=None):
        """First half of search(): enqueue the whole first pass on the current stream and return without waiting.
        -> a handle for search_end(); the index must not be used for anything else in between."""
        q, ex = self._prep_queries(q, exclude_ids)
        nq = q.shape[0]
        ids = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        sc = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        s64 = torch.empty((nq, k), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mirx_index_search_begin(self._h, ctypes.c_void_p(q.data_ptr()), nq, int(k),
                                                         ctypes.c_void_p(ex.data_ptr()) if ex is not None else None,
                                                         ctypes.c_void_p(sc.data_ptr()), ctypes.c_void_p(s64.data_ptr()),
                                                         ctypes.c_void_p(ids.data_ptr()), _stream_ptr(self.device)),
                       "mirx_index_search_begin")
        return (q, ex, sc, s64, ids)                         # keeps the buffers alive until search_end

    def search_end(self, handle, return_f64=False):
        """Second half: wait for the first pass's counters (host wait on an event), run the rare follow-up passes.
        -> (scores, ids) like search()."""
        _lib.check(self._lib.mirx_index_search_end(self._h), "mirx_index_search_end")
        _, _, sc, s64, ids = handle
        return (s64 if return_f64 else sc), ids

    def rank_top(self, q, k, exclude_ids=None, return_f64=False, allow=None):
        """The first k entries, 1 <= k <= ntotal, of the full ranking, with search()'s outputs and conventions: -> (scores [nq,k],
        ids [nq,k]); the excluded id is left out and slots past the eligible rows read (-inf, -1).  Sorts the whole gallery per
        query (a radix sort, 32 bytes of workspace per row and query): for k <= 1024 search() is the faster call.  allow: search()'s
        row mask; the cost stays that of the unmasked call (every row is scored and sorted, masked rows end behind the rest)."""
        c = self._topk_call(q, int(k), exclude_ids, allow, return_f64)
        if c.am is None:
            self._call("mirx_index_rank_top", *c.head, *c.outs)
        else:
            self._call("mirx_index_rank_top_masked", *c.head, _ptr_or_null(c.am), c.am.numel(), *c.outs)
        return c.sc, c.ids

    def rank_all(self, q, exclude_ids=None, with_scores=False):
        """Full ranking [nq, ntotal] (row = query, excluded id last): score descending, equal scores by ascending id.  Any
        gallery size the [nq, ntotal] outputs and the sort's workspace fit (a radix sort above 65536 rows)."""
        q, ex = self._prep_queries(q, exclude_ids)
        nq, n = q.shape[0], len(self)
        ids = torch.empty((nq, n), dtype=torch.int64, device=self.device)
        sc = torch.empty((nq, n), dtype=torch.float32, device=self.device) if with_scores else None
        with torch.cuda.device(self.device):
            rc = self._lib.mirx_index_rank_all(
                self._h, ctypes.c_void_p(q.data_ptr()), nq,
                ctypes.c_void_p(ex.data_ptr()) if ex is not None else None,
                ctypes.c_void_p(ids.data_ptr()),
                ctypes.c_void_p(sc.data_ptr()) if sc is not None else None, _stream_ptr(self.device))
        _lib.check(rc, "mirx_index_rank_all")
        return (ids, sc) if with_scores else ids

    def rank_metrics(self, q, row_labels, query_labels, kappas=(), exclude_ids=None, self_kind=0, row_codes=None,
                     query_codes=None, jaccard_threshold=None, standard_ap=False):
        """The metric tail of the FULL ranking of every query without the ranking (mirx_index_rank_metrics): what
        metrics.rank_metrics_device returns for rank_all(q, exclude_ids) -- the same dict: ap [nq] f64 (NaN = no relevant
        row), cnt [nq, len(kappas)], nrel, maxpos int64, on the index's device -- evaluated batch by batch out of the sort's
        workspace, so no [nq, ntotal] tensor exists and the gallery size is bounded by the sort alone.
        row_labels: int64 tensor on the index's device, one label (class id, or multi-hot bit mask with jaccard_threshold)
        per row in the order of ids(); query_labels: nq ints.  self_kind says what the excluded id is: 0 an ordinary last
        entry (compute_map's quirk), 1 never relevant (compute_map_multilabel), 2 also taken out of the list
        (fusion_eval/metrics.py); 1 and 2 need exclude_ids.  row_codes (int32 tensor on the device, one per row) with
        query_codes (nq ints): query i's list loses every row r with query_codes[i] >= 0 and row_codes[r] ==
        query_codes[i] before anything is counted -- leave-group-out; negative codes are nulls.  Wrong dtypes, devices or
        lengths: ValueError before any device work."""
        who = "rank_metrics"
        if self_kind not in (0, 1, 2):
            raise ValueError(f"{who}: self_kind must be 0, 1 or 2, got {self_kind!r}")
        if self_kind != 0 and exclude_ids is None:
            raise ValueError(f"{who}: self_kind {self_kind} needs exclude_ids")
        if (row_codes is None) != (query_codes is None):
            raise ValueError(f"{who}: row_codes and query_codes come together")
        ks = [int(k) for k in kappas]
        if len(ks) > 8 or any(k < 1 for k in ks):
            raise ValueError(f"{who}: at most 8 kappas, each at least 1, got {ks}")
        size = len(self)
        rl = self._per_row(row_labels, torch.int64, who, "row_labels")
        rc_t = None if row_codes is None else self._per_row(row_codes, torch.int32, who, "row_codes")
        q, ex = self._prep_queries(q, exclude_ids)
        nq = q.shape[0]
        ql = self._per_query(query_labels, nq, torch.int64, who, "query_labels")
        qc = None if query_codes is None else self._per_query(query_codes, nq, torch.int32, who, "query_codes")
        ap = torch.empty(nq, dtype=torch.float64, device=self.device)
        cnt = torch.empty((nq, len(ks)), dtype=torch.int64, device=self.device)
        nrel = torch.empty(nq, dtype=torch.int64, device=self.device)
        maxpos = torch.empty(nq, dtype=torch.int64, device=self.device)
        out = {"ap": ap, "cnt": cnt, "nrel": nrel, "maxpos": maxpos}
        if nq == 0:
            return out
        if size == 0 and rc_t is not None:
            rc_t = torch.full((1,), -1, dtype=torch.int32, device=self.device)   # no code to read, and codes come in pairs
        karr = (ctypes.c_int32 * max(1, len(ks)))(*ks)
        vp = _ptr_or_null
        self._call("mirx_index_rank_metrics", vp(q), nq, vp(ex), int(self_kind), vp(rl), vp(ql), vp(rc_t), vp(qc),
                   0 if jaccard_threshold is None else 1, float(jaccard_threshold or 0.0), 1 if standard_ap else 0, karr, len(ks),
                   vp(ap), vp(cnt), vp(nrel), vp(maxpos))
        return out

    def range_search(self, q, lo, hi=float("inf"), exclude_ids=None, allow=None, return_f64=False):
        """Every row whose fp64 ranking score s (dot product; NEGATIVE SQUARED distance for L2) has lo < s <= hi -- not the
        best k.  -> (lims int64 [nq + 1], scores [total], ids int64 [total]) on the index device: the hits of query i are
        ids[lims[i]:lims[i + 1]], best first (score descending, equal scores by ascending id: rank_all's order).  scores holds
        the fp32 reported values, or the fp64 ranking scores with return_f64=True.  exclude_ids / allow as in search(): a row is
        a hit only when its mask entry is non-zero and its id is not the query's excluded id.  lo = -inf returns every eligible
        row, hi <= lo nothing; a NaN bound raises ValueError.  range_bounds() maps pymilvus' radius / range_filter onto lo, hi.
        The answer does not depend on the route (filter GEMM + fp64 re-score of every candidate, or the exact scan)."""
        lo, hi = _bound(lo, "lo"), _bound(hi, "hi")
        c = self._topk_call(q, None, exclude_ids, allow, return_f64, mask_who="range_search")
        lims = torch.empty((c.nq + 1,), dtype=torch.int64, device=self.device)
        total = ctypes.c_int64(0)
        self._call("mirx_index_range_search", _ptr(c.q), c.nq, lo, hi, _ptr(c.ex), _ptr(c.am), 0 if c.am is None else c.am.numel(),
                   _ptr(lims), ctypes.byref(total))
        n = int(total.value)
        sc = torch.empty((n,), dtype=torch.float64 if return_f64 else torch.float32, device=self.device)
        ids = torch.empty((n,), dtype=torch.int64, device=self.device)
        self._call("mirx_index_range_fetch", *_score_ptrs(sc, return_f64), _ptr_or_null(ids))
        return lims, sc, ids

    # -- grouping search -------------------------------------------------------------------------------------
    def ids(self):
        """The ids of the index's rows, in row order: int64 on the index device, no row is copied.  Kept until add() / remove()."""
        n = len(self)
        if self._ids is None or self._ids.shape[0] != n:
            out = torch.empty((n,), dtype=torch.int64, device=self.device)
            if n:
                with torch.cuda.device(self.device):
                    torch.cuda.current_stream(self.device).synchronize()
                    _lib.check(self._lib.mirx_index_get_ids(self._h, 0, n, ctypes.c_void_p(out.data_ptr())), "mirx_index_get_ids")
            self._ids, self._id_table = out, None
        return self._ids

    def _group_id_table(self):
        """(identity, sorted ids, their rows): how a ranked id becomes a row position.  identity = the ids are 0 .. n-1, the id
        is the position.  A repeated id cannot be grouped (its rows would be told apart by nothing): ValueError."""
        ids = self.ids()
        if self._id_table is None:
            n = ids.shape[0]
            if bool((ids == torch.arange(n, dtype=torch.int64, device=self.device)).all()):
                self._id_table = (True, None, None)
            else:
                sorted_ids, order = torch.sort(ids)
                if n > 1 and bool((sorted_ids[1:] == sorted_ids[:-1]).any()):
                    raise ValueError("search_grouped: an id repeats in the index; grouping needs one row per id")
                self._id_table = (False, sorted_ids, order)
        return self._id_table

    def _positions(self, ids):
        """row position of each id of an int64 tensor on the device, -1 for ids the index does not hold (the -1 padding too)"""
        identity, sorted_ids, order = self._group_id_table()
        n = len(self)
        if identity:
            return torch.where((ids >= 0) & (ids < n), ids, torch.full_like(ids, -1))
        p = torch.searchsorted(sorted_ids, ids.contiguous()).clamp_(max=n - 1)
        return torch.where(sorted_ids[p] == ids, order[p], torch.full_like(ids, -1))

    def _group_walk(self, rid, s64, g, rows, live, eg, limit, group_size):
        """mirx_group_walk over the ranked prefixes rid / s64 [m, depth] -> (ids, fp64 scores, codes, kept, state)"""
        m, depth = rid.shape
        rid, s64 = rid.contiguous(), s64.contiguous()
        tix = None if self._group_id_table()[0] else self._positions(rid).contiguous()
        ids = torch.empty((m, limit, group_size), dtype=torch.int64, device=self.device)
        sc = torch.empty((m, limit, group_size), dtype=torch.float64, device=self.device)
        codes = torch.empty((m, limit), dtype=torch.int64, device=self.device)
        kept = torch.empty((m, limit), dtype=torch.int32, device=self.device)
        state = torch.empty((m, 2), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mirx_group_walk(_ptr(rid), _ptr(tix), _ptr(s64), m, depth, depth, _ptr(g), g.shape[0], _ptr(rows),
                                                 rows.shape[0], live, _ptr(eg), limit, group_size, _ptr(ids), _ptr(sc), _ptr(codes),
                                                 _ptr(kept), _ptr(state), _stream_ptr(self.device)), "mirx_group_walk")
        return ids, sc, codes, kept, state

    def _group_count(self, g, am, n_groups):
        """mirx_group_count: eligible rows per code, int64 [n_groups]"""
        rows = torch.empty((n_groups,), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mirx_group_count(_ptr(g), _ptr(am), g.shape[0], n_groups, _ptr(rows), _stream_ptr(self.device)),
                       "mirx_group_count")
        return rows

    def _group_fill(self, q, ex, limit, group_size, pq, ps, pf, pl, members, ids, s64):
        """mirx_index_group_fill: the pairs' groups, best group_size members each, into ids / s64 [nq, limit, group_size]"""
        pq, ps, pf, pl = (t.contiguous() for t in (pq, ps, pf, pl))
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mirx_index_group_fill(
                self._h, _ptr(q), q.shape[0], _ptr(ex), limit, group_size, _ptr(pq), _ptr(ps), _ptr(pf), _ptr(pl), pq.shape[0],
                _ptr(members), members.shape[0], int(pl.max()), _ptr(ids), _ptr(s64), _stream_ptr(self.device)),
                "mirx_index_group_fill")

    def search_grouped(self, q, groups, limit, group_size=1, exclude_ids=None, allow=None, return_f64=False, route="auto"):
        """Grouping search: the best hits per GROUP instead of the best rows (pymilvus' group_by_field / group_size with
        strict_group_size=True).  groups: one integer code >= 0 per row of the index, in row order, like `allow`.  Per query,
        over rank_all's order (fp64 score descending, equal scores by ascending id) restricted to the eligible rows (mask entry
        non-zero, id not the query's excluded id): the min(limit, groups with an eligible row) groups whose best row ranks
        highest, ordered by that row, each with its first min(group_size, its eligible rows) rows in ranking order.
        -> (ids [nq, limit, group_size] int64, -1 in empty slots; scores alike: fp32 reported values, or the fp64 ranking scores
        with return_f64=True, -inf in empty slots; group_codes [nq, limit] int64, -1 in empty slots) on the index device.  The
        scores are the bits search() returns for the same (query, row).
        1 <= limit <= 1024, 1 <= group_size <= 64, limit * group_size <= 16384.  ValueError: negative or non-integer codes,
        len(groups) != len(index), an id that repeats in the index.
        route: "auto", or one of "direct" / "walk" / "deepen" to force it -- the answer never depends on the route:
          direct  at most GROUP_DIRECT_MAX groups have eligible rows: one masked search(k=group_size) per group, the groups
                  ordered by their best row (two stable sorts);
          walk    a ranked prefix from search() (63 / 64 deep: the filter-GEMM tier; min(1024, 4 * limit) when limit is too large
                  for that: the exact tier), walked by mirx_group_walk; queries whose groups are decided but short have those
                  groups completed by mirx_index_group_fill (groups of up to GROUP_FILL_MAX rows), the others go to
          deepen  rank_top() prefixes of 8x the previous depth, walked again, the last the whole ranking: slow and exact.
        group_last_stats() says which route answered how many queries."""
        if route not in _GROUP_ROUTES:
            raise ValueError(f"route must be one of {', '.join(_GROUP_ROUTES)}, got {route!r}")
        limit, group_size = group_bounds(limit, group_size)
        n = len(self)
        g = groups if torch.is_tensor(groups) else torch.as_tensor(np.asarray(groups))
        if g.dtype in (torch.bool,) or g.is_floating_point() or g.is_complex():
            raise ValueError(f"groups must be integer codes, got {g.dtype}")
        g = g.detach().reshape(-1)
        if g.shape[0] != n:
            raise ValueError(f"groups needs one code per row of the index ({n}), got {g.shape[0]}")
        g = g.to(device=self.device, dtype=torch.int64).contiguous()
        q, ex = self._prep_queries(q, exclude_ids)
        am = None if allow is None else self._prep_allow(allow).to(self.device)
        if am is not None and am.numel() != n:
            raise ValueError(f"allow needs one entry per row of the index ({n}), got {am.numel()}")
        nq = q.shape[0]
        ids = torch.full((nq, limit, group_size), -1, dtype=torch.int64, device=self.device)
        s64 = torch.full((nq, limit, group_size), float("-inf"), dtype=torch.float64, device=self.device)
        codes = torch.full((nq, limit), -1, dtype=torch.int64, device=self.device)
        stats = {"nq": nq, "route": route, "direct": 0, "walk": 0, "fill": 0, "deepen": 0, "passes": 0, "max_depth": 0,
                 "groups": 0}
        self._group_stats = stats
        uniq = None
        if n:
            if int(g.min()) < 0:
                raise ValueError("groups holds a negative code")
            self._group_id_table()                               # (a repeated id raises before anything is searched)
            if int(g.max()) >= 2 * n + 1024:                     # sparse codes: the count table is indexed by code
                uniq, g = torch.unique(g, return_inverse=True)
                g = g.contiguous()
        if n and nq:
            n_groups = int(g.max()) + 1
            rows = self._group_count(g, am, n_groups)
            live = int((rows > 0).sum())
            stats["groups"] = live
            if live:
                eg = None
                if ex is not None:                               # the group each query's excluded row takes a row from
                    pos = self._positions(ex)
                    ok = pos >= 0
                    if am is not None:
                        ok &= am[pos.clamp(min=0)] != 0
                    eg = torch.where(ok, g[pos.clamp(min=0)], torch.full_like(pos, -1)).contiguous()
                if route == "direct" or (route == "auto" and live <= GROUP_DIRECT_MAX):
                    self._grouped_direct(q, ex, am, g, rows, limit, group_size, ids, s64, codes, stats)
                else:
                    self._grouped_walk(q, ex, am, g, rows, live, eg, limit, group_size, ids, s64, codes, stats,
                                       deepen_only=route == "deepen")
        if uniq is not None:
            codes = torch.where(codes >= 0, uniq[codes.clamp(min=0)], codes)
        if return_f64:
            return ids, s64, codes
        val = s64 if self.metric == METRIC_IP else -torch.sqrt(torch.clamp(-s64, min=0.0))
        return ids, val.to(torch.float32), codes

    def _grouped_direct(self, q, ex, am, g, rows, limit, group_size, ids, s64, codes, stats):
        """one masked search per group with eligible rows, then the groups of each query in the order of their best rows"""
        live_codes = torch.nonzero(rows > 0).flatten()
        allowed = None if am is None else am != 0
        ss, ii = [], []
        for c in live_codes.tolist():
            mask = g == c
            if allowed is not None:
                mask &= allowed
            s, i = self.search(q, group_size, exclude_ids=ex, return_f64=True, allow=mask)
            ss.append(s)
            ii.append(i)
        s_all, i_all = torch.stack(ss, 1), torch.stack(ii, 1)          # [nq, groups, group_size]
        # (best score descending, best id ascending): a stable sort by id, then a stable sort by score.  A group without an
        # eligible row for the query (its only one was the excluded id) reads (-inf, -1), lands last and is dropped.
        o1 = torch.sort(i_all[:, :, 0], dim=1, stable=True).indices
        o2 = torch.sort(s_all[:, :, 0].gather(1, o1), dim=1, descending=True, stable=True).indices
        order = o1.gather(1, o2)[:, :limit]
        t = order.shape[1]
        pick = order[:, :, None].expand(-1, -1, group_size)
        ids[:, :t] = i_all.gather(1, pick)
        s64[:, :t] = s_all.gather(1, pick)
        codes[:, :t] = torch.where(ids[:, :t, 0] >= 0, live_codes[order], torch.full_like(order, -1))
        stats["direct"] = q.shape[0]
        stats["passes"] = int(live_codes.shape[0])
        stats["max_depth"] = group_size

    def _grouped_walk(self, q, ex, am, g, rows, live, eg, limit, group_size, ids, s64, codes, stats, deepen_only):
        n, nq = len(self), q.shape[0]
        depth = GROUP_FIRST_DEPTH
        todo = torch.arange(nq, device=self.device)
        if not deepen_only:
            depth = GROUP_FIRST_DEPTH - (1 if ex is not None else 0)      # k (+1 with exclude ids) <= 64: the filter-GEMM tier
            if limit > depth // 4:
                depth = min(1024, 4 * limit)                              # the exact tier
            depth = min(depth, n)
            sc, rid = self.search(q, depth, exclude_ids=ex, return_f64=True, allow=am)
            w_ids, w_sc, w_codes, w_kept, state = self._group_walk(rid, sc, g, rows, live, eg, limit, group_size)
            ids.copy_(w_ids), s64.copy_(w_sc), codes.copy_(w_codes)
            stats["passes"] += 1
            stats["max_depth"] = depth
            complete, final = (state[:, 1] & 1) != 0, (state[:, 1] & 2) != 0
            stats["walk"] = int(complete.sum())
            deep = ~final
            fill_q = torch.nonzero(final & ~complete).flatten()
            if fill_q.numel():
                # the groups of these queries are decided; the ones that are short get their rows from the group's member list
                c = codes[fill_q]
                cnt = rows[c.clamp(min=0)]
                short = (c >= 0) & (w_kept[fill_q] < (cnt - (0 if eg is None else (c == eg[fill_q][:, None]).to(cnt.dtype)))
                                    .clamp(max=group_size))
                too_big = (short & (cnt > GROUP_FILL_MAX)).any(1)         # such a group is cheaper to reach by deepening
                deep[fill_q[too_big]] = True
                short &= ~too_big[:, None]
                a, slot = torch.nonzero(short, as_tuple=True)
                if a.numel():
                    elig = torch.arange(n, device=self.device) if am is None else torch.nonzero(am).flatten()
                    members = elig[torch.argsort(g[elig], stable=True)].contiguous()      # eligible rows, group after group
                    first = torch.cumsum(rows, 0) - rows
                    pc = c[a, slot]
                    self._group_fill(q, ex, limit, group_size, fill_q[a], slot, first[pc], rows[pc], members, ids, s64)
                stats["fill"] = int(fill_q.numel() - too_big.sum())
            todo = torch.nonzero(deep).flatten()
        stats["deepen"] = int(todo.numel())
        whole = False                                                     # the last prefix was the whole ranking
        while todo.numel():
            if whole:
                raise MirxError("search_grouped: the whole ranking left a query incomplete (the group counts and the ranking disagree)")
            depth = min(n, depth * GROUP_DEEPEN_FACTOR)
            whole = depth == n
            per = max(1, GROUP_DEEPEN_BYTES // (16 * depth))
            rest = []
            for b in range(0, todo.numel(), per):
                sub = todo[b:b + per]
                sc, rid = self.rank_top(q[sub], depth, exclude_ids=None if ex is None else ex[sub], return_f64=True, allow=am)
                w_ids, w_sc, w_codes, _, state = self._group_walk(rid, sc, g, rows, live, None if eg is None else eg[sub].contiguous(),
                                                                  limit, group_size)
                done = (state[:, 1] & 1) != 0
                ids[sub[done]], s64[sub[done]], codes[sub[done]] = w_ids[done], w_sc[done], w_codes[done]
                rest.append(sub[~done])
                stats["passes"] += 1
            stats["max_depth"] = depth
            todo = torch.cat(rest)

    def group_last_stats(self):
        """What the last search_grouped did: nq; route = the `route` argument; direct / walk / fill / deepen = the queries each
        route answered (walk: complete after the first prefix; fill: completed by mirx_index_group_fill; deepen: needed deeper
        prefixes); passes = search / rank_top calls made; max_depth = the deepest prefix; groups = codes with an eligible row."""
        return dict(self._group_stats)

    def range_last_stats(self):
        s = _lib.RangeStats()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mirx_index_range_last_stats(self._h, ctypes.byref(s)), "mirx_index_range_last_stats")
        return s.as_dict()

    def last_stats(self):
        s = _lib.SearchStats()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mirx_index_last_stats(self._h, _stream_ptr(self.device), ctypes.byref(s)),
                       "mirx_index_last_stats")
        return s.as_dict()

    def last_timings(self):
        """Stage -> milliseconds of the last search (needs set_option(OPT_PROFILE, 1))."""
        arr = (ctypes.c_float * len(_lib.STAGES))()
        _lib.check(self._lib.mirx_index_last_timings(self._h, arr), "mirx_index_last_timings")
        return dict(zip(_lib.STAGES, [float(v) for v in arr]))

    def rows(self, first=0, n=None):
        n = len(self) - first if n is None else n
        out = torch.empty((n, self.dim), dtype=torch.float32, device=self.device)
        ids = torch.empty((n,), dtype=torch.int64, device=self.device)
        _lib.check(self._lib.mirx_index_get_rows(self._h, first, n, ctypes.c_void_p(out.data_ptr()),
                                                 ctypes.c_void_p(ids.data_ptr())), "mirx_index_get_rows")
        return out, ids


IVF_TRAIN_ROWS_PER_LIST = 256              # IvfFlatIndex.train(max_rows=None) trains on at most this many rows per list


def strided_sample(rows, limit):
    """The training sample of the IVF family: all of rows [n, .] when n <= limit, else the `limit` rows floor(i n / limit), as a
    contiguous copy that is complete when this returns."""
    n = rows.shape[0]
    if n <= limit:
        return rows
    pick = (torch.arange(limit, dtype=torch.int64) * n) // limit
    rows = rows[pick.to(rows.device)].contiguous()
    if rows.is_cuda:
        torch.cuda.current_stream(rows.device).synchronize()
    return rows


def ivf_search_bounds(k, nprobe):
    """k / nprobe of an IVF search as ints, ValueError outside mirx_ivf_search's contract"""
    for name, v in (("k", k), ("nprobe", nprobe)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {type(v).__name__}")
    k, nprobe = int(k), int(nprobe)
    if not 1 <= k <= _lib.MAX_SEARCH_K:
        raise ValueError(f"IVF search: k must be in [1, {_lib.MAX_SEARCH_K}], got {k}")
    if nprobe < 1:
        raise ValueError(f"IVF search: nprobe must be at least 1, got {nprobe}")
    return k, nprobe


class IvfFlatIndex:
    """IVF_FLAT over fp32 rows resident on one GPU (mirx_ivf_*, include/mirx.h): the reference's own index type
    (milvus/milvus_setup.py:191-213) and search parameters (nprobe, milvus/milvus_retrieval.py:69-86).

    The rows live in `nlist` lists, each row in the list of its nearest centroid; search() scans the lists of the query's
    `nprobe` nearest centroids and returns THE EXACT TOP-K OF THOSE ROWS: fp64 lane-tree scores, ties to the lowest id, bit for
    bit what FlatIndex.search(allow=rows whose list is probed) returns.  Only the choice of lists is approximate; nprobe >= nlist
    is FlatIndex.search's answer.  "Nearest" is FlatIndex's own ranking over the centroids (ties to the lowest list)."""

    KIND = _lib.IVF_FLAT
    STATE_KEYS = ("centroids",)                # the trained parts, as state() names them; the subclasses append theirs

    def __init__(self, dim, metric="COSINE", nlist=1024, device=None):
        if isinstance(nlist, bool) or not isinstance(nlist, (int, np.integer)) or not 1 <= int(nlist) <= _lib.IVF_MAX_NLIST:
            raise ValueError(f"nlist must be an integer in [1, {_lib.IVF_MAX_NLIST}], got {nlist!r}")
        if not 1 <= int(dim) <= _lib.IVF_MAX_DIM:
            raise ValueError(f"{type(self).__name__}: dim must be in [1, {_lib.IVF_MAX_DIM}], got {dim}")
        self.metric = metric_code(metric)
        if not torch.cuda.is_available():
            raise MirxError(f"{type(self).__name__} needs a GPU: libmirx has no CPU path")
        self._lib = _lib.load()
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        self.dim, self.nlist = int(dim), int(nlist)
        h = ctypes.c_void_p()
        self._create(h)
        self._h = h

    def _create(self, h):
        _lib.check(self._lib.mirx_ivf_create_typed(self.dim, self.metric, self.nlist, self.KIND, self.device.index,
                                                   ctypes.byref(h)), "mirx_ivf_create_typed")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.mirx_ivf_destroy(h)
            self._h = None

    def __len__(self):
        return int(self._lib.mirx_ivf_size(self._h))

    def _rows(self, rows, who):
        rows = torch.as_tensor(rows)
        if rows.dim() != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"{who}: expected [n, {self.dim}] rows, got {tuple(rows.shape)}")
        rows = rows.detach().to(torch.float32).contiguous()
        if rows.is_cuda and rows.device != self.device:
            rows = rows.to(self.device)
        if rows.is_cuda:
            torch.cuda.current_stream(self.device).synchronize()
        return rows

    def _call(self, name, *args):
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._lib, name)(self._h, *args), name)

    @classmethod
    def min_train_rows(cls, nlist):
        """the fewest rows train() accepts for an index of nlist lists"""
        return nlist

    def state(self):
        """-> the trained parts as a dict of device tensors, keys STATE_KEYS: what set_state() of an index built with the same
        arguments takes"""
        return {"centroids": self.centroids}

    def set_state(self, state):
        """Fix the trained parts to another index's state().  A missing key: ValueError before anything is set."""
        for key in self.STATE_KEYS:
            if key not in state:
                raise ValueError(f"set_state: the state of {type(self).__name__} needs {key!r}")
        self.set_centroids(state["centroids"])

    def _train(self, rows, iters, init_positions, max_rows):
        """train(): the argument checks and mirx_ivf_train -> the rows it trained on (at most max_rows at an even stride)"""
        rows = self._rows(rows, "train")
        limit = IVF_TRAIN_ROWS_PER_LIST * self.nlist if max_rows is None else int(max_rows)
        if limit < self.nlist:
            raise ValueError(f"train: max_rows ({limit}) is below nlist ({self.nlist})")
        if rows.shape[0] < self.nlist:
            raise ValueError(f"train: {rows.shape[0]} rows cannot seed {self.nlist} lists")
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
            raise ValueError(f"train: iters must be a non-negative integer, got {iters!r}")
        rows = strided_sample(rows, limit)
        pos = None
        if init_positions is not None:
            pos = np.ascontiguousarray(np.asarray(init_positions).reshape(-1), dtype=np.int64)
            if pos.size != self.nlist or (pos < 0).any() or (pos >= rows.shape[0]).any():
                raise ValueError(f"train: init_positions needs {self.nlist} row numbers in [0, {rows.shape[0]})")
        self._call("mirx_ivf_train", _ptr(rows), rows.shape[0], None if pos is None else ctypes.c_void_p(pos.ctypes.data),
                   int(iters), _stream_ptr(self.device))
        return rows

    def train(self, rows, iters=10, init_positions=None, max_rows=None):
        """Lloyd's k-means (mirx_ivf_train) and fix the centroids: start from rows[init_positions] (default: the rows at
        floor(j n / nlist)), `iters` updates at most, stop early when no row changes its list.  It trains on at most max_rows
        rows taken at an even stride (row floor(i n / max_rows)); max_rows=None means 256 * nlist.  Deterministic: two calls
        give equal bits."""
        self._train(rows, iters, init_positions, max_rows)

    def set_centroids(self, centroids):
        """Fix the centroids to a caller's [nlist, dim] array; rows already added are re-assigned."""
        c = self._rows(centroids, "set_centroids")
        if c.shape[0] != self.nlist:
            raise ValueError(f"set_centroids: expected {self.nlist} centroids, got {c.shape[0]}")
        self._call("mirx_ivf_set_centroids", _ptr(c))

    @property
    def centroids(self):
        out = torch.empty((self.nlist, self.dim), dtype=torch.float32, device=self.device)
        self._call("mirx_ivf_get_centroids", _ptr(out))
        return out

    def add(self, rows, ids=None):
        """Append rows (cpu or this GPU) to their lists; ids as FlatIndex.add.  Every call rebuilds the list-major layout: the
        resident rows move once, so add in large batches."""
        rows = self._rows(rows, "add")
        idp = None
        if ids is not None:
            ids = torch.as_tensor(ids).detach().to(torch.int64).contiguous()
            if ids.numel() != rows.shape[0]:
                raise ValueError("ids and rows disagree in length")
            if ids.is_cuda:
                ids = ids.to(self.device)
                torch.cuda.current_stream(self.device).synchronize()
            idp = _ptr(ids)
        self._call("mirx_ivf_add", _ptr(rows), rows.shape[0], idp)

    def remove(self, ids):
        """FlatIndex.remove's contract -> the number of rows removed."""
        ids = torch.as_tensor(ids).detach().to(torch.int64).reshape(-1).contiguous()
        if ids.is_cuda:
            ids = ids.to(self.device)
            torch.cuda.current_stream(self.device).synchronize()
        removed = ctypes.c_int64(0)
        self._call("mirx_ivf_remove_ids", _ptr_or_null(ids), ids.numel(), ctypes.byref(removed), _stream_ptr(self.device))
        return int(removed.value)

    def assign(self, rows):
        """-> int64 [n] on the index device: the list each row would be added to"""
        rows = self._rows(rows, "assign").to(self.device)
        out = torch.empty((rows.shape[0],), dtype=torch.int64, device=self.device)
        self._call("mirx_ivf_assign", _ptr_or_null(rows), rows.shape[0], _ptr_or_null(out), _stream_ptr(self.device))
        return out

    def list_sizes(self):
        out = np.empty((self.nlist,), dtype=np.int64)
        _lib.check(self._lib.mirx_ivf_list_sizes(self._h, ctypes.c_void_p(out.ctypes.data)), "mirx_ivf_list_sizes")
        return out

    def set_option(self, option, value):
        _lib.check(self._lib.mirx_ivf_set_option(self._h, option, int(value)), "mirx_ivf_set_option")

    def search(self, q, k, nprobe=10, exclude_ids=None, return_f64=False, return_probes=False):
        """-> (scores [nq, k], ids [nq, k]) as FlatIndex.search (fp32 reported values, or the fp64 ranking scores with
        return_f64), over the rows of the `nprobe` lists nearest to each query (nprobe is clamped to nlist); with
        return_probes a third tensor [nq, min(nprobe, nlist)] int32 names those lists, nearest first.  1 <= k <= 1024."""
        k, nprobe = ivf_search_bounds(k, nprobe)
        q, ex = FlatIndex._prep_queries(self, q, exclude_ids)
        nq, npc = q.shape[0], min(nprobe, self.nlist)
        ids = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        sc = torch.empty((nq, k), dtype=torch.float64 if return_f64 else torch.float32, device=self.device)
        probes = torch.empty((nq, npc), dtype=torch.int32, device=self.device) if return_probes else None
        self._call("mirx_ivf_search", _ptr_or_null(q), nq, k, nprobe, _ptr(ex), *_score_ptrs(sc, return_f64), _ptr_or_null(ids),
                   _ptr_or_null(probes), _stream_ptr(self.device))
        return (sc, ids, probes) if return_probes else (sc, ids)

    def last_stats(self):
        """nq, rows_scored ((query, row) pairs scored), pairs ((query, list) pairs), work_items and batches of the last search"""
        s = _lib.IvfStats()
        self._call("mirx_ivf_last_stats", _stream_ptr(self.device), ctypes.byref(s))
        return s.as_dict()


class _CodedIvfIndex(IvfFlatIndex):
    """What IVF_SQ8 and IVF_PQ share: the rows are kept as uint8 codes of `code_width` bytes, and the originals are gone"""

    def codes(self):
        """-> (codes uint8 [n, code_width], ids int64 [n], lists int64 [n]) on the index device, in list-major order; a code row
        is dim bytes for IVF_SQ8 and m bytes for IVF_PQ"""
        n = len(self)
        codes = torch.empty((n, self.code_width), dtype=torch.uint8, device=self.device)
        ids = torch.empty((n,), dtype=torch.int64, device=self.device)
        lists = torch.empty((n,), dtype=torch.int64, device=self.device)
        self._call("mirx_ivf_get_codes", _ptr_or_null(codes), _ptr_or_null(ids), _ptr_or_null(lists))
        return codes, ids, lists

    def reconstruct(self):
        """-> (decoded rows fp32 [n, dim], ids int64 [n]) on the index device, in list-major order.  IVF_SQ8: the rows search()
        scores.  IVF_PQ: each row's codewords concatenated (with residual coding: plus the centroid of its list)"""
        n = len(self)
        rows = torch.empty((n, self.dim), dtype=torch.float32, device=self.device)
        ids = torch.empty((n,), dtype=torch.int64, device=self.device)
        self._call("mirx_ivf_reconstruct", _ptr_or_null(rows), _ptr_or_null(ids))
        return rows, ids


class IvfSq8Index(_CodedIvfIndex):
    """IVF_SQ8 (mirx_ivf_create_typed(MIRX_IVF_SQ8), include/mirx.h): IvfFlatIndex with the rows kept as 8-bit codes, a quarter
    of the fp32 master.  The quantiser is per column and global: code = round((x - vmin[d]) / scale[d]) clamped to 0 .. 255, the
    decoded value (float)(vmin[d] + code * scale[d]) in double arithmetic.  A row's list comes from its original values; then the
    row is encoded and the original is gone.  search() returns THE EXACT TOP-K OVER THE DECODED ROWS of the probed lists: bit for
    bit FlatIndex.search(allow=rows whose list is probed) on a FlatIndex over reconstruct()'s rows.  An index that holds rows
    keeps its centroids and its range (MirxError from train / set_centroids / train_range / set_range): remove the rows first."""

    KIND = _lib.IVF_SQ8
    STATE_KEYS = IvfFlatIndex.STATE_KEYS + ("vmin", "scale")
    code_width = property(lambda self: self.dim)

    def train(self, rows, iters=10, init_positions=None, max_rows=None):
        """IvfFlatIndex.train, and the range (train_range) from the same strided sample"""
        self.train_range(self._train(rows, iters, init_positions, max_rows))

    def state(self):
        vmin, scale = self.range
        return dict(super().state(), vmin=vmin, scale=scale)

    def set_state(self, state):
        super().set_state(state)
        self.set_range(state["vmin"], state["scale"])

    def train_range(self, rows):
        """Fix the range to the rows' per-column minimum and (maximum - minimum) / 255 (NaN ignored); every row is read."""
        rows = self._rows(rows, "train_range")
        if rows.shape[0] < 1:
            raise ValueError("train_range: no rows")
        self._call("mirx_ivf_sq8_train", _ptr(rows), rows.shape[0], _stream_ptr(self.device))

    def set_range(self, vmin, scale):
        """Fix the range to a caller's vmin [dim] and scale [dim]."""
        arrs = []
        for name, v in (("vmin", vmin), ("scale", scale)):
            v = torch.as_tensor(v).detach().to(torch.float32).reshape(-1).contiguous()
            if v.numel() != self.dim:
                raise ValueError(f"set_range: {name} needs {self.dim} values, got {v.numel()}")
            arrs.append(v.to(self.device) if v.is_cuda else v)
        torch.cuda.current_stream(self.device).synchronize()
        self._call("mirx_ivf_sq8_set_range", _ptr(arrs[0]), _ptr(arrs[1]))

    @property
    def range(self):
        """(vmin [dim], scale [dim]) fp32 on the index device"""
        vmin = torch.empty((self.dim,), dtype=torch.float32, device=self.device)
        scale = torch.empty((self.dim,), dtype=torch.float32, device=self.device)
        self._call("mirx_ivf_sq8_get_range", _ptr(vmin), _ptr(scale))
        return vmin, scale


PQ_TRAIN_ROWS = 65536                      # IvfPqIndex.train trains the codebooks on at most this many rows


def pq_bounds(dim, m):
    """m of an IVF_PQ index as an int, ValueError outside mirx_ivf_create_pq's contract (m % 4 == 0, 4 <= m <= 64,
    dim % (4 m) == 0)"""
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)):
        raise ValueError(f"m must be an integer, got {m!r}")
    m = int(m)
    if m % 4 or not 4 <= m <= _lib.PQ_MAX_M:
        raise ValueError(f"m must be a multiple of 4 in [4, {_lib.PQ_MAX_M}], got {m}")
    if int(dim) % (4 * m):
        raise ValueError(f"m = {m} needs a dim that is a multiple of 4 m = {4 * m}, got dim {dim}")
    return m


class IvfPqIndex(_CodedIvfIndex):
    """IVF_PQ (mirx_ivf_create_pq, include/mirx.h): IvfFlatIndex with every row kept as `m` codeword numbers (m bytes).  Sub-space
    j (columns [j dim/m, (j+1) dim/m)) has a codebook of 256 codewords, k-means under L2 whatever the index metric; a row's code
    is its nearest codeword per sub-space (FlatIndex's own ranking, ties to the lowest code).  A row's list comes from its
    original values; then the row is encoded and the original is gone.  search() returns THE EXACT TOP-K OF THE ADC SCORE over
    the rows of the probed lists: per query a float64 table T[j][c] (one sequential sum over the sub-space's columns), a row's
    score the sequential sum over j of T[j][code[j]] -- defined to the bit in include/mirx.h, restated in tests/_pq_ref.py.  It is
    not a search over reconstruct()'s rows (the sums associate differently).  An index that holds rows keeps its centroids and
    codebooks (MirxError from train / set_centroids / train_codebooks / set_codebooks): remove the rows first."""

    KIND = _lib.IVF_PQ
    STATE_KEYS = IvfFlatIndex.STATE_KEYS + ("codebooks",)
    code_width = property(lambda self: self.m)
    by_residual = False                        # IvfResidualPqIndex turns it on

    def __init__(self, dim, metric="COSINE", nlist=1024, m=None, device=None):
        if m is None:
            raise ValueError("IvfPqIndex needs m, the number of sub-quantisers")
        self.m = pq_bounds(dim, m)
        super().__init__(dim, metric, nlist, device)

    def _create(self, h):
        _lib.check(self._lib.mirx_ivf_create_pq(self.dim, self.metric, self.nlist, self.m, 8, self.device.index, ctypes.byref(h)),
                   "mirx_ivf_create_pq")

    @classmethod
    def min_train_rows(cls, nlist):
        return max(nlist, 256)                 # 256 codewords to seed

    def state(self):
        return dict(super().state(), codebooks=self.codebooks)

    def set_state(self, state):
        super().set_state(state)
        self.set_codebooks(state["codebooks"])

    def train(self, rows, iters=10, init_positions=None, max_rows=None, codebook_iters=10):
        """IvfFlatIndex.train for the centroids, and the codebooks (train_codebooks) from at most 65 536 rows of the same data at
        an even stride"""
        IvfFlatIndex.train(self, rows, iters, init_positions, max_rows)
        self.train_codebooks(rows, codebook_iters)

    def train_codebooks(self, rows, iters=10, max_rows=PQ_TRAIN_ROWS):
        """Fix the codebooks: per sub-space Lloyd's k-means with 256 codewords under L2 (mirx_ivf_pq_train: mirx_ivf_train's
        loop, start at the rows floor(c n / 256)), on at most max_rows rows taken at an even stride.  Needs 256 rows."""
        rows = self._rows(rows, "train_codebooks")
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
            raise ValueError(f"train_codebooks: iters must be a non-negative integer, got {iters!r}")
        limit, n = int(max_rows), rows.shape[0]
        if min(limit, n) < 256:
            raise ValueError(f"train_codebooks: {min(limit, n)} rows cannot seed 256 codewords")
        rows = strided_sample(rows, limit)
        self._call("mirx_ivf_pq_train", _ptr(rows), rows.shape[0], int(iters), _stream_ptr(self.device))

    def set_codebooks(self, codebooks):
        """Fix the codebooks to a caller's [m, 256, dim / m] array."""
        cb = torch.as_tensor(codebooks).detach().to(torch.float32).contiguous()
        if tuple(cb.shape) != (self.m, 256, self.dim // self.m):
            raise ValueError(f"set_codebooks: expected [{self.m}, 256, {self.dim // self.m}], got {tuple(cb.shape)}")
        if cb.is_cuda:
            cb = cb.to(self.device)
            torch.cuda.current_stream(self.device).synchronize()
        self._call("mirx_ivf_pq_set_codebooks", _ptr(cb))

    @property
    def codebooks(self):
        """[m, 256, dim / m] fp32 on the index device"""
        out = torch.empty((self.m, 256, self.dim // self.m), dtype=torch.float32, device=self.device)
        self._call("mirx_ivf_pq_get_codebooks", _ptr(out))
        return out

    def tables(self, q):
        """-> float64 [nq, m, 256] on the index device: the ADC tables search() builds for q under the index metric (with
        residual coding: the inner-product tables of the residual codebooks, whatever the metric)"""
        return pq_tables(self._rows(q, "tables").to(self.device), self.codebooks, "IP" if self.by_residual else self.metric)


def residual_flag(value, key="by_residual"):
    """by_residual as a bool, ValueError naming the key for anything else"""
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"{key} must be True or False, got {value!r}")
    return bool(value)


class IvfResidualPqIndex(IvfPqIndex):
    """IVF_PQ with residual coding (mirx_ivf_create_pq_ex, include/mirx.h; restated in tests/_rpq_ref.py): a row is encoded as
    row - centroid of its list, so the codewords describe the spread inside a list.  Per query there is still ONE table -- the
    inner-product table of the residual codebooks, for both metrics; an entry's sum starts from the base of its (query, probed
    list), <q, centroid>, and L2 ranks by -((|q|^2 + |centroid + codewords|^2) - 2 ip) with the row's squared norm N2 kept from
    add() on (8 bytes a row).  train() fixes the centroids first and trains the codebooks on the residuals; train_codebooks needs
    fixed centroids.  reconstruct() returns centroid + codewords.  by_residual=False gives IvfPqIndex's raw form through the same
    create call.  IvfPqIndex keeps its own signature and behaviour."""

    def __init__(self, dim, metric="COSINE", nlist=1024, m=None, device=None, by_residual=True):
        self.by_residual = residual_flag(by_residual)
        super().__init__(dim, metric, nlist, m, device)

    def _create(self, h):
        _lib.check(self._lib.mirx_ivf_create_pq_ex(self.dim, self.metric, self.nlist, self.m, 8, int(self.by_residual),
                                                   self.device.index, ctypes.byref(h)), "mirx_ivf_create_pq_ex")

    def norms(self):
        """-> float64 [n] on the index device, in list-major order: N2 of the resident rows (L2 with residual coding only)"""
        out = torch.empty((len(self),), dtype=torch.float64, device=self.device)
        self._call("mirx_ivf_get_norms", _ptr_or_null(out))
        return out

    def bases(self, q, lists):
        """-> (B float64 [nq, nprobe], QQ float64 [nq]) for queries q and list numbers lists [nq, nprobe] under the index's
        centroids: what search() starts every entry's sum from, and L2's |q|^2"""
        return pq_bases(self._rows(q, "bases").to(self.device), lists, self.centroids, self.m)


IVF_INDEX_TYPES = {"IVF_FLAT": IvfFlatIndex, "IVF_SQ8": IvfSq8Index, "IVF_PQ": IvfPqIndex}    # by_residual: IvfResidualPqIndex


def ivf_index_spec(dim, index_type, params):
    """(dim, a Milvus index_type, its inner params dict) -> (the index class, its constructor keywords beside dim, metric and
    device): the one place that knows which parameters a member of the IVF family takes.  ValueError for an unknown type, an m
    that pq_bounds refuses, a by_residual that is no bool, an nlist outside [1, 65536].  Needs no GPU."""
    if not isinstance(index_type, str) or index_type not in IVF_INDEX_TYPES:
        raise ValueError(f"approximate=True needs index_type 'IVF_FLAT', 'IVF_SQ8' or 'IVF_PQ', got {index_type!r}")
    params = params if isinstance(params, dict) else {}
    cls, kwargs = IVF_INDEX_TYPES[index_type], {}
    if cls is IvfPqIndex:
        if "m" not in params:
            raise ValueError("index_type 'IVF_PQ' needs params['m'], the number of sub-quantisers; "
                             "'IVF_FLAT' and 'IVF_SQ8' take nlist alone")
        kwargs["m"] = pq_bounds(dim, params["m"])
        if residual_flag(params.get("by_residual", False), "params['by_residual']"):
            cls = IvfResidualPqIndex
    nlist = params.get("nlist", 1024)
    if isinstance(nlist, bool) or not isinstance(nlist, (int, np.integer)) or not 1 <= int(nlist) <= _lib.IVF_MAX_NLIST:
        raise ValueError(f"nlist must be an integer in [1, {_lib.IVF_MAX_NLIST}], got {nlist!r}")
    kwargs["nlist"] = int(nlist)
    return cls, kwargs


def _device_call(name, device, *args):
    """A stand-alone libmirx call on tensors of `device`: the device selected, its current stream's pending work done, the call
    made on that stream and its return code checked"""
    with torch.cuda.device(device):
        torch.cuda.current_stream().synchronize()
        _lib.check(getattr(_lib.load(), name)(*args, _stream_ptr(device)), name)


def _pq_args(first, codebooks, who, dtype):
    first = torch.as_tensor(first).to(dtype).contiguous()
    cb = torch.as_tensor(codebooks).to(torch.float32).contiguous()
    if not first.is_cuda or first.dim() != 2 or cb.dim() != 3 or cb.shape[1] != 256:
        raise ValueError(f"{who} expects a CUDA [n, .] array and codebooks [m, 256, dsub]")
    m, dim = int(cb.shape[0]), int(cb.shape[0] * cb.shape[2])
    pq_bounds(dim, m)
    return first, cb.to(first.device), m, dim


def pq_encode(rows, codebooks):
    """mirx_pq_encode: CUDA fp32 rows [n, dim] -> uint8 codes [n, m] under codebooks [m, 256, dim / m]"""
    rows, cb, m, dim = _pq_args(rows, codebooks, "pq_encode", torch.float32)
    if rows.shape[1] != dim:
        raise ValueError(f"pq_encode: rows of {rows.shape[1]} columns under codebooks of {dim}")
    out = torch.empty((rows.shape[0], m), dtype=torch.uint8, device=rows.device)
    _device_call("mirx_pq_encode", rows.device, _ptr_or_null(rows), rows.shape[0], dim, m, _ptr(cb), _ptr_or_null(out))
    return out


def pq_decode(codes, codebooks):
    """mirx_pq_decode: CUDA uint8 codes [n, m] -> fp32 rows [n, dim], each row's codewords concatenated"""
    if torch.as_tensor(codes).dtype != torch.uint8:
        raise ValueError("pq_decode expects uint8 codes")
    codes, cb, m, dim = _pq_args(codes, codebooks, "pq_decode", torch.uint8)
    if codes.shape[1] != m:
        raise ValueError(f"pq_decode: codes of {codes.shape[1]} columns under {m} codebooks")
    out = torch.empty((codes.shape[0], dim), dtype=torch.float32, device=codes.device)
    _device_call("mirx_pq_decode", codes.device, _ptr_or_null(codes), codes.shape[0], dim, m, _ptr(cb), _ptr_or_null(out))
    return out


def pq_residuals(rows, lists, centroids):
    """mirx_pq_residuals: CUDA fp32 rows [n, dim], int64 lists [n], centroids [nlist, dim] -> fp32 [n, dim], row - centroid of its
    list with one rounding per column (a list number outside 0 .. nlist-1: a NaN row)"""
    rows = torch.as_tensor(rows).to(torch.float32).contiguous()
    cent = torch.as_tensor(centroids).to(torch.float32).contiguous()
    if not rows.is_cuda or rows.dim() != 2 or cent.dim() != 2 or cent.shape[1] != rows.shape[1] or cent.shape[0] < 1:
        raise ValueError("pq_residuals expects CUDA rows [n, dim] and centroids [nlist, dim]")
    lists = torch.as_tensor(lists).to(torch.int64).reshape(-1).contiguous().to(rows.device)
    if lists.numel() != rows.shape[0]:
        raise ValueError("pq_residuals: lists and rows disagree in length")
    cent = cent.to(rows.device)
    out = torch.empty_like(rows)
    _device_call("mirx_pq_residuals", rows.device, _ptr_or_null(rows), rows.shape[0], rows.shape[1], _ptr_or_null(lists),
                 _ptr(cent), cent.shape[0], _ptr_or_null(out))
    return out


def pq_bases(q, lists, centroids, m):
    """mirx_pq_bases: CUDA fp32 queries [nq, dim], int32 list numbers [nq, nprobe], centroids [nlist, dim] -> (B float64
    [nq, nprobe], QQ float64 [nq]): B[q][s] = <q, centroid lists[q][s]> and QQ[q] = <q, q> as two-level sequential float64 sums
    (per sub-space of dim / m columns, then over the sub-spaces; include/mirx.h)"""
    q = torch.as_tensor(q).to(torch.float32).contiguous()
    cent = torch.as_tensor(centroids).to(torch.float32).contiguous()
    if not q.is_cuda or q.dim() != 2 or cent.dim() != 2 or cent.shape[1] != q.shape[1] or cent.shape[0] < 1:
        raise ValueError("pq_bases expects CUDA queries [nq, dim] and centroids [nlist, dim]")
    m = pq_bounds(q.shape[1], m)
    lists = torch.as_tensor(lists).to(torch.int32).contiguous().to(q.device)
    if lists.dim() != 2 or lists.shape[0] != q.shape[0] or lists.shape[1] < 1:
        raise ValueError("pq_bases: lists must be [nq, nprobe] with nprobe >= 1")
    cent = cent.to(q.device)
    base = torch.empty(tuple(lists.shape), dtype=torch.float64, device=q.device)
    qq = torch.empty((q.shape[0],), dtype=torch.float64, device=q.device)
    _device_call("mirx_pq_bases", q.device, _ptr_or_null(q), q.shape[0], q.shape[1], m, _ptr_or_null(lists), lists.shape[1],
                 _ptr(cent), cent.shape[0], _ptr_or_null(base), _ptr_or_null(qq))
    return base, qq


def pq_tables(q, codebooks, metric="COSINE"):
    """mirx_pq_tables: CUDA fp32 queries [nq, dim] -> float64 [nq, m, 256], T[q][j][c] = the metric's score of q's sub-vector j
    against codeword c as one sequential float64 sum over the sub-space's columns (include/mirx.h)"""
    q, cb, m, dim = _pq_args(q, codebooks, "pq_tables", torch.float32)
    if q.shape[1] != dim:
        raise ValueError(f"pq_tables: queries of {q.shape[1]} columns under codebooks of {dim}")
    out = torch.empty((q.shape[0], m, 256), dtype=torch.float64, device=q.device)
    _device_call("mirx_pq_tables", q.device, _ptr_or_null(q), q.shape[0], dim, m, metric_code(metric), _ptr(cb), _ptr_or_null(out))
    return out


def sq8_encode(rows, vmin, scale):
    """mirx_sq8_encode: CUDA fp32 rows [n, dim] -> uint8 codes [n, dim] under vmin / scale [dim]"""
    rows, vmin, scale = (torch.as_tensor(t).to(torch.float32).contiguous() for t in (rows, vmin, scale))
    if not rows.is_cuda or rows.dim() != 2 or vmin.shape != (rows.shape[1],) or scale.shape != (rows.shape[1],):
        raise ValueError("sq8_encode expects CUDA rows [n, dim] and vmin / scale [dim]")
    vmin, scale = vmin.to(rows.device), scale.to(rows.device)
    out = torch.empty(rows.shape, dtype=torch.uint8, device=rows.device)
    _device_call("mirx_sq8_encode", rows.device, _ptr_or_null(rows), rows.shape[0], rows.shape[1], _ptr(vmin), _ptr(scale),
                 _ptr_or_null(out))
    return out


def sq8_decode(codes, vmin, scale):
    """mirx_sq8_decode: CUDA uint8 codes [n, dim] -> fp32 rows [n, dim], (float)(vmin + code * scale) in double arithmetic"""
    codes = torch.as_tensor(codes).contiguous()
    vmin, scale = (torch.as_tensor(t).to(torch.float32).contiguous() for t in (vmin, scale))
    if not codes.is_cuda or codes.dtype != torch.uint8 or codes.dim() != 2 or vmin.shape != (codes.shape[1],) or \
            scale.shape != (codes.shape[1],):
        raise ValueError("sq8_decode expects CUDA uint8 codes [n, dim] and vmin / scale [dim]")
    vmin, scale = vmin.to(codes.device), scale.to(codes.device)
    out = torch.empty(codes.shape, dtype=torch.float32, device=codes.device)
    _device_call("mirx_sq8_decode", codes.device, _ptr_or_null(codes), codes.shape[0], codes.shape[1], _ptr(vmin), _ptr(scale),
                 _ptr_or_null(out))
    return out


def l2_normalize_(x):
    """In-place F.normalize(x, dim=1) on a CUDA fp32 tensor (model.py:83)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2):
        raise ValueError("l2_normalize_ expects a contiguous CUDA float32 [n, d] tensor")
    lib = _lib.load()
    with torch.cuda.device(x.device):
        _lib.check(lib.mirx_l2_normalize(ctypes.c_void_p(x.data_ptr()), x.shape[0], x.shape[1],
                                         _stream_ptr(x.device)), "mirx_l2_normalize")
    return x


def topk_merge(scores_f64, ids, metric=METRIC_IP):
    """Merge [nshard, nq, k] per-shard hits (fp64 ranking scores) -> (f64 [nq,k], f32 reported, ids)."""
    if scores_f64.dim() != 3 or scores_f64.shape != ids.shape:
        raise ValueError("expected [nshard, nq, k] scores and ids")
    ns, nq, k = scores_f64.shape
    scores_f64 = scores_f64.contiguous()
    ids = ids.contiguous()
    dev = scores_f64.device
    o64 = torch.empty((nq, k), dtype=torch.float64, device=dev)
    o32 = torch.empty((nq, k), dtype=torch.float32, device=dev)
    oid = torch.empty((nq, k), dtype=torch.int64, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.mirx_topk_merge(ctypes.c_void_p(scores_f64.data_ptr()), ctypes.c_void_p(ids.data_ptr()),
                                       ns, nq, k, metric_code(metric), ctypes.c_void_p(o64.data_ptr()),
                                       ctypes.c_void_p(o32.data_ptr()), ctypes.c_void_p(oid.data_ptr()),
                                       _stream_ptr(dev)), "mirx_topk_merge")
    return o64, o32, oid


# -- hybrid search's fusion ----------------------------------------------------------------------------------
def fuse_bounds(segments, limit):
    """The list lengths (one per request) and the limit of a fusion as ints, ValueError outside the contract's bounds:
    1 to 8 requests, every list at least one slot, at most 4096 slots together, 1 <= limit <= 1024."""
    try:
        segments = list(segments)
    except TypeError:
        raise ValueError(f"segments must be a sequence of list lengths, got {type(segments).__name__}") from None
    for name, v in [("limit", limit)] + [("a request's limit", s) for s in segments]:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {type(v).__name__}")
    segments, limit = [int(s) for s in segments], int(limit)
    if not 1 <= len(segments) <= _lib.FUSE_MAX_REQUESTS:
        raise ValueError(f"hybrid search: the number of requests must be in [1, {_lib.FUSE_MAX_REQUESTS}], got {len(segments)}")
    if min(segments) < 1:
        raise ValueError(f"hybrid search: a request's limit must be at least 1, got {min(segments)}")
    if sum(segments) > _lib.FUSE_MAX_ENTRIES:
        raise ValueError(f"hybrid search: the requests' limits must not exceed {_lib.FUSE_MAX_ENTRIES} together, got {sum(segments)}")
    if not 1 <= limit <= _lib.FUSE_MAX_LIMIT:
        raise ValueError(f"hybrid search: limit must be in [1, {_lib.FUSE_MAX_LIMIT}], got {limit}")
    return segments, limit


def fuse_ranker(ranker, n_requests):
    """A ranker in kernel form -- ("rrf", k) or ("weighted", weights, norms), norms among RAW / COSINE / IP / L2 -- as
    (kind, k, weights, norms) for mirx_fuse_ranked; ValueError for anything else."""
    if not isinstance(ranker, (tuple, list)) or not ranker or ranker[0] not in ("rrf", "weighted"):
        raise ValueError('ranker must be ("rrf", k) or ("weighted", weights, norms)')
    if ranker[0] == "rrf":
        if len(ranker) != 2:
            raise ValueError('the RRF ranker is ("rrf", k)')
        k = _bound(ranker[1], "RRF k")
        if not 0 < k < 16384:
            raise ValueError(f"RRF k must be in (0, 16384), got {k}")
        return _lib.FUSE_RRF, k, None, None
    if len(ranker) != 3:
        raise ValueError('the weighted ranker is ("weighted", weights, norms)')
    weights = [_bound(w, "a weight") for w in ranker[1]]
    norms = list(ranker[2])
    if len(weights) != n_requests or len(norms) != n_requests:
        raise ValueError(f"the weighted ranker needs one weight and one norm per request ({n_requests}), got {len(weights)} and "
                         f"{len(norms)}")
    for w in weights:
        if not 0.0 <= w <= 1.0:
            raise ValueError(f"a weight must be in [0, 1], got {w}")
    for n in norms:
        if n not in _lib.FUSE_NORMS:
            raise ValueError(f"unknown norm {n!r}: one of {', '.join(_lib.FUSE_NORMS)}")
    return _lib.FUSE_WEIGHTED, 0.0, weights, [_lib.FUSE_NORMS[n] for n in norms]


def fuse_ranked(codes, distances, segments, ranker, limit, n_codes=None):
    """Fuse ranked lists into one ranking per query (mirx_fuse_ranked; the contract is in include/mirx.h).

    codes [nq, m] int64 and distances [nq, m] float32 on one GPU: the requests' lists side by side, request r in the next
    segments[r] columns, best first; a code of -1 is an empty slot.  ranker: ("rrf", k), or ("weighted", weights, norms)
    with one weight in [0, 1] and one norm of RAW / COSINE / IP / L2 per request.  n_codes: one past the largest code (codes
    at or above it count as empty; default 2^31 - 1).
    -> (codes [nq, limit] int64, fp64 scores [nq, limit], request [nq, limit] int32, slot [nq, limit] int32, count [nq]
    int32): the best min(limit, distinct codes) documents by (score descending, code ascending), where each was first found,
    and how many there are; (-1, -inf, -1, -1) past them."""
    segments, limit = fuse_bounds(segments, limit)
    kind, k, weights, norms = fuse_ranker(ranker, len(segments))
    m = sum(segments)
    if not (torch.is_tensor(codes) and codes.is_cuda and codes.dtype == torch.int64 and codes.dim() == 2 and codes.shape[1] == m):
        raise ValueError(f"codes must be a CUDA int64 [nq, {m}] tensor")
    if not (torch.is_tensor(distances) and distances.dtype == torch.float32 and distances.shape == codes.shape
            and distances.device == codes.device):
        raise ValueError("distances must be a float32 tensor shaped like codes, on the same device")
    n_codes = 2 ** 31 - 1 if n_codes is None else int(n_codes)
    codes, distances = codes.contiguous(), distances.contiguous()
    dev, nq = codes.device, codes.shape[0]
    out_codes = torch.empty((nq, limit), dtype=torch.int64, device=dev)
    out_scores = torch.empty((nq, limit), dtype=torch.float64, device=dev)
    out_req = torch.empty((nq, limit), dtype=torch.int32, device=dev)
    out_slot = torch.empty((nq, limit), dtype=torch.int32, device=dev)
    out_count = torch.empty((nq,), dtype=torch.int32, device=dev)
    offsets = (ctypes.c_int32 * (len(segments) + 1))(*np.concatenate([[0], np.cumsum(segments)]).tolist())
    w = (ctypes.c_double * len(segments))(*weights) if weights is not None else None
    nm = (ctypes.c_int32 * len(segments))(*norms) if norms is not None else None
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.mirx_fuse_ranked(_ptr(codes), _ptr(distances), nq, m, n_codes, offsets, len(segments), kind, k, w, nm, limit,
                                        _ptr(out_codes), _ptr(out_scores), _ptr(out_req), _ptr(out_slot), _ptr(out_count),
                                        _stream_ptr(dev)), "mirx_fuse_ranked")
    return out_codes, out_scores, out_req, out_slot, out_count
