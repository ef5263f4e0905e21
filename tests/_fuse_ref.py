"""Plain-Python float64 restatement of hybrid search's fusion (the contract of mirx_fuse_ranked in include/mirx.h):
dictionaries, one Python float operation at a time, `sorted` by (-score, code).

A query's input is one ranked list per request: [(code, distance), ..] best first, code -1 (or None) marking an empty slot
-- an empty slot still occupies its rank.  `distance` is the fp32 value a hit reports, held as a Python float.
ranker: ("rrf", k) or ("weighted", weights, norms), norms among "RAW" / "COSINE" / "IP" / "L2", as mirx.index.fuse_ranked
takes it."""
import math


def term(ranker, r, slot, distance):
    """contribution of the entry in slot `slot` (rank slot + 1) of request r's list"""
    if ranker[0] == "rrf":
        return 1.0 / (float(ranker[1]) + float(slot + 1))
    d = float(distance)
    norm = ranker[2][r]
    if norm == "COSINE":
        n = (1.0 + d) * 0.5
    elif norm == "IP":
        n = 0.5 + math.atan(d) / math.pi
    elif norm == "L2":
        n = 1.0 - 2.0 * math.atan(d) / math.pi
    else:
        assert norm == "RAW", norm
        n = d
    return float(ranker[1][r]) * n


def fuse_query(lists, ranker, limit, n_codes=None):
    """-> [(code, score, request, slot)] of one query: the best min(limit, distinct codes) documents by (score descending,
    code ascending); request / slot = where the document was first found.  A score is 0.0 plus the document's terms, added
    in ascending request (and slot inside a request)."""
    score, first = {}, {}
    for r, entries in enumerate(lists):
        for slot, (code, distance) in enumerate(entries):
            if code is None or code < 0 or (n_codes is not None and code >= n_codes):
                continue
            code = int(code)
            score[code] = score.get(code, 0.0) + term(ranker, r, slot, distance)
            first.setdefault(code, (r, slot))
    order = sorted(score, key=lambda c: (-score[c], c))[:limit]
    return [(c, score[c], first[c][0], first[c][1]) for c in order]


def fuse(codes, distances, segments, ranker, limit, n_codes=None):
    """The tensor-level form: codes / distances [nq, sum(segments)] arrays -> one fuse_query result per query."""
    out = []
    for crow, drow in zip(codes, distances):
        lists, off = [], 0
        for w in segments:
            lists.append([(int(c), float(d)) for c, d in zip(crow[off:off + w], drow[off:off + w])])
            off += w
        out.append(fuse_query(lists, ranker, limit, n_codes))
    return out


def min_gap(results):
    """smallest difference between adjacent scores of different value over all queries (inf when there is none)"""
    gap = math.inf
    for res in results:
        for (_, a, _, _), (_, b, _, _) in zip(res, res[1:]):
            if a != b:
                gap = min(gap, a - b)
    return gap


def fuse_by_key(hit_lists, code_of, ranker, limit, key=lambda h: h.entity.get("image_path")):
    """One query at collection level: hit_lists = the requests' own search() results (lists of Hit), code_of = {key: code}
    in the contract's join order.  -> [(key, score)] in result order."""
    name = {c: k for k, c in code_of.items()}
    lists = [[(code_of[key(h)], h.distance) for h in hits] for hits in hit_lists]
    return [(name[c], s) for c, s, _, _ in fuse_query(lists, ranker, limit)]


def join_order(collections_rows):
    """{key: code}: collections_rows = per collection (request order, each collection once) the keys of its live rows in index
    order; a key's code is the index of its first appearance."""
    code_of = {}
    for keys in collections_rows:
        for k in keys:
            code_of.setdefault(k, len(code_of))
    return code_of
