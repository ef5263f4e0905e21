"""The grouping search's contract (include/mirx.h) as a numpy walk over a given ranking -- the reference of
test_group_cpu.py, test_group_kernels_gpu.py and test_group_search_gpu.py.  Plain Python, no tolerance: the tests compare ids,
codes and score bits with ==.

A *ranking* here is what the index's searches return for one query: the eligible rows (mask entry non-zero, id not the query's
excluded id), best first (fp64 score descending, equal scores by ascending id), as parallel sequences of ids, the index into the
code table of each entry, and optionally fp64 scores."""
import numpy as np


def walk(entries, group_of, limit, group_size):
    """Walk a ranking: a group opens at its first row while fewer than `limit` groups are open; a row is kept while its group is
    open and holds fewer than `group_size` rows.  entries: indexes into group_of, in ranking order (a negative entry ends the
    list).  -> [(code, [positions in `entries` of the kept rows]), ...] in the order the groups opened."""
    slots, where = [], {}
    for pos, e in enumerate(entries):
        if e < 0:
            break
        code = int(group_of[e])
        s = where.get(code)
        if s is None:
            if len(slots) >= limit:
                continue
            s = where[code] = len(slots)
            slots.append((code, []))
        if len(slots[s][1]) < group_size:
            slots[s][1].append(pos)
    return slots


def tensors(entries, ids, scores, group_of, limit, group_size):
    """walk() as the arrays the device calls return for one query: ids [limit, group_size] (-1 in empty slots), fp64 scores
    alike (-inf), codes [limit] (-1), kept [limit]."""
    out_ids = np.full((limit, group_size), -1, dtype=np.int64)
    out_sc = np.full((limit, group_size), -np.inf, dtype=np.float64)
    out_codes = np.full((limit,), -1, dtype=np.int64)
    out_kept = np.zeros((limit,), dtype=np.int32)
    for s, (code, kept) in enumerate(walk(entries, group_of, limit, group_size)):
        out_codes[s] = code
        out_kept[s] = len(kept)
        for m, pos in enumerate(kept):
            out_ids[s, m] = ids[pos]
            if scores is not None:
                out_sc[s, m] = scores[pos]
    return out_ids, out_sc, out_codes, out_kept


def prefix_state(prefix, group_of, group_rows, excl_group, limit, group_size):
    """What a ranked PREFIX can decide, given c(g) = group_rows[g] eligible rows per code (one less for excl_group, the code of
    the query's excluded row, or -1).  -> (groups open, complete, groups final):
      final     T = min(limit, groups with c_i(g) > 0) groups are open: membership and order of the groups are decided;
      complete  final and every open group holds min(group_size, c_i(g)) rows -- or the prefix holds a negative entry, i.e. it is
                the whole eligible ranking."""
    cnt = {g: int(c) for g, c in enumerate(group_rows) if c > 0}
    if excl_group is not None and excl_group >= 0 and excl_group in cnt:
        cnt[excl_group] -= 1
        if cnt[excl_group] == 0:
            del cnt[excl_group]
    target = min(limit, len(cnt))
    slots = walk(prefix, group_of, limit, group_size)
    ended = any(e < 0 for e in prefix)
    final = len(slots) == target
    complete = ended or (final and all(len(kept) == min(group_size, cnt[code]) for code, kept in slots))
    return len(slots), complete, final or complete


def brute_force(ids, scores, codes, limit, group_size):
    """The same answer without a walk, from the definition's first form: per group the members sorted by (score descending, id
    ascending), the groups ordered by their best member, the first `limit` groups, the first `group_size` members each.
    ids / scores / codes: the eligible rows in any order.  -> [(code, [row numbers into ids]), ...]"""
    groups = {}
    for r in range(len(ids)):
        groups.setdefault(int(codes[r]), []).append(r)
    key = lambda r: (-scores[r], ids[r])
    ranked = sorted((sorted(rows, key=key) for rows in groups.values()), key=lambda rows: key(rows[0]))
    return [(int(codes[rows[0]]), rows[:group_size]) for rows in ranked[:limit]]


def ranking_of(ids, scores, eligible=None):
    """row numbers of the eligible rows in ranking order (score descending, equal scores by ascending id)"""
    rows = np.arange(len(ids)) if eligible is None else np.nonzero(eligible)[0]
    return rows[np.lexsort((np.asarray(ids)[rows], -np.asarray(scores)[rows]))]
