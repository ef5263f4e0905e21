"""Hybrid search's fusion kernel (k_fuse.hip) on its own: mirx.index.fuse_ranked against the float64 restatement
(tests/_fuse_ref.py).  GPU only.  RRF, COSINE-weighted and norm_score=False: codes, fp64 score BITS, where each document was
first found and the count are compared with ==.  The IP / L2 forms go through the device's atan: equal codes, scores within
1e-12 (at most 8 terms of weight <= 1, a few ulp of atan each: the error is of the order of 1e-14), on inputs whose
non-tied adjacent scores are at least 1e-9 apart in the restatement alone -- asserted, not skipped.

Shapes: every sort width's edges (m one below, at and one above a power of two, from 1 to the 4096 limit), one and eight
requests, lists fully shared / disjoint / partly shared, empty tails and wholly empty lists, duplicate distances, limit 1 /
above the documents / 1024, nq 1 / 3 / 1000."""
import numpy as np
import pytest
import torch

import _fuse_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

RRF = ("rrf", 60)


def _ranker(kind, n):
    """the three bit-exact forms, for n requests (weights k / 8 and their like: no two requests weigh the same)"""
    if kind == "rrf":
        return RRF
    weights = [(1 + (3 * r) % 8) / 8.0 for r in range(n)]
    return ("weighted", weights, ["COSINE" if kind == "cosine" else "RAW"] * n)


def _split(m, parts):
    """m as `parts` unequal positive list lengths (fewer when m is too small)"""
    parts = min(parts, m)
    cuts = [m * (i + 1) * (i + 2) // (parts * (parts + 1)) for i in range(parts)]      # triangular: unequal, the last is m
    seg = [b - a for a, b in zip([0] + cuts, cuts)]
    return [s for s in seg if s > 0]


def _lists(rng, nq, segments, n_keys, mode="partial", empty_tails=False, values=None):
    """codes [nq, m] int64 (-1 in empty slots, distinct inside a list) and float32 distances in [-1, 1) (or drawn from
    `values`).  partial: every list draws from the same n_keys; shared: every list is a permutation of ALL keys (segments all
    n_keys); disjoint: list r draws from its own n_keys."""
    m = sum(segments)
    codes = np.full((nq, m), -1, dtype=np.int64)
    for q in range(nq):
        off = 0
        for r, w in enumerate(segments):
            have = min(w, n_keys)
            if empty_tails:
                have = int(rng.integers(0, have + 1))
            pool = rng.permutation(n_keys)[:have] + (r * n_keys if mode == "disjoint" else 0)
            codes[q, off:off + have] = pool
            off += w
    if values is None:
        dist = rng.uniform(-1.0, 1.0, size=(nq, m)).astype(np.float32)
    else:
        dist = rng.choice(np.asarray(values, dtype=np.float32), size=(nq, m))
    return codes, dist


def _run(codes, dist, segments, ranker, limit, n_codes=None):
    from mirx.index import fuse_ranked
    out = fuse_ranked(torch.from_numpy(codes).to(DEV), torch.from_numpy(dist).to(DEV), segments, ranker, limit, n_codes=n_codes)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _expected(codes, dist, segments, ranker, limit, n_codes=None):
    """the restatement as the kernel's five arrays"""
    res = R.fuse(codes, dist, segments, ranker, limit, n_codes)
    nq = len(res)
    e_codes = np.full((nq, limit), -1, dtype=np.int64)
    e_scores = np.full((nq, limit), -np.inf, dtype=np.float64)
    e_req = np.full((nq, limit), -1, dtype=np.int32)
    e_slot = np.full((nq, limit), -1, dtype=np.int32)
    e_count = np.zeros((nq,), dtype=np.int32)
    for q, rows in enumerate(res):
        e_count[q] = len(rows)
        for p, (c, s, r, slot) in enumerate(rows):
            e_codes[q, p], e_scores[q, p], e_req[q, p], e_slot[q, p] = c, s, r, slot
    return res, (e_codes, e_scores, e_req, e_slot, e_count)


def _check_exact(codes, dist, segments, ranker, limit, n_codes=None):
    """every output equals the restatement's, scores to the bit; -> the restatement's result lists"""
    res, exp = _expected(codes, dist, segments, ranker, limit, n_codes)
    got = _run(codes, dist, segments, ranker, limit, n_codes)
    assert np.array_equal(got[4], exp[4]), "counts"
    assert np.array_equal(got[0], exp[0]), "codes"
    assert np.array_equal(got[1].view(np.int64), exp[1].view(np.int64)), "fp64 score bits"
    assert np.array_equal(got[2], exp[2]) and np.array_equal(got[3], exp[3]), "request / slot of the first entry"
    # every tie is resolved by code (implied by the equality above; stated on the kernel's own output)
    tie = (got[1][:, 1:] == got[1][:, :-1]) & (got[0][:, 1:] >= 0)
    assert np.all(got[0][:, 1:][tie] > got[0][:, :-1][tie])
    return res


def _ties(res):
    return sum(1 for rows in res for a, b in zip(rows, rows[1:]) if a[1] == b[1])


# ---- the sort widths' edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rrf", "cosine", "raw"])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096])
def test_every_sort_width_edge(m, kind):
    """three unequal, partly shared lists of m slots together (one list at m = 1 and 2), three queries, two limits"""
    rng = np.random.default_rng(1000 + m)
    segments = _split(m, 3)
    assert sum(segments) == m
    n_keys = max(2, (max(segments) * 3) // 2)
    codes, dist = _lists(rng, 3, segments, n_keys)
    ranker = _ranker(kind, len(segments))
    res = _check_exact(codes, dist, segments, ranker, min(1024, m + 3))
    _check_exact(codes, dist, segments, ranker, max(1, min(1024, m // 3)))
    if kind == "rrf" and m >= 63:
        assert _ties(res) > 0                                                    # RRF ties are the common case


@pytest.mark.parametrize("kind", ["rrf", "cosine", "raw"])
def test_two_slots_same_code_and_different_codes(kind):
    ranker = _ranker(kind, 2)
    codes = np.array([[5, 5], [5, 2], [2, 5], [-1, 5], [-1, -1]], dtype=np.int64)
    dist = np.array([[0.5, -0.25], [0.5, 0.5], [0.125, 0.75], [0.0, 1.0], [0.0, 0.0]], dtype=np.float32)
    for limit in (1, 2, 3):
        res = _check_exact(codes, dist, [1, 1], ranker, limit)
    assert [len(r) for r in res] == [1, 2, 2, 1, 0]
    if kind == "rrf":
        assert [c for c, *_ in res[1]] == [2, 5] and res[1][0][1] == res[1][1][1]            # equal ranks: the lower code first
    # one list of two slots: both codes, in list order under RRF
    res = _check_exact(np.array([[9, 4]], dtype=np.int64), np.array([[0.1, 0.9]], dtype=np.float32), [2], _ranker(kind, 1), 2)
    if kind == "rrf":
        assert [c for c, *_ in res[0]] == [9, 4]


# ---- one request and eight -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 100, 1024])
def test_one_request_returns_its_list_under_rrf(w):
    rng = np.random.default_rng(7 + w)
    codes, dist = _lists(rng, 3, [w], 3 * w)
    res = _check_exact(codes, dist, [w], RRF, min(1024, w))
    for q in range(3):
        assert [c for c, *_ in res[q]] == codes[q].tolist()                      # strictly falling 1 / (k + rank): the input order
    got = _run(codes, dist, [w], RRF, min(1024, w))
    assert np.array_equal(got[0], codes[:, :1024]) and np.array_equal(got[3], np.tile(np.arange(w, dtype=np.int32), (3, 1)))


@pytest.mark.parametrize("kind", ["rrf", "cosine", "raw"])
@pytest.mark.parametrize("mode", ["shared", "disjoint", "partial"])
def test_eight_requests_shared_disjoint_and_partly_shared(mode, kind):
    rng = np.random.default_rng({"shared": 1, "disjoint": 2, "partial": 3}[mode])
    segments = [37] * 8 if mode == "shared" else [37, 5, 64, 1, 20, 33, 50, 8]
    n_keys = 37 if mode == "shared" else 70
    codes, dist = _lists(rng, 3, segments, n_keys, mode=mode)
    res = _check_exact(codes, dist, segments, _ranker(kind, 8), 1024)
    if mode == "shared":
        assert all(len(r) == 37 for r in res)                                    # every document adds eight terms
    if mode == "disjoint":
        assert all(len(r) == sum(segments) for r in res)                         # every document adds one term
        if kind == "rrf":
            assert _ties(res) > 0


def test_empty_tails_and_wholly_empty_lists():
    rng = np.random.default_rng(11)
    segments = [40, 17, 64, 9]
    codes, dist = _lists(rng, 40, segments, 90, empty_tails=True)
    codes[0, :] = -1                                                             # a query without a single entry
    codes[1, 40:57] = -1                                                         # a wholly empty second list
    codes[2, :40] = -1                                                           # a wholly empty first list
    codes[3, :121] = -1                                                          # only the last list speaks
    for kind in ("rrf", "cosine", "raw"):
        for limit in (1, 10, 200):
            res = _check_exact(codes, dist, segments, _ranker(kind, 4), limit)
        assert len(res[0]) == 0 and 0 < len(res[5]) < 200
    got = _run(codes, dist, segments, RRF, 200)
    assert got[4][0] == 0 and np.all(got[0][0] == -1) and np.all(np.isneginf(got[1][0])) and np.all(got[2][0] == -1)
    # codes at or above n_codes are empty slots too
    _check_exact(codes, dist, segments, RRF, 50, n_codes=45)


def test_duplicate_distances_tie_by_code():
    rng = np.random.default_rng(12)
    segments = [30, 30, 30]
    codes, dist = _lists(rng, 20, segments, 45, values=[-0.5, -0.0, 0.0, 0.25, 0.25, 1.0])
    for kind in ("cosine", "raw"):
        ranker = ("weighted", [0.5, 0.5, 0.5], ["COSINE" if kind == "cosine" else "RAW"] * 3)
        res = _check_exact(codes, dist, segments, ranker, 45)
        assert _ties(res) > 20                                                   # few values, equal weights: ties everywhere


@pytest.mark.parametrize("kind", ["rrf", "cosine", "raw"])
def test_limits_one_above_the_documents_and_1024(kind):
    rng = np.random.default_rng(13)
    segments = [1500, 1100, 1496]                                                # 4096 slots over 2000 keys: more than 1024 documents
    codes, dist = _lists(rng, 3, segments, 2000)
    ranker = _ranker(kind, 3)
    res = _check_exact(codes, dist, segments, ranker, 1024)
    assert all(len(r) == 1024 for r in res)
    assert all(len(r) == 1 for r in _check_exact(codes, dist, segments, ranker, 1))
    small, sd = _lists(rng, 3, [20, 30], 35)
    res = _check_exact(small, sd, [20, 30], _ranker(kind, 2), 1024)              # padding: -1 / -inf past the documents
    assert all(30 <= len(r) <= 35 for r in res)


@pytest.mark.parametrize("nq", [1, 3, 1000])
def test_query_counts(nq):
    rng = np.random.default_rng(14 + nq)
    segments = [40, 17, 64]
    codes, dist = _lists(rng, nq, segments, 90, empty_tails=nq == 1000)
    for kind in ("rrf", "cosine", "raw"):
        _check_exact(codes, dist, segments, _ranker(kind, 3), 10)


def test_results_are_identical_between_calls():
    rng = np.random.default_rng(15)
    segments = [700, 300, 1000, 48]
    codes, dist = _lists(rng, 64, segments, 1200)
    ranker = ("weighted", [0.5, 0.3, 0.2, 1.0], ["IP", "L2", "COSINE", "RAW"])
    first = _run(codes, dist, segments, ranker, 100)
    for _ in range(3):
        again = _run(codes, dist, segments, ranker, 100)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(first, again))


# ---- the atan forms ------------------------------------------------------------------------------------------------------
def test_ip_and_l2_forms_within_1e12_on_separated_scores():
    """64 queries, lists of 40 / 17 / 64 over 90 keys, weights 0.5 / 0.3 / 0.2; an IP list uniform in [-3, 3], an L2 list in
    [0, 2], a COSINE list in [-1, 1], as float32."""
    rng = np.random.default_rng(2026)
    segments = [40, 17, 64]
    codes, _ = _lists(rng, 64, segments, 90)
    dist = np.concatenate([rng.uniform(-3.0, 3.0, (64, 40)), rng.uniform(0.0, 2.0, (64, 17)), rng.uniform(-1.0, 1.0, (64, 64))],
                          axis=1).astype(np.float32)
    ranker = ("weighted", [0.5, 0.3, 0.2], ["IP", "L2", "COSINE"])
    limit = 90
    res, exp = _expected(codes, dist, segments, ranker, limit)
    gap = R.min_gap(res)
    print(f"smallest non-tied adjacent gap of the restatement: {gap:.3e}")
    assert gap >= 1e-9, gap                                                      # the precondition of comparing codes
    got = _run(codes, dist, segments, ranker, limit)
    have = exp[0] >= 0
    err = float(np.max(np.abs(got[1][have] - exp[1][have])))
    print(f"largest |device - restatement| of a fused score: {err:.3e}")
    assert np.array_equal(got[4], exp[4]) and np.array_equal(got[0], exp[0])
    assert np.array_equal(got[2], exp[2]) and np.array_equal(got[3], exp[3])
    assert err <= 1e-12, err
    assert np.all(np.isneginf(got[1][~have]))
