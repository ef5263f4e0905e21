"""CPU-side checks of the radix ranking's boundary: the order-preserving key of an fp64 ranking score (mirx_rank_key), and
the argument checks of mirx_index_rank_top / MIRX_OPT_RANK_SORT, which answer before any device call."""
import ctypes

import numpy as np


def _lib():
    from mirx import _lib as L
    return L, L.load()


def _grid():
    """float64 values around every edge of the bit trick: both zeros, both infinities, the denormals, +-1 and the largest
    numbers, each with its neighbours, plus a few thousand random values of both signs over the whole exponent range."""
    tiny, big = np.float64(5e-324), np.finfo(np.float64).max
    smallest_normal = np.finfo(np.float64).tiny
    seeds = [0.0, -0.0, np.inf, -np.inf, tiny, -tiny, smallest_normal, -smallest_normal, 1.0, -1.0, big, -big,
             2.0 ** -1022 - tiny, 0.5, -0.5, 1e-300, -1e-300]
    vals = []
    with np.errstate(over="ignore"):                 # nextafter(max, inf) = inf is meant
        for v in seeds:
            v = np.float64(v)
            vals += [v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)]
    rng = np.random.default_rng(7)
    vals += list(rng.standard_normal(2000))
    vals += list(rng.standard_normal(1000) * 10.0 ** rng.integers(-300, 300, 1000))
    bits = rng.integers(0, 2 ** 63, 1000, dtype=np.uint64) | (rng.integers(0, 2, 1000, dtype=np.uint64) << np.uint64(63))
    rnd = bits.view(np.float64)
    vals += list(rnd[~np.isnan(rnd)])
    a = np.array(vals, dtype=np.float64)
    return a[~np.isnan(a)]


def test_rank_key_orders_like_the_scores():
    L, lib = _lib()
    a = _grid()
    assert a.size > 4000 and np.any(np.signbit(a) & (a == 0)) and np.any(~np.signbit(a) & (a == 0))
    keys = np.array([lib.mirx_rank_key(float(v)) for v in a], dtype=np.uint64)
    # every pair: key(a) < key(b) iff a > b (so equal values, -0.0 and +0.0 among them, share a key)
    assert np.array_equal(keys[:, None] < keys[None, :], a[:, None] > a[None, :])
    assert lib.mirx_rank_key(-0.0) == lib.mirx_rank_key(0.0)
    assert lib.mirx_rank_key(float("-inf")) == 0xFFF0000000000000        # the excluded id's key: the largest of any number
    assert lib.mirx_rank_key(float("inf")) < lib.mirx_rank_key(np.finfo(np.float64).max)


def test_rank_sort_tile_is_exported():
    L, lib = _lib()
    t = lib.mirx_rank_sort_tile()
    assert t >= 256 and t % 64 == 0


def test_rank_top_argument_checks_without_gpu():
    """Every bad argument is MIRX_EINVAL before the index or a device is touched.  No index can exist on a box without a GPU, so the
    calls whose fault is another argument pass a null index as well and name their own fault in the message."""
    L, lib = _lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.mirx_index_rank_top(None, p, 1, 1, None, p, None, p, None) == -1 and b"null index" in lib.mirx_last_error()
    assert lib.mirx_index_rank_top(None, p, 1, 0, None, p, None, p, None) == -1 and b"k must be" in lib.mirx_last_error()
    assert lib.mirx_index_rank_top(None, p, 1, -3, None, p, None, p, None) == -1 and b"k must be" in lib.mirx_last_error()
    assert lib.mirx_index_rank_top(None, p, 1, 1, None, p, p, None, None) == -1 and b"out_ids" in lib.mirx_last_error()
    assert lib.mirx_index_rank_top(None, p, 1, 1, None, None, None, p, None) == -1 and b"score outputs" in lib.mirx_last_error()
    assert lib.mirx_index_rank_top(None, p, 1, 1, None, None, None, None, None) == -1


def test_rank_sort_option_value_is_checked():
    L, lib = _lib()
    assert (L.OPT_RANK_SORT, L.RANK_SORT_AUTO, L.RANK_SORT_BITONIC, L.RANK_SORT_RADIX) == (5, 0, 1, 2)
    assert lib.mirx_index_set_option(None, L.OPT_RANK_SORT, 3) == -1
