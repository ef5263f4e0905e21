"""The IVF family's seam on the device: state() of a trained index, handed to set_state() of a second index built with the same
arguments, gives the same index -- trained parts, codes, norms and answers bit for bit -- for every member and both metrics.
Shapes are the smallest that exercise every member: IVF_PQ needs 256 rows to seed its codewords."""
import numpy as np
import pytest
import torch

from _ivf_cases import _lib, _np, _unit

pytestmark = pytest.mark.gpu

DIM, NLIST, M, ROWS, NQ, K, NPROBE = 32, 4, 4, 320, 8, 5, 2
KINDS = {"flat": ("IVF_FLAT", {}), "sq8": ("IVF_SQ8", {}), "pq": ("IVF_PQ", {"m": M}),
         "rpq": ("IVF_PQ", {"m": M, "by_residual": True})}


def _same(a, b):
    """equal dtype, shape and bytes: bit-equal"""
    a, b = _np(a), _np(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_state_round_trip_gives_the_same_index(kind, metric):
    from mirx.index import IvfResidualPqIndex, ivf_index_spec
    MirxError = _lib().MirxError
    index_type, params = KINDS[kind]
    cls, kwargs = ivf_index_spec(DIM, index_type, dict(params, nlist=NLIST))
    rng = np.random.default_rng(7)
    centres = _unit(rng.standard_normal((NLIST, DIM)))
    rows = centres[rng.integers(0, NLIST, ROWS)] + 0.1 * rng.standard_normal((ROWS, DIM)).astype(np.float32)
    rows = _unit(rows) if metric == "COSINE" else np.ascontiguousarray(rows, dtype=np.float32)
    q = torch.from_numpy(np.ascontiguousarray(rows[rng.choice(ROWS, NQ, replace=False)] +
                                              0.05 * rng.standard_normal((NQ, DIM)).astype(np.float32)))
    rows, ids = torch.from_numpy(rows), torch.from_numpy(10 ** 6 - 3 * np.arange(ROWS, dtype=np.int64))
    assert ROWS >= cls.min_train_rows(NLIST)

    a = cls(DIM, metric, **kwargs)
    a.train(rows)
    a.add(rows, ids)
    state = a.state()
    assert tuple(state) == cls.STATE_KEYS and all(t.is_cuda for t in state.values())

    b = cls(DIM, metric, **kwargs)
    for key in cls.STATE_KEYS:                                             # a missing key: named, and nothing was set
        with pytest.raises(ValueError, match=repr(key)):
            b.set_state({k: v for k, v in state.items() if k != key})
        with pytest.raises(MirxError, match="centroids are not fixed"):
            b.centroids
    b.set_state(state)
    b.add(rows, ids)
    got = b.state()
    assert tuple(got) == cls.STATE_KEYS and all(_same(got[k], state[k]) for k in state)
    assert len(a) == len(b) == ROWS and a.list_sizes().tolist() == b.list_sizes().tolist()
    if kind != "flat":
        assert all(_same(x, y) for x, y in zip(a.codes(), b.codes()))
        assert a.codes()[0].shape == (ROWS, DIM if kind == "sq8" else M)
    if cls is IvfResidualPqIndex and metric == "L2":
        assert _same(a.norms(), b.norms())
    sa, ia = a.search(q, K, NPROBE, return_f64=True)
    sb, ib = b.search(q, K, NPROBE, return_f64=True)
    assert sa.dtype == torch.float64 and (_np(ia) >= 0).all()
    assert np.array_equal(_np(ia), _np(ib)) and _same(sa, sb)

    if kind == "flat":                                                     # fp32 rows are re-assigned: the same state, the same answer
        b.set_state(state)
        sc, ic = b.search(q, K, NPROBE, return_f64=True)
        assert np.array_equal(_np(ia), _np(ic)) and _same(sa, sc)
    else:                                                                  # a coded index that holds rows keeps its trained parts
        with pytest.raises(MirxError, match=r"\(-4\).*ivf_set_centroids.*holds rows keeps its centroids"):
            b.set_centroids(state["centroids"])
        with pytest.raises(MirxError, match=r"\(-4\).*ivf_set_centroids.*holds rows keeps its centroids"):
            b.set_state(state)
