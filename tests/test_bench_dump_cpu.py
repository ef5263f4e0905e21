"""bench.py --dump-outputs: the writer of the last timed step's results, fed host tensors of the step's shapes."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _step_outputs(nq, dim, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn((nq, dim), generator=g)
    s64 = torch.rand((nq, k), generator=g, dtype=torch.float64)
    ids = torch.randint(0, 1 << 40, (nq, k), generator=g)
    return emb, (s64, s64.float(), ids)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_every_row_is_written_exactly(bench, tmp_path):
    emb, (s64, s32, ids) = _step_outputs(37, 16, 5)
    bench.dump_outputs(str(tmp_path / "out"), emb, (s64, s32, ids))
    z = _load(tmp_path / "out")
    assert sorted(z) == ["embeddings", "ids", "query_rows", "scores", "scores_f64"]
    assert all(a.dtype in (np.float32, np.float64) for a in z.values())
    assert np.array_equal(z["embeddings"], emb.numpy()) and z["embeddings"].dtype == np.float32
    assert np.array_equal(z["scores_f64"], s64.numpy()) and z["scores_f64"].dtype == np.float64
    assert np.array_equal(z["scores"], s32.numpy())
    assert np.array_equal(z["ids"].astype(np.int64), ids.numpy())          # ids below 2**53 survive fp64
    assert np.array_equal(z["query_rows"], np.arange(37))


def test_large_outputs_become_a_fixed_sample_within_the_limit(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20_000)
    emb, out = _step_outputs(200, 32, 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), emb, out)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= 20_000
    rows = a["query_rows"].astype(np.int64)
    assert 0 < len(rows) < 200 and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["embeddings"], emb.numpy()[rows])
    assert np.array_equal(a["ids"].astype(np.int64), out[2].numpy()[rows])
    assert all(np.array_equal(a[n], b[n]) for n in a)                       # the same rows every time


def test_steps_below_one_are_refused():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
