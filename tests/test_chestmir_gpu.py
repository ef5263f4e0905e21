"""mirx.chestmir on the device: mirx_lesion_rerank (k_rerank.hip) and the native evaluate_dataset equal the float64
restatement of tests/_chestmir_ref.py exactly: ids, counted matches, flags and stats dicts; reports to 1e-12.

The restatement sums the dot products behind a combined score in the kernel's documented order; the base ranking comes from
plain float64 dots, so every case first asserts (a precondition on the inputs) that no two different base scores of one
query lie closer than 1e-12."""
import ctypes

import numpy as np
import pytest
import torch

import _chestmir_ref as R
from _chestmir_fixture import CASE_NAMES, load_case
from mirx import _lib
from mirx import chestmir as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

VINDR_SPELL = [(name, C.canonical_lesion_name(name)) for name in C.DEFAULT_VINDR_LESIONS] + [
    ("opacities", "lung opacity"), ("plural effusion", "pleural effusion"), ("mass", "nodule mass"), ("Fibrosis", "pulmonary fibrosis")]


def _dataset(gv, labels, maps):
    return C.EvalDataset(image_names=[f"{i}.png" for i in range(len(labels))], labels=np.asarray(labels, dtype=object),
                         global_vectors=gv, lesion_vectors=maps)


def _device_stages(gv, maps, targets, topk, w):
    store = C.RegionStore(maps)
    g, dstore, plans, ql, qr, ix = C.upload_dataset(gv, store, targets, DEV)
    n = gv.shape[0]
    base = ix.rank_all(g, exclude_ids=torch.arange(n, device=DEV))
    out, m, f = C.lesion_rerank_device(base, dstore, ql, qr, min(topk, n - 1), w, gvec=g)
    return {"g": g, "dstore": dstore, "ql": ql, "qr": qr, "base": base, "out": out, "matched": m, "flags": f, "store": store}


def _check_against_restatement(gv, labels, maps, targets, targets_canonical, kappas, cls_k, topk, w):
    gap = R.min_base_gap(R.base_scores(gv))
    print(f"smallest float64 base gap {gap:.3e}")
    assert gap > 1e-12
    ref = R.evaluate(gv, labels, maps, targets_canonical, kappas, cls_k, topk, w)
    d = _device_stages(gv, maps, targets, topk, w)
    n = len(labels)
    assert np.array_equal(d["base"].cpu().numpy().T, ref["ranks"][0])
    out = d["out"].cpu().numpy()
    for s in range(out.shape[0]):
        assert np.array_equal(out[s].T, ref["ranks"][1 + s]), f"stage {s}"
        assert np.array_equal(d["matched"][s].cpu().numpy(), ref["matched"][s]), f"stage {s}"
        assert np.array_equal(d["flags"][s].cpu().numpy(), ref["reranked"][s]), f"stage {s}"
    res = C.evaluate_dataset(_dataset(gv, labels, maps), targets, kappas=kappas, classification_k=cls_k, rerank_topk=topk,
                             global_weight=w)
    assert C.evaluate_dataset.last_native is True
    R.assert_report_close(res["stage1"], ref["reports"][0])
    R.assert_report_close(res["adaptive"][0], ref["reports"][1])
    assert res["adaptive"][1] == R.stats({"mode": "adaptive"}, n, ref["topk"], ref["matched"][0], ref["reranked"][0], topk, w,
                                         R.usage(ref["plans"][0], ref["reranked"][0]))
    assert [x[0] for x in res["lesions"]] == list(targets)
    for i, (name, rep, st) in enumerate(res["lesions"]):
        R.assert_report_close(rep, ref["reports"][2 + i])
        assert st == R.stats({"lesion": name}, n, ref["topk"], ref["matched"][1 + i], ref["reranked"][1 + i], topk, w)
    assert abs(res["summary"]["mean_mAP"] - float(np.mean([r["mAP"] for r in ref["reports"][2:]]))) <= 1e-12
    return d, ref


@pytest.mark.parametrize("case", CASE_NAMES)
def test_fixture_cases_equal_the_restatement(case):
    z = load_case(case)
    cfg = z["cfg"]
    _check_against_restatement(z["gv"], z["labels"], z["maps"], z["targets"], z["targets_canonical"], cfg["kappas"], cfg["cls_k"],
                               cfg["topk"], cfg["weight"])


@pytest.fixture(scope="module")
def vindr():
    raw = R.synthetic_raw(2026, 3000, 64, 32, 6, VINDR_SPELL, 4)
    ds = C.load_eval_dataset(R.rows_from_raw(raw))
    # planted exact ties: image 11 repeats image 10 (global vector and regions), so the id / base-position rules decide
    ds.global_vectors[11] = ds.global_vectors[10]
    ds.lesion_vectors[11] = {k: [v.copy() for v in vs] for k, vs in ds.lesion_vectors[10].items()}
    return ds


def test_vindr_shape_equals_the_restatement(vindr):
    targets = list(C.DEFAULT_VINDR_LESIONS)
    d, ref = _check_against_restatement(vindr.global_vectors, vindr.labels, vindr.lesion_vectors, targets,
                                        [C.canonical_lesion_name(t) for t in targets], [1, 5, 10], [1, 5, 10], 50, 0.5)
    assert int(d["flags"].sum()) > 3000                       # the case really re-ranks

    # one stage alone, the same stage among 17 and a permuted stage order give the same bits
    s = 5
    alone = C.lesion_rerank_device(d["base"], d["dstore"], d["ql"][s:s + 1].contiguous(), d["qr"][s:s + 1].contiguous(), 50, 0.5, gvec=d["g"])
    assert torch.equal(alone[0][0], d["out"][s]) and torch.equal(alone[1][0], d["matched"][s]) and torch.equal(alone[2][0], d["flags"][s])
    perm = torch.randperm(17, generator=torch.Generator().manual_seed(3)).to(DEV)
    mixed = C.lesion_rerank_device(d["base"], d["dstore"], d["ql"][perm].contiguous(), d["qr"][perm].contiguous(), 50, 0.5, gvec=d["g"])
    assert torch.equal(mixed[0], d["out"][perm]) and torch.equal(mixed[1], d["matched"][perm]) and torch.equal(mixed[2], d["flags"][perm])

    # a query's result does not change when the regions of images outside its candidates change
    changed = torch.arange(100, 140, device=DEV)
    other = C._DeviceStore(d["store"], DEV)
    rp = other.row_ptr
    for i in changed.tolist():
        other.vectors[int(rp[i]):int(rp[i + 1])] *= -1.0
    again = C.lesion_rerank_device(d["base"], other, d["ql"], d["qr"], 50, 0.5, gvec=d["g"])
    touched = torch.isin(d["base"][:, :50], changed).any(dim=1)
    touched[changed] = True
    keep = ~touched
    assert int(keep.sum()) > 300 and int(touched.sum()) > 300
    assert torch.equal(again[0][:, keep], d["out"][:, keep]) and torch.equal(again[1][:, keep], d["matched"][:, keep])
    assert not torch.equal(again[0][:, touched], d["out"][:, touched])


def test_wide_vectors_and_a_long_candidate_list_equal_the_restatement():
    """D = 96 and Dr = 300 give every lane several elements of a dot (the l, l + 64, ... order) and stage the query vector in
    more than one pass; topk = 1000 runs the match count and every bitonic step over several passes of the workgroup."""
    spell = [(name, C.canonical_lesion_name(name)) for name in C.DEFAULT_COVID_LESIONS[:3]]
    raw = R.synthetic_raw(99, 1200, 96, 300, 5, spell, 3)
    ds = C.load_eval_dataset(R.rows_from_raw(raw))
    targets = list(C.DEFAULT_COVID_LESIONS[:3])
    d, ref = _check_against_restatement(ds.global_vectors, ds.labels, ds.lesion_vectors, targets,
                                        [C.canonical_lesion_name(t) for t in targets], [1, 5, 10], [1, 5, 10], 1000, 0.3)
    assert ref["topk"] == 1000 and int(d["flags"].sum()) > 1200


def test_device_wrapper_checks_its_inputs():
    z = load_case("cone")
    d = _device_stages(z["gv"], z["maps"], z["targets"], 5, 0.5)
    n = z["gv"].shape[0]
    sim = torch.zeros((n, n), dtype=torch.float64, device=DEV)
    for kw in (dict(gvec=d["g"].double()), dict(gvec=d["g"].t()), dict(gvec=d["g"].cpu()), dict(gvec=d["g"][:-1].contiguous()),
               dict(base_sim=sim.float()), dict(base_sim=sim[:, :-1].contiguous()), dict(), dict(base_sim=sim, gvec=d["g"])):
        with pytest.raises(ValueError, match="lesion_rerank_device"):
            C.lesion_rerank_device(d["base"], d["dstore"], d["ql"], d["qr"], 5, 0.5, **kw)
    with pytest.raises(ValueError, match="lesion_rerank_device"):
        C.lesion_rerank_device(d["base"], d["dstore"], d["ql"].long(), d["qr"], 5, 0.5, gvec=d["g"])


def test_public_functions_run_on_the_device_and_agree_with_evaluate_dataset():
    z = load_case("a")
    cfg = z["cfg"]
    sim = R.base_scores(z["gv"])
    ranks_base = np.argsort(-sim, axis=0, kind="stable")
    ref = R.evaluate(z["gv"], z["labels"], z["maps"], z["targets_canonical"], cfg["kappas"], cfg["cls_k"], cfg["topk"], cfg["weight"])
    whole = C.evaluate_dataset(_dataset(z["gv"], z["labels"], z["maps"]), z["targets"], kappas=cfg["kappas"],
                               classification_k=cfg["cls_k"], rerank_topk=cfg["topk"], global_weight=cfg["weight"])
    n = len(z["labels"])
    # the rank matrices of evaluate_dataset's route (one upload, base scores recomputed in the kernel), id for id
    route = _device_stages(z["gv"], z["maps"], z["targets"], cfg["topk"], cfg["weight"])["out"].cpu().numpy()
    r, st = C.rerank_with_adaptive_lesion(sim, z["maps"], z["targets"], cfg["topk"], cfg["weight"])
    assert np.array_equal(r, route[0].T)
    assert C.rerank_with_adaptive_lesion.last_native is True
    want = R.rerank(ranks_base, z["maps"], ref["plans"][0], cfg["topk"], cfg["weight"], base_sim=sim)
    assert r.dtype == np.int64 and np.array_equal(r, want[0])
    assert st == R.stats({"mode": "adaptive"}, n, ref["topk"], want[1], want[2], cfg["topk"], cfg["weight"], R.usage(ref["plans"][0], want[2]))
    assert st == whole["adaptive"][1]
    rep = C.evaluate_rankings(r, z["labels"], cfg["kappas"], cfg["cls_k"])
    assert C.evaluate_rankings.last_native is True
    R.assert_report_close(rep, R.report(want[0], z["labels"], cfg["kappas"], cfg["cls_k"]))
    R.assert_report_close(rep, whole["adaptive"][0])
    for i, t in enumerate(z["targets"]):
        r, st = C.rerank_with_specific_lesion(sim, z["maps"], t, cfg["topk"], cfg["weight"])
        assert C.rerank_with_specific_lesion.last_native is True
        want = R.rerank(ranks_base, z["maps"], ref["plans"][1 + i], cfg["topk"], cfg["weight"], base_sim=sim)
        assert np.array_equal(r, want[0]) and np.array_equal(r, route[1 + i].T)
        assert st == whole["lesions"][i][2]
        R.assert_report_close(C.evaluate_rankings(r, z["labels"], cfg["kappas"], cfg["cls_k"]), whole["lesions"][i][1])


def test_ragged_region_vectors_take_the_numpy_path():
    z = load_case("b0")
    cfg = z["cfg"]
    maps = [dict(m) for m in z["maps"]]
    maps[3]["ild"] = [np.full(5, 5.0 ** -0.5, dtype=np.float32)]      # another dimension than the other regions' 16
    sim = (z["gv"] @ z["gv"].T).astype(np.float32)
    np.fill_diagonal(sim, -np.inf)
    C.rerank_with_specific_lesion(sim, z["maps"], z["targets"][0], cfg["topk"], cfg["weight"])
    assert C.rerank_with_specific_lesion.last_native is True
    C.rerank_with_specific_lesion(sim, maps, z["targets"][1], cfg["topk"], cfg["weight"])
    assert C.rerank_with_specific_lesion.last_native is False
    C.rerank_with_specific_lesion(sim, z["maps"], z["targets"][0], 5000, cfg["weight"])           # min(topk, N - 1) counts
    assert C.rerank_with_specific_lesion.last_native is True
    C.evaluate_dataset(_dataset(z["gv"], z["labels"], maps), z["targets"], rerank_topk=cfg["topk"])
    assert C.evaluate_dataset.last_native is False


def test_limits_return_einval():
    lib = _lib.load()
    z = load_case("cone")
    d = _device_stages(z["gv"], z["maps"], z["targets"], 5, 0.5)
    n, ds = z["gv"].shape[0], d["dstore"]
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    out = torch.full_like(d["out"], -7)

    def call(n_=n, dr=ds.dr, topk=5, w=0.5, stages=d["ql"].shape[0], dvec=z["gv"].shape[1], gvec=d["g"], base=d["base"]):
        return lib.mirx_lesion_rerank(p(base) if base is not None else None, n_, None, p(gvec) if gvec is not None else None, dvec,
                                      p(ds.row_ptr), p(ds.lesion), p(ds.vectors), ds.n_regions, dr, p(d["ql"]), p(d["qr"]), stages,
                                      topk, w, p(out), p(d["matched"]), p(d["flags"]), None)

    for kw in (dict(n_=1), dict(n_=65537), dict(dr=0), dict(dr=4097), dict(topk=0), dict(topk=1025), dict(topk=n), dict(w=-0.01),
               dict(w=1.01), dict(w=float("nan")), dict(stages=-1), dict(stages=65536), dict(gvec=None), dict(dvec=0), dict(base=None)):
        assert call(**kw) == -1, kw                                       # MIRX_EINVAL
        assert b"lesion_rerank" in lib.mirx_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                        # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, d["out"])


def test_native_evaluate_dataset_runs_no_library_gemm_or_sort(vindr):
    ds = _dataset(vindr.global_vectors[:600], vindr.labels[:600], vindr.lesion_vectors[:600])
    C.evaluate_dataset(ds, C.DEFAULT_VINDR_LESIONS)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        C.evaluate_dataset(ds, C.DEFAULT_VINDR_LESIONS)
    assert C.evaluate_dataset.last_native is True
    names = {e.key for e in prof.key_averages()}
    banned = {"aten::mm", "aten::bmm", "aten::matmul", "aten::addmm", "aten::linear", "aten::sort", "aten::argsort", "aten::topk",
              "aten::msort", "aten::kthvalue"}
    assert not (names & banned), names & banned
    low = [n.lower() for n in names]
    assert not [n for n in low if "gemm" in n and "mirx" not in n or "cijk" in n or "radixsort" in n or "rocprim" in n and "sort" in n], names
    assert any("k_lesion_rerank" in n for n in names), names               # the kernel trace saw the mirx kernels
