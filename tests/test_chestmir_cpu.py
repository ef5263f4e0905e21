"""mirx.chestmir without a GPU: the host helpers and the numpy path of the ranking functions against the fixture made by the
reference's own functions (tests/golden/make_golden_chestmir.py), and the float64 restatement (tests/_chestmir_ref.py)
against the same fixture under the near-tie audit of DESIGN 22.

The audit may excuse a position only when the float64 keys of the two ids differ by at most 2 * max(D, Dr) * 2^-24 (unit
float32 vectors: a float32 dot of d terms is within d * 2^-24 of the exact one), and at most 0.05 % of the positions of one
stage's rank matrix.  Stats and reports are compared with the reference's when no position was excused, otherwise with the
restatement's (reports to 1e-12)."""
import io
import contextlib

import numpy as np
import pytest

import _chestmir_ref as R
from _chestmir_fixture import CASE_NAMES, audit, load_case, load_meta
from mirx import chestmir as C


def _same_maps(a, b):
    assert len(a) == len(b)
    for ma, mb in zip(a, b):
        assert list(ma) == list(mb)
        for k in ma:
            assert len(ma[k]) == len(mb[k])
            for va, vb in zip(ma[k], mb[k]):
                assert np.asarray(va).dtype == np.float32 and np.array_equal(va, vb)


def test_tables_and_canonical_names():
    meta = load_meta()
    assert C.DEFAULT_COVID_LESIONS == meta["default_covid"] and C.DEFAULT_VINDR_LESIONS == meta["default_vindr"]
    for raw, canon in meta["canonical"]:
        assert C.canonical_lesion_name(raw) == canon
    assert C._normalize_lesion_text("  Lung_Opacity/x-Y ") == "lung opacity x y"
    assert C.parse_json_list(None) == [] and C.parse_json_list("") == [] and C.parse_json_list("{") == []
    assert C.parse_json_list('{"a": 1}') == [] and C.parse_json_list("[1, 2]") == [1, 2]


def test_build_lesion_vector_map_json_strings():
    for case in load_meta()["json_cases"]:
        got = C.build_lesion_vector_map(case["labels"], case["vectors"])
        assert list(got) == list(case["map"])
        for k, vs in case["map"].items():
            assert len(got[k]) == len(vs)
            for v, want in zip(got[k], vs):
                assert v.dtype == np.float32 and np.array_equal(v, np.asarray(want, dtype=np.float32))


class _Paged:
    def __init__(self, rows):
        self.rows, self.num_entities, self.calls = rows, len(rows), []

    def query(self, expr, output_fields, limit, offset):
        self.calls.append((expr, tuple(output_fields), limit, offset))
        return self.rows[offset:offset + limit]


def test_load_eval_dataset():
    z = load_case("d")
    rows = R.rows_from_raw(z["raw"])
    paged = _Paged(rows)
    for ds in (C.load_eval_dataset(rows), C.load_eval_dataset(paged, fetch_batch_size=50)):
        assert ds.image_names == [str(x) for x in z["raw"]["image_names"]]
        assert ds.labels.dtype == object and list(ds.labels) == list(z["labels"])
        assert ds.global_vectors.dtype == np.float32 and np.array_equal(ds.global_vectors, z["gv"])
        _same_maps(ds.lesion_vectors, z["maps"])
    assert [(c[2], c[3]) for c in paged.calls] == [(50, 0), (50, 50), (20, 100)]
    assert paged.calls[0][:2] == ("id >= 0", tuple(C.EVAL_FIELDS))
    # rows without a usable global vector are skipped; overrides go by file stem; the default label
    extra = [dict(rows[0], global_vector=[]), dict(rows[1], global_vector=[[1.0, 2.0]]), {k: v for k, v in rows[2].items() if k != "label"},
             dict(rows[3], image_name="dir/abc.png")]
    ds = C.load_eval_dataset(extra, label_overrides={"abc": "Edema | ILD"})
    assert list(ds.labels) == ["unknown", "Edema | ILD"] and ds.image_names[1] == "dir/abc.png"
    with pytest.raises(ValueError, match="too few entities: 1"):
        C.load_eval_dataset(rows[:1])
    with pytest.raises(ValueError, match="too few entities: 1"):
        C.load_eval_dataset(_Paged(rows[:1]))
    with pytest.raises(ValueError, match="Insufficient valid vectors"):
        C.load_eval_dataset([rows[0], extra[0]])


def test_vindr_label_lookup(tmp_path):
    p = tmp_path / "labels.csv"
    p.write_text("image_id,Edema,ILD,No finding\na,1,0,0\nb,0,0,1\nc,yes,TRUE,1\n,1,1,1\nd,0,0,0\n")
    assert C.build_vindr_label_lookup(p) == {"a": "Edema", "b": "No finding", "c": "Edema | ILD", "d": "No finding"}
    with pytest.raises(FileNotFoundError):
        C.build_vindr_label_lookup(tmp_path / "missing.csv")
    (tmp_path / "bad.csv").write_text("x,y\n1,2\n")
    with pytest.raises(ValueError, match="missing image_id"):
        C.build_vindr_label_lookup(tmp_path / "bad.csv")


def test_choosers_and_candidate_score():
    v = [np.asarray(x, dtype=np.float32) for x in ([1, 0], [0, 1], [-1, 0], [0.6, 0.8])]
    m = {"edema": [v[0]], "lung opacity": [v[1], v[2]], "consolidation": [v[3], v[0]]}
    assert C.choose_query_lesion_vector(m, "EDEMA") is v[0] and C.choose_query_lesion_vector(m, "ILD") is None
    # most vectors wins; strict >, so the target order breaks the 2 : 2 tie; the first stored vector is the query vector
    assert C.choose_query_adaptive_lesion_vector(m, ["Edema", "opacity", "Consolidation"])[0] == "lung opacity"
    name, q = C.choose_query_adaptive_lesion_vector(m, ["Edema", "Consolidation", "opacity"])
    assert name == "consolidation" and q is v[3]
    assert C.choose_query_adaptive_lesion_vector(m, ["ILD"]) == (None, None)
    assert C.best_candidate_lesion_score(v[0], m, "Lung_Opacity") == 0.0            # max(0, -1)
    assert C.best_candidate_lesion_score(v[0], m, "ILD") == -1.0
    assert C.best_candidate_lesion_score(v[2], {"edema": [v[0]]}, "edema") == -1.0  # a real score of -1


def _same_candidates(ranks, ref_ranks, topk):
    """Every query's first topk ids are the same set in both rankings: no near-tie swap straddles the re-rank boundary."""
    assert np.array_equal(np.sort(ranks[:topk], axis=0), np.sort(ref_ranks[:topk], axis=0))


def test_vectorised_majority_vote_equals_the_metrics_module():
    """chestmir votes with array operations (18 stages x 3000 queries per evaluation); the result is metrics.py's."""
    from mirx import metrics as M
    z = load_case("a")
    for r in z["ref_ranks"][:3]:
        got = C._classification_from_top(z["labels"], r[:10], [1, 3, 10])
        want = M.compute_classification_metrics(z["labels"], None, [1, 3, 10], ranks=r[:10])
        assert set(got) == set(want)
        for k in got:
            assert set(got[k]) == set(want[k])
            for name in got[k]:
                assert abs(got[k][name] - want[k][name]) <= 1e-12, (k, name)


def _numpy_path(z):
    """Every stage through the public functions (no GPU here: their numpy path), main()'s sequence."""
    cfg = z["cfg"]
    sim = z["gv"] @ z["gv"].T
    np.fill_diagonal(sim, -np.inf)
    ranks, stats = [C.similarity_to_ranks(sim)], []
    assert C.similarity_to_ranks.last_native is False
    r, st = C.rerank_with_adaptive_lesion(sim, z["maps"], z["targets"], cfg["topk"], cfg["weight"])
    assert C.rerank_with_adaptive_lesion.last_native is False
    ranks.append(r)
    stats.append(st)
    for t in z["targets"]:
        r, st = C.rerank_with_specific_lesion(sim, z["maps"], t, cfg["topk"], cfg["weight"])
        assert C.rerank_with_specific_lesion.last_native is False
        ranks.append(r)
        stats.append(st)
    return ranks, stats


@pytest.mark.parametrize("case", CASE_NAMES)
def test_numpy_path_against_the_reference(case):
    z = load_case(case)
    cfg = z["cfg"]
    ref = R.evaluate(z["gv"], z["labels"], z["maps"], z["targets_canonical"], cfg["kappas"], cfg["cls_k"], cfg["topk"], cfg["weight"])
    s64 = R.base_scores(z["gv"])
    ranks, stats = _numpy_path(z)
    assert len(ranks) == len(z["ref_ranks"]) == 2 + len(z["targets"])
    for s, (r, want) in enumerate(zip(ranks, z["ref_ranks"])):
        assert r.shape == want.shape and r.dtype == np.int64
        excused = audit(r, want, s64, ref["keys"][s - 1] if s else None, z["bound"])
        print(f"case {case} stage {s}: numpy path differs from the fixture at {excused} of {r.size} positions")
        rep = C.evaluate_rankings(r, z["labels"], cfg["kappas"], cfg["cls_k"])
        assert C.evaluate_rankings.last_native is False
        if s:                                                   # an excused swap inside the head or the tail moves no count
            _same_candidates(r, want, ref["topk"])
            assert stats[s - 1] == z["ref_stats"][s - 1]
            assert list(stats[s - 1]) == list(z["ref_stats"][s - 1])                # key for key, in the reference's order
        if excused == 0:
            R.assert_report_close(rep, z["ref_reports"][s])
        else:
            R.assert_report_close(rep, R.report(r, z["labels"], cfg["kappas"], cfg["cls_k"]))


@pytest.mark.parametrize("case", CASE_NAMES)
def test_restatement_against_the_reference(case):
    z = load_case(case)
    cfg = z["cfg"]
    s64 = R.base_scores(z["gv"])
    gap = R.min_base_gap(s64)
    print(f"case {case}: smallest float64 base gap {gap:.3e}, audit bound {z['bound']:.3e}")
    assert gap > 1e-12
    ref = R.evaluate(z["gv"], z["labels"], z["maps"], z["targets_canonical"], cfg["kappas"], cfg["cls_k"], cfg["topk"], cfg["weight"])
    n = len(z["labels"])
    for s, (r, want) in enumerate(zip(ref["ranks"], z["ref_ranks"])):
        excused = audit(r, want, s64, ref["keys"][s - 1] if s else None, z["bound"])
        print(f"case {case} stage {s}: restatement differs from the fixture at {excused} of {r.size} positions")
        _same_candidates(r, want, ref["topk"])
        if s:               # no excused swap straddles the topk boundary, so the counted matches and stats are the reference's
            head = {"mode": "adaptive"} if s == 1 else {"lesion": z["targets"][s - 2]}
            use = R.usage(ref["plans"][0], ref["reranked"][0]) if s == 1 else None
            assert R.stats(head, n, ref["topk"], ref["matched"][s - 1], ref["reranked"][s - 1], cfg["topk"], cfg["weight"],
                           use) == z["ref_stats"][s - 1]
        if excused == 0:
            R.assert_report_close(ref["reports"][s], z["ref_reports"][s])


def test_fixture_holds_the_quirks():
    """Case (d) really contains what it was planted for (checked on the restatement's keys)."""
    z = load_case("d")
    cfg = z["cfg"]
    ref = R.evaluate(z["gv"], z["labels"], z["maps"], z["targets_canonical"], cfg["kappas"], cfg["cls_k"], cfg["topk"], cfg["weight"])
    assert z["targets_canonical"][-1] == "lung cyst" and not any("lung cyst" in m for m in z["maps"])
    assert ref["reranked"][-1].sum() == 0 and z["ref_stats"][-1]["queries_fallback_global"] == len(z["labels"])
    edema = 1 + z["targets_canonical"].index("edema")
    used_not_counted = 0
    for q, (ids, comb, base) in ref["keys"][edema].items():
        region = (comb - cfg["weight"] * base) / (1.0 - cfg["weight"])
        used_not_counted += int(np.count_nonzero((region < -1e-6) & (region > -1.0 + 1e-6)))
    assert used_not_counted > 0                                                   # a negative real score: used, not counted
    assert any(len(v) >= 2 for m in z["maps"] for v in m.values())                # several regions of one lesion: the max
    tie = [m for m in z["maps"] if m.get("edema") and m.get("lung opacity") and len(m["edema"]) == len(m["lung opacity"])
           and len(m["edema"]) > len(m.get("consolidation", []))]
    assert tie                                                                    # equal counts: the target order decides
    assert all(R.plan_adaptive([m], z["targets_canonical"])[0][0] == "edema" for m in tie)
    for name in ("call", "cone"):
        c = load_case(name)
        assert (c["cfg"]["topk"] >= len(c["labels"]) - 1) == (name == "call")


def test_evaluate_dataset_numpy_path(capsys):
    z = load_case("b0")
    cfg = z["cfg"]
    ds = C.EvalDataset(image_names=[str(x) for x in z["raw"]["image_names"]], labels=z["labels"], global_vectors=z["gv"],
                       lesion_vectors=z["maps"])
    out = C.evaluate_dataset(ds, z["targets"], kappas=cfg["kappas"], classification_k=cfg["cls_k"], rerank_topk=cfg["topk"],
                             global_weight=cfg["weight"])
    assert C.evaluate_dataset.last_native is False
    ranks, stats = _numpy_path(z)
    reps = [C.evaluate_rankings(r, z["labels"], cfg["kappas"], cfg["cls_k"]) for r in ranks]
    assert out["stage1"] == reps[0] and out["adaptive"] == (reps[1], stats[0])
    assert out["lesions"] == [(t, reps[2 + i], stats[1 + i]) for i, t in enumerate(z["targets"])]
    assert out["summary"]["mean_mAP"] == float(np.mean([r["mAP"] for r in reps[2:]]))
    assert out["summary"]["mean_R@1"] == float(np.mean([r["R@K"][1] for r in reps[2:]]))
    assert out["summary"]["mean_R@5"] == float(np.mean([r["R@K"][5] for r in reps[2:]]))
    assert [r["fallback"] for r in out["summary"]["per_lesion"]] == [s["queries_fallback_global"] for s in stats[1:]]
    for w in (-0.1, 1.5):
        with pytest.raises(ValueError, match="global-weight must be in"):
            C.evaluate_dataset(ds, z["targets"], global_weight=w)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        C.print_stage_report("Stage 1 - Global Retrieval", z["ref_reports"][0], cfg["kappas"], [1])
    rep = z["ref_reports"][0]
    m = rep["classification"][1]
    assert buf.getvalue() == (
        "\n=== Stage 1 - Global Retrieval ===\n"
        + ", ".join(f"R@{k}: {rep['R@K'][k]:.2f}%" for k in cfg["kappas"]) + "\n" + f"mAP: {rep['mAP']:.2f}%\n"
        + ", ".join(f"P@{k}: {rep['mP@K'][k]:.2f}%" for k in cfg["kappas"]) + "\n"
        + f"Top-1: Acc {m['accuracy']:.2f}% | P_macro {m['precision_macro']:.2f}% | R_macro {m['recall_macro']:.2f}% | "
        f"F1_macro {m['f1_macro']:.2f}%\n")


def test_region_store_is_a_csr_in_stored_order():
    z = load_case("d")
    st = C.RegionStore(z["maps"])
    assert st.dr == z["cfg"]["dr"] and st.row_ptr[-1] == st.lesion.shape[0] == st.vectors.shape[0]
    for i, m in enumerate(z["maps"]):
        a = int(st.row_ptr[i])
        for name, cands in m.items():
            lid = st.lesion_id(name)
            assert st.first[i][lid] == a and np.array_equal(st.vectors[a], cands[0])
            assert list(st.lesion[a:a + len(cands)]) == [lid] * len(cands)
            a += len(cands)
        assert a == st.row_ptr[i + 1]
    ragged = [{"edema": [np.ones(3, dtype=np.float32)]}, {"edema": [np.ones(4, dtype=np.float32)]}]
    assert C.RegionStore(ragged).dr is None and C.RegionStore([{}, {}]).vectors.shape == (0, 1)
