"""Filter expressions (mirx.expr) through Collection.query / Collection.expr_mask, without a GPU.

The oracle is this file's own: Python's eval of the expression against each row's dict (the library never calls eval; here it
is the independent restatement).  Collections: the default schema (image_path, label as integers) held in memory, and the NIH
schema (string fields only) -- about 200 rows each, some deleted, so that live_ids() is no longer the row number."""
import numpy as np
import pytest
import torch

N, DIM = 200, 8


def _rows(n, seed):
    return torch.randn(n, DIM, generator=torch.Generator().manual_seed(seed))


class _HostIndex:
    """stands where an in-memory collection keeps its FlatIndex, so that insert / delete run without a device: it only
    follows the ids, which is all the metadata layer asks of it"""

    def __init__(self):
        self.ids = []

    def add(self, rows, ids):
        self.ids.extend(int(i) for i in ids)

    def remove(self, ids):
        gone = {int(i) for i in ids} & set(self.ids)
        self.ids = [i for i in self.ids if i not in gone]
        return len(gone)


def _in_memory(*args, **kw):
    from mirx.retriever import Collection
    col = Collection(*args, **kw)
    col._index = _HostIndex()
    return col


def _default_collection():
    col = _in_memory("t", DIM, extra_fields=("source",))
    col.insert([[f"img/{i}.png" for i in range(N)], [i % 3 for i in range(N)], _rows(N, 1),
                [("site-a", "site-b", "site c")[(i // 7) % 3] for i in range(N)]])
    col.delete("id in [0, 5, 6, 77, 199]")
    col.delete('image_path == "img/100.png"')
    return col


def _nih_collection():
    col = _in_memory("nih", DIM, extra_fields=("image_name", "label_text", "label_vector_json"), has_label=False)
    names = ("No Finding", "Effusion", "Mass|Nodule", "COVID-19")
    col.insert([[f"images/{i:05d}.png" for i in range(N)], [f"{i:05d}.png" for i in range(N)],
                [names[(i * 7) % 4] for i in range(N)], ["[%d, %d]" % (i % 2, (i // 2) % 2) for i in range(N)], _rows(N, 2)])
    col.delete("id in [3, 4, 150]")
    return col


def _oracle_ids(col, expr):
    out = []
    for i in col.live_ids().tolist():
        row = dict(col.entity(i), id=i)
        if eval(expr, {"__builtins__": {}}, row):          # the test's own oracle, never the library's way
            out.append(i)
    return out


DEFAULT_EXPRS = [
    "label == 1", "label != 1", "label < 1", "label <= 1", "label > 1", "label >= 1", "label == 1.0", "label > 0.5",
    "label in [0, 2]", "label not in [0, 2]", "label in []", "label not in []", "label == 7",
    "id == 42", "id == 5", "id != 42", "id < 10", "id <= 10", "id > 190", "id >= 190", "id >= -3", "id < -1",
    "id in [1, 2, 5, 77, 78, 1000, 2]", "id not in [1, 2, 3]",
    'source == "site-a"', 'source != "site c"', 'source in ["site-a", "site c"]', 'source not in ["site-b"]',
    'source < "site-b"', 'source >= "site-a"',
    'image_path == "img/17.png"', 'image_path in ["img/17.png", "img/0.png", "nope"]',
    "label == 1 and id < 100", "label == 1 or id < 10", "not label == 1", "not (label == 1 or id >= 50)",
    '(label == 0 and source == "site-a") or (label == 2 and not id in [2, 8, 11])',
    'label == 0 and label == 1', 'not (not (id > 20 and id <= 30)) and label != 2 and source != "site-b"',
    "id >= 0",
]

NIH_EXPRS = [
    'label_text == "COVID-19"', 'label_text != "No Finding"', 'label_text in ["Effusion", "Mass|Nodule"]',
    'label_text not in ["Effusion"] and id >= 100', 'image_name == "00017.png" or image_name == "00003.png"',
    'label_vector_json == "[1, 0]"', 'not label_text == "COVID-19" and (id < 20 or id > 180)',
    'image_name >= "00150.png"',
]


@pytest.fixture(scope="module")
def default_col():
    return _default_collection()


@pytest.fixture(scope="module")
def nih_col():
    return _nih_collection()


def _check(col, expr):
    want = _oracle_ids(col, expr)
    mask = col.expr_mask(expr)
    assert mask.dtype == np.bool_ and mask.shape == col.live_ids().shape          # aligned with live_ids()
    assert col.live_ids()[mask].tolist() == want, expr
    got = col.query(expr, ["image_path"])
    assert [r["id"] for r in got] == want, expr
    assert all(r["image_path"] == col.entity(r["id"])["image_path"] for r in got)
    assert [r["id"] for r in col.query(expr, limit=3, offset=2)] == want[2:5]


@pytest.mark.parametrize("expr", DEFAULT_EXPRS)
def test_default_schema_expressions(default_col, expr):
    _check(default_col, expr)


@pytest.mark.parametrize("expr", NIH_EXPRS)
def test_nih_schema_expressions(nih_col, expr):
    _check(nih_col, expr)


def test_some_expressions_select_something(default_col, nih_col):
    """the oracle comparison above is not a comparison of empty lists"""
    assert 50 < len(default_col.query("label == 1")) < 80
    assert len(default_col.query('(label == 0 and source == "site-a") or (label == 2 and not id in [2, 8, 11])')) > 20
    assert len(nih_col.query('label_text == "COVID-19"')) > 30
    assert default_col.query("id == 5") == [] and default_col.query("id == 42") == [{"id": 42}]


@pytest.mark.parametrize("expr, message", [
    ("colour == 1", "unknown field 'colour'"),
    ("embedding == 1", "unknown field 'embedding'"),
    ('__import__("os").system("true") == 0', "not a field name"),
    ('id in [__import__("os")]', "not a string or number literal"),
    ("label.real == 1", "not a field name"),
    ("label[0] == 1", "not a field name"),
    ("label + 1 == 2", "not a field name"),
    ("label == 1 + 1", "not a string or number literal"),
    ("0 < label < 2", "chained comparisons"),
    ('image_path like "img/1%"', "cannot parse"),
    ('label == "1"', "type mismatch"),
    ('source == 3', "type mismatch"),
    ('source in ["site-a", 3]', "type mismatch"),
    ("label == True", "not a string or number literal"),
    ("id == 2.5", "id takes integers"),
    ('id == "7"', "id takes integers"),
    ("id in (1, 2)", r"needs a \[..\] list"),
    ("label is 1", "not supported"),
    ("label", "not a comparison"),
    ("label == 1 if id else 2", "not a comparison"),
    ("", "empty expression"),
    ("   ", "empty expression"),
])
def test_rejections_name_the_supported_forms(default_col, expr, message):
    with pytest.raises(ValueError, match=message) as e:
        default_col.query(expr)
    assert "supported forms" in str(e.value)
    with pytest.raises(ValueError, match=message):
        default_col.expr_mask(expr)


def test_expression_must_be_a_string():
    for bad in (None, 3, ["label == 1"]):
        col = _default_collection()                        # a fresh collection each time: no expression evaluated before
        with pytest.raises(ValueError, match="must be a string"):
            col.expr_mask(bad)
        with pytest.raises(ValueError, match="must be a string"):
            _default_collection().query(bad)
        col.expr_mask("label == 1")
        with pytest.raises(ValueError, match="must be a string"):
            col.query(bad)


def test_deep_nesting_and_huge_ids_are_value_errors(default_col):
    for expr in ("not " * 3000 + "label == 1", "(" * 3000 + "label == 1" + ")" * 3000):
        with pytest.raises(ValueError, match="supported forms"):
            default_col.expr_mask(expr)
    for expr in ("id == 1000000000000000000000000000000", "id in [1, 1000000000000000000000000000000]",
                 "id < -1000000000000000000000000000000"):
        with pytest.raises(ValueError, match="64-bit integers"):
            default_col.expr_mask(expr)
    assert default_col.query("id == 9223372036854775807") == []


def test_library_never_evals():
    import os
    import mirx.expr
    src = open(os.path.join(os.path.dirname(mirx.expr.__file__), "expr.py")).read()
    import ast
    calls = [n.func.id for n in ast.walk(ast.parse(src)) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)]
    assert "eval" not in calls and "exec" not in calls and "compile" not in calls


def test_mask_cache_is_reused_and_rebuilt():
    col = _default_collection()
    m1 = col.expr_mask("label == 1")
    cache = col._expr
    assert col.expr_mask("label == 1") is m1 and col._expr is cache          # same expression, same collection: reused
    codes = cache.codes["label"]
    m2 = col.expr_mask("label == 2 and id > 3")
    assert col._expr is cache and cache.codes["label"] is codes               # another expression: the codes are reused
    assert m2 is not m1 and not m1.flags.writeable
    before = m2.shape[0]
    col.insert([["img/new.png"], [2], _rows(1, 9), ["site-a"]])
    m3 = col.expr_mask("label == 2 and id > 3")
    assert col._expr is not cache and m3.shape[0] == before + 1 and bool(m3[-1])   # rebuilt after insert
    cache = col._expr
    col.delete("id == 200")
    m4 = col.expr_mask("label == 2 and id > 3")
    assert col._expr is not cache and m4.shape[0] == before                  # rebuilt after delete
    assert col.live_ids()[m4].tolist() == _oracle_ids(col, "label == 2 and id > 3")
    assert col._index.ids == col.live_ids().tolist()                         # the mask is in the index's row order
    cache = col._expr
    col.compact()
    assert col.live_ids()[col.expr_mask("label == 2 and id > 3")].tolist() == _oracle_ids(col, "label == 2 and id > 3")
    assert col._expr is not cache


def test_persistent_collection_answers_without_a_gpu(tmp_path):
    from mirx.retriever import MilvusManager
    uri = str(tmp_path / "db")
    col = MilvusManager(uri=uri).create_collection("dinov2")
    col.insert([[f"img/{i}.png" for i in range(30)], [i % 3 for i in range(30)], torch.randn(30, 512)])
    col.delete("id in [1, 4]")
    col.flush()
    again = MilvusManager(uri=uri).create_collection("dinov2")
    assert again._index is None                                               # nothing resident, no device touched
    want = [i for i in range(30) if i % 3 == 1 and i not in (1, 4) and i < 20]
    assert [r["id"] for r in again.query("label == 1 and id < 20", ["label"])] == want
    assert all(r["label"] == 1 for r in again.query("label == 1 and id < 20", ["label"]))
    assert again._index is None
