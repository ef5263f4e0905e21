"""Scalar filter expressions: the `expr` of pymilvus' collection.search / collection.query, evaluated on the host columns.

The language is a whitelist walk over `ast.parse(text, mode="eval")` -- nothing is ever handed to eval():

    field == literal    field != literal    field < <= > >= literal
    field in [literal, ..]                  field not in [literal, ..]
    a and b             a or b              not a               ( .. )

`field` is `id` or a scalar field of the collection's schema; a literal is a string or a number (a sign in front of a number is
part of it).  Everything else -- unknown names, calls, attributes, subscripts, arithmetic, chained comparisons, `like`, a
literal whose type is not that of the column's values -- is a ValueError that names these forms.

Evaluation is vectorised: a comparison on a scalar column is decided once per DISTINCT value and broadcast through the column's
dictionary codes (built once per collection state, ExprCache); comparisons on `id` run on the id array.  The result is a bool
array aligned with Collection.live_ids(), i.e. with the row order of the resident index: the mask of FlatIndex.search(allow=).
"""
import ast
import operator

import numpy as np

FORMS = ("the supported forms are: <field> ==|!=|<|<=|>|>= <literal>, <field> in [..], <field> not in [..], "
         "combined with and / or / not and parentheses; <field> is id or a scalar field of the schema, "
         "a literal is a string or a number")

_CMP = {ast.Eq: operator.eq, ast.NotEq: operator.ne, ast.Lt: operator.lt, ast.LtE: operator.le, ast.Gt: operator.gt,
        ast.GtE: operator.ge}


def _bad(text, why):
    return ValueError(f"expr {text!r}: {why}; {FORMS}")


def _literal(node, text):
    """the value of a string / number literal node (with an optional sign), else ValueError"""
    if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)) and isinstance(node.operand, ast.Constant):
        v = node.operand.value
        if type(v) in (int, float):
            return -v if isinstance(node.op, ast.USub) else v
    if isinstance(node, ast.Constant) and type(node.value) in (int, float, str):
        return node.value
    raise _bad(text, f"{ast.unparse(node)!r} is not a string or number literal")


def parse(text, fields):
    """-> the checked expression as nested tuples: ("and" | "or", [terms]), ("not", term), ("cmp", field, op, literal),
    ("in", field, [literals], negated).  `fields` = the names a comparison may use.  ValueError for anything outside the language."""
    if not isinstance(text, str):
        raise ValueError(f"expr: the expression must be a string, got {type(text).__name__}")
    if not text.strip():
        raise ValueError(f"expr: empty expression; {FORMS}")
    try:
        tree = ast.parse(text.strip(), mode="eval")
    except (SyntaxError, ValueError, MemoryError, RecursionError):
        raise _bad(text, "cannot parse") from None

    def field_of(node):
        if not isinstance(node, ast.Name):
            raise _bad(text, f"the left-hand side {ast.unparse(node)!r} is not a field name")
        if node.id not in fields:
            raise _bad(text, f"unknown field {node.id!r} (fields: {', '.join(fields)})")
        return node.id

    def walk(node):
        if isinstance(node, ast.BoolOp):
            return ("and" if isinstance(node.op, ast.And) else "or", [walk(v) for v in node.values])
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.Not):
            return ("not", walk(node.operand))
        if isinstance(node, ast.Compare):
            if len(node.ops) != 1:
                raise _bad(text, "chained comparisons are not supported")
            op, rhs = node.ops[0], node.comparators[0]
            name = field_of(node.left)
            if isinstance(op, (ast.In, ast.NotIn)):
                if not isinstance(rhs, ast.List):
                    raise _bad(text, f"`{name} in` needs a [..] list")
                return ("in", name, [_literal(e, text) for e in rhs.elts], isinstance(op, ast.NotIn))
            if type(op) not in _CMP:
                raise _bad(text, f"operator {type(op).__name__} is not supported")
            return ("cmp", name, _CMP[type(op)], _literal(rhs, text))
        raise _bad(text, f"{ast.unparse(node)!r} is not a comparison")

    try:
        return walk(tree.body)
    except RecursionError:
        raise _bad(text, "nested too deeply") from None


def _kind(v):
    """'str', 'num' or None (bool is neither: pymilvus keeps booleans apart from integers)"""
    if isinstance(v, str):
        return "str"
    if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)):
        return "num"
    return None


class ExprCache:
    """What the expression layer keeps for ONE state of a collection (the collection drops it with every change): the
    dictionary codes of each column it has met, and the mask of the last expression -- on the host and, once a search has
    used it, on the index's device."""

    def __init__(self, ids, column):
        self.ids = ids                    # live ids, numpy int64
        self._column = column             # name -> the field's values for the live rows
        self.codes = {}                   # name -> (distinct values, int64 code per live row)
        self.text = None
        self.mask = None
        self.device_mask = None
        self.device_codes = {}            # name -> the column's codes on the index's device (grouping search); (name, "int32") ->
                                          # the same as int32 (leave-group-out search)
        self.tables = {}                  # name -> ({value: code}, rows per code) (leave-group-out search)

    def _coded(self, name):
        got = self.codes.get(name)
        if got is None:
            table = {}
            values = self._column(name)
            codes = np.fromiter((table.setdefault(v, len(table)) for v in values), dtype=np.int64, count=len(values))
            got = self.codes[name] = (list(table), codes)
        return got

    def table(self, name):
        """({value: code}, numpy int64 rows per code) of column `name`"""
        got = self.tables.get(name)
        if got is None:
            distinct, codes = self._coded(name)
            got = self.tables[name] = ({v: j for j, v in enumerate(distinct)}, np.bincount(codes, minlength=len(distinct)))
        return got

    def _compare(self, text, name, test, literals):
        """test(value) per distinct value of column `name` (or per id), broadcast to the live rows"""
        if name == "id":
            for v in literals:
                if type(v) is not int:
                    raise _bad(text, f"id takes integers, got {v!r}")
                if not -2 ** 63 <= v < 2 ** 63:
                    raise _bad(text, f"id takes 64-bit integers, got {v!r}")
            return None
        kinds = {_kind(v) for v in literals}
        distinct, codes = self._coded(name)
        truth = np.zeros(len(distinct), dtype=bool)
        for j, u in enumerate(distinct):
            if kinds - {_kind(u)}:
                raise _bad(text, f"type mismatch: {name} holds {type(u).__name__} values such as {u!r}, compared with "
                                 f"{', '.join(repr(v) for v in literals)}")
            truth[j] = test(u)
        return truth[codes] if len(distinct) else np.zeros(codes.shape[0], dtype=bool)

    def _eval(self, text, node):
        tag = node[0]
        if tag in ("and", "or"):
            parts = [self._eval(text, t) for t in node[1]]
            return np.logical_and.reduce(parts) if tag == "and" else np.logical_or.reduce(parts)
        if tag == "not":
            return ~self._eval(text, node[1])
        if tag == "cmp":
            _, name, op, lit = node
            out = self._compare(text, name, lambda u: bool(op(u, lit)), [lit])
            return op(self.ids, lit) if out is None else out
        _, name, lits, negated = node
        wanted = set(lits)
        out = self._compare(text, name, lambda u: u in wanted, lits)
        if out is None:
            out = np.isin(self.ids, np.asarray(lits, dtype=np.int64)) if lits else np.zeros(self.ids.shape[0], dtype=bool)
        return ~out if negated else out

    def evaluate(self, text, fields):
        """the bool mask of `text` over the live rows; the last expression's mask is kept and returned again as it is"""
        if not isinstance(text, str) or text != self.text:          # (anything but a string is parse()'s to reject)
            tree = parse(text, fields)
            try:
                mask = np.ascontiguousarray(self._eval(text, tree), dtype=bool)
            except RecursionError:
                raise _bad(text, "nested too deeply") from None
            mask.setflags(write=False)
            self.text, self.mask, self.device_mask = text, mask, None
        return self.mask
