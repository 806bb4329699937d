"""CASE and the conditional functions as values: the yardstick of tests/test_cond_cpu.py and tests/test_gpu_cond.py.

A Python restatement, over json.loads-style values, of
  * SearchedCase.Evaluate (expression/case_searched.go:73-100) and SimpleCase.Evaluate (case_simple.go:78-110),
  * IfMissing / IfNull / IfMissingOrNull.Apply (func_cond_unknown.go:61-69, 132-140, 209-217),
  * NullIf / MissingIf.Apply (func_cond_unknown.go:278-290, 347-359),
with MISSING, Equals, Compare and the 4-valued AND / OR of tests/coll_util.py; the writers of the expression.Stringer text of
such expressions; a small table with every value class in its columns; and a seeded generator of conditional expressions
over that table.

Expressions (values):   ("col", name) | ("const", v) | ("arith", "+" | "-" | "*", x, y)
                        | ("case", [(cond, value), ...], else or None) | ("simple", search, [(when, value), ...], else or None)
                        | ("fn", name, [values])
Conditions:             ("cmp", "=" | "<" | "<=", x, y) | ("between", x, lo, hi) | ("is", x, kind) | ("and" | "or", [conds])
                        | ("not", cond) | ("truth", value)
"""
import json
import random

import numpy as np

import coll_util as cu
from oracle import n1o
from query_amd import plan

MISSING = cu.MISSING
FUNCTIONS = ("ifmissing", "ifnull", "ifmissingornull", "nullif", "missingif")


# ---------------------------------------------------------------- the mirror

def _is_num(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def equals(a, b):
    """X.Equals(Y) in four values; two arrays / objects are equal when their canonical texts are."""
    if a is MISSING or b is MISSING:
        return MISSING
    if a is None or b is None:
        return None
    if cu._cls(a) != cu._cls(b):
        return False
    if isinstance(a, (list, dict)):
        return cu.canon(a) == cu.canon(b)
    return cu._collate(a, b) == 0


def truth(v):
    """What a bare value is as a condition (TERM_TRUTH): MISSING and NULL stay, else Truth() (value/*.go)."""
    if v is MISSING or v is None or isinstance(v, bool):
        return v
    if _is_num(v):
        return v == v and v != 0
    return len(v) > 0


def arith(op, x, y):
    """Add / Sub / Mult.Apply (expression/arith_add.go:51-70): MISSING first, then NULL for a non-number."""
    if x is MISSING or y is MISSING:
        return MISSING
    if not _is_num(x) or not _is_num(y):
        return None
    r = x + y if op == "+" else (x - y if op == "-" else x * y)
    return cu.norm(r)


def eval_cond(c, row):
    k = c[0]
    if k == "cmp":
        a, b = eval_value(c[2], row), eval_value(c[3], row)
        if c[1] == "=":
            return equals(a, b)
        r = cu._compare(a, b)
        if r is MISSING or r is None:
            return r
        return r < 0 if c[1] == "<" else r <= 0
    if k == "between":
        a = eval_value(c[1], row)
        lo, hi = cu._compare(a, eval_value(c[2], row)), cu._compare(a, eval_value(c[3], row))
        if lo is MISSING or hi is MISSING:
            return MISSING
        if lo is None or hi is None:
            return None
        return lo >= 0 and hi <= 0
    if k == "is":
        v = eval_value(c[1], row)
        kind = c[2]
        if kind == "missing":
            return v is MISSING
        if kind == "not missing":
            return v is not MISSING
        if kind == "valued":
            return v is not MISSING and v is not None
        if kind == "not valued":
            return v is MISSING or v is None
        if v is MISSING:
            return MISSING
        return (v is None) == (kind == "null")
    if k == "and":
        return cu._and([eval_cond(x, row) for x in c[1]])
    if k == "or":
        return cu._or([eval_cond(x, row) for x in c[1]])
    if k == "not":
        v = eval_cond(c[1], row)
        return v if (v is MISSING or v is None) else (not v)
    assert k == "truth", c
    return truth(eval_value(c[1], row))


def cond_fn_apply(name, args):
    """The five functions over evaluated arguments."""
    if name == "ifmissing":
        return next((a for a in args if a is not MISSING), None)
    if name == "ifnull":
        return next((a for a in args if a is not None), None)  # (a MISSING argument IS returned)
    if name == "ifmissingornull":
        return next((a for a in args if a is not MISSING and a is not None), None)
    assert name in ("nullif", "missingif") and len(args) == 2
    eq = equals(args[0], args[1])
    if eq is MISSING or eq is None:
        return eq
    if eq:
        return None if name == "nullif" else MISSING
    return args[0]


def eval_value(e, row):
    k = e[0]
    if k == "col":
        return row[e[1]]
    if k == "const":
        return e[1]
    if k == "arith":
        return arith(e[1], eval_value(e[2], row), eval_value(e[3], row))
    if k == "case":
        for cond, val in e[1]:
            if eval_cond(cond, row) is True:
                return eval_value(val, row)
        return None if e[2] is None else eval_value(e[2], row)
    if k == "simple":
        s = eval_value(e[1], row)
        for when, val in e[2]:
            if equals(s, eval_value(when, row)) is True:
                return eval_value(val, row)
        return None if e[3] is None else eval_value(e[3], row)
    assert k == "fn", e
    return cond_fn_apply(e[1], [eval_value(a, row) for a in e[2]])


# ---------------------------------------------------------------- text

def D(name):
    return plan.field_path("default", name)


def value_text(e, col=D):
    k = e[0]
    if k == "col":
        return col(e[1])
    if k == "const":
        return "missing" if e[1] is MISSING else json.dumps(e[1], ensure_ascii=False)
    if k == "arith":
        return "(%s %s %s)" % (value_text(e[2], col), e[1], value_text(e[3], col))
    if k == "case":
        return plan.case_when([(cond_text(c, col), value_text(v, col)) for c, v in e[1]], None if e[2] is None else value_text(e[2], col))
    if k == "simple":
        return plan.case_of(value_text(e[1], col), [(value_text(w, col), value_text(v, col)) for w, v in e[2]],
                            None if e[3] is None else value_text(e[3], col))
    return plan.cond_fn(e[1], *[value_text(a, col) for a in e[2]])


def cond_text(c, col=D):
    k = c[0]
    if k == "cmp":
        return "(%s %s %s)" % (value_text(c[2], col), c[1], value_text(c[3], col))
    if k == "between":
        return "(%s between %s and %s)" % tuple(value_text(x, col) for x in c[1:4])
    if k == "is":
        return "(%s is %s)" % (value_text(c[1], col), c[2])
    if k in ("and", "or"):
        return "(%s)" % (" %s " % k).join(cond_text(x, col) for x in c[1])
    if k == "not":
        return "(not %s)" % cond_text(c[1], col)
    return value_text(c[1], col)


def columns_of(e, out=None):
    """column names in first-use text order"""
    out = [] if out is None else out
    if isinstance(e, tuple) and not isinstance(e[0], str):  # an arm: (condition, value)
        for x in e:
            columns_of(x, out)
    elif isinstance(e, tuple):
        if e[0] == "col":
            if e[1] not in out:
                out.append(e[1])
        elif e[0] != "const":
            for x in e[1:]:
                columns_of(x, out)
    elif isinstance(e, list):
        for x in e:
            columns_of(x, out)
    return out


# ---------------------------------------------------------------- the table

WORDS = ["", "a", "ab", "b", "t_1", "é", "low", "mid", "high", "cat_1", "cat_2", "cat_3", "zz"]
KEY0 = WORDS.index("cat_1")
ARRAYS = [[], ["a"], [1, 2], [{"f": 1}]]
OBJECTS = [{}, {"f": 1}]
DICT = [w.encode() for w in WORDS] + [cu.canon(v).encode() for v in ARRAYS + OBJECTS]
CODE = {bytes(b): i for i, b in enumerate(DICT)}


def to_tagged(values):
    """mirror values -> (tags, payload) of a TAGGED64 column over DICT"""
    n = len(values)
    tags, pay = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    for i, v in enumerate(values):
        if v is MISSING:
            tags[i] = n1o.T_MISSING
        elif v is None:
            tags[i] = n1o.T_NULL
        elif isinstance(v, bool):
            tags[i] = n1o.T_TRUE if v else n1o.T_FALSE
        elif isinstance(v, int):
            tags[i] = n1o.T_INT
            pay[i] = np.int64(v).view(np.uint64)
        elif isinstance(v, float):
            tags[i] = n1o.T_FLOAT
            pay[i] = np.float64(v).view(np.uint64)
        elif isinstance(v, str):
            tags[i] = n1o.T_STRING
            pay[i] = CODE[v.encode()]
        else:
            tags[i] = n1o.T_ARRAY if isinstance(v, list) else n1o.T_OBJECT
            pay[i] = CODE[cu.canon(v).encode()]
    return tags, pay


A_POOL = [MISSING, None, True, False, 0, 1, 3, 7, 2.5, 0.5, 3.0, 7.0, "a", "ab", "t_1", "", "cat_1"] + ARRAYS + OBJECTS


def make_rows(rng, n):
    """n rows as dicts of mirror values.  a: every value class (integral floats among them); x: numbers, never integral as
    floats (k / 8 + 1 / 16), some NULL / MISSING; s: strings with NULL / MISSING; k: the key strings; g: small ints."""
    rows = []
    for _ in range(n):
        r = rng.random()
        x = MISSING if r < 0.04 else (None if r < 0.08 else (rng.randrange(0, 100) if r < 0.4 else rng.randrange(0, 800) / 8.0 + 0.0625))
        r = rng.random()
        s = MISSING if r < 0.06 else (None if r < 0.12 else rng.choice(WORDS[:KEY0]))
        r = rng.random()
        k = MISSING if r < 0.03 else (None if r < 0.07 else rng.choice(WORDS[KEY0:]))
        rows.append({"a": rng.choice(A_POOL), "x": x, "s": s, "k": k, "g": rng.randrange(0, 7)})
    return rows


def dict_codes(values):
    return np.array([0xFFFFFFFF if v is MISSING else (0xFFFFFFFE if v is None else CODE[v.encode()]) for v in values], np.uint32)


def make_table(rows):
    """the rows as an oracle / device table: a, x, g TAGGED64; s, k DICT32"""
    cols = []
    for name in ("a", "x", "g"):
        t, p = to_tagged([r[name] for r in rows])
        cols.append(n1o.Column(D(name), n1o.COL_TAGGED64, tags=t, payload=p))
    for name in ("s", "k"):
        cols.append(n1o.Column(D(name), n1o.COL_DICT32, codes=dict_codes([r[name] for r in rows])))
    return n1o.Table(cols, list(DICT))


def helper_column(name, values):
    t, p = to_tagged(values)
    return n1o.Column(D(name), n1o.COL_TAGGED64, tags=t, payload=p)


# ---------------------------------------------------------------- the generator
#
# What it draws stays inside what the device takes and what the mirror states: arithmetic over x and g only (results never
# integral floats), no negative constants (the stringer writes them as a negation), arrays / objects ordered or compared only
# against scalars (type order decides; two of them under < raise N1K_UNSUPPORTED_DATA), numbers small enough to stay exact.

NUM_CONSTS = [0, 1, 3, 7, 50, 2.5, 40.5]
STR_CONSTS = ["a", "ab", "t_1", "", "low", "mid", "high", "cat_1", "cat_2"]


def rand_number(rng, depth=0):
    r = rng.random()
    if r < 0.35:
        return ("col", "x")
    if r < 0.55:
        return ("col", "g")
    if r < 0.75 or depth >= 1:
        return ("const", rng.choice(NUM_CONSTS))
    return ("arith", rng.choice("+-*"), rand_number(rng, depth + 1), ("const", rng.choice([1, 2, 3])) if rng.random() < 0.5 else ("col", "g"))


def rand_scalar_value(rng, depth=0, numeric=False):
    """a value that is a number, a string, NULL or MISSING (an aggregate's operand, a THEN)"""
    r = rng.random()
    if numeric or r < 0.5:
        return rand_number(rng, depth)
    if r < 0.7:
        return ("col", rng.choice(["s", "k"]))
    if r < 0.9:
        return ("const", rng.choice(STR_CONSTS))
    return ("const", rng.choice([None, MISSING, True]))


def rand_cond(rng, depth=0):
    r = rng.random()
    if depth < 2 and r < 0.2:
        return (rng.choice(["and", "or"]), [rand_cond(rng, depth + 1) for _ in range(rng.randint(2, 3))])
    if depth < 2 and r < 0.27:
        return ("not", rand_cond(rng, depth + 1))
    if r < 0.5:
        a, b = rand_number(rng), ("const", rng.choice(NUM_CONSTS))
        return ("cmp", rng.choice(["=", "<", "<="]), a, b) if rng.random() < 0.7 else ("cmp", rng.choice(["<", "<="]), b, a)
    if r < 0.62:
        return ("cmp", rng.choice(["=", "<", "<="]), ("col", rng.choice(["s", "k", "a"])), ("const", rng.choice(STR_CONSTS + [3, 2.5])))
    if r < 0.7:
        return ("cmp", rng.choice(["=", "<"]), ("col", "x"), ("col", "g"))
    if r < 0.85:
        return ("is", ("col", rng.choice(["a", "x", "s"])), rng.choice(["null", "not null", "missing", "not missing", "valued", "not valued"]))
    if r < 0.92:
        return ("between", ("col", rng.choice(["x", "g"])), ("const", rng.choice([0, 1, 3])), ("const", rng.choice([7, 40.5, 50])))
    return ("truth", ("col", "a"))


def rand_node(rng, depth=0, scalar=False, numeric=False):
    """one conditional expression.  scalar: its values are numbers / strings / NULL / MISSING; numeric: numbers where it can."""
    def val(d=depth + 1):
        if d < 2 and rng.random() < 0.2:
            return rand_node(rng, d, scalar, numeric)
        if not scalar and rng.random() < 0.3:
            return ("col", "a")
        return rand_scalar_value(rng, d, numeric)

    r = rng.random()
    if r < 0.4:
        arms = [(rand_cond(rng), val()) for _ in range(rng.randint(1, 3))]
        return ("case", arms, val() if rng.random() < 0.6 else None)
    if r < 0.55:
        search = ("col", rng.choice(["g", "s", "a"] if not numeric else ["g"]))
        whens = [("const", rng.choice([0, 1, 3, 3.0, "a", "t_1", ""])) for _ in range(rng.randint(1, 3))]
        return ("simple", search, [(w, val()) for w in whens], val() if rng.random() < 0.6 else None)
    if r < 0.85:
        name = rng.choice(FUNCTIONS[:3])
        first = ("col", rng.choice(["x", "s", "a"] if not scalar else ["x", "s"])) if not numeric else ("col", "x")
        return ("fn", name, [first] + [val() for _ in range(rng.randint(1, 3))])
    name = rng.choice(FUNCTIONS[3:])
    first = ("col", rng.choice(["x", "g", "s"] + ([] if scalar else ["a"]))) if not numeric else ("col", rng.choice(["x", "g"]))
    return ("fn", name, [first, ("const", rng.choice([3, 3.0, 0, "a", "t_1"])) if rng.random() < 0.7 else ("col", "g")])


# how the differential uses the node: (use, aggregate)
USES = ["key", "sum", "avg", "min", "max", "count", "count_distinct", "filter_cmp", "filter_bare"]


def draw_plan(seed):
    """One plan of the differential: the rows, the device's and the oracle's (condition, keys, aggregates), the helper
    column's values.  The oracle reads the helper column `h` where the device evaluates the node."""
    rng = random.Random(880_000 + seed)
    rows = make_rows(rng, rng.randint(1, 1500))
    use = USES[seed % len(USES)]
    scalar = use != "key" and use != "filter_bare" and use != "count"
    node = rand_node(rng, 0, scalar=scalar, numeric=use in ("sum", "avg"))
    text, h = value_text(node), D("h")
    where = cond_text(rand_cond(rng)) if rng.random() < 0.5 else None
    dcond, ocond = where, where
    dkeys = okeys = [[D("k")], [D("g")], []][rng.randrange(3)]
    if use == "key":
        dkeys, okeys = [text] + dkeys[:1], [h] + okeys[:1]
        daggs = oaggs = sorted(["count(*)", "sum(%s)" % D("x")])
    elif use in ("filter_cmp", "filter_bare"):
        wrap = (lambda t: "(%s <= 3)" % t if seed % 2 else "(%s = %s)" % (t, D("g"))) if use == "filter_cmp" else (lambda t: t)
        extra = lambda t: wrap(t) if where is None else "(%s and %s)" % (where, wrap(t))  # noqa: E731
        dcond, ocond = extra(text), extra(h)
        daggs = oaggs = sorted(["count(*)", "max(%s)" % D("x")])
    else:
        f = "count(distinct %s)" if use == "count_distinct" else use + "(%s)"
        # (not sorted by text as the planner would: the two sides' texts differ inside the parentheses, and the results are
        #  compared aggregate by aggregate)
        daggs, oaggs = [f % text, "count(*)"], [f % h, "count(*)"]
    values = [eval_value(node, r) for r in rows]
    return {"rows": rows, "node": node, "use": use, "values": values, "device": (dcond, dkeys, daggs), "oracle": (ocond, okeys, oaggs)}
