"""The numeric library functions as values: the yardstick of tests/test_mathfn_cpu.py and tests/test_gpu_mathfn.py.

A Python restatement, over json.loads-style values (MISSING is tests/cond_util.MISSING), of
  * Acos ... Tan, Exp, Ln (math.Log), Log (math.Log10), Degrees, Radians, Atan2, Power .Apply (expression/func_num.go): any
    MISSING argument gives MISSING, else any non-number NULL, else the arguments go through float64 and the result through
    value.NewValue (an integral result folds to INT);
  * IfInf / IfNaN / IfNaNOrInf.Apply (func_cond_num.go:64-79 and siblings) and NaNIf / PosInfIf / NegInfIf.Apply (:293-305);
  * pi() e() nan() posinf() neginf().
The functions are numpy float64 under np.errstate(all="ignore"): plain `math` raises on domain errors where Go returns NaN or
an infinity.  numpy's routines are the C library's; the device's are its own — both within a few ulp of the true value and not
bit-identical, so a library function's result is compared as a NUMBER within 1e-9 relative (the project's float tolerance),
whatever its INT / FLOAT tag; everything else — propagation, constants, DEGREES / RADIANS, the conditionals, NaN and
infinities, results the yardstick gives as exactly 0 — is compared exactly.

Expressions:  ("col", name) | ("const", v) | ("arith", "+" | "-" | "*" | "/", x, y) | ("num", name, [args])
              | ("cond", name, [args])        ifmissing ... neginfif (tests/cond_util.py's five and the three new ones)
              | ("case", [(("cmp", "<" | "<=" | "=", x, y), value), ...], else or None)
"""
import json
import math
import os
import random

import numpy as np

import cond_util as cn
import coll_util as cu
import golden_util as gu
from query_amd import plan

MISSING = cn.MISSING
REL_TOL = 1e-9
NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")

UNARY = ("acos", "asin", "atan", "cos", "sin", "tan", "exp", "ln", "log", "degrees", "radians")
BINARY = ("atan2", "power")
NULLARY = {"pi": math.pi, "e": math.e, "nan": NAN, "posinf": PINF, "neginf": NINF}
IFNUM = ("ifinf", "ifnan", "ifnanorinf")
EQNUM = {"nanif": NAN, "posinfif": PINF, "neginfif": NINF}
LIBRARY = ("acos", "asin", "atan", "atan2", "cos", "sin", "tan", "exp", "ln", "log", "power")  # compared as numbers
EXACT = ("degrees", "radians") + IFNUM + tuple(EQNUM) + tuple(NULLARY)                          # compared exactly


def nan_first(values):
    """ascending, NaN first (collateFloat, value/float.go:123-172): the order of SELECT f(x) AS v ... ORDER BY v"""
    return sorted(values, key=lambda v: (0, 0) if v != v else (1, v))


def load_cases():
    """tests/golden/cases_num.json.  Where the reference's result is the STRING "NaN" (value/float.go:31-48 marshals a NaN
    as a JSON string; acos(3), asin(10)) the expected value is FLOAT NaN: same_value takes either spelling from the device."""
    with open(os.path.join(gu.GOLDEN, "cases_num.json")) as fh:
        return json.load(fh)["cases"]


# ---------------------------------------------------------------- the yardstick

def is_num(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def new_value(f):
    """value.NewValue(float64): an integral value inside int64 IS the int (value/value.go:377-382); -0.0 is 0"""
    f = float(f)
    if f != f or f in (PINF, NINF):
        return f
    return int(f) if f == math.floor(f) and -2.0 ** 63 <= f < 2.0 ** 63 else f


_NP = {"acos": np.arccos, "asin": np.arcsin, "atan": np.arctan, "cos": np.cos, "sin": np.sin, "tan": np.tan, "exp": np.exp,
       "ln": np.log, "log": np.log10, "atan2": np.arctan2, "power": np.power}


def fn_float(name, *xs):
    """the function itself over float64 arguments"""
    xs = [np.float64(x) for x in xs]
    with np.errstate(all="ignore"):
        if name == "degrees":
            return float(xs[0] * np.float64(180.0) / np.float64(math.pi))  # (func_num.go:427-434: in this order)
        if name == "radians":
            return float(xs[0] * np.float64(math.pi) / np.float64(180.0))
        return float(_NP[name](*xs))


def fn_apply(name, args):
    """one function over evaluated arguments"""
    if name in NULLARY:
        assert not args
        return NULLARY[name]
    if name in IFNUM:
        for a in args:
            if a is MISSING:
                return MISSING
            if not is_num(a):
                return None
            f = float(a)
            bad = math.isinf(f) if name == "ifinf" else (f != f if name == "ifnan" else (f != f or math.isinf(f)))
            if not bad:
                return new_value(f)
        return None
    assert len(args) == (2 if name in BINARY else 1), (name, args)
    if any(a is MISSING for a in args):
        return MISSING
    if not all(is_num(a) for a in args):
        return None
    return new_value(fn_float(name, *[float(a) for a in args]))


def cond_apply(name, args):
    if name in EQNUM:
        eq = cn.equals(args[0], args[1])
        if is_num(args[0]) and is_num(args[1]) and (args[0] != args[0] or args[1] != args[1]):
            eq = False  # (floatValue.Equals is ==: a NaN equals nothing, itself included)
        if eq is MISSING or eq is None:
            return eq
        return EQNUM[name] if eq else args[0]
    return cn.cond_fn_apply(name, args)


def arith(op, x, y):
    if op != "/":
        return cn.arith(op, x, y)
    if x is MISSING or y is MISSING:  # Div.Apply (arith_div.go:46-64): a zero or non-number divisor is NULL
        return MISSING
    if not is_num(y) or y == 0 or not is_num(x):
        return None
    return new_value(float(x) / float(y))


def eval_cmp(c, row):
    _k, op, x, y = c
    a, b = eval_value(x, row), eval_value(y, row)
    if op == "=":
        return cn.equals(a, b)
    r = cu._compare(a, b)
    if r is MISSING or r is None:
        return r
    return r < 0 if op == "<" else r <= 0


def eval_value(e, row):
    k = e[0]
    if k == "col":
        return row[e[1]]
    if k == "const":
        return e[1]
    if k == "arith":
        return arith(e[1], eval_value(e[2], row), eval_value(e[3], row))
    if k == "num":
        return fn_apply(e[1], [eval_value(a, row) for a in e[2]])
    if k == "cond":
        return cond_apply(e[1], [eval_value(a, row) for a in e[2]])
    assert k == "case", e
    for cond, val in e[1]:
        if eval_cmp(cond, row) is True:
            return eval_value(val, row)
    return None if e[2] is None else eval_value(e[2], row)


# ---------------------------------------------------------------- text

D = cn.D


def value_text(e, col=D):
    k = e[0]
    if k == "col":
        return col(e[1])
    if k == "const":
        return "missing" if e[1] is MISSING else json.dumps(e[1])
    if k == "arith":
        return "(%s %s %s)" % (value_text(e[2], col), e[1], value_text(e[3], col))
    if k == "num":
        return plan.num_fn(e[1], *[value_text(a, col) for a in e[2]])
    if k == "cond":
        return plan.cond_fn(e[1], *[value_text(a, col) for a in e[2]])
    arms = [("(%s %s %s)" % (value_text(c[2], col), c[1], value_text(c[3], col)), value_text(v, col)) for c, v in e[1]]
    return plan.case_when(arms, None if e[2] is None else value_text(e[2], col))


def columns_of(e, out=None):
    return cn.columns_of(e, out)


def uses_library(e):
    """does the expression hold one of the eleven library functions (its value then carries the float tolerance)?"""
    if isinstance(e, tuple):
        if e and e[0] == "num" and e[1] in LIBRARY:
            return True
        return any(uses_library(x) for x in e[1:])
    if isinstance(e, list):
        return any(uses_library(x) for x in e)
    return False


# ---------------------------------------------------------------- comparing

def as_number(v):
    """a decoded result as a float, NaN for either spelling of it ("NaN": a NaN that went through a group key or JSON)"""
    if isinstance(v, str) and v in ("NaN", "+Infinity", "-Infinity"):
        return {"NaN": NAN, "+Infinity": PINF, "-Infinity": NINF}[v]
    return float(v) if is_num(v) else None


def same_value(got, want, exact):
    """got: what the device gave; want: the yardstick's (or the reference's) value.  exact: the same value and — for
    numbers — the same INT / FLOAT kind (a zero too: NewValue folds 0.0 and -0.0 to INT 0).  Otherwise numbers agree within
    REL_TOL whatever their kind; NaN, the infinities and an expected 0 are exact values in both modes."""
    if want is MISSING or got is MISSING:
        return want is got
    g, w = as_number(got), as_number(want)
    if w is None or g is None:
        return type(got) is type(want) and got == want
    if w != w or g != g:
        return w != w and g != g
    if math.isinf(w) or math.isinf(g):
        return g == w
    if w == 0 and not exact:
        return g == 0
    if exact:
        return g == w and isinstance(got, int) == isinstance(want, int)
    return abs(g - w) <= REL_TOL * max(abs(g), abs(w))


def assert_same_groups(gpu, ora, aggs, numeric):
    """tests/parity_util.assert_same_groups with one difference: with `numeric` (the plan holds a library function) an
    aggregate's INT and FLOAT results are compared as numbers — a result one ulp off an integer does not fold to INT where the
    other side's does."""
    import parity_util as pu
    from oracle import n1o
    if not numeric:
        return pu.assert_same_groups(gpu, ora, aggs=aggs)
    gmap = {pu._canon_key(k): a for k, a in zip(gpu.keys, gpu.aggs)}
    omap = {pu._canon_key(k): a for k, a in zip(ora.keys, ora.aggs)}
    assert len(gmap) == len(gpu.keys) and set(gmap) == set(omap), ("group sets differ", sorted(set(gmap) ^ set(omap), key=repr)[:6])
    nums = (n1o.T_INT, n1o.T_FLOAT)
    for k, oa in omap.items():
        for i, (g, o) in enumerate(zip(gmap[k], oa)):
            if g[0] in nums and o[0] in nums:
                ok = same_value(g[1], o[1], exact=False)
            else:
                ok = g[0] == o[0] and g[1] == o[1]
            assert ok, "aggregate %d (%s) of group %r: device %r oracle %r" % (i, aggs[i], k, g, o)


# ---------------------------------------------------------------- the special-case table (hand-written)
#
# (function, arguments) -> expected value, written down from Go's documentation of math.Pow / Atan2 / Log / Exp / Acos ...
# (the special cases of C99 Annex F) and from value.NewValue; "nan" stands for any NaN.  2 ** 53 + 1 as an INT argument
# goes through float64 (intValue.Actual()): it IS 2 ** 53 there.
BIG = 2 ** 53 + 1
PI = math.pi
SPECIALS = [
    ("acos", [1], 0), ("acos", [3], "nan"), ("acos", [-1.5], "nan"), ("acos", [NAN], "nan"), ("acos", [PINF], "nan"), ("acos", [0], PI / 2),
    ("asin", [0], 0), ("asin", [-0.0], 0), ("asin", [10], "nan"), ("asin", [NINF], "nan"), ("asin", [1], PI / 2),
    ("atan", [0], 0), ("atan", [PINF], PI / 2), ("atan", [NINF], -PI / 2), ("atan", [NAN], "nan"), ("atan", [BIG], PI / 2),
    ("cos", [0], 1), ("cos", [PINF], "nan"), ("cos", [NINF], "nan"), ("cos", [NAN], "nan"), ("cos", [-0.0], 1),
    ("sin", [0], 0), ("sin", [-0.0], 0), ("sin", [PINF], "nan"), ("sin", [NAN], "nan"),
    ("tan", [0], 0), ("tan", [NINF], "nan"), ("tan", [NAN], "nan"),
    ("exp", [0], 1), ("exp", [-0.0], 1), ("exp", [1000], PINF), ("exp", [-1000], 0), ("exp", [PINF], PINF), ("exp", [NINF], 0), ("exp", [NAN], "nan"),
    ("ln", [1], 0), ("ln", [0], NINF), ("ln", [-0.0], NINF), ("ln", [-1], "nan"), ("ln", [PINF], PINF), ("ln", [NINF], "nan"), ("ln", [NAN], "nan"),
    ("log", [1], 0), ("log", [0], NINF), ("log", [-1], "nan"), ("log", [PINF], PINF), ("log", [NAN], "nan"), ("log", [1000], 3), ("log", [100], 2),
    ("degrees", [0], 0), ("degrees", [-0.0], 0), ("degrees", [PINF], PINF), ("degrees", [NAN], "nan"), ("degrees", [PI], 180), ("degrees", [BIG], float(2 ** 53) * 180.0 / PI),
    ("radians", [0], 0), ("radians", [NINF], NINF), ("radians", [NAN], "nan"), ("radians", [180], PI), ("radians", [BIG], float(2 ** 53) * PI / 180.0),
    # Pow
    ("power", [0, -1], PINF), ("power", [-0.0, -1], NINF), ("power", [-0.0, -2], PINF), ("power", [0, 0], 1), ("power", [NAN, 0], 1), ("power", [PINF, 0], 1),
    ("power", [7.5, 0], 1), ("power", [1, NAN], 1), ("power", [1, PINF], 1), ("power", [-8, 0.5], "nan"), ("power", [-8, 1 / 3.0], "nan"), ("power", [-8, 2], 64),
    ("power", [-2, 3], -8), ("power", [2, PINF], PINF), ("power", [2, NINF], 0), ("power", [0.5, PINF], 0), ("power", [0.5, NINF], PINF), ("power", [-1, PINF], 1),
    ("power", [-1, NINF], 1), ("power", [PINF, -1], 0), ("power", [PINF, 2], PINF), ("power", [NINF, 3], NINF), ("power", [NINF, 2], PINF), ("power", [NAN, 1], "nan"),
    ("power", [2, NAN], "nan"), ("power", [0, 3], 0), ("power", [12, 2], 144), ("power", [BIG, 1], 2 ** 53), ("power", [10, 400], PINF), ("power", [10, -400], 0),
    # Atan2(y, x): the four quadrants, both zeros of y and of x, the infinities
    ("atan2", [1, 1], PI / 4), ("atan2", [1, -1], 3 * PI / 4), ("atan2", [-1, -1], -3 * PI / 4), ("atan2", [-1, 1], -PI / 4),
    ("atan2", [0, 1], 0), ("atan2", [-0.0, 1], 0), ("atan2", [0, -1], PI), ("atan2", [-0.0, -1], -PI), ("atan2", [0, 0], 0), ("atan2", [-0.0, 0], 0),
    ("atan2", [0, -0.0], PI), ("atan2", [-0.0, -0.0], -PI), ("atan2", [1, 0], PI / 2), ("atan2", [-1, 0], -PI / 2), ("atan2", [1, -0.0], PI / 2),
    ("atan2", [1, PINF], 0), ("atan2", [1, NINF], PI), ("atan2", [-1, NINF], -PI), ("atan2", [PINF, 1], PI / 2), ("atan2", [NINF, 1], -PI / 2),
    ("atan2", [PINF, PINF], PI / 4), ("atan2", [PINF, NINF], 3 * PI / 4), ("atan2", [NINF, NINF], -3 * PI / 4), ("atan2", [NAN, 1], "nan"), ("atan2", [1, NAN], "nan"),
    # propagation: MISSING before NULL over all arguments; a non-number is NULL
    ("sin", [MISSING], MISSING), ("sin", [None], None), ("sin", ["a"], None), ("sin", [True], None), ("sin", [[1, 2]], None),
    ("power", [MISSING, None], MISSING), ("power", [None, MISSING], MISSING), ("power", ["a", MISSING], MISSING), ("power", [None, 2], None),
    ("power", [2, "a"], None), ("atan2", [None, MISSING], MISSING), ("atan2", [1, None], None), ("atan2", [False, 1], None),
    # the eager numeric conditionals, in argument order
    ("ifinf", [1, 2], 1), ("ifinf", [PINF, 2], 2), ("ifinf", [NINF, PINF], None), ("ifinf", [NAN, 2], "nan"), ("ifinf", [PINF, MISSING], MISSING),
    ("ifinf", [1, MISSING], 1), ("ifinf", [PINF, "a", 3], None), ("ifinf", [2.0, 3], 2), ("ifinf", [PINF, NINF, PINF, 2.5], 2.5), ("ifinf", [None, 1], None),
    ("ifnan", [NAN, 2], 2), ("ifnan", [PINF, 2], PINF), ("ifnan", [NAN, NAN], None), ("ifnan", [NAN, MISSING, 1], MISSING), ("ifnan", [3, MISSING], 3),
    ("ifnanorinf", [NAN, PINF, 5.0], 5), ("ifnanorinf", [NAN, NINF], None), ("ifnanorinf", [0.5, NAN], 0.5), ("ifnanorinf", [NAN, "a"], None),
    ("pi", [], PI), ("e", [], math.e), ("nan", [], "nan"), ("posinf", [], PINF), ("neginf", [], NINF),
]
# (first, second) -> what NANIF gives: Equals, then NaN on TRUE, `first` otherwise; POSINFIF / NEGINFIF alike
EQ_SPECIALS = [([3, 3], "hit"), ([3, 3.0], "hit"), ([3, 4], 3), (["a", "a"], "hit"), (["a", "b"], "a"), ([3, "a"], 3), ([None, 3], None), ([3, None], None),
               ([MISSING, 3], MISSING), ([None, MISSING], MISSING), ([True, True], "hit"), ([NAN, NAN], NAN)]


def special_matches(got, want):
    if isinstance(want, str) and want == "nan":
        return isinstance(got, float) and got != got
    if want is MISSING or want is None or got is MISSING or got is None:
        return got is want
    if isinstance(want, float) and want != want:
        return isinstance(got, float) and got != got
    if isinstance(want, int):  # an integral expectation is written as the INT NewValue makes of it
        return isinstance(got, int) and got == want or (isinstance(got, float) and abs(got - want) <= REL_TOL * abs(want))
    return is_num(got) and (got == want or abs(got - want) <= REL_TOL * abs(want))


# ---------------------------------------------------------------- the element-wise table
#
# One column `v` with every value class and the special-case table's numbers, one column `w` for the second argument, and a
# DICT32 column `s` (a string, NULL or MISSING per row: a library function of it is NULL, NULL, MISSING).
ELEM_NUMBERS = [0, -0.0, 1, -1, 2, 3, 0.5, -0.5, 1.5, -8, 10, 12, 100, 0.25, 700, -700, 1000, -1000, 2 ** 20, -(2 ** 20), BIG, PINF, NINF, NAN, 1e-300, 1e300,
                PI, PI / 2, -PI, 1 / 3.0, 7.5, 34, 180, -180, 90]
ELEM_OTHERS = [MISSING, None, True, False, "a", "", [1, 2], {"f": 1}]
ELEM_SECOND = [0, -0.0, 1, -1, 2, 0.5, 3, 1 / 3.0, PINF, NINF, NAN, 10, -2, MISSING, None, "ab"]


def special_args(name):
    """the argument lists the special-case table holds for `name` (one or two arguments: the element-wise node's)"""
    return [args for f, args, _want in SPECIALS if f == name and len(args) == (2 if name in BINARY else 1)]


def elem_rows(n, name):
    """n rows for function `name`.  The first rows are the special-case table's own argument lists for it, in the table's
    order (all of them from 64 rows on; tests/test_mathfn_cpu.py asserts that the 769-row table holds every one).  Behind
    them (v, w, s) cycle through the pools: v with stride 7 over 43 values, w so that a given v meets all 16 second
    arguments (for v fixed, i grows by 43 and w's index by 2 * 43 + 1 = 87, odd against 16)."""
    pool = ELEM_NUMBERS + ELEM_OTHERS
    first = special_args(name)
    assert len(first) <= 64
    rows = []
    for i in range(n):
        v = pool[(i * 7 + 3) % len(pool)]
        w = ELEM_SECOND[(i * 2 + i // len(pool)) % len(ELEM_SECOND)]
        if i < len(first):
            v, w = first[i][0], (first[i][1] if len(first[i]) > 1 else w)
        if name in ("cos", "sin", "tan") and is_num(v) and abs(v) > 2 ** 20 and not math.isinf(v):
            v = 2 ** 20  # (argument reduction of huge arguments differs between library generations)
        if name == "power" and is_num(v) and is_num(w) and not _power_in_range(v, w):
            w = 2
        s = [MISSING, None, "a", "ab", "t_1"][i % 5]
        rows.append({"v": v, "w": w, "s": s, "id": i})
    return rows


def _power_in_range(x, y):
    r = fn_float("power", x, y)
    return r != r or math.isinf(r) or r == 0 or 1e-300 <= abs(r) <= 1e300


def elem_table(rows):
    from oracle import n1o
    cols = [cn.helper_column(name, [r[name] for r in rows]) for name in ("v", "w", "id")]
    cols.append(n1o.Column(D("s"), n1o.COL_DICT32, codes=cn.dict_codes([r["s"] for r in rows])))
    return n1o.Table(cols, list(cn.DICT))


def elem_node(name, second="w", first="v"):
    if name in IFNUM:
        return ("num", name, [("col", first), ("col", second), ("const", 7.0)])
    return ("num", name, [("col", first)] + ([("col", second)] if name in BINARY else []))


# ---------------------------------------------------------------- the seeded generator
#
# Over tests/cond_util.py's table: x numbers in [0, 100) (ints and k / 8 + 1 / 16) with some NULL / MISSING, g ints 0..6,
# s / k strings.  The input rules, by construction: trigonometric arguments stay below 2^20 and EXP's below 700 (x * g <
# 700, x / 10 < 10), POWER's results inside 1e+-300 ((x + 1) ^ (g / 2) < 101 ^ 3); a library function's result is never a
# group key nor an operand of `=`; the constant it is compared with keeps 1e-6 relative off every value the node takes
# (threshold_for asserts it).  LN((x - 50)) is the source of NaN (x < 50) and -Inf (x = 50).

def lib_call(rng):
    name = rng.choice(LIBRARY)
    x, g = ("col", "x"), ("col", "g")
    if name in ("acos", "asin"):
        arg = [("arith", "/", x, ("const", 100))]
    elif name in ("atan", "cos", "sin", "tan"):
        arg = [rng.choice([x, ("arith", "*", x, g), ("arith", "-", x, ("const", 50))])]
    elif name == "exp":
        arg = [rng.choice([("arith", "/", x, ("const", 10)), g, ("arith", "-", g, x)])]
    elif name in ("ln", "log"):
        arg = [rng.choice([("arith", "+", x, ("const", 1)), ("arith", "-", x, ("const", 50))])]
    elif name == "atan2":
        arg = [rng.choice([x, ("arith", "-", x, ("const", 50))]), rng.choice([g, ("arith", "-", g, ("const", 3)), ("const", 10)])]
    else:
        arg = [("arith", "+", x, ("const", 1)), rng.choice([("const", 2), ("arith", "/", g, ("const", 2)), ("const", 0.5), ("const", 0)])]
    return ("num", name, arg)


def exact_call(rng):
    x, g = ("col", "x"), ("col", "g")
    r = rng.random()
    lnx = ("num", "ln", [("arith", "-", ("col", "g"), ("const", 3))])  # NaN for g < 3, -Inf for g = 3 (exactly), else finite
    if r < 0.2:
        return ("num", rng.choice(["degrees", "radians"]), [rng.choice([x, g, ("col", "s")])])
    if r < 0.5:
        name = rng.choice(IFNUM)
        tail = [rng.choice([("const", 7), ("const", 2.5), g, ("num", "posinf", []), ("num", "nan", []), ("col", "s"), ("const", MISSING)])
                for _ in range(rng.randint(1, 3))]
        # (the first argument: a library function only where its result is then NaN / an infinity or replaced by a constant)
        first = rng.choice([x, ("num", rng.choice(["nan", "posinf", "neginf"]), []), ("arith", "*", x, ("num", "posinf", []))])
        return ("num", name, [first] + tail)
    if r < 0.75:
        return ("cond", rng.choice(sorted(EQNUM)), [rng.choice([x, g, ("col", "s")]), rng.choice([("const", 3), ("const", "a"), g, ("const", 2.5)])])
    if r < 0.85:
        return ("arith", "*", ("num", rng.choice(["pi", "e"]), []), g)
    # NaN / -Inf from LN told apart exactly: the finite results (g > 3) are replaced, so no library value reaches the key
    # (the THEN strings are words of tests/cond_util.py's dictionary)
    # The constant keeps the input rule: the node takes NaN, -Inf, ln 1 = 0, ln 2 = 0.69..., ln 3 = 1.09..., all further than
    # 1e-6 relative from LN_SPLIT (asserted below, since threshold_for does not see a constant inside a CASE).
    return ("case", [(("cmp", "<", lnx, ("const", LN_SPLIT)), ("const", "low")), (("cmp", "<=", ("const", LN_SPLIT), lnx), ("const", "high"))], ("const", "mid"))


LN_SPLIT = 0.3
assert all(abs(math.log(k) - LN_SPLIT) > 1e-6 * max(abs(math.log(k)), LN_SPLIT) for k in (1, 2, 3))  # g - 3 for g = 4, 5, 6


USES = ["filter_lib", "sum_lib", "avg_lib", "min_lib", "max_lib", "case_arm_lib", "key_exact", "sum_exact", "filter_exact", "max_exact"]


def threshold_for(values):
    """a constant that keeps 1e-6 relative off every finite value in `values` (asserted), near their median"""
    finite = sorted({float(v) for v in values if is_num(v) and v == v and not math.isinf(v)})
    cands = [(a + b) / 2 for a, b in zip(finite, finite[1:]) if a >= 0 and b - a > 1e-4 * max(abs(a), abs(b), 1e-300)]
    cands = sorted(cands, key=lambda c: abs(c - (finite[len(finite) // 2] if finite else 0))) + [0.5, 1.5, 2.5, 1e6]
    for c in cands:
        c = float("%.6g" % c)
        if c >= 0 and all(abs(v - c) > 1e-6 * max(abs(v), abs(c)) for v in finite):
            return int(c) if c == int(c) else c
    raise AssertionError("no constant keeps off the node's values")


def draw_plan(seed):
    """One plan of the differential: the rows, the device's and the oracle's (condition, keys, aggregates), the helper
    columns' values.  The oracle reads helper column `h` where the device evaluates the node."""
    rng = random.Random(990_000 + seed)
    rows = cn.make_rows(rng, rng.randint(1, 1200))
    use = USES[seed % len(USES)]
    h = D("h")
    keys = [[D("k")], [D("g")], []][rng.randrange(3)]
    dcond = ocond = None
    if use.endswith("_lib"):
        node = lib_call(rng)
        if rng.random() < 0.3:  # a two-node chain, an argument of one another
            node = ("num", rng.choice(["atan", "exp", "sin"]), [("num", "atan", [node[2][0]])]) if rng.random() < 0.5 else \
                   ("arith", "+", node, ("const", 1))
    else:
        node = exact_call(rng)
    if use == "case_arm_lib":  # a library function as THEN and ELSE, an exact condition in front
        node = ("case", [(("cmp", "<", ("col", "x"), ("const", 40)), node)], ("num", "atan", [("col", "g")]))
    values = [eval_value(node, r) for r in rows]
    text = value_text(node)
    if use in ("filter_lib", "filter_exact"):
        c = threshold_for(values)
        dcond, ocond = "(%s < %s)" % (text, json.dumps(c)), "(%s < %s)" % (h, json.dumps(c))
        daggs = oaggs = sorted(["count(*)", "max(%s)" % D("x")])
    elif use == "key_exact":
        dkeys, okeys = [text] + keys[:1], [h] + keys[:1]
        return {"rows": rows, "node": node, "use": use, "values": values, "numeric": False,
                "device": (None, dkeys, sorted(["count(*)", "sum(%s)" % D("x")])), "oracle": (None, okeys, sorted(["count(*)", "sum(%s)" % D("x")]))}
    else:
        f = {"sum": "sum(%s)", "avg": "avg(%s)", "min": "min(%s)", "max": "max(%s)", "case": "sum(%s)"}[use.split("_")[0]]
        if f[:3] in ("sum", "avg") and any(is_num(v) and (v != v or math.isinf(v)) for v in values):
            # (a SUM over NaN / infinities is NaN or depends on the order of the rows: keep them out of it, exactly)
            node = ("num", "ifnanorinf", [node, ("const", 0)])
            values = [eval_value(node, r) for r in rows]
            text = value_text(node)
        daggs, oaggs = [f % text, "count(*)"], [f % h, "count(*)"]
    return {"rows": rows, "node": node, "use": use, "values": values, "numeric": uses_library(node),
            "device": (dcond, keys, daggs), "oracle": (ocond, keys, oaggs)}
