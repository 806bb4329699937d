"""The fifteen arithmetic nodes as values: the yardstick and the pools of tests/test_arith_cpu.py and tests/test_gpu_arith.py.

A Python restatement, from the reference's Go text, of
  * intValue.Add / IDiv / IMod / Mult / Neg / Sub and IsInt (value/integer.go:266-356), floatValue's (value/float.go:331-385),
  * value.NewValue(float64) (value/value.go:377-382; tests/mathfn_util.new_value says the same and is used),
  * Add / Sub / Mult / Div / Mod / Neg / IDiv / IMod .Apply (expression/arith_*.go),
  * Abs / Ceil / Floor / Round / Sign / Sqrt / Trunc .Apply with roundFloat and truncateFloat (expression/func_num.go).
INTs are Python ints (overflow is decided exactly, then wrapped as int64 wraps), FLOATs are Python floats with ONE IEEE
operation per rounding; float64 -> int64 follows amd64 (NaN or out of range: MinInt64).  Where plain Python raises (0.0 / 0.0,
floor of an infinity, fmod of one) the operation goes through numpy's float64, which is IEEE and silent.

Every operation here is exact or correctly rounded, so the yardstick's bits are the answer: same_exact() has no tolerance.
The one exception is listed apart (LOOSE_DIGITS): ROUND / TRUNC with 22 < |digits| <= 308, where 10^digits comes from a
library pow that is a few ulp off on either side.

One place where the Go text gives no value: IDIV / IMOD by a FLOAT that is not zero but truncates to 0 (0.5, 1e-7) divides
an int64 by zero, which panics at run time.  The project (oracle and device alike) gives NULL, the value of a zero divisor;
so does the yardstick.

Nodes:  ("col", name) | ("const", v) | ("op", name, [args]) with name in OPS."""
import fractions
import math

import numpy as np

import cond_util as cn
import golden_util as gu
import mathfn_util as mu
import parity_util as pu
from oracle import n1o

MISSING = cn.MISSING
REL_TOL = pu.REL_TOL
NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
MIN64, MAX64 = -(2 ** 63), 2 ** 63 - 1
D = cn.D

NARY = ("+", "*")
BINARY = ("-", "/", "%", "idiv", "imod")
UNARY = ("neg", "abs", "ceil", "floor", "sign", "sqrt")
DIGITS = ("round", "trunc")  # one argument or two
OPS = NARY + BINARY + UNARY + DIGITS
assert len(OPS) == 15


# ---------------------------------------------------------------- the yardstick

def is_num(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def wrap64(x):
    """an exact integer as int64 arithmetic leaves it"""
    return (x + 2 ** 63) % 2 ** 64 - 2 ** 63


def go_f2i(f):
    """int64(float64) on amd64 (CVTTSD2SI): NaN or out of range is MinInt64"""
    if f != f or not (-2.0 ** 63 <= f < 2.0 ** 63):
        return MIN64
    return int(f)


def go_quo(x, d):
    """int64 x / d, d != 0: truncated; MinInt64 / -1 wraps to MinInt64 (the Go spec's one overflow)"""
    q = abs(x) // abs(d)
    return wrap64(q if (x < 0) == (d < 0) else -q)


def go_rem(x, d):
    """int64 x % d, d != 0: the sign of x; MinInt64 % -1 is 0"""
    r = abs(x) % abs(d)
    return -r if x < 0 else r


def actual(n):
    """NumberValue.Actual(): float64(this) for an intValue (value/integer.go:57-59)"""
    return float(n)


def _f(op, *xs):
    """one IEEE operation that plain Python may refuse"""
    with np.errstate(all="ignore"):
        return float(op(*[np.float64(x) for x in xs]))


def fdiv(a, b):
    return _f(np.divide, a, b)


def num_add(a, b):
    if isinstance(a, int) and isinstance(b, int):  # value/integer.go:266-277
        rv = wrap64(a + b)
        if (a >= 0 and b >= 0 and rv >= 0) or (a < 0 and b < 0 and rv < 0):
            return rv
    return actual(a) + actual(b)


def num_mult(a, b):
    if isinstance(a, int) and isinstance(b, int):  # value/integer.go:319-329
        rv = wrap64(a * b)
        if a == 0 or go_quo(rv, a) == b:
            return rv
    return actual(a) * actual(b)


def num_neg(a):
    if isinstance(a, int):  # value/integer.go:331-337
        return -actual(a) if a == MIN64 else -a
    return -a


def num_sub(a, b):
    if isinstance(a, int) and isinstance(b, int) and b > MIN64:  # value/integer.go:339-348
        return num_add(a, -b)
    return actual(a) - actual(b)


def num_idiv_imod(a, b, mod):
    """value/integer.go:279-313, value/float.go:335-369: NULL on a zero divisor (INT 0, 0.0, -0.0)"""
    if isinstance(b, int):
        d = b
    else:
        if b == 0.0:
            return None
        d = go_f2i(b)
    if d == 0:
        return None  # (Go panics here: see the module's docstring)
    x = a if isinstance(a, int) else go_f2i(a)
    return go_rem(x, d) if mod else go_quo(x, d)


def pow10(p):
    """math.Pow(10, p) for an int p: the exact power up to 1e22 (a repeated product), its correctly rounded reciprocal below
    zero (Pow inverts the positive power), 0 / +Inf where float64 ends; in between the nearest double (LOOSE_DIGITS)"""
    a = abs(p)
    if a > 400:
        return 0.0 if p < 0 else PINF
    if a <= 22:
        pw = 1.0
        for _ in range(a):
            pw *= 10.0
    elif a <= 308:
        pw = float(10 ** a)
    else:
        return float(fractions.Fraction(1, 10 ** a)) if p < 0 else PINF
    return fdiv(1.0, pw) if p < 0 else pw


def round_float(x, p):
    """roundFloat (expression/func_num.go:1715-1736)"""
    if x != x or math.isinf(x):
        return x
    pw = pow10(p)
    if abs(p) <= 22 and math.isfinite(abs(x) * pw + 0.5):
        return gu.round_float(x, p)  # (the same statement, for finite intermediates)
    sign = 1.0
    if x < 0:
        sign, x = -1.0, -x
    intermed = x * pw + 0.5
    rounder = _f(np.floor, intermed)
    if rounder == intermed and _f(np.fmod, rounder, 2.0) != 0:
        rounder -= 1
    return fdiv(sign * rounder, pw)


def truncate_float(x, p):
    """truncateFloat (expression/func_num.go:1703-1708)"""
    pw = pow10(p)
    return fdiv(_f(np.trunc, x * pw), pw)


def digits_of(prec):
    """Round.Apply / Trunc.Apply on the digits argument: (MISSING | None | int).  p = int(pf) is an amd64 conversion."""
    if prec is MISSING:
        return MISSING
    if not is_num(prec):
        return None
    pf = actual(prec)
    if pf != _f(np.trunc, pf):  # (a NaN too)
        return None
    return go_f2i(pf)


def apply(op, args):
    """one node over evaluated arguments"""
    if op in NARY:  # Add.Apply / Mult.Apply: MISSING returns at once, a non-number makes NULL, the fold starts at int 0 / int 1
        null, acc = False, (0 if op == "+" else 1)
        for a in args:
            if not null and is_num(a):
                acc = num_add(acc, a) if op == "+" else num_mult(acc, a)
            elif a is MISSING:
                return MISSING
            else:
                null = True
        return None if null else acc
    if op in ("-", "neg"):  # Sub.Apply / Neg.Apply: numbers first, then MISSING, else NULL
        if all(is_num(a) for a in args):
            return num_sub(*args) if op == "-" else num_neg(args[0])
        return MISSING if any(a is MISSING for a in args) else None
    if op in ("/", "%"):  # Div.Apply / Mod.Apply
        x, y = args
        if x is MISSING or y is MISSING:
            return MISSING
        if not is_num(y) or actual(y) == 0.0 or not is_num(x):
            return None
        return mu.new_value(fdiv(actual(x), actual(y)) if op == "/" else _f(np.fmod, actual(x), actual(y)))
    if op in ("idiv", "imod"):
        x, y = args
        if x is MISSING or y is MISSING:
            return MISSING
        if not (is_num(x) and is_num(y)):
            return None
        return num_idiv_imod(x, y, op == "imod")
    # expression/func_num.go: the FIRST argument decides before the digits are looked at (round(NULL, MISSING) is NULL)
    x = args[0]
    if x is MISSING:
        return MISSING
    if not is_num(x):
        return None
    v = actual(x)
    if op in DIGITS:
        p = 0
        if len(args) == 2:
            p = digits_of(args[1])
            if p is MISSING or p is None:
                return p
        return mu.new_value(round_float(v, p) if op == "round" else truncate_float(v, p))
    if op == "abs":
        r = abs(v)
    elif op == "ceil":
        r = _f(np.ceil, v)
    elif op == "floor":
        r = _f(np.floor, v)
    elif op == "sign":
        r = -1.0 if v < 0.0 else (1.0 if v > 0.0 else 0.0)
    else:
        assert op == "sqrt", op
        r = _f(np.sqrt, v)
    return mu.new_value(r)


def eval_node(e, row):
    if e[0] == "col":
        return row[e[1]]
    if e[0] == "const":
        return e[1]
    return apply(e[1], [eval_node(a, row) for a in e[2]])


def text(e):
    """expression.Stringer text: (a + b + c), (a % b), (-a), idiv(a, b), round(a, d)"""
    if e[0] == "col":
        return D(e[1])
    if e[0] == "const":
        return mu.value_text(e)
    args = [text(a) for a in e[2]]
    if e[1] == "neg":
        return "(-%s)" % args[0]
    if e[1] in NARY or e[1] in ("-", "/", "%"):
        return "(%s)" % (" %s " % e[1]).join(args)
    return "%s(%s)" % (e[1], ", ".join(args))


def node(op, *cols):
    return ("op", op, [c if isinstance(c, tuple) else ("col", c) for c in cols])


# ---------------------------------------------------------------- comparing

def _norm(v):
    return MISSING if v is gu.MISSING else v


def same_exact(got, want):
    """MISSING and NULL by identity, NaN matches NaN, infinities by sign, everything else as exact rationals: an integral
    FLOAT and the INT of the same value are one number (MAX and group keys fold the kind on the device), -0.0 is 0."""
    got, want = _norm(got), _norm(want)
    if got is MISSING or got is None or want is MISSING or want is None:
        return got is want
    if not (is_num(got) and is_num(want)):
        return False
    gn, wn = got != got, want != want
    if gn or wn:
        return gn and wn
    gi, wi = isinstance(got, float) and math.isinf(got), isinstance(want, float) and math.isinf(want)
    if gi or wi:
        return gi and wi and got == want
    return fractions.Fraction(got) == fractions.Fraction(want)


LOOSE_DIGITS = (23, 30, -30)  # 22 < |digits| <= 308: the only rows same_loose may judge


def is_loose(op, args):
    return op in DIGITS and len(args) == 2 and is_num(args[1]) and 22 < abs(args[1]) <= 308


def same_loose(got, want):
    """REL_TOL on finite non-zero numbers; NaN, the infinities, 0, NULL and MISSING exactly"""
    got, want = _norm(got), _norm(want)
    if not (is_num(got) and is_num(want)) or got != got or want != want or math.isinf(got) or math.isinf(want) or got == 0 or want == 0:
        return same_exact(got, want)
    return abs(float(got) - float(want)) <= REL_TOL * max(abs(float(got)), abs(float(want)))


def same(op, args, got, want):
    return same_loose(got, want) if is_loose(op, args) else same_exact(got, want)


# ---------------------------------------------------------------- the pools

HEX = [float.fromhex(h) for h in ("0x1.2508d28549423p+46", "0x1.0a28348d2081ep+46", "0x1.435215dffc70fp+49", "0x1.03eb4351d1bedp+56")]
BELOW_2_63 = math.nextafter(2.0 ** 63, 0.0)
INT_POOL = [0, 1, -1, 2, -2, 3, 7, -7, 10,
            2 ** 31 - 1, 2 ** 31, -(2 ** 31), 2 ** 32, 2 ** 32 + 1,
            3037000499, 3037000500, -3037000500,
            2 ** 52 + 1,
            2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, -(2 ** 53 + 1),
            2 ** 62, -(2 ** 62), 2 ** 62 + 1,
            2 ** 63 - 2, 2 ** 63 - 1, -(2 ** 63), -(2 ** 63) + 1]
FLOAT_POOL = [0.0, -0.0, 0.5, -0.5, 1.5, 2.5, -2.5, 3.5, 0.125, 7.0,
              2.675, 1.005, 0.285,
              1e-7, 5e-324, 2.2250738585072014e-308,
              1e22, 1e23, 2.0 ** 52 + 0.5, 2.0 ** 53,
              2.0 ** 63, -(2.0 ** 63), BELOW_2_63,
              1e300, -1e300, 1.7976931348623157e308, PINF, NINF, NAN] + HEX + [-h for h in HEX]
OTHER_POOL = [MISSING, None, True, "a", [1, 2], {"f": 1}]
VALUE_POOL = INT_POOL + FLOAT_POOL + OTHER_POOL
DIGIT_POOL = [0, 1, -1, 2, -2, 3, -3, 15, 16, 17, 22, -22,
              2.0, 2.5, NAN,
              PINF, NINF, 400, -400, 1e300,
              MISSING, None, "a"] + list(LOOSE_DIGITS)
FOLD_POOL = [2 ** 62, -(2 ** 62), 2 ** 63 - 1, 1, -1, 0.5, MISSING, None]


def odd(rows):
    """an odd row count (the wide scan's narrow tail): the first row once more"""
    rows = list(rows)
    if len(rows) % 2 == 0:
        rows.append(dict(rows[0]))
    for i, r in enumerate(rows):
        r["id"] = i
    return rows


def unary_rows():
    return odd({"v": v} for v in VALUE_POOL)


def pair_rows():
    return odd({"v": v, "w": w} for v in VALUE_POOL for w in VALUE_POOL)


def digit_rows():
    return odd({"v": v, "d": d} for v in VALUE_POOL for d in DIGIT_POOL)


def fold_rows(n):
    rows = [{}]
    for name in "abce"[:n]:
        rows = [dict(r, **{name: x}) for r in rows for x in FOLD_POOL]
    return odd(rows)


def sample(rows, n):
    """n of the rows, a stride through them that is co-prime to their count, renumbered"""
    step = 37
    assert math.gcd(step, len(rows)) == 1
    out = [dict(rows[(7 + i * step) % len(rows)]) for i in range(n)]
    for i, r in enumerate(out):
        r["id"] = i
    return out


def table(rows):
    names = [k for k in rows[0]]
    return n1o.Table([cn.helper_column(name, [r[name] for r in rows]) for name in names], list(cn.DICT))


# op name -> (node, rows): the element-wise forms of the fifteen ops ("round" / "trunc": one argument; "round2" / "trunc2": two)
def forms():
    out = {}
    for op in UNARY + DIGITS:
        out[op] = (node(op, "v"), "unary")
    for op in NARY + BINARY:
        out[op] = (node(op, "v", "w"), "pair")
    for op in DIGITS:
        out[op + "2"] = (node(op, "v", "d"), "digit")
    return out


FORMS = forms()
ROWS = {"unary": unary_rows, "pair": pair_rows, "digit": digit_rows}

# the fused route: three nodes a plan (kFastDerived) over at most three input columns, the key among them (kFastCols)
FUSED_GROUPS = [("+", "-", "*"), ("/", "%", "neg"), ("idiv", "imod", "abs"), ("round2", "trunc2", "sqrt"), ("ceil", "floor", "sign"),
                ("round", "trunc")]
FUSED_IDS = ["add-sub-mul", "div-mod-neg", "idiv-imod-abs", "round2-trunc2-sqrt", "ceil-floor-sign", "round1-trunc1"]


def fused_group_nodes(group):
    """the group's nodes over ONE table: a unary form beside binary ones reads the pair table's `v`"""
    kinds = {FORMS[f][1] for f in group}
    rows = "digit" if "digit" in kinds else ("pair" if "pair" in kinds else "unary")
    return [FORMS[f][0] for f in group], rows


# a node over a node
NESTED = {
    "round-of-product": ("op", "round", [node("*", "v", "w"), ("const", 2)]),
    "idiv-plus-imod": ("op", "+", [node("idiv", "v", "w"), node("imod", "v", "w")]),
    "neg-of-difference": ("op", "neg", [node("-", "v", "w")]),
}

# The n-ary folds on the fused route.  Its three input columns are the key and two operands, so the further operands are a
# constant: each of FOLD_CONSTS in turn (a negative constant prints as a negation, one more node; MISSING and NULL come
# from the columns).  Two plans of three nodes: the constant last, in the middle and first; three and four operands.
FOLD_CONSTS = [2 ** 62, 2 ** 63 - 1, 1, 0.5]


def fused_fold_nodes(which, c):
    a, b, k = ("col", "a"), ("col", "b"), ("const", c)
    if which == 0:
        return [("op", "+", [a, b, k]), ("op", "*", [a, b, k]), ("op", "+", [a, k, b, k])]
    return [("op", "*", [a, k, b, k]), ("op", "+", [k, a, b]), ("op", "*", [k, b, a])]


def max_value(v):
    """what MAX over a one-row group gives: MISSING and NULL alike are NULL"""
    return None if v is MISSING else v


def fused_intermediate_result(x, p):
    """roundFloat with x * pow + 0.5 rounded ONCE (a contracted multiply-add), for finite x and |p| <= 22: what the
    sensitivity condition of tests/test_arith_cpu.py compares the yardstick with"""
    sign = 1.0
    if x < 0:
        sign, x = -1.0, -x
    pw = pow10(p)
    exact = fractions.Fraction(x) * fractions.Fraction(pw) + fractions.Fraction(1, 2)
    try:
        intermed = float(exact)  # (correctly rounded)
    except OverflowError:
        intermed = PINF
    rounder = _f(np.floor, intermed)
    if rounder == intermed and _f(np.fmod, rounder, 2.0) != 0:
        rounder -= 1
    return fdiv(sign * rounder, pw)
