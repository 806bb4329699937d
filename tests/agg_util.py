"""The six aggregates over one group's operands: the yardstick and the pools of tests/test_agg_cpu.py and
tests/test_gpu_agg_edges.py.

A Python restatement, from the reference's Go text, of CumulateInitial / CumulateIntermediate / ComputeFinal of
  * Count (algebra/agg_count.go:102-116: every operand of type > NULL) and Countn (agg_countn.go:84-97: NUMBERs),
  * Sum (agg_sum.go:86-97, 118-136: NUMBERs only, NumberValue.Add; Default() NULL, :77),
  * Avg (agg_avg.go:85-97, 136-157 and ComputeFinal :111-129: float64(sum) / float64(count), then value.NewValue),
  * Min / Max (agg_min.go:83-94, 117-127; agg_max.go likewise: operands of type > NULL, value.Collate, the first of a tie stays),
with intValue.Add (value/integer.go:266-277), collateFloat (value/float.go:123-172: NaN first) and floatValue.MarshalJSON
(value/float.go:31-48: -0 prints as 0).  It does not call the oracle.

An operand and a result are (tag, value) pairs with the tags of oracle/n1o.py; a STRING's value is its bytes.

The yardstick says what the DEVICE documents: SUM over ints is the exact total, an INT when all ints have
one sign, no float took part and the total fits int64, else the FLOAT float(exact total) + fsum(floats) — deviations (ii) and
(iii) from the reference, whose own answer is a left-to-right chain of Add.  reference_sum() is that chain; where the two
differ the group is `deviates` and only the chain is compared with the oracle.

A group whose answer depends on the order of its rows is not `well_defined`, and no test draws one:
  * two operands of different bits that collate equal (an int and the float equal to it, 0.0 and -0.0, ints beyond 2^53
    whose float64 image is a float of the group): MIN / MAX keep whichever came first;
  * finite floats of both signs whose partial sums can overflow where the total does not.
Float sums of more than one term are order dependent in their last bits only: they stay well defined and are compared
within the derived bound of geometry_util.assert_float_sums_exact, |got - exact| <= n 2^-53 sum|x| plus one rounding; an
exact result that is NaN or an infinity has to match as it is."""
import fractions
import functools
import math

import numpy as np

import arith_util as au
import golden_util as gu
import mathfn_util as mu
from oracle import n1o
from query_amd import plan as qplan

T_MISSING, T_NULL, T_FALSE, T_TRUE, T_INT, T_FLOAT, T_STRING, T_ARRAY, T_OBJECT = range(9)
assert (T_MISSING, T_INT, T_OBJECT) == (n1o.T_MISSING, n1o.T_INT, n1o.T_OBJECT)
MIN64, MAX64 = -(2 ** 63), 2 ** 63 - 1
NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
DBL_MAX = 1.7976931348623157e308
KINDS = ("count", "countn", "sum", "avg", "min", "max")
UNSUPPORTED = ("unsupported",)  # MIN / MAX of a group that holds an ARRAY / OBJECT: the device's N1K_UNSUPPORTED_DATA

DICT = [b"", b"m", b"zz", b"[1,2]"]  # code 0 is the empty string; the last entry is the ARRAY operand's text


def I(x):
    assert MIN64 <= x <= MAX64
    return (T_INT, int(x))


def F(x):
    return (T_FLOAT, float(x))


def S(b):
    return (T_STRING, b)


TRUE, FALSE, NULL, MISSING, ARRAY = (T_TRUE, None), (T_FALSE, None), (T_NULL, None), (T_MISSING, None), (T_ARRAY, b"[1,2]")


def D(*names):
    return qplan.field_path("default", *names)


# ---------------------------------------------------------------- the yardstick

_CLASS = {T_FALSE: 2, T_TRUE: 2, T_INT: 3, T_FLOAT: 3, T_STRING: 4, T_ARRAY: 5, T_OBJECT: 6}


def collate(a, b):
    """value.Collate of two operands of type > NULL (not arrays / objects among themselves)"""
    ca, cb = _CLASS[a[0]], _CLASS[b[0]]
    if ca != cb:
        return -1 if ca < cb else 1
    if ca == 2:
        return (a[0] == T_TRUE) - (b[0] == T_TRUE)
    if ca == 4:
        return (a[1] > b[1]) - (a[1] < b[1])  # bytes (value/string.go:116-130)
    assert ca == 3
    if a[0] == T_INT and b[0] == T_INT:  # value/integer.go:100-118: exact
        return (a[1] > b[1]) - (a[1] < b[1])
    x, y = float(a[1]), float(b[1])  # collateFloat
    xn, yn = x != x, y != y
    if xn or yn:
        return 0 if (xn and yn) else (-1 if xn else 1)
    return (x > y) - (x < y)


def same_bits(a, b):
    if a[0] != b[0]:
        return False
    if a[0] == T_FLOAT:
        return (a[1] != a[1] and b[1] != b[1]) or (a[1] == b[1] and math.copysign(1.0, a[1]) == math.copysign(1.0, b[1]))
    return a[1] == b[1]


def extreme(ops, want_min):
    """(winner, tied): the left-to-right fold of Min / Max.cumulatePart; tied: another order could give other bits"""
    vals = [o for o in ops if o[0] > T_NULL]
    if not vals:
        return NULL, False
    if any(o[0] in (T_ARRAY, T_OBJECT) for o in vals):
        return UNSUPPORTED, False
    best = vals[0]
    for o in vals[1:]:
        c = collate(o, best)
        if (c < 0) if want_min else (c > 0):
            best = o
    # Collate is not transitive beyond 2^53 (ints exactly, an int and a float through float64): any int that a float of the
    # group cannot be told apart from makes the fold order dependent, whether or not it wins this order
    tied = any(collate(o, p) == 0 and not same_bits(o, p) for o in vals for p in vals if _CLASS[o[0]] == 3 and _CLASS[p[0]] == 3)
    return best, tied


def float_total(floats):
    """(exact sum of the floats as IEEE arithmetic in ANY order gives it, or None when the order decides, is_special)"""
    if any(x != x for x in floats) or (PINF in floats and NINF in floats):
        return NAN, True
    finite = [x for x in floats if not math.isinf(x)]
    mag = sum((abs(fractions.Fraction(x)) for x in finite), fractions.Fraction(0))
    over = mag > fractions.Fraction(DBL_MAX)
    inf = PINF if PINF in floats else (NINF if NINF in floats else None)
    if over and len(finite) == 2 and not (finite[0] >= 0) == (finite[1] >= 0):
        over = False  # (one addition of opposite signs: no partial sum, nothing overflows)
    if over:
        exact = sum((fractions.Fraction(x) for x in finite), fractions.Fraction(0))
        one_sign = all(x >= 0 for x in finite) or all(x <= 0 for x in finite)
        if not one_sign or abs(exact) < fractions.Fraction(2) ** 1024:
            return None, True  # a partial sum may reach an infinity that the total does not
        own = PINF if exact > 0 else NINF
        if inf is not None and inf != own:
            return NAN, True
        return own, True
    if inf is not None:
        return inf, True
    if finite and all(x == 0 and math.copysign(1.0, x) < 0 for x in finite):
        return -0.0, False  # (-0 + -0 is -0, and a lone operand is itself; math.fsum gives +0)
    return math.fsum(finite), False


def summed(ops):
    """-> dict(sum=, n=, float_part=, special=, bound=, well_defined=): SUM as the device documents it"""
    ints = [v for t, v in ops if t == T_INT]
    floats = [v for t, v in ops if t == T_FLOAT]
    n = len(ints) + len(floats)
    out = {"n": n, "float_part": bool(floats), "special": False, "bound": 0.0, "well_defined": True}
    if n == 0:
        out["sum"] = NULL  # Default() (agg_sum.go:77)
        return out
    total = sum(ints)
    nonneg, neg = any(v >= 0 for v in ints), any(v < 0 for v in ints)
    if not floats and not (nonneg and neg) and MIN64 <= total <= MAX64:
        out["sum"] = (T_INT, total)
        return out
    ipart = float(total) if ints else 0.0  # (Python rounds an int correctly; deviations (ii), (iii))
    if not floats:
        out["sum"] = (T_FLOAT, ipart)
        return out
    ftot, special = float_total(floats + ([ipart] if ints else []))
    out["special"] = special
    if ftot is None:
        out["well_defined"] = False
        out["sum"] = (T_FLOAT, NAN)
        return out
    out["sum"] = (T_FLOAT, ftot)
    if not special:
        mag = sum((abs(fractions.Fraction(x)) for x in floats + [float(v) for v in ints]), fractions.Fraction(0))
        out["bound"] = float(fractions.Fraction(n, 2 ** 53) * mag)  # (sum|x| itself may be beyond float64: 1e308 and -1e308)
    return out


def averaged(s):
    """Avg.ComputeFinal over summed(): NULL without a number"""
    if s["n"] == 0:
        return NULL
    f = au.fdiv(float(s["sum"][1]), float(s["n"]))
    v = mu.new_value(f)
    return (T_INT, v) if isinstance(v, int) else (T_FLOAT, v)


def yardstick(ops):
    """{kind: (tag, value)} of the six aggregates over the group's operands, with
    well_defined, float_part (SUM / AVG carry the bound), special (their exact result is NaN / an infinity), bound"""
    s = summed(ops)
    mn, t1 = extreme(ops, True)
    mx, t2 = extreme(ops, False)
    return {"count": (T_INT, sum(1 for t, _ in ops if t > T_NULL)), "countn": (T_INT, s["n"]),
            "sum": s["sum"], "avg": averaged(s) if s["well_defined"] else (T_FLOAT, NAN), "min": mn, "max": mx,
            "well_defined": s["well_defined"] and not t1 and not t2,
            "float_part": s["float_part"], "special": s["special"], "bound": s["bound"], "n": s["n"]}


def reference_sum(ops):
    """Sum.cumulatePart as the reference runs it over rows in THIS order: the first number, then NumberValue.Add"""
    acc = None
    for t, v in ops:
        if t in (T_INT, T_FLOAT):
            acc = v if acc is None else au.num_add(acc, v)
    if acc is None:
        return NULL
    return (T_INT, acc) if isinstance(acc, int) else (T_FLOAT, acc)


def reference_avg(ops):
    s, n = reference_sum(ops), sum(1 for t, _ in ops if t in (T_INT, T_FLOAT))
    if n == 0:
        return NULL
    v = mu.new_value(au.fdiv(float(s[1]), float(n)))
    return (T_INT, v) if isinstance(v, int) else (T_FLOAT, v)


def deviates(ops, y=None):
    """the documented deviations (ii) / (iii) apply: the reference's chain of Add in this order is another value"""
    y = y or yardstick(ops)
    return not y["float_part"] and not same_bits(reference_sum(ops), y["sum"])


# ---------------------------------------------------------------- comparing

def text_of(v):
    """the JSON text of a result (value.MarshalJSON): what a client reads"""
    t, x = v
    if t == T_FLOAT:
        if x != x:
            return '"NaN"'
        if math.isinf(x):
            return '"+Infinity"' if x > 0 else '"-Infinity"'
        return gu.go_format_float(x)  # (-0.0 prints as 0: value/float.go:41-43)
    if t == T_INT:
        return str(x)
    return repr((t, x))


def same_value(kind, got, want, y):
    """tag and payload bit for bit, but: a FLOAT zero by its JSON text (both signs print 0), and a
    SUM / AVG with a float part within the group's bound (its NaN / infinities exactly)"""
    if want == UNSUPPORTED:
        return False
    if kind in ("sum", "avg") and y["float_part"] and not y["special"]:
        if got[0] not in (T_INT, T_FLOAT):
            return False
        g, w = float(got[1]), float(want[1])
        if g != g or math.isinf(g):
            return False
        if kind == "sum":
            return got[0] == T_FLOAT and abs(g - w) <= y["bound"] + abs(w) * 2.0 ** -53
        return abs(g - w) <= y["bound"] / y["n"] + abs(w) * 2.0 ** -52
    if got[0] != want[0]:
        return False
    if got[0] == T_FLOAT and got[1] == 0.0 and want[1] == 0.0:
        return text_of(got) == text_of(want) == "0"
    return same_bits(got, want)


def differences(ops, got, y=None, kinds=KINDS):
    """got: {kind: (tag, value)} -> [(kind, got, want)] that same_value refuses"""
    y = y or yardstick(ops)
    return [(k, got[k], y[k]) for k in kinds if not same_value(k, got[k], y[k], y)]


# ---------------------------------------------------------------- the pools

SINGLE_INTS = [0, 1, -1, 2 ** 40 - 1, -(2 ** 40 - 1), 2 ** 40, -(2 ** 40), 2 ** 53, -(2 ** 53), 2 ** 53 + 1, -(2 ** 53 + 1),
               MAX64, MAX64 - 1, MIN64, MIN64 + 1]
SINGLE_FLOATS = [0.0, -0.0, 5e-324, 2.2250738585072014e-308, 0.1, 1e308, -1e308, PINF, NINF, NAN]
NUMERIC = [I(x) for x in SINGLE_INTS] + [F(x) for x in SINGLE_FLOATS]
SINGLETONS = [[o] for o in NUMERIC + [S(b""), S(b"m"), TRUE, FALSE, NULL, MISSING]]

Q = 2 ** 61
DIRECTED = {
    "total-int64-max": [I(MAX64 - 5), I(2), I(3)],
    "total-int64-max-plus-1": [I(MAX64 - 5), I(2), I(4)],
    "total-int64-min": [I(MIN64 + 5), I(-2), I(-3)],
    "total-int64-min-minus-1": [I(MIN64 + 5), I(-2), I(-4)],
    # The running total overflows at the second row and fits again at the third.  Signs are mixed, so a FLOAT either way: the
    # device's is the exact total, 1.0 (deviation (ii)); the reference's chain has gone through float64 and gives 0.0
    "transient-overflow-mixed": [I(MAX64), I(1), I(-MAX64)],
    "same-sign-overflow": [I(Q), I(Q), I(Q), I(Q)],
    "lds-cut-off-both-sides": [I(2 ** 40 - 1), I(2 ** 40), I(2 ** 40 - 1), I(2 ** 40)],
    "lds-cut-off-both-sides-negative": [I(-(2 ** 40 - 1)), I(-(2 ** 40)), I(-(2 ** 40 - 1)), I(-(2 ** 40))],
    "lds-cut-off-both-signs": [I(2 ** 40 - 1), I(-(2 ** 40)), I(2 ** 40), I(-(2 ** 40 - 1)), I(7)],
    "mixed-sign-total-zero": [I(5), I(-7), I(2)],
    "mixed-sign-huge-total-zero": [I(MAX64), I(MIN64), I(1)],
    "ints-plus-one-float": [I(3), I(4), F(0.25), I(-1)],
    "big-ints-plus-one-float": [I(2 ** 40), I(2 ** 40 - 1), F(0.5)],
    "cancelling-floats": [F(1e16), F(1.0), F(-1e16)],
    "float-overflow": [F(1e308), F(1e308)],
    "inf-minus-inf": [F(PINF), F(NINF)],
    "nan-and-one": [F(NAN), I(1)],
    "inf-one-null": [F(PINF), I(1), NULL],
    "classes-mixed": [TRUE, I(3), S(b"m"), NULL, F(2.5), FALSE, MISSING, S(b"")],
    "all-null": [NULL, NULL, NULL],
    "all-missing": [MISSING, MISSING],
    "null-and-missing": [NULL, MISSING, NULL],
    "strings-only": [S(b"zz"), S(b""), S(b"m")],
    "empty-string-only": [S(b""), S(b"")],
    "bools-only": [TRUE, FALSE, TRUE],
    "true-only": [TRUE, TRUE],
    "min-identity-with-smaller": [I(MAX64), I(MAX64 - 1)],
    "max-identity-with-larger": [I(MIN64), I(MIN64 + 1)],
    "nan-twice": [F(NAN), F(NAN)],
    "int-below-float-beyond-2p53": [I(2 ** 53 + 1), F(2.0 ** 53 + 2.0)],
}
ARRAY_GROUP = [ARRAY, I(1)]


@functools.lru_cache(maxsize=None)
def pair_groups():
    """every ordered pair of the numeric pool that is well defined"""
    return tuple((a, b) for a in NUMERIC for b in NUMERIC if yardstick([a, b])["well_defined"])


@functools.lru_cache(maxsize=None)
def all_groups():
    """[(name, operands)]: singletons, pairs, directed multisets — every group the GPU tests draw from"""
    out = [("single-%d" % i, list(g)) for i, g in enumerate(SINGLETONS)]
    out += [("pair-%d" % i, list(g)) for i, g in enumerate(pair_groups())]
    out += [(name, list(g)) for name, g in DIRECTED.items()]
    return tuple(out)


# ---------------------------------------------------------------- tables and plans

V, W, G = D("v"), D("w"), D("g")
AGGS = sorted("%s(%s)" % (k, V) for k in KINDS)  # (the planner's order: by text)
AGG_KIND = [a.split("(")[0] for a in AGGS]


def encode(ops):
    n = len(ops)
    tags, pay = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    for i, (t, v) in enumerate(ops):
        tags[i] = t
        if t == T_INT:
            pay[i] = np.int64(v).view(np.uint64)
        elif t == T_FLOAT:
            pay[i] = np.float64(v).view(np.uint64)
        elif t in (T_STRING, T_ARRAY):
            pay[i] = DICT.index(v)
    return tags, pay


def key_name(i):
    return b"k%05d" % i


def table(groups, interleave=True, second=False, key="int", pad_to=0):
    """(g, v[, w]): group i's operands under the INT key i, or (key="dict") under a DICT32 key column whose string is
    key_name(i) — a dictionary-coded key is what the DIRECT tables and their slabs take.
    interleave: rows round-robin over the groups (row j of every group, then row j + 1), so that a batch boundary, a tile or a
    rank split cuts through the groups; else group after group.
    pad_to: rows with a NULL / MISSING operand (they enter none of the six aggregates) after every round, dealt over the groups,
    up to that many rows in all: the rounds, and with them the parts of one group, lie tiles apart.
    second: a second operand column w = v (plans over two operand columns: no 16-byte record, the exact partitioned path)."""
    rows = []
    if interleave:
        depth = max(len(ops) for ops in groups)
        real = sum(len(ops) for ops in groups)
        pad = max(0, pad_to - real)
        for j in range(depth):
            rows += [(i, ops[j]) for i, ops in enumerate(groups) if j < len(ops)]
            share = pad // depth + (1 if j < pad % depth else 0)
            rows += [((j + 7 * p) % len(groups), NULL if p % 2 else MISSING) for p in range(share)]
    else:
        assert not pad_to
        rows = [(i, o) for i, ops in enumerate(groups) for o in ops]
    n = len(rows)
    tags, pay = encode([o for _, o in rows])
    dictionary = list(DICT)
    if key == "int":
        kcol = n1o.Column(G, n1o.COL_TAGGED64, tags=np.full(n, T_INT, np.uint8), payload=np.array([i for i, _ in rows], np.uint64))
    else:
        dictionary += [key_name(i) for i in range(len(groups))]
        kcol = n1o.Column(G, n1o.COL_DICT32, codes=np.array([len(DICT) + i for i, _ in rows], np.uint32))
    cols = [kcol, n1o.Column(V, n1o.COL_TAGGED64, tags=tags, payload=pay)]
    if second:
        cols.append(n1o.Column(W, n1o.COL_TAGGED64, tags=tags.copy(), payload=pay.copy()))
    return n1o.Table(cols, dictionary)


def by_group(result, ngroups, aggs=None):
    """a GroupResult / GroupRows over table() -> [ {kind: (tag, value)} per group ]"""
    kinds = [a.split("(")[0] for a in (aggs or AGGS)]
    out = [None] * ngroups
    for k, a in zip(result.keys, result.aggs):
        i = k[0][1] if k[0][0] == T_INT else int(k[0][1][1:])
        assert k[0][0] in (T_INT, T_STRING) and out[i] is None, k
        out[i] = dict(zip(kinds, a))
    assert all(o is not None for o in out), "a group is missing"
    return out


def window(n, offset=0):
    """n groups of all_groups() from `offset` on, cyclically -> (names, groups)"""
    every = all_groups()
    picked = [every[(offset + i) % len(every)] for i in range(n)]
    return [p[0] for p in picked], [p[1] for p in picked]
