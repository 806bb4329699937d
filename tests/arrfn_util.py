"""Array functions yardstick shared by tests/test_arrfn_cpu.py and tests/test_gpu_arrfn.py.

`apply` restates, over Python lists, the six Apply functions of expression/func_array.go: ArrayLength (:888-897), ArrayCount
(:376-393), ArraySum (:1911-1928), ArrayAvg (:141-164), ArrayContains (:307-323), ArrayPosition (:1094-1110).  MISSING for a
MISSING first (or second) argument, NULL for a first argument that is no ARRAY (or a NULL second one), in the reference's
order.  Elements are typed by `new_value`, the way func_array.go types them: value.NewValue(x) over
arg.Actual().([]interface{}) — the array went through encoding/json, so every number is a float64 first and an integral one
folds to int64 (value/value.go:367-381, value/parsed.go:120-122, 362): 2^53 + 1 is the INT 2^53.  array_sum adds with
`num_add`, intValue.Add / floatValue.Add (value/integer.go:266-277): INT while both are INTs of one sign and the sum does not
wrap, else through float64 — from INT 0, so a leading negative INT already makes the sum a FLOAT.

A result is (tag, payload): the N1K_T_* tag and the 64 payload bits (INT: two's complement, FLOAT: the float64's), compared
bit for bit.  A second argument is a Python value, or MISSING.
"""
from __future__ import annotations

import ctypes as C
import json
import random
import struct
from typing import List, Sequence

import numpy as np

import coll_util as cu
import like_util as lu
from oracle import n1o
from query_amd import _ffi, plan

MISSING = cu.MISSING
FUNCTIONS = ("array_length", "array_count", "array_sum", "array_avg", "array_contains", "array_position")
UNARY, BINARY = FUNCTIONS[:4], FUNCTIONS[4:]
MAX_TERMS = 4  # kArrFnMaxTerms
DEV_MAX_LEN = 192  # bytes of canonical text arrfn_table_kernel takes (include/n1k.h, n1k_arrfn_eval_device)

T_MISSING, T_NULL, T_FALSE, T_TRUE, T_INT, T_FLOAT = n1o.T_MISSING, n1o.T_NULL, n1o.T_FALSE, n1o.T_TRUE, n1o.T_INT, n1o.T_FLOAT
R_MISSING, R_NULL, R_TRUE, R_FALSE = (T_MISSING, 0), (T_NULL, 0), (T_TRUE, 0), (T_FALSE, 0)


# ---------------------------------------------------------------- the yardstick

def f64_bits(f: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", f))[0]


def r_int(v: int):
    return (T_INT, v & 0xFFFFFFFFFFFFFFFF)


def r_float(f: float):
    return (T_FLOAT, f64_bits(f))


def is_number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def is_int_f64(f: float) -> bool:
    """value.IsInt (value/integer.go:354-356): x == float64(int64(x)), where int64 of an out-of-range x is MinInt64"""
    return -9223372036854775808.0 <= f < 9223372036854775808.0 and f == int(f)


def new_value(x):
    """value.NewValue over one element of the decoded array: a NUMBER through float64"""
    if not is_number(x):
        return x
    f = float(x)
    return int(f) if is_int_f64(f) else f


def num_add(a, b):
    """NumberValue.Add over new_value numbers (int = intValue, float = floatValue)"""
    if isinstance(a, int) and isinstance(b, int):
        rv = (a + b + 2 ** 63) % 2 ** 64 - 2 ** 63
        if (a >= 0 and b >= 0 and rv >= 0) or (a < 0 and b < 0 and rv < 0):
            return rv
    return float(a) + float(b)


def result_of_number(v):
    return r_int(v) if isinstance(v, int) else r_float(v)


def equals_truth(c, e) -> bool:
    """c.Equals(e).Truth() for a constant c above NULL and a typed element e"""
    if e is None or cu._cls(c) != cu._cls(e):
        return False
    if is_number(c):
        return c == e if isinstance(c, int) and isinstance(e, int) else float(c) == float(e)
    if isinstance(c, str):
        return c.encode() == e.encode()
    return c is e  # booleans


def apply(fn: str, a, c=None):
    """(tag, payload) of fn(a[, c]); `a` is a Python value or MISSING"""
    binary = fn in BINARY
    if a is MISSING or (binary and c is MISSING):
        return R_MISSING
    if not isinstance(a, list) or (binary and c is None):
        return R_NULL
    elems = [new_value(x) for x in a]
    if fn == "array_length":
        return r_int(len(elems))
    if fn == "array_count":
        return r_int(sum(1 for e in elems if e is not None))
    if fn in ("array_sum", "array_avg"):
        total, count = 0, 0
        for e in elems:
            if is_number(e):
                total = num_add(total, e)
                count += 1
        if fn == "array_sum":
            return result_of_number(total)
        if count == 0:
            return R_NULL
        return result_of_number(new_value(float(total) / float(count)))
    for i, e in enumerate(elems):
        if equals_truth(c, e):
            return R_TRUE if fn == "array_contains" else r_int(i)
    return R_FALSE if fn == "array_contains" else r_int(-1)


def result_json(r):
    """a (tag, payload) result as the JSON value a recorded result holds"""
    t, p = r
    if t in (T_MISSING, T_NULL):
        return None
    if t in (T_TRUE, T_FALSE):
        return t == T_TRUE
    if t == T_INT:
        return p - 2 ** 64 if p >= 2 ** 63 else p
    return struct.unpack("<d", struct.pack("<Q", p))[0]


def result_value(r):
    """a (tag, payload) result as a mirror value (cond_util.to_tagged takes it): MISSING, None, bool, int or float"""
    return MISSING if r[0] == T_MISSING else result_json(r)


# ---------------------------------------------------------------- text

def D(name):
    return plan.field_path("default", name)


def const_text(c) -> str:
    """a second argument as the stringer writes a constant (a negative number in parentheses)"""
    if c is MISSING:
        return "missing"
    if is_number(c) and (c < 0 or (c == 0 and str(c).startswith("-"))):
        return "(%s)" % cu.canon(c) if isinstance(c, int) else "(%s)" % repr(c)
    if isinstance(c, float):
        return repr(c)
    return cu.canon(c)


def term_text(fn: str, c=None, over: str = "(`d`.`a`)") -> str:
    return "%s(%s)" % (fn, over) if fn in UNARY else "%s(%s, %s)" % (fn, over, const_text(c))


# ---------------------------------------------------------------- seeded material
# a small alphabet, so that hits are common; every element class, numbers on both sides of every typing rule
STRINGS = ["a", "b", "ab", "t_1", "", "é", 'x"y', "a\\b", "a\nb"]
NUMBERS = [0, 1, 2, -1, -3, 7, 1.5, 2.5, -0.5, 0.1, -0.0, 3.0, 2 ** 53, 2 ** 53 + 1, -(2 ** 53) - 1, 2 ** 62, 2 ** 63 - 1, -(2 ** 63), 2 ** 63, 10 ** 20,
           1e-7, 123456789012345.5, 1e300, 999999999999999999, 1234567890123456789]
CONSTS = ["a", "ab", "t_1", "", 'x"y', "é", 0, 1, 2, -1, 1.5, 3.0, 2 ** 53, 2 ** 53 + 1, 1e300, 10 ** 20, True, False, None, MISSING]


def random_element(rng: random.Random, depth: int = 0):
    r = rng.random()
    if r < 0.3:
        return rng.choice(STRINGS)
    if r < 0.7:
        return rng.choice(NUMBERS)
    if r < 0.85 or depth >= 2:
        return rng.choice([None, True, False])
    if r < 0.93:
        return [random_element(rng, depth + 1) for _ in range(rng.randint(0, 3))]
    return {f: random_element(rng, depth + 1) for f in ("f", "g") if rng.random() < 0.6}


def random_array(rng: random.Random):
    r = rng.random()
    if r < 0.08:
        return [None] * rng.randint(1, 4)
    if r < 0.3:  # numbers only: sums that stay INT, overflow to FLOAT, mix INT and FLOAT
        return [rng.choice(NUMBERS) for _ in range(rng.randint(1, 6))]
    return [random_element(rng) for _ in range(rng.choice([0, 1, 1, 2, 3, 4, 6, 9]))]


def random_term(rng: random.Random):
    """(function, second argument or None)"""
    fn = rng.choice(FUNCTIONS)
    return fn, (rng.choice(CONSTS) if fn in BINARY else None)


def random_pairs(seed: int, nterms: int, per_term: int):
    """[(function, constant, [array...])]: nterms seeded terms — every function at least nterms // 6 times — with per_term arrays each"""
    rng = random.Random(seed)
    out = []
    for k in range(nterms):
        fn = FUNCTIONS[k % len(FUNCTIONS)]
        c = rng.choice(CONSTS) if fn in BINARY else None
        arrays = [random_array(rng) for _ in range(per_term)]
        if fn in BINARY and c is not None and c is not MISSING:  # hits: the constant itself among the elements of every third array
            for a in arrays[::3]:
                a.insert(rng.randint(0, len(a)), c)
        out.append((fn, c, arrays))
    return out


def texts_of(arrays: Sequence) -> List[bytes]:
    return [cu.canon(a).encode() for a in arrays]


def loads(text: bytes):
    """the decoded array as Python holds it: integers exact (new_value makes float64s of them)"""
    return json.loads(text.decode())


def want_block(fn, c, texts: Sequence[bytes]):
    """the yardstick over a block of dictionary entries: an entry that is no array text is NULL"""
    tags, pay = np.zeros(len(texts), np.uint8), np.zeros(len(texts), np.uint64)
    for i, t in enumerate(texts):
        r = apply(fn, loads(t), c) if len(t) >= 2 and t[:1] == b"[" else R_NULL
        tags[i], pay[i] = r
    return tags, pay


# ---------------------------------------------------------------- the library's evaluators

def host_eval(term: str, texts: Sequence[bytes]):
    """n1k_arrfn_eval over a block of canonical texts: (tags, payload); raises on a status other than N1K_OK"""
    offs, blob = lu.pack(texts)
    tags = np.full(max(len(texts), 1), 99, dtype=np.uint8)
    pay = np.full(max(len(texts), 1), 0xDEAD, dtype=np.uint64)
    t = term.encode()
    st = _ffi.lib().n1k_arrfn_eval(t, len(t), len(texts), offs.ctypes.data, blob, tags.ctypes.data, pay.ctypes.data)
    if st != _ffi.OK:
        raise RuntimeError("n1k_arrfn_eval: status %d for %s" % (st, term))
    return tags[:len(texts)], pay[:len(texts)]


def host_status(term: bytes) -> int:
    offs, blob = lu.pack([b"[]"])
    tags, pay = np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    return _ffi.lib().n1k_arrfn_eval(term, len(term), 1, offs.ctypes.data, blob, tags.ctypes.data, pay.ctypes.data)


def device_eval(term: str, texts: Sequence[bytes], device: int = 0):
    """n1k_arrfn_eval_device: (tags, payload, arrays left to the host evaluator)"""
    offs, blob = lu.pack(texts)
    tags = np.full(max(len(texts), 1), 99, dtype=np.uint8)
    pay = np.full(max(len(texts), 1), 0xDEAD, dtype=np.uint64)
    left = C.c_uint64(0)
    t = term.encode()
    st = _ffi.lib().n1k_arrfn_eval_device(device, t, len(t), len(texts), offs.ctypes.data, blob, tags.ctypes.data, pay.ctypes.data, C.byref(left))
    if st != _ffi.OK:
        raise RuntimeError("n1k_arrfn_eval_device: status %d for %s" % (st, term))
    return tags[:len(texts)], pay[:len(texts)], int(left.value)


# ---------------------------------------------------------------- a table with an array column
#
# a: every value class, arrays of every element class among them (TAGGED64); x: numbers, some NULL / MISSING (TAGGED64);
# g: small ints (TAGGED64); k, s: strings with NULL / MISSING (DICT32).

WORDS = ["", "a", "ab", "b", "t_1", "cat_1", "cat_2", "cat_3"]
TABLE_ARRAYS = [[], [None], [None, None], ["a"], ["t_1", "a"], [1, 2], [7, 18, 16], [-3, -2, -1, 0, 1, 2, 3, 4], [1.5, 2], [0.5, 0.25, "a"], [-0.0],
                [2 ** 62, 2 ** 62], [2 ** 53 + 1], [2 ** 53, 1], ['x"y', "a"], ["a", 'x"y'], [{"f": 1}, [1, 2], None, "a"], [[1], [2, [3]]],
                [True, False, 1], ["a", "a", "ab", "a"], list(range(40)), ["t_1"] * 50, [1234567890123456789, 1], [3.0, 1e300], [10 ** 20]]
OTHERS = [MISSING, None, True, False, 0, 3, 2.5, "a", "t_1", {"f": 1}, {}]
ROW_DICT = [w.encode() for w in WORDS] + texts_of(TABLE_ARRAYS) + [cu.canon(v).encode() for v in ({"f": 1}, {})]
ROW_CODE = {bytes(b): i for i, b in enumerate(ROW_DICT)}


def to_tagged(values):
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
            tags[i], pay[i] = n1o.T_INT, v & 0xFFFFFFFFFFFFFFFF
        elif isinstance(v, float):
            tags[i], pay[i] = n1o.T_FLOAT, f64_bits(v)
        elif isinstance(v, str):
            tags[i], pay[i] = n1o.T_STRING, ROW_CODE[v.encode()]
        else:
            tags[i], pay[i] = (n1o.T_ARRAY if isinstance(v, list) else n1o.T_OBJECT), ROW_CODE[cu.canon(v).encode()]
    return tags, pay


def make_rows(rng: random.Random, n: int):
    rows = []
    for _ in range(n):
        r = rng.random()
        a = rng.choice(TABLE_ARRAYS) if r < 0.75 else rng.choice(OTHERS)
        r = rng.random()
        x = MISSING if r < 0.04 else (None if r < 0.08 else (rng.randrange(0, 100) if r < 0.5 else rng.randrange(0, 800) / 8.0 + 0.0625))
        r = rng.random()
        k = MISSING if r < 0.03 else (None if r < 0.07 else rng.choice(WORDS[5:]))
        r = rng.random()
        s = MISSING if r < 0.06 else (None if r < 0.12 else rng.choice(WORDS[:5]))
        rows.append({"a": a, "x": x, "g": rng.randrange(0, 7), "k": k, "s": s})
    return rows


def dict_codes(values):
    return np.array([0xFFFFFFFF if v is MISSING else (0xFFFFFFFE if v is None else ROW_CODE[v.encode()]) for v in values], np.uint32)


def column(name, values):
    t, p = to_tagged(values)
    return n1o.Column(D(name), n1o.COL_TAGGED64, tags=t, payload=p)


def make_table(rows):
    cols = [column(name, [r[name] for r in rows]) for name in ("a", "x", "g")]
    cols += [n1o.Column(D(name), n1o.COL_DICT32, codes=dict_codes([r[name] for r in rows])) for name in ("k", "s")]
    return n1o.Table(cols, list(ROW_DICT))


# ---------------------------------------------------------------- seeded plans of the differential by substitution
#
# The oracle does not know the functions: where the device's plan holds fn(a[, c]) the oracle's reads the TAGGED64 helper
# column `h` with the yardstick's value of every row.  What is drawn stays where both sides are exact: the helper is compared
# with small constants, summed only where the values are small numbers (array_length / array_count / array_position; the sums
# of array_sum / array_avg over the table's arrays reach 2^63 and 1e300, where the order of a float SUM matters).

USES = ["filter_cmp", "key", "count", "count_distinct", "min", "max", "sum", "avg", "arith_key", "filter_bare"]
SMALL = ("array_length", "array_count", "array_position")
PLAN_CONSTS = ["a", "t_1", 'x"y', 1, 2, 1.5, 3.0, 2 ** 53, True, None]


def draw_plan(seed: int):
    rng = random.Random(770_000 + seed)
    rows = make_rows(rng, rng.randint(1, 1500))
    use = USES[seed % len(USES)]
    fn = rng.choice(SMALL if use in ("sum", "avg", "arith_key") else FUNCTIONS)
    c = rng.choice(PLAN_CONSTS) if fn in BINARY else None
    text, h = term_text(fn, c, over=D("a")), D("h")
    values = [result_value(apply(fn, r["a"], c)) for r in rows]
    where = rng.choice([None, "(10 < %s)" % D("x"), "(%s is not missing)" % D("k"), "(%s = 3)" % D("g")])
    dkeys = okeys = [[D("k")], [D("g")], []][rng.randrange(3)]
    dcond = ocond = where
    if use == "key":
        dkeys, okeys = [text] + dkeys[:1], [h] + okeys[:1]
        daggs = oaggs = sorted(["count(*)", "max(%s)" % D("x")])
    elif use == "arith_key":
        wrap = lambda t: "(%s + %s)" % (t, D("g"))  # noqa: E731
        dkeys, okeys = [wrap(text)], [wrap(h)]
        daggs = oaggs = ["count(*)"]
    elif use in ("filter_cmp", "filter_bare"):
        wrap = (lambda t: "(1 < %s)" % t if seed % 4 < 2 else "(%s = %s)" % (t, D("g"))) if use == "filter_cmp" else (lambda t: t)
        extra = lambda t: wrap(t) if where is None else "(%s and %s)" % (where, wrap(t))  # noqa: E731
        dcond, ocond = extra(text), extra(h)
        daggs = oaggs = sorted(["count(*)", "max(%s)" % D("x")])
    else:
        f = "count(distinct %s)" if use == "count_distinct" else use + "(%s)"
        daggs, oaggs = [f % text, "count(*)"], [f % h, "count(*)"]
    return {"rows": rows, "use": use, "fn": fn, "const": c, "values": values, "device": (dcond, dkeys, daggs), "oracle": (ocond, okeys, oaggs)}
