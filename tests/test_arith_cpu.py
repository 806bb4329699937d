"""The arithmetic yardstick (tests/arith_util.py) checked without a GPU: against a hand-written table of the reference's
branches, against the reference's own recorded results, against the C oracle over the whole pools, and for the condition that
makes tests/test_gpu_arith.py fail on a contracted multiply-add in roundFloat."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import arith_util as au
import golden_util as gu
import mathfn_util as mu
import query_amd
from oracle import n1o
from query_amd import _ffi, plan

M = au.MISSING
NAN, PINF, NINF = au.NAN, au.PINF, au.NINF
MIN64, MAX64 = au.MIN64, au.MAX64
F = float

# (op, arguments, expected), written down from the Go text, at least one line per branch.  An expected int is an INT, an
# expected float a FLOAT: the kind is checked here (the yardstick's own kind), "nan" is any NaN.
SPECIALS = [
    # intValue.Add (integer.go:266-277): same sign and no overflow keeps the int64; everything else is float64(a) + float64(b)
    ("+", [2, 3], 5), ("+", [-2, -3], F(-5)),               # (the fold starts at int 0: 0 + -2 is mixed-sign, a FLOAT from there on)
    ("+", [MAX64, 1], F(2 ** 63)), ("+", [2 ** 62, 2 ** 62], F(2 ** 63)),      # same-sign overflow
    ("+", [5, -3], F(2)), ("+", [0, -1], F(-1)), ("+", [2 ** 53 + 1, -1], F(2 ** 53 - 1)),  # mixed sign: a FLOAT, through float64 (2^53 + 1 is 2^53 there)
    ("+", [1, 0.5], 1.5), ("+", [0.5, 1], 1.5), ("+", [0.5, 0.5], F(1)), ("+", [PINF, NINF], "nan"),
    ("+", [1, 2, 3, 4], 10), ("+", [2 ** 62, 2 ** 62, -(2 ** 62)], F(2 ** 62)), ("+", [], 0),
    ("+", [1, None], None), ("+", [None, 1, M], M), ("+", ["a", 1], None), ("+", [M, None], M), ("+", [True, 2], None),
    # intValue.Sub (integer.go:339-348): Add(-n) unless n is MinInt64
    ("-", [5, 3], F(2)), ("-", [5, -3], 8), ("-", [-5, 3], -8), ("-", [0, MIN64], F(2 ** 63)), ("-", [-1, MIN64], F(2 ** 63)),
    ("-", [MIN64, 1], F(-(2 ** 63))), ("-", [MAX64, -1], F(2 ** 63)), ("-", [2.5, 1], 1.5), ("-", [1, 2.5], -1.5),
    ("-", [M, 1], M), ("-", [None, M], M), ("-", [None, 1], None), ("-", [1, "a"], None),
    # intValue.Mult (integer.go:319-329): `this == 0 || rv / this == n`
    ("*", [3, 4], 12), ("*", [0, MIN64], 0), ("*", [MIN64, 0], 0), ("*", [3037000500, 3037000500], F(3037000500) * F(3037000500)),
    ("*", [3037000499, 3037000499], 3037000499 ** 2), ("*", [-1, MIN64], MIN64), ("*", [MIN64, -1], F(2 ** 63)),
    ("*", [2 ** 32, 2 ** 32], F(2 ** 64)), ("*", [2 ** 62, 2], F(2 ** 63)), ("*", [2 ** 62, -2], MIN64), ("*", [2, 0.5], F(1)),
    ("*", [2, 3, 4], 24), ("*", [], 1), ("*", [M, 2], M), ("*", [2, None], None), ("*", [None, M], M), ("*", [1e300, 1e300], PINF),
    # Neg (integer.go:331-337, float.go:375-377)
    ("neg", [5], -5), ("neg", [0], 0), ("neg", [MIN64], F(2 ** 63)), ("neg", [MAX64], -MAX64), ("neg", [2.5], -2.5), ("neg", [0.0], -0.0),
    ("neg", [M], M), ("neg", [None], None), ("neg", ["a"], None),
    # Div.Apply (arith_div.go:46-64): a zero divisor of any kind is NULL, the quotient goes through NewValue
    ("/", [5, 2], 2.5), ("/", [6, 2], 3), ("/", [5, 0], None), ("/", [5, 0.0], None), ("/", [5, -0.0], None), ("/", [0, 5], 0),
    ("/", [MIN64, -1], F(2 ** 63)), ("/", [2 ** 53 + 1, 1], 2 ** 53), ("/", [1, PINF], 0), ("/", [PINF, PINF], "nan"),
    ("/", [M, 0], M), ("/", [0, M], M), ("/", ["a", 0], None), ("/", ["a", 2], None), ("/", [2, "a"], None), ("/", [None, 2], None),
    # Mod.Apply (arith_mod.go:48-66): math.Mod, the sign of the dividend
    ("%", [7, 3], 1), ("%", [-7, 3], -1), ("%", [7, -3], 1), ("%", [7.5, 2], 1.5), ("%", [5, 0], None), ("%", [5, 0.0], None),
    ("%", [5, -0.0], None), ("%", [-2.5, 0.5], 0), ("%", [PINF, 2], "nan"), ("%", [7, PINF], 7), ("%", [MIN64, -1], 0),
    ("%", [M, 2], M), ("%", [2, M], M), ("%", [None, 2], None), ("%", [2, "a"], None),
    # IDiv / IMod (integer.go:279-313, float.go:335-369)
    ("idiv", [7, 2], 3), ("idiv", [-7, 2], -3), ("idiv", [7, -2], -3), ("idiv", [7, 0], None), ("idiv", [7, 0.0], None), ("idiv", [7, -0.0], None),
    ("idiv", [MIN64, -1], MIN64), ("idiv", [7, 2.9], 3), ("idiv", [7.9, 2], 3), ("idiv", [7.9, 2.9], 3), ("idiv", [-7.9, 2], -3),
    ("idiv", [7.5, 0], None), ("idiv", [7.5, 0.0], None), ("idiv", [7, 0.5], None), ("idiv", [1e300, 2], MIN64 // 2), ("idiv", [NAN, 1], MIN64),
    ("idiv", [7, PINF], 0), ("idiv", [MIN64, -1.0], MIN64), ("idiv", [M, 0], M), ("idiv", [0, M], M), ("idiv", [None, 1], None), ("idiv", [1, "a"], None),
    ("imod", [7, 2], 1), ("imod", [-7, 2], -1), ("imod", [7, -2], 1), ("imod", [7, 0], None), ("imod", [7, 0.0], None), ("imod", [7, -0.0], None),
    ("imod", [MIN64, -1], 0), ("imod", [7, 2.9], 1), ("imod", [7.9, 2], 1), ("imod", [7.9, 4.9], 3), ("imod", [7.5, 0], None), ("imod", [7, 0.5], None),
    ("imod", [7, PINF], 7), ("imod", [NAN, 3], -2), ("imod", [M, 1], M), ("imod", [None, M], M), ("imod", [None, 1], None),
    # Abs / Ceil / Floor / Sign / Sqrt: float64 in, NewValue out
    ("abs", [-5], 5), ("abs", [MIN64], F(2 ** 63)), ("abs", [-2.5], 2.5), ("abs", [-0.0], 0), ("abs", [NINF], PINF), ("abs", [2 ** 53 + 1], 2 ** 53),
    ("abs", [M], M), ("abs", [None], None), ("abs", [True], None),
    ("ceil", [-0.5], 0), ("ceil", [1.4], 2), ("ceil", [2 ** 53 + 1], 2 ** 53), ("ceil", [au.BELOW_2_63], int(au.BELOW_2_63)), ("ceil", [PINF], PINF),
    ("ceil", [NAN], "nan"), ("ceil", [M], M), ("ceil", ["a"], None),
    ("floor", [-0.5], -1), ("floor", [1.7], 1), ("floor", [2.0 ** 63], F(2 ** 63)), ("floor", [-(2.0 ** 63)], MIN64), ("floor", [M], M), ("floor", [None], None),
    ("sign", [NAN], 0), ("sign", [-3], -1), ("sign", [2.5], 1), ("sign", [0], 0), ("sign", [-0.0], 0), ("sign", [NINF], -1), ("sign", [M], M), ("sign", [[1, 2]], None),
    ("sqrt", [-0.0], 0), ("sqrt", [4], 2), ("sqrt", [2], math.sqrt(2.0)), ("sqrt", [-1], "nan"), ("sqrt", [PINF], PINF), ("sqrt", [M], M), ("sqrt", [None], None),
    # Round.Apply / roundFloat: half away from zero, an exact .5 to the even neighbour
    ("round", [2.5], 2), ("round", [3.5], 4), ("round", [-2.5], -2), ("round", [0.5], 0), ("round", [1.5], 2), ("round", [2.4], 2), ("round", [-2.6], -3),
    ("round", [NAN], "nan"), ("round", [NINF], NINF), ("round", [MAX64], F(2 ** 63)), ("round", [M], M), ("round", [None], None), ("round", ["a"], None),
    ("round", [1.8343534, 3], 1.834), ("round", [8.8343534, -1], 10), ("round", [2.675, 2], 2.68), ("round", [1.005, 2], 1), ("round", [0.285, 2], 0.28),  # (1.005 * 100 is 100.49999999999999 in float64, 0.285 * 100 is 28.499999999999996)
    ("round", [1234, -2], 1200), ("round", [1250, -2], 1200), ("round", [1350, -2], 1400),
    ("round", [7, 2.5], None), ("round", [7, NAN], None), ("round", [7, 2.0], 7), ("round", [7, M], M), ("round", [7, None], None), ("round", [7, "a"], None),
    ("round", [M, None], M), ("round", [None, M], None), ("round", ["a", M], None),   # (the first argument decides first)
    ("round", [7, 400], "nan"), ("round", [7, -400], "nan"), ("round", [7, PINF], "nan"), ("round", [7, NINF], "nan"), ("round", [7, 1e300], "nan"),
    ("round", [PINF, 400], PINF), ("round", [0, 400], "nan"),
    # the issue's four inputs: two roundings, product then sum
    ("round", [au.HEX[0], 2], 80548699656784.56), ("round", [au.HEX[1], 2], 73160693336096.48), ("round", [au.HEX[2], 1], 710989620181218),
    ("round", [au.HEX[3], -1], 73160693336096480),
    # Trunc.Apply / truncateFloat
    ("trunc", [2.9], 2), ("trunc", [-2.9], -2), ("trunc", [-0.5], 0), ("trunc", [-2.2544, 2], -2.25), ("trunc", [0.2544, 3], 0.254), ("trunc", [1299, -2], 1200),
    ("trunc", [7, 2.5], None), ("trunc", [7, M], M), ("trunc", [None, M], None), ("trunc", [M, 2], M), ("trunc", [7, "a"], None), ("trunc", [NAN, 2], "nan"),
    ("trunc", [PINF, 2], PINF), ("trunc", [7, 400], "nan"), ("trunc", [7, -400], "nan"), ("trunc", [PINF, PINF], "nan"),
]


def matches_special(got, want):
    if isinstance(want, str):
        return isinstance(got, float) and got != got
    if want is M or want is None:
        return got is want
    return type(got) is type(want) and got == want and (got != 0 or not isinstance(got, float) or math.copysign(1, got) == math.copysign(1, want))


def test_the_yardstick_gives_the_hand_written_table():
    bad = [(op, args, want, au.apply(op, args)) for op, args, want in SPECIALS if not matches_special(au.apply(op, args), want)]
    assert not bad, bad[:8]
    # every op has lines, and the cases the kernels are most likely to get wrong are among them
    assert {op for op, _a, _w in SPECIALS} == set(au.OPS)
    required = [("+", [MAX64, 1]), ("+", [5, -3]), ("idiv", [MIN64, -1]), ("imod", [MIN64, -1]), ("neg", [MIN64]), ("-", [0, MIN64]), ("/", [5, 0]),
                ("/", [5, 0.0]), ("/", [5, -0.0]), ("abs", [MIN64]), ("sqrt", [-0.0]), ("ceil", [-0.5]), ("sign", [NAN]), ("round", [2.5]), ("round", [3.5]),
                ("round", [-2.5]), ("round", [7, 2.5])]
    have = [(op, args) for op, args, _w in SPECIALS]
    assert all(any(op == o and repr(args) == repr(a) for o, a in have) for op, args in required)


def test_the_pools_hold_every_required_value():
    ints = [0, 1, -1, 2, -2, 3, 7, -7, 10, 2 ** 31 - 1, 2 ** 31, -(2 ** 31), 2 ** 32, 2 ** 32 + 1, 3037000499, 3037000500, -3037000500, 2 ** 52 + 1,
            2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 62, -(2 ** 62), 2 ** 62 + 1, 2 ** 63 - 2, 2 ** 63 - 1, -(2 ** 63), -(2 ** 63) + 1]
    assert all(any(isinstance(p, int) and not isinstance(p, bool) and p == v for p in au.VALUE_POOL) for v in ints)
    bits = lambda f: np.float64(f).view(np.uint64)  # noqa: E731  (-0.0 is not 0.0 here)
    floats = [0.0, -0.0, 0.5, -0.5, 1.5, 2.5, -2.5, 3.5, 0.125, 7.0, 2.675, 1.005, 0.285, 1e-7, 5e-324, 2.2250738585072014e-308, 1e22, 1e23,
              2.0 ** 52 + 0.5, 2.0 ** 53, 2.0 ** 63, -(2.0 ** 63), 9223372036854774784.0, 1e300, -1e300, 1.7976931348623157e308, PINF, NINF]
    floats += [s * float.fromhex(h) for s in (1, -1) for h in ("0x1.2508d28549423p+46", "0x1.0a28348d2081ep+46", "0x1.435215dffc70fp+49", "0x1.03eb4351d1bedp+56")]
    have = {int(bits(p)) for p in au.VALUE_POOL if isinstance(p, float)}
    assert all(int(bits(v)) in have for v in floats) and any(isinstance(p, float) and p != p for p in au.VALUE_POOL)
    assert au.BELOW_2_63 == 9223372036854774784.0
    others = [p for p in au.VALUE_POOL if not au.is_num(p)]
    assert any(p is M for p in others) and any(p is None for p in others) and True in others and "a" in others
    assert any(isinstance(p, list) for p in others) and any(isinstance(p, dict) for p in others)
    digits = [0, 1, -1, 2, -2, 3, -3, 15, 16, 17, 22, -22, 2.5, PINF, NINF, 400, -400, 1e300, 23, 30, -30, "a"]
    assert all(any(type(p) is type(v) and p == v for p in au.DIGIT_POOL) for v in digits)
    assert any(isinstance(p, float) and p == 2.0 for p in au.DIGIT_POOL) and any(isinstance(p, float) and p != p for p in au.DIGIT_POOL)
    assert any(p is M for p in au.DIGIT_POOL) and any(p is None for p in au.DIGIT_POOL)
    assert set(au.FOLD_POOL) - {M, None} == {2 ** 62, -(2 ** 62), 2 ** 63 - 1, 1, -1, 0.5} and len(au.FOLD_POOL) == 8
    # the exception cannot spread: exactly the three listed digit counts are judged with a tolerance
    assert [d for d in au.DIGIT_POOL if au.is_loose("round", [1, d])] == list(au.LOOSE_DIGITS)
    assert all(math.pow(10, p) == au.pow10(p) for p in range(-22, 23))  # (what gu.round_float computes is the exact power)


# ------------------------------------------------------------------ the reference's own recorded results

_TOK = re.compile(r"\s*(?:(\d+(?:\.\d+)?(?:[eE][-+]?\d+)?)|([a-z_][a-z_0-9]*)|(.))")
_NULLARY = {"nan": NAN, "posinf": PINF, "neginf": NINF}


def parse_constant_expression(s):
    """the stringer text of a constant arithmetic expression -> a node of tests/arith_util.py (None: something else)"""
    toks = [m.groups() for m in _TOK.finditer(s) if any(m.groups())]
    pos = [0]

    def peek():
        return toks[pos[0]] if pos[0] < len(toks) else (None, None, None)

    def take(ch=None):
        t = peek()
        if ch is not None and t[2] != ch:
            raise ValueError(s)
        pos[0] += 1
        return t

    def number(text, neg):
        v = gu.fold_number(int(text)) if re.fullmatch(r"\d+", text) else mu.new_value(float(text))
        return ("const", -v if neg else v)

    def expr():
        num, name, ch = peek()
        if num is not None:
            take()
            return number(num, False)
        if ch == "-":
            take()
            num2 = take()[0]
            if num2 is None:
                raise ValueError(s)
            return number(num2, True)
        if name is not None:
            take()
            take("(")
            args = []
            while peek()[2] != ")":
                args.append(expr())
                if peek()[2] == ",":
                    take()
            take(")")
            if name in _NULLARY and not args:
                return ("const", _NULLARY[name])
            if name not in au.OPS:
                raise ValueError(s)
            return ("op", name, args)
        take("(")
        if peek()[2] == "-" and toks[pos[0] + 1][0] is None:  # (-expr)
            take()
            e = ("op", "neg", [expr()])
            take(")")
            return e
        first = expr()
        if peek()[2] == ")":
            take()
            return first
        args, op = [first], None
        while peek()[2] != ")":
            o = take()[2]
            if o not in ("+", "-", "*", "/", "%") or (op is not None and o != op):
                raise ValueError(s)
            op = o
            args.append(expr())
        take(")")
        return ("op", op, args)

    try:
        e = expr()
        return e if pos[0] == len(toks) else None
    except (ValueError, IndexError, TypeError):
        return None


def reference_statements():
    out = []
    with open(os.path.join(gu.GOLDEN, "cases_num.json")) as fh:
        cases = gu.load_cases() + json.load(fh)["cases"]
    for c in cases:
        for alias, text in c["plan"].get("exprs", []):
            e = parse_constant_expression(text)
            if e is not None and e[0] == "op":
                out.append((c["id"], text, e, c["results"][0].get(alias, M)))
    return out


def test_the_yardstick_gives_the_references_recorded_results():
    stmts = reference_statements()
    ops = {e[1] for _i, _t, e, _w in stmts}
    assert len(stmts) >= 25 and {"+", "-", "*", "/", "idiv", "imod", "round", "trunc", "ceil", "floor", "abs", "sign", "sqrt"} <= ops, (len(stmts), ops)
    for cid, text, e, want in stmts:
        got = au.eval_node(e, {})
        # (a JSON result has no INT / FLOAT kind; as numbers they are the same bits: repr round-trips)
        assert au.same_exact(got, want), (cid, text, got, want)


# ------------------------------------------------------------------ the C oracle, over the whole pools

def decode(tv):
    return au._norm(gu.decode_value(tv))


def sweep(form_or_node, rows, name=None):
    e = au.FORMS[form_or_node][0] if isinstance(form_or_node, str) else form_or_node
    got = n1o.eval_expr(au.table(rows), au.text(e))
    bad = []
    for r, g in zip(rows, got):
        args = [au.eval_node(a, r) for a in e[2]]
        want = au.apply(e[1], args)
        if not au.same(e[1], args, decode(g), want):
            bad.append((au.text(e), args, decode(g), want))
    return bad


@pytest.mark.parametrize("form", sorted(au.FORMS))
def test_the_oracle_agrees_with_the_yardstick_over_the_pools(form):
    """every unary op over the value pool, every binary op over all ordered pairs, ROUND / TRUNC over value x digits"""
    rows = au.ROWS[au.FORMS[form][1]]()
    assert len(rows) >= {"unary": len(au.VALUE_POOL), "pair": len(au.VALUE_POOL) ** 2, "digit": len(au.VALUE_POOL) * len(au.DIGIT_POOL)}[au.FORMS[form][1]]
    bad = sweep(form, rows)
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("op", au.NARY)
def test_the_oracle_agrees_on_the_n_ary_folds(op, n):
    rows = au.fold_rows(n)
    assert len(rows) >= 8 ** n
    bad = sweep(au.node(op, *"abce"[:n]), rows)
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("name", sorted(au.NESTED))
def test_the_oracle_agrees_on_a_node_over_a_node(name):
    e = au.NESTED[name]
    rows = au.pair_rows()
    got = n1o.eval_expr(au.table(rows), au.text(e))
    bad = [(r["v"], r["w"], decode(g), au.eval_node(e, r)) for r, g in zip(rows, got) if not au.same_exact(decode(g), au.eval_node(e, r))]
    assert not bad, (len(bad), bad[:6])


# ------------------------------------------------------------------ sensitivity: the inputs tell one rounding from two

def test_the_round_rows_tell_a_contracted_multiply_add_from_two_roundings():
    """roundFloat computes x * pow + 0.5 with two roundings (Go on amd64 does not fuse).  A device compiler may contract it
    into one fused multiply-add.  For every (value, digits) row of the ROUND test the once-rounded intermediate is computed
    exactly and run through the rest of roundFloat: enough rows must then differ from the yardstick, in both directions of
    the digits, for the GPU test to fail on a contracted kernel."""
    differ = []
    for r in au.digit_rows():
        v, d = r["v"], r["d"]
        if not (au.is_num(v) and au.is_num(d)) or au.is_loose("round", [v, d]):
            continue
        p = au.digits_of(d)
        x = float(v)
        if p is None or abs(p) > 22 or x != x or math.isinf(x):
            continue
        two, one = au.round_float(x, p), au.fused_intermediate_result(x, p)
        if not au.same_exact(mu.new_value(one), mu.new_value(two)):
            differ.append((v, p))
    differ = sorted(set(differ), key=repr)
    assert len(differ) >= 8, differ
    assert sum(1 for _v, p in differ if p >= 1) >= 2 and sum(1 for _v, p in differ if p <= -1) >= 2, differ
    # the four derived inputs are among them, at their digits
    assert {(au.HEX[0], 2), (au.HEX[1], 2), (au.HEX[2], 1), (au.HEX[3], -1)} <= set(differ)


# ------------------------------------------------------------------ the fused shapes are shapes the run-time-built scan takes

def fused_plan(nodes, key="id"):
    return None, [au.D(key)], ["max(%s)" % au.text(e) for e in nodes]


@pytest.mark.parametrize("group", au.FUSED_GROUPS, ids=au.FUSED_IDS)
def test_the_fused_groups_are_shapes_of_the_runtime_built_scan(group):
    """tests/test_gpu_arith.py asserts spec_kernel == 3 on the device.  That build_fast_args takes each group of nodes with its
    arithmetic in registers, and that the shape compiles for gfx950, is decided on the host (n1k_jit_check) — here with a
    DICT32 key in the place of `id`: the layout of a TAGGED64 key needs its value tables on a device."""
    nodes, _rows = au.fused_group_nodes(group)
    cond, keys, aggs = fused_plan(nodes, key="k")
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs))
    try:
        assert len(op.column_paths) <= 3 and op.column_paths[0] == au.D("k")
        kinds = np.array([_ffi.COL_DICT32] + [_ffi.COL_TAGGED64] * (len(op.column_paths) - 1), dtype=np.uint32)
        log = C.create_string_buffer(8192)
        st = _ffi.lib().n1k_jit_check(op._h, kinds.ctypes.data, len(kinds), log, 8192)
        assert st == _ffi.OK, (st, aggs, log.value.decode(errors="replace"))
    finally:
        op.done()


def test_the_library_takes_every_plan_of_the_gpu_tests():
    """tests/test_gpu_arith.py counts a refusal as a failure: every plan it runs is one n1k_create accepts"""
    import test_gpu_arith as tg
    all_plans = tg.plans()
    assert len(all_plans) > 70
    for cond, keys, aggs, having, project in all_plans:
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs, having=having, project=project))
        assert len(op.column_paths) >= 1
        op.done()
