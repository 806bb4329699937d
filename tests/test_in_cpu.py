"""IN / NOT IN over a constant list without a GPU: what the parser takes and refuses, the host matcher of a list's strings
against python's set, the yardstick of the GPU differential (in4 against the oracle's OR of equalities), and that every plan
the GPU differential draws is accepted — its bounded ones by the bounded kernel family too."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import golden_util as gu
import in_util as iu
import query_amd
from oracle import n1o
from query_amd import _ffi, plan

D = lambda name: "(`d`.`%s`)" % name  # noqa: E731
MISSING = iu.MISSING


def _create(cond, keys=(), aggs=(), **kw):
    return query_amd.GpuFilterGroup(plan.filter_group_plan(cond, list(keys), list(aggs), filter_only=not aggs and not keys, **kw))


# ------------------------------------------------------------------ the parser

def test_both_spellings_duplicates_and_the_empty_list():
    for cond in ('(%s in ["a", "b", 3, (-4), -5.5, true, false, null])' % D("s"),  # the ArrayConstruct stringer
                 '(%s in ["a","b",3,-4,-5.5,true,false,null])' % D("s"),             # a folded constant's JSON
                 '(%s in [ "a" , "a", "a", 3, 3.0, 3e0 ])' % D("s"),                 # duplicates collapse under Equals
                 '(%s in [])' % D("s"), '(not (%s in []))' % D("s"), '(%s in [(- 4)])' % D("s"),
                 '(5 in [5, 6])', '((%s + 1) in [5, 6])' % D("n"), plan.in_list(D("s"), ["q\"\\\n", -1, -2.5, None, True])):
        op = _create(cond)
        assert op.in_stats() == {"lists": 1, "device_strings": 0, "host_strings": 0, "device_threshold": op.like_stats()["device_threshold"]}, cond
        op.done()
    assert plan.in_list(D("s"), ["a", 3, -4, 2.5, True, None]) == '(%s in ["a", 3, (-4), 2.5, true, null])' % D("s")
    # two terms with the same list text are one list; another spelling of the same constants is another
    op = _create('((%s in ["a", 1]) or (%s in ["a", 1]) or (%s in ["a",1]))' % (D("s"), D("t"), D("s")))
    assert op.in_stats()["lists"] == 2 and op.column_paths == [D("s"), D("t")]
    op.done()


def test_column_paths_in_first_use_order_inside_and_or_not():
    cond = '((%s in ["ab"]) and ((not (%s in [1, "z"])) or (%s is null) or ((%s + 1) in [4])) and (3 < %s))' % (D("s"), D("t"), D("t"), D("n"), D("n"))
    op = _create(cond, [D("k")], ["count(*)"])
    assert op.column_paths == [D("s"), D("t"), D("n"), D("k")] and op.in_stats()["lists"] == 3
    op.done()


def _nums(n, start=0):
    return "[%s]" % ", ".join(str(i) for i in range(start, start + n))


REFUSALS = [
    ("(%s in %s)" % (D("s"), D("t")), "not a constant list (a path)"),
    ("(%s in (select raw 1))" % D("s"), "not a constant list (a subquery)"),
    ("(%s in (%s + 1))" % (D("s"), D("t")), "not a constant list"),
    ("(%s in [%s])" % (D("s"), D("t")), "not a constant (a path"),
    ("(%s in [(1 + 2)])" % D("s"), "not a constant"),
    ("(%s in [[1]])" % D("s"), "nested array or object"),
    ('(%s in [{\\"a\\": 1}])' % D("s"), "nested array or object"),
    ("(%s in [missing])" % D("s"), "missing"),
    ("(%s in [9007199254740993])" % D("s"), "2^53"),
    ("(%s in [-9007199254740993])" % D("s"), "2^53"),
    ("(%s in [1e300])" % D("s"), "2^53"),
    ("(%s in %s)" % (D("s"), _nums(iu.IN_MAX_NUMBERS + 1)), "more than 1024 distinct number"),
    ("((%s in %s) or (%s in %s))" % (D("s"), _nums(1000), D("s"), _nums(25, 2000)), "more than 1024 distinct number"),
    ("(%s in [%s])" % (D("s"), ", ".join('\\"s%d\\"' % i for i in range(iu.IN_MAX_STRINGS + 1))), "more than 4096 distinct strings"),
    ('any `v` in %s satisfies (`v` in [1, 2]) end' % D("a"), "IN inside SATISFIES"),
    ("(%s)" % " or ".join('(%s in [\\"p%d\\"])' % (D("s"), i) for i in range(9)), "more than 8"),
]


@pytest.mark.parametrize("cond,word", REFUSALS, ids=[w for _, w in REFUSALS[:11]] + ["1025 numbers", "1025 numbers in two lists", "4097 strings", "satisfies", "nine bits"])
def test_create_refuses_what_lies_outside_the_subset(cond, word):
    """N1K_UNSUPPORTED with the construct named, never N1K_INVALID."""
    with pytest.raises(query_amd.N1kError) as ei:
        query_amd.GpuFilterGroup(('{"#operator":"Filter","condition":"%s"}' % cond).encode())
    assert ei.value.status == _ffi.UNSUPPORTED and word in ei.value.message and "IN" in ei.value.message, ei.value.message


def test_what_stays_as_it_was():
    """`= [..]` as a comparison operand, the array constructor inside SATISFIES and ANY ... IN [constants] keep their refusals."""
    for cond, word in (("(%s = [1, 2])" % D("s"), "array constructor"), ('any `v` in %s satisfies (`v` = [1]) end' % D("a"), "array constructor"),
                       ('any `v` in [1, 2] satisfies (`v` = 1) end', "ANY / EVERY over a constant array")):
        with pytest.raises(query_amd.N1kError) as ei:
            _create(cond)
        assert ei.value.status == _ffi.UNSUPPORTED and word in ei.value.message, ei.value.message


def test_the_explain_subtrees_with_in_over_a_subquery_stay_refused():
    """tests/golden/plans.json, lines 1255 and 1277: `cover (...) in (select raw ...)`, the Parallel subtree and its Filter."""
    path = os.path.join(gu.GOLDEN, "plans.json")
    with open(path) as fh:
        lines = fh.read().split("\n")
    assert all(" in (select raw " in lines[n - 1] for n in (1255, 1277))
    with open(path) as fh:
        plans = json.load(fh)
    hits = [i for i, e in enumerate(plans) if " in (select raw " in json.dumps(e["plan"])]
    assert len(hits) == 2 and [plans[i]["kind"] for i in hits] == ["Parallel", "Filter"]
    for i in hits:
        with pytest.raises(query_amd.N1kError) as ei:
            query_amd.GpuFilterGroup(json.dumps(plans[i]["plan"]))
        assert ei.value.status == _ffi.UNSUPPORTED and "not a constant list (a subquery)" in ei.value.message, (i, ei.value.message)


def test_limits_that_fit():
    op = _create("(%s in %s)" % (D("x"), _nums(iu.IN_MAX_NUMBERS)))
    op.done()
    # the same 1024 numbers in another list of the plan are 1024 more: distinct per list, counted per plan
    with pytest.raises(query_amd.N1kError):
        _create("((%s in %s) or (%s in %s))" % (D("x"), _nums(iu.IN_MAX_NUMBERS), D("y"), _nums(iu.IN_MAX_NUMBERS).replace(", ", ",")))
    op = _create(iu.term(D("s"), ["s%d" % i for i in range(iu.IN_MAX_STRINGS)] + ["s0", "s1"]))  # 4096 distinct, two repeated
    op.done()
    # eight bits: IN lists with strings, LIKE patterns and collection predicates together; lists of numbers take none
    parts = ['(%s in ["p%d"])' % (D("s"), i) for i in range(3)] + ['(%s like "q%d%%")' % (D("s"), i) for i in range(3)] + \
            ['any `v` in %s satisfies (`v` = "c%d") end' % (D("a"), i) for i in range(2)] + ["(%s in [%d, true, null])" % (D("x"), i) for i in range(4)]
    for order in (parts, parts[::-1]):
        op = _create("(%s)" % " or ".join(order))
        assert op.in_stats()["lists"] == 7 and op.like_stats()["patterns"] == 3 and op.coll_stats()["predicates"] == 2
        op.done()
        for ninth in ('(%s in ["z", 1])' % D("t"), '(%s like "z%%")' % D("t"), 'any `v` in %s satisfies (`v` = "z") end' % D("a")):
            with pytest.raises(query_amd.N1kError) as ei:
                _create("(%s)" % " or ".join(order + [ninth]))
            assert ei.value.status == _ffi.UNSUPPORTED and "more than 8" in ei.value.message, ei.value.message


# ------------------------------------------------------------------ the host matcher

@pytest.mark.parametrize("size", [1, 2, 1000, iu.IN_MAX_STRINGS])
def test_host_matcher_against_set_membership(size):
    rng = np.random.default_rng(size)
    n = 20_000
    lens = rng.integers(0, 12, n)
    raw = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8).tobytes()
    cuts = np.concatenate([[0], np.cumsum(lens)])
    strings = [raw[cuts[i]:cuts[i + 1]] for i in range(n)]
    special = [b"", b"a\0b", b"\0", b"\xff", b"\xff\xfe\0", b"x" * 300, b"x" * 299, b"a\0"]
    strings[:len(special)] = special
    distinct = list(dict.fromkeys(strings))
    half = [distinct[i] for i in rng.choice(len(distinct), min(size // 2, len(distinct) // 2), replace=False)]
    consts = list(dict.fromkeys(([b""] if size > 1 else [b"a\0b"]) + (special[1:7:2] if size > 2 else []) + half))[:size]
    k = 0
    while len(consts) < size:  # the rest: strings that are not in the block
        c = b"absent-%d" % k
        k += 1
        consts.append(c)
    assert len(set(consts)) == size
    got = iu.host_match(iu.list_text(consts), strings)
    cs = set(consts)
    want = np.fromiter((s in cs for s in strings), dtype=np.uint8, count=n)
    assert np.array_equal(got, want) and 0 < int(want.sum()) < n, (size, int(want.sum()))
    assert set(np.unique(got).tolist()) <= {0, 1}


def test_host_matcher_arguments_and_other_elements():
    offs, blob = iu.pack([b"5", b"true", b"a"])
    out = np.zeros(3, dtype=np.uint8)
    L = _ffi.lib()
    text = b'[5, true, null, "a", "a"]'  # elements that are no strings hold no entry
    assert L.n1k_in_match(text, len(text), 3, offs.ctypes.data, blob, out.ctypes.data) == _ffi.OK and out.tolist() == [0, 0, 1]
    assert L.n1k_in_match(b"[]", 2, 3, offs.ctypes.data, blob, out.ctypes.data) == _ffi.OK and out.tolist() == [0, 0, 0]
    for bad, status in ((b'["a"', _ffi.INVALID), (b'"a"', _ffi.UNSUPPORTED), (b"[`x`]", _ffi.UNSUPPORTED), (b"[[1]]", _ffi.UNSUPPORTED), (b'["a"] x', _ffi.INVALID)):
        assert L.n1k_in_match(bad, len(bad), 3, offs.ctypes.data, blob, out.ctypes.data) == status, bad
    assert list(iu.host_match(b'["a"]', [])) == []


# ------------------------------------------------------------------ the yardstick

def test_matcher_by_sets_is_in4():
    big = 1 << 53
    values = [MISSING, None, True, False, 0, 3, -2, big, big + 1, 3.0, 2.5, -0.0, float(big), float("nan"), "", "a", "3", "true", []]
    lists = [[], [3], [3.0], [2.5, "a"], [None], [None, 3, "3"], [True], [False, 0], [big], [float(big)], ["", "true"], [0.0], [-2, 2.5, None, "a", True]]
    for consts in lists:
        f = iu.matcher(consts)
        for v in values:
            a, b = iu.in4(v, consts), f(v)
            assert a is b, (v, consts, a, b)


def test_in4_is_the_oracles_or_of_equalities_on_every_tag():
    """Soundness of the GPU differential's yardstick: In.Apply restated in python gives, plain and under NOT, the rows the
    oracle gives for the expanded form — over a table with STRING, INT, FLOAT, NULL, MISSING, TRUE, FALSE and ARRAY values."""
    import test_gpu_in as tg
    rng = np.random.default_rng(5)
    t = tg.make_table(rng, 3000)
    lists = [["a", "ab", "nope"], [3], [3.0, 2.5], ["3", 3, True], [None, "a", 1], [False, None], [0], ["", -2, 9.25, "zz"], [None]]
    for col in ("m", "s", "x"):
        vals = tg.column_values(t, col)
        assert col != "m" or {type(v) for v in vals if v is not MISSING} >= {str, int, float, bool, type(None), list}
        for consts in lists:
            res = [iu.in4(v, consts) for v in vals]
            e = iu.expand(tg.D(col), consts)
            for cond, keep in ((e, lambda r: r is True), ("(not %s)" % e, lambda r: r is False),
                               ("((not %s) or (%s is null))" % (e, e), lambda r: r is False or r is None)):
                got = n1o.run(t, cond, [], [], has_group=False).selected
                assert sorted(got.tolist()) == [i for i, r in enumerate(res) if keep(r)], (col, consts, cond)


# ------------------------------------------------------------------ without a device

@pytest.mark.parametrize("kind", ["DICT32", "TAGGED64"])
def test_two_term_in_plan_compiles_for_gfx950_without_a_gpu(kind):
    """scan_spec_kernel / scan_spec_records_kernel / scan_spec_partition_body with an IN term, through hiprtc."""
    op = _create('((%s in ["ab", 3, true]) and (5 < %s))' % (D("s"), D("x")), [D("k")], ["sum(%s)" % D("x")])
    assert op.column_paths == [D("s"), D("x"), D("k")]
    skind = _ffi.COL_DICT32 if kind == "DICT32" else _ffi.COL_TAGGED64
    kinds = np.array([skind, _ffi.COL_TAGGED64, _ffi.COL_DICT32], dtype=np.uint32)
    log = C.create_string_buffer(8192)
    st = _ffi.lib().n1k_jit_check(op._h, kinds.ctypes.data, 3, log, 8192)
    assert st == _ffi.OK, log.value.decode(errors="replace")
    op.done()


def test_every_plan_of_the_gpu_differential_is_accepted_and_the_bounded_family_takes_its_bounded_ones():
    """tests/test_gpu_in.py runs its bounded plans with `spec` off and reads stats["spec_kernel"] == 0, which the interpreter
    reports too.  What tells them apart is decided on the host: n1k_jit_check answers N1K_UNSUPPORTED unless build_fast_args
    takes the plan — here six distinct bounded shapes those seeds draw, IN term included.  Every drawn plan, Filter-only
    and grouped, is one n1k_create accepts."""
    import test_gpu_in as tg
    seen = set()
    for seed in range(tg.SEEDS):
        opts, bounded, _ = tg.FAMILIES[seed % len(tg.FAMILIES)]
        rng = np.random.default_rng(tg.SEED_BASE + seed)
        t = tg.make_table(rng, int(rng.integers(1, 5000)))
        dcond, ocond, keys, aggs = tg.rand_in_plan(rng, bounded)
        assert " in [" in dcond and " in [" not in ocond
        query_amd.GpuFilterGroup(plan.filter_group_plan(dcond, [], [], filter_only=True)).done()
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(dcond, keys, aggs))
        if bounded:
            by_name = {c.name: c for c in t.columns}
            kinds = np.array([by_name[p].kind for p in op.column_paths], dtype=np.uint32)
            shape = (tuple(kinds.tolist()), tuple(op.column_paths), dcond.split(" in [")[0].count("("), " and " in dcond, tuple(aggs))
            if shape not in seen and len(seen) < 6:
                seen.add(shape)
                log = C.create_string_buffer(4096)
                st = _ffi.lib().n1k_jit_check(op._h, kinds.ctypes.data, len(kinds), log, 4096)
                assert st == _ffi.OK, (st, dcond, keys, aggs, log.value.decode(errors="replace"))
        op.done()
    assert len(seen) >= 6
