"""ORDER BY / OFFSET / LIMIT over the rows of a Filter-only plan, the part that needs no GPU: the plan contract, the order
key (n1k_order_key: the function the key kernel compiles) against topk_util.collate_exact over every pair of a pool, and the
reference of tests/test_gpu_order.py (order_util) against the golden cases' own results."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest

import golden_util as gu
import order_util as ou
import query_amd
import topk_util as tk
from query_amd import _ffi, plan

D = lambda *n: plan.field_path("default", *n)
PRICE, CAT, A, B, X = D("price"), D("cat"), D("a"), D("b"), D("x")
COND = "(50 < %s)" % PRICE


def ordered(order=None, cond=COND, **kw):
    return plan.filter_group_plan(cond, [], [], filter_only=True, order=order, **kw)


def refused(pj):
    with pytest.raises(query_amd.N1kError) as ei:
        query_amd.GpuFilterGroup(pj)
    return ei.value


# ------------------------------------------------------------------------------------------------ 1. the plan contract
@pytest.mark.parametrize("order,kw,paths", [
    ([(PRICE, True)], {"limit": 100}, [PRICE]),                                   # the condition's own path: no new column
    ([(CAT, False), (PRICE, True)], {}, [PRICE, CAT]),                            # condition paths, then new sort paths
    ([(A, False), (CAT, True), (A, True), (B, False)], {"offset": 3, "limit": 10}, [PRICE, A, CAT, B]),  # 4 terms, none twice
    (None, {"limit": 10}, [PRICE]),                                               # Limit alone
    (None, {"offset": 5}, [PRICE]),                                               # Offset alone
    (None, {"offset": 5, "limit": 10}, [PRICE]),
])
def test_accepted_forms_and_their_column_paths(order, kw, paths):
    pj = ordered(order, **kw)
    nodes = [c["#operator"] for c in json.loads(pj)["~children"]]
    assert nodes[0] == "Parallel" and set(nodes[1:]) <= {"Order", "Offset", "Limit"} and len(nodes) > 1
    op = query_amd.GpuFilterGroup(pj)
    assert op.column_paths == paths
    op.done()


def test_order_after_a_bare_filter_node_is_accepted():
    pj = json.dumps({"#operator": "Sequence", "~children": [{"#operator": "Filter", "condition": COND},
                                                             {"#operator": "Order", "sort_terms": [{"expr": CAT, "desc": True}], "limit": "7"},
                                                             {"#operator": "Limit", "expr": "7"}]})
    op = query_amd.GpuFilterGroup(pj)
    assert op.column_paths == [PRICE, CAT]
    op.done()


@pytest.mark.parametrize("term,word", [("(%s + 1)" % PRICE, "leaf path"), ("lower(%s)" % CAT, "leaf path"), ("count(*)", "leaf path"),
                                       ("sum(%s)" % PRICE, "leaf path"), ("5", "leaf path"), ("\"x\"", "leaf path")])
def test_a_sort_term_that_is_no_leaf_path_is_unsupported(term, word):
    e = refused(ordered([(term, False)]))
    assert e.status == _ffi.UNSUPPORTED and word in e.message and term in e.message


def test_more_than_four_terms_are_unsupported():
    e = refused(ordered([(D("t%d" % i), False) for i in range(5)]))
    assert e.status == _ffi.UNSUPPORTED and "5 sort terms" in e.message


@pytest.mark.parametrize("field", ["limit", "offset"])
def test_offset_and_limit_must_be_integer_constants(field):
    pj = ordered([(PRICE, False)], limit=5, offset=6).replace('"%s": "%d"' % (field, 5 if field == "limit" else 6), '"%s": "(1 + 1)"' % field)
    assert "(1 + 1)" in pj
    e = refused(pj)
    assert e.status == _ffi.UNSUPPORTED and field in e.message
    pj = ordered(None, limit=5, offset=6).replace('"expr": "%d"' % (5 if field == "limit" else 6), '"expr": "$n"')
    assert "$n" in pj
    assert refused(pj).status == _ffi.UNSUPPORTED


def test_what_stays_refused():
    nothing = '{"#operator":"Sequence","~children":[{"#operator":"Order","sort_terms":[{"expr":"count(*)"}]}]}'  # nothing to order
    assert refused(nothing).status == _ffi.UNSUPPORTED
    no_filter = json.dumps({"#operator": "Sequence", "~children": [{"#operator": "Order", "sort_terms": [{"expr": PRICE}]}]})
    assert refused(no_filter).status == _ffi.UNSUPPORTED
    for node in ({"#operator": "InitialProject", "result_terms": [{"expr": PRICE}]}, {"#operator": "FinalProject"}):
        pj = json.dumps({"#operator": "Sequence", "~children": [{"#operator": "Filter", "condition": COND}, node]})
        e = refused(pj)
        assert e.status == _ffi.UNSUPPORTED and node["#operator"] in e.message
    with pytest.raises(ValueError):
        plan.filter_group_plan(COND, [], [], filter_only=True, order=[(PRICE, False)], project=[(PRICE, "p")])


@pytest.mark.parametrize("kw", [{"order": [(PRICE, False)]}, {"limit": 3}, {"offset": 3}])
def test_the_multi_batch_calls_are_unsupported(kw):
    op = query_amd.GpuFilterGroup(ordered(**kw))
    L = _ffi.lib()
    tags, pay = np.full(4, _ffi.T_INT, np.uint8), np.arange(4, dtype=np.uint64)
    b = op.make_device_batch(4, [(_ffi.COL_TAGGED64, tags.ctypes.data, pay.ctypes.data, None)])  # (host memory: the calls stop before it)
    res = _ffi.Result()
    doc = b'{"price": 60}'
    offs = np.array([0, len(doc)], dtype=np.uint64)
    calls = {"n1k_push_batch": lambda: L.n1k_push_batch(op._h, C.byref(b[0])),
             "n1k_push_device_batch": lambda: L.n1k_push_device_batch(op._h, C.byref(b[0])),
             "n1k_run_device_batch": lambda: L.n1k_run_device_batch(op._h, C.byref(b[0]), C.byref(res)),
             "n1k_push_json": lambda: L.n1k_push_json(op._h, 1, offs.ctypes.data_as(C.POINTER(C.c_uint64)), doc)}
    for name, call in calls.items():
        assert call() == _ffi.UNSUPPORTED, name
        msg = L.n1k_last_error(op._h).decode()
        assert name in msg and "one batch" in msg and "n1k_filter_device_batch" in msg
    op.done()


# ------------------------------------------------------------------------------------------------ 2. the order key
def key_pool():
    pool = dict(tk.POOL)
    pool.update({"MISSING": tk.MISSING, "int1": tk.I(1), "int-1": tk.I(-1), "int2^53-1": tk.I(2 ** 53 - 1), "int-2^53+1": tk.I(-2 ** 53 + 1),
                 "flt9007199254740992.0": tk.F(9007199254740992.0), "flt-2^63": tk.F(-9.223372036854775808e18),
                 "flt9.223372036854775808e18": tk.F(9.223372036854775808e18), "int-2^63+1": tk.I(-2 ** 63 + 1),
                 "int2^63-1025": tk.I(2 ** 63 - 1025), "int2^62+257": tk.I(2 ** 62 + 257), "int-2^62-255": tk.I(-2 ** 62 - 255),
                 "NaN2": tk.F(float(np.uint64(0xFFF8000000000001).view(np.float64)))})
    return pool


def device_pair(v, desc):
    tag, x = v
    rank = 0
    if tag == tk.T_INT:
        pay = x & 0xFFFFFFFFFFFFFFFF
    elif tag == tk.T_FLOAT:
        pay = int(np.float64(x).view(np.uint64))
    elif tag == tk.T_STRING:
        pay, rank = 7, sorted(tk.STRINGS).index(x)  # (the code is not read: the rank is the string's place)
    else:
        pay = 0
    return query_amd.order_key(tag, pay, rank, desc)


@pytest.mark.parametrize("desc", [False, True])
def test_order_key_is_collate_exact_over_every_pair(desc):
    pool = key_pool()
    assert {"-0.0", "0.0", "int0", "int2^53", "int2^53+1", "flt2^53", "int2^63-1", "int-2^63", "flt2^63", "flt-2^63", "+inf", "-inf", "NaN",
            "NULL", "false", "true", "MISSING", "1+0ulp", "1+7ulp"} <= set(pool)
    pairs = {n: device_pair(v, desc) for n, v in pool.items()}
    for n, (k, r) in pairs.items():
        assert 0 <= k < 2 ** 64 and 0 <= r < 2 ** 16, n
    for (na, a), (nb, b) in itertools.product(pool.items(), repeat=2):
        want = tk.collate_exact(a, b)
        ka, kb = pairs[na], pairs[nb]
        got = (ka > kb) - (ka < kb)
        assert got == (-want if desc else want), (na, nb, ka, kb)


def test_order_key_layout():
    L = _ffi.lib()
    assert "n1k_order_key" in _ffi.SYMBOLS and hasattr(L, "n1k_order_key")
    k = lambda v: device_pair(v, False)
    assert [k(v)[0] for v in (tk.MISSING, tk.NULL, tk.FALSE, tk.TRUE, tk.F(tk.NAN))] == [0, 1, 2, 3, 4]
    assert k(tk.F(-tk.INF))[0] == 0x000FFFFFFFFFFFFF and k(tk.F(tk.INF))[0] == 0xFFF0000000000000
    assert k(tk.S(sorted(tk.STRINGS)[0]))[0] == 0xFFF0000000000001
    assert k(tk.F(-0.0)) == k(tk.F(0.0)) == k(tk.I(0))
    # the residual: the bias for everything that is its own float64, the distance from it beyond 2^53
    assert k(tk.I(2 ** 53))[1] == k(tk.F(2.5))[1] == k(tk.NULL)[1] == 1024
    assert k(tk.I(2 ** 53 + 1))[1] == 1025 and k(tk.I(2 ** 63 - 1))[1] == 1023 and k(tk.I(-2 ** 63))[1] == 1024
    key, res = C.c_uint64(), C.c_uint32()
    assert L.n1k_order_key(_ffi.T_ARRAY, 0, 0, 0, C.byref(key), C.byref(res)) == _ffi.UNSUPPORTED_DATA
    assert L.n1k_order_key(_ffi.T_OBJECT, 0, 0, 1, C.byref(key), C.byref(res)) == _ffi.UNSUPPORTED_DATA
    assert L.n1k_order_key(9, 0, 0, 0, C.byref(key), C.byref(res)) == _ffi.INVALID
    assert L.n1k_order_key(_ffi.T_INT, 0, 0, 0, None, C.byref(res)) == _ffi.INVALID


# ------------------------------------------------------------------------------------------------ 3. the check of the checker
GOLDEN = ou.golden_sortable_cases()  # (an array / object as a sort value keeps the reference's Order: left out)


def test_the_golden_file_holds_ungrouped_order_by_cases():
    assert len(ou.golden_order_cases()) > len(GOLDEN) >= 10


@pytest.mark.parametrize("case", GOLDEN, ids=[c["id"] for c in GOLDEN])
def test_reference_order_reproduces_the_golden_results(case):
    table, terms, proj, sel = ou.golden_setup(case)
    by = {c.name: c for c in table.columns}
    values = [ou.column_values(by[t].tags, by[t].payload, table.dictionary) for t, _ in terms]
    desc = [d for _, d in terms]
    want = ou.expected(values, desc, sel=sel)
    ou.check_sorted(values, want, desc, sel=sel)
    assert gu.same_json(ou.golden_rows(table, proj, want), case["results"])
    # the verifier refuses anything else: two rows swapped, a row dropped under a cut
    if len(want) > 1:
        swapped = want.copy()
        swapped[[0, 1]] = swapped[[1, 0]]
        with pytest.raises(AssertionError):
            ou.check_sorted(values, swapped, desc, sel=sel)
        ou.check_sorted(values, want[1:], desc, sel=sel, offset=1)
        with pytest.raises(AssertionError):
            ou.check_sorted(values, want[:-1], desc, sel=sel, offset=1, limit=len(want) - 1)
