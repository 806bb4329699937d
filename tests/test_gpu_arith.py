"""The fifteen arithmetic nodes of arith_apply (n1k_device.h) on the device, bit for bit against the yardstick of
tests/arith_util.py, on both routes: materialised by arith_kernel (fuse_arith = 0) and in the registers of the run-time-built
scan (jit = 2, spec_kernel 3).  MAX(expr) GROUP BY id with one row per group gives the node's value of every row.  No
tolerance: same_exact compares exact rationals; the one listed exception (ROUND / TRUNC with 22 < |digits| <= 308) is
au.is_loose.  A refusal is a failure.

What was seen before round_float was kept from contracting x * pow + 0.5 into one fused multiply-add is in DESIGN.md
("Arithmetic in registers", the exactness contract)."""
import functools

import pytest

import arith_util as au
import golden_util as gu
import parity_util as pu
import query_amd

pytestmark = pytest.mark.gpu

D = au.D
M = au.MISSING
ID = D("id")


def must_run(fn, *a, **kw):
    """a refusal is a failure here, never a skip"""
    try:
        return fn(*a, **kw)
    except query_amd.N1kError as e:
        raise AssertionError("the device refused: %s" % e.message)


@functools.lru_cache(maxsize=None)
def pool(kind):
    rows = au.ROWS[kind]()
    return rows, au.table(rows)


@functools.lru_cache(maxsize=None)
def sampled(kind, n):
    rows = au.sample(pool(kind)[0], n)
    return rows, au.table(rows)


@functools.lru_cache(maxsize=None)
def folds(n):
    rows = au.fold_rows(n)
    return rows, au.table(rows)


def run_nodes(table, nodes, **opts):
    """MAX(node) GROUP BY id for every node -> ({id: [value per node]}, stats)"""
    out, st = must_run(pu.run_gpu, table, None, [ID], ["max(%s)" % au.text(e) for e in nodes], **opts)
    return {gu.decode_value(k[0]): [gu.decode_value(a) for a in aggs] for k, aggs in zip(out.keys, out.aggs)}, st


def check_nodes(rows, nodes, got):
    assert len(got) == len(rows)
    bad = []
    for r in rows:
        for e, g in zip(nodes, got[r["id"]]):
            args = [au.eval_node(a, r) for a in e[2]]
            want = au.max_value(au.apply(e[1], args))
            if not au.same(e[1], args, g, want):
                bad.append((au.text(e), args, "device %r" % (g,), "yardstick %r" % (want,)))
    assert not bad, ("%d of %d values differ" % (len(bad), len(rows) * len(nodes)), bad[:8])


def materialised(rows, table, nodes, **opts):
    got, st = run_nodes(table, nodes, fuse_arith=0, **opts)
    assert st["spec_kernel"] != 3 and st["rows_in"] == len(rows), st
    check_nodes(rows, nodes, got)


def fused(rows, table, nodes):
    assert len(rows) % 2 == 1
    for batches in (1, 2):
        got, st = run_nodes(table, nodes, jit=2, batches=batches)
        assert st["spec_kernel"] == 3, st
        check_nodes(rows, nodes, got)


# ------------------------------------------------------------------ the materialised route: arith_kernel, one op at a time

@pytest.mark.parametrize("form", sorted(au.FORMS))
def test_every_value_of_the_pool_materialised(form):
    """unary ops over the value pool, binary ops over all ordered pairs of it, ROUND / TRUNC with one argument and over
    value x digits"""
    e, kind = au.FORMS[form]
    rows, table = pool(kind)
    materialised(rows, table, [e])


@pytest.mark.parametrize("n,batches", [(1, 1), (257, 2)])
@pytest.mark.parametrize("form", sorted(au.FORMS))
def test_one_row_and_two_batches_materialised(form, n, batches):
    """arith_kernel's geometry is one row per lane in 256-lane workgroups: one row; one workgroup + 1 in two batches"""
    e, kind = au.FORMS[form]
    rows, table = sampled(kind, n)
    materialised(rows, table, [e], batches=batches)


# ------------------------------------------------------------------ the fused route: three nodes a plan, in registers

@pytest.mark.parametrize("group", au.FUSED_GROUPS, ids=au.FUSED_IDS)
def test_every_value_of_the_pool_fused(group):
    nodes, kind = au.fused_group_nodes(group)
    rows, table = pool(kind)
    fused(rows, table, nodes)


# ------------------------------------------------------------------ n-ary folds

@pytest.mark.parametrize("n", [3, 4])
def test_n_ary_folds_materialised(n):
    """Add.Apply / Mult.Apply fold from int 0 / int 1: every triple and quadruple of the eight-value pool"""
    rows, table = folds(n)
    materialised(rows, table, [au.node("+", *"abce"[:n]), au.node("*", *"abce"[:n])])


@pytest.mark.parametrize("c", au.FOLD_CONSTS, ids=["2p62", "max", "1", "half"])
@pytest.mark.parametrize("which", [0, 1])
def test_n_ary_folds_fused(which, c):
    """three and four operands in registers: every ordered pair of the pool in two columns, the further operands a constant"""
    rows, table = folds(2)
    fused(rows, table, au.fused_fold_nodes(which, c))


# ------------------------------------------------------------------ MISSING against NULL

@pytest.mark.parametrize("form", sorted(au.FORMS))
def test_missing_and_null_are_told_apart(form):
    """(MAX folds both to NULL: COUNT over `is missing` / `is null` of the node tells them apart)"""
    e, kind = au.FORMS[form]
    rows, table = pool(kind)
    vals = [au.eval_node(e, r) for r in rows]
    assert any(v is M for v in vals) and any(v is None for v in vals)
    for pred, want in (("missing", sum(v is M for v in vals)), ("null", sum(v is None for v in vals))):
        _out, st = must_run(pu.run_gpu, table, "(%s is %s)" % (au.text(e), pred), [], ["count(*)"])
        assert st["rows_selected"] == want, (form, pred, st["rows_selected"], want)


# ------------------------------------------------------------------ a node over a node

@pytest.mark.parametrize("route", ["materialised", "fused"])
@pytest.mark.parametrize("name", sorted(au.NESTED))
def test_a_node_over_a_node(name, route):
    rows, table = pool("pair")
    (materialised if route == "materialised" else fused)(rows, table, [au.NESTED[name]])


# ------------------------------------------------------------------ the grouped tail

TAIL_C = 73160693336096464  # between 73160693336096448 (one rounding) and 73160693336096480 (two)
TAIL_DIGITS = (2, 1, -1)


def tail_plan():
    v = D("v")
    project = [(D("g"), "g")] + [("round(max(%s), %d)" % (v, d), "r%d" % i) for i, d in enumerate(TAIL_DIGITS)]
    return None, [D("g")], ["max(%s)" % v], "(round(max(%s), -1) < %d)" % (v, TAIL_C), project


def plans():
    """every (condition, keys, aggregates, having, project) this file runs: tests/test_arith_cpu.py creates each without a GPU"""
    node_lists = [[au.FORMS[f][0]] for f in sorted(au.FORMS)] + [au.fused_group_nodes(g)[0] for g in au.FUSED_GROUPS]
    node_lists += [[au.node("+", *"abce"[:n]), au.node("*", *"abce"[:n])] for n in (3, 4)]
    node_lists += [au.fused_fold_nodes(w, c) for w in (0, 1) for c in au.FOLD_CONSTS] + [[e] for e in au.NESTED.values()]
    out = [(None, [ID], ["max(%s)" % au.text(e) for e in nodes], None, None) for nodes in node_lists]
    out += [("(%s is %s)" % (au.text(au.FORMS[f][0]), pred), [], ["count(*)"], None, None) for f in sorted(au.FORMS) for pred in ("missing", "null")]
    return out + [tail_plan()]


def test_having_and_a_projection_round_the_groups_maxima_exactly():
    """round(max(v), 2 | 1 | -1) as projection terms and round(max(v), -1) < c in HAVING, over groups whose MAX is one of
    the four inputs (and their negatives) on which one rounding and two differ.  The HAVING constant lies between the two
    candidates of the fourth input: a once-rounded intermediate lets that group through."""
    maxima = au.HEX + [-h for h in au.HEX]
    rows = []
    for g, h in enumerate(maxima):
        rows += [{"g": g, "v": h - abs(h) / 2}, {"g": g, "v": h}, {"g": g, "v": None}, {"g": g, "v": h - abs(h)}]
    table = au.table(rows)
    c = TAIL_C
    assert au.apply("round", [au.HEX[3], -1]) == 73160693336096480 and au.mu.new_value(au.fused_intermediate_result(au.HEX[3], -1)) == 73160693336096448
    digits = TAIL_DIGITS
    cond, keys, aggs, having, project = tail_plan()
    out, _st = must_run(pu.run_gpu, table, cond, keys, aggs, having=having, project=project)
    got = {gu.decode_value(r[0]): [gu.decode_value(x) for x in r[1:]] for r in out.proj}
    want = {g: [au.apply("round", [h, d]) for d in digits] for g, h in enumerate(maxima) if au.apply("round", [h, -1]) < c}
    assert set(got) == set(want) and 3 not in want and len(want) == 7, (sorted(got), sorted(want))
    for g in want:
        assert all(au.same_exact(x, y) for x, y in zip(got[g], want[g])), (g, maxima[g], got[g], want[g])
