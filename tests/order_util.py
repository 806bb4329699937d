"""An independent reference for ORDER BY <terms> OFFSET o LIMIT l over the rows a Filter selects (execution/order.go:121-169).

The order: topk_util.collate_exact term by term (value.Collate with an INT and a FLOAT compared exactly), DESC flipping a term,
and rows that tie on every term in ascending ordinal.  That order is total, so exactly one sequence of ordinals is right.

`values` is one column per sort term, indexed by ROW ORDINAL of the batch: a sequence of (tag, python value) pairs as
everywhere in the tests — or a numpy float64 array without NaN, standing for FLOAT values (the vectorised form, for the sizes
at which a python comparison per row would take too long).  `sel` is the ascending selection (default: every row).

  expected(values, desc, offset, limit, sel)      the ordinals, by python's sorted (n <= 20 000)
  check_sorted(values, got, desc, offset, limit, sel)   the O(n) verifier: raises AssertionError unless `got` is that sequence
"""
from __future__ import annotations

import functools
from typing import Optional, Sequence

import numpy as np

from topk_util import collate_exact

MAX_SORTED = 20000


def _cmp_rows(values, desc, i: int, j: int) -> int:
    for col, d in zip(values, desc):
        if isinstance(col, np.ndarray):
            c = int(col[i] > col[j]) - int(col[i] < col[j])
        else:
            c = collate_exact(col[i], col[j])
        if c:
            return -c if d else c
    return int(i > j) - int(i < j)


def _bounds(n: int, offset: int, limit: Optional[int]):
    first = min(n, offset)
    return first, (n if limit is None else min(n, first + limit))


def expected(values, desc: Sequence[bool], offset: int = 0, limit: Optional[int] = None, sel=None) -> np.ndarray:
    sel = np.arange(len(values[0])) if sel is None else np.asarray(sel)
    assert len(sel) <= MAX_SORTED, "expected() sorts in python: use check_sorted beyond %d rows" % MAX_SORTED
    order = sorted((int(i) for i in sel), key=functools.cmp_to_key(lambda i, j: _cmp_rows(values, desc, i, j)))
    first, last = _bounds(len(order), offset, limit)
    return np.array(order[first:last], dtype=np.uint32)


def _cmp_vec(values, desc, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Element-wise comparison of rows a[k] and b[k] in the full order (terms, then ordinal): -1 / 0 / 1."""
    out = np.zeros(len(a), dtype=np.int64)
    for col, d in zip(values, desc):
        if isinstance(col, np.ndarray):
            c = (col[a] > col[b]).astype(np.int64) - (col[a] < col[b]).astype(np.int64)
        else:
            c = np.fromiter((collate_exact(col[int(i)], col[int(j)]) for i, j in zip(a, b)), dtype=np.int64, count=len(a))
        out = np.where(out == 0, -c if d else c, out)
    return np.where(out == 0, (a > b).astype(np.int64) - (a < b).astype(np.int64), out)


def check_sorted(values, got, desc: Sequence[bool], offset: int = 0, limit: Optional[int] = None, sel=None) -> None:
    sel = np.arange(len(values[0]), dtype=np.int64) if sel is None else np.asarray(sel).astype(np.int64)
    got = np.asarray(got).astype(np.int64)
    first, last = _bounds(len(sel), offset, limit)
    assert len(got) == last - first, "%d rows, expected %d" % (len(got), last - first)
    nrows = len(values[0])
    assert ((got >= 0) & (got < nrows)).all(), "an ordinal outside the batch"
    in_sel = np.zeros(nrows, dtype=bool)
    in_sel[sel] = True
    in_got = np.zeros(nrows, dtype=bool)
    in_got[got] = True
    assert in_sel[got].all(), "a row that was not selected"
    assert int(in_got.sum()) == len(got), "a row twice"
    if len(got) > 1:  # every adjacent pair strictly ascending: the terms' order, and the ordinal on a full tie
        c = _cmp_vec(values, desc, got[:-1], got[1:])
        bad = np.nonzero(c >= 0)[0]
        assert bad.size == 0, "rows %d, %d at positions %d, %d are out of order" % (got[bad[0]], got[bad[0] + 1], bad[0], bad[0] + 1)
    out = sel[~in_got[sel]]
    if len(out) and len(got):  # a cut: exactly `first` rows left out lie before the first one kept, the others behind the last
        before = _cmp_vec(values, desc, out, np.full(len(out), got[0])) < 0
        assert int(before.sum()) == first, "%d rows left out before the first one kept, the offset is %d" % (int(before.sum()), first)
        rest = out[~before]
        assert (_cmp_vec(values, desc, rest, np.full(len(rest), got[-1])) > 0).all(), "a row left out that is before the last one kept"


def column_values(tags: np.ndarray, payload: np.ndarray, dictionary: Sequence[bytes]):
    """A TAGGED64 column as (tag, python value) pairs: INT from the two's complement, FLOAT from the bits, STRING / ARRAY /
    OBJECT as the dictionary's bytes."""
    from oracle import n1o
    ints, flts = payload.view(np.int64), payload.view(np.float64)
    out = []
    for i, t in enumerate(tags):
        t = int(t)
        if t == n1o.T_INT:
            out.append((t, int(ints[i])))
        elif t == n1o.T_FLOAT:
            out.append((t, float(flts[i])))
        elif t >= n1o.T_STRING:
            out.append((t, bytes(dictionary[int(payload[i])])))
        else:
            out.append((t, None))
    return out


def codes_values(codes: np.ndarray, dictionary: Sequence[bytes]):
    """A DICT32 column as (tag, python value) pairs."""
    from oracle import n1o
    return [(n1o.T_MISSING, None) if c == 0xFFFFFFFF else (n1o.T_NULL, None) if c == 0xFFFFFFFE else (n1o.T_STRING, bytes(dictionary[int(c)]))
            for c in codes]


# ------------------------------------------------------------------ the golden cases: SELECT ... WHERE ... ORDER BY, no group

def _path_text(alias: str, steps) -> str:
    """Stringer text of a field / element chain below the keyspace alias, as a Filter condition writes it."""
    s = "`%s`" % alias
    for st in steps:
        s = "(%s[%d])" % (s, st) if isinstance(st, int) else "(%s.`%s`)" % (s, st)
    return s


def golden_order_cases():
    """The ungrouped ORDER BY cases of tests/golden/cases.json whose sort terms and result terms are paths of the document."""
    import golden_util as gu
    out = []
    for case in gu.load_cases():
        p, post = case["plan"], case.get("post", {})
        if not p.get("filter_only") or "order" not in post or "raw" in post:
            continue
        if all("doc" in spec for spec, _ in post["order"]) and all("doc" in t for t in post["project"]):
            out.append(case)
    return out


def golden_setup(case):
    """(table over the condition's, sort terms' and result terms' paths; sort terms [(path text, desc)]; result terms
    [(alias, path text)]; the oracle's selection)."""
    import golden_util as gu
    from oracle import n1o
    docs = gu.load_docs(case["keyspace"])
    alias, post = case["keyspace"], case["post"]
    terms = [(_path_text(alias, spec["doc"]), direction == "desc") for spec, direction in post["order"]]
    proj = [(t["as"], _path_text(alias, t["doc"])) for t in post["project"]]
    paths = gu.leaf_paths(case["plan"])
    for p in [t for t, _ in terms] + [p for _, p in proj]:
        if p not in paths:
            paths.append(p)
    table = gu.build_table(docs, paths)
    sel = n1o.run(table, case["plan"]["condition"], [], [], has_group=False).selected
    return table, terms, proj, sel


def golden_sortable(table, terms, sel) -> bool:
    """No ARRAY / OBJECT among the selected rows' sort values (those keep the reference's Order)."""
    from oracle import n1o
    by = {c.name: c for c in table.columns}
    return all((by[t].tags[np.asarray(sel, dtype=np.int64)] < n1o.T_ARRAY).all() for t, _ in terms)


def golden_sortable_cases():
    out = []
    for case in golden_order_cases():
        table, terms, _, sel = golden_setup(case)
        if golden_sortable(table, terms, sel):
            out.append(case)
    return out


def golden_rows(table, proj, ordinals, columns=None):
    """Result rows {alias: value} of the rows `ordinals`, MISSING terms left out; `columns`: per result term (tags, payload)
    of exactly those rows (a device gather) instead of the table's columns indexed by the ordinals."""
    import golden_util as gu
    by = {c.name: c for c in table.columns}
    cols = []
    for k, (_, path) in enumerate(proj):
        if columns is not None:
            tags, pay = columns[k]
        else:
            ix = np.asarray(ordinals, dtype=np.int64)
            tags, pay = by[path].tags[ix], by[path].payload[ix]
        cols.append(column_values(np.asarray(tags), np.asarray(pay, dtype=np.uint64), table.dictionary))
    rows = []
    for i in range(len(ordinals)):
        r = {}
        for (alias, _), col in zip(proj, cols):
            v = gu.decode_value(col[i])
            if v is not gu.MISSING:
                r[alias] = v
        rows.append(r)
    return rows
