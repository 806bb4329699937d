"""An independent reference for SELECT DISTINCT over the rows a Filter selects (execution/distinct.go:60-71): which survivor
stands for each distinct row of the result terms.

The reference keys its set by the JSON text of the projected object (value/set.go:100-103).  normalise() maps one value, a
(tag, python value) pair as everywhere in the tests, to a hashable that is equal exactly for equal values under that rule:
MISSING is left out of the object (so it is no NULL), FALSE / TRUE / NULL are themselves, numbers are equal when numerically
equal — an integral FLOAT in int64 range is its INT, -0.0 is 0 (value/float.go:41-45), anything else its own double — and
STRING / ARRAY / OBJECT are their bytes within their tag.  Documented divergence of the device: every NaN is one value and
each infinity its own (the reference would print them as the strings "NaN" / "+Infinity" / "-Infinity").

`values` is one column per result term, indexed by ROW ORDINAL: a sequence of (tag, python value) pairs, or a numpy integer
array standing for INT values (the vectorised form, for sizes at which a python loop per row takes too long).  `sel` is the
ascending selection (default: every row).  representatives() keeps the smallest ordinal per key, ascending."""
from __future__ import annotations

import math

import numpy as np

T_MISSING, T_NULL, T_FALSE, T_TRUE, T_INT, T_FLOAT, T_STRING, T_ARRAY, T_OBJECT = range(9)


def normalise(v):
    t, x = v
    if t == T_INT:
        return ("number", int(x))
    if t == T_FLOAT:
        if math.isnan(x):
            return ("nan",)
        if not math.isinf(x) and x == math.floor(x) and -2 ** 63 <= int(x) < 2 ** 63:
            return ("number", int(x))
        return ("float", float(x))
    return (t, bytes(x)) if t >= T_STRING else (t,)


def row_key(values, i: int):
    return tuple(int(col[i]) if isinstance(col, np.ndarray) else normalise(col[i]) for col in values)


def representatives(values, sel=None) -> np.ndarray:
    sel = np.arange(len(values[0]), dtype=np.int64) if sel is None else np.asarray(sel).astype(np.int64)
    if len(sel) and all(isinstance(col, np.ndarray) for col in values):
        _, first = np.unique(np.stack([col[sel] for col in values], axis=1), axis=0, return_index=True)  # (the first occurrence of each)
        return np.sort(sel[first]).astype(np.uint32)
    seen, out = set(), []
    for i in sel:  # ascending: the first survivor that brings a key has its smallest ordinal
        k = row_key(values, int(i))
        if k not in seen:
            seen.add(k)
            out.append(int(i))
    return np.array(out, dtype=np.uint32)


# ------------------------------------------------------------------ the golden cases: SELECT DISTINCT <paths> ... ORDER BY <paths>

def golden_cases():
    import json
    import os

    import golden_util as gu
    with open(os.path.join(gu.GOLDEN, "cases_distinct.json")) as fh:
        return json.load(fh)["cases"]


def golden_setup(case):
    """(table over the condition's, result terms' and sort terms' paths; result terms [(path text, alias or None)]; sort terms
    [(path text, desc)]; projection [(alias, path text)]; the survivors: the oracle's Filter-only selection, or every row)."""
    import golden_util as gu
    import order_util as ou
    from oracle import n1o
    docs, alias, post = gu.load_docs(case["keyspace"]), case["alias"], case["post"]
    terms = [(ou._path_text(alias, steps), name) for steps, name in case["plan"]["distinct"]]
    order = [(ou._path_text(alias, spec["doc"]), direction == "desc") for spec, direction in post["order"]]
    proj = [(t["as"], ou._path_text(alias, t["doc"])) for t in post["project"]]
    cond = case["plan"]["condition"]
    paths = gu.leaf_paths({"condition": cond}) if cond else []
    for p in [t for t, _ in terms] + [t for t, _ in order] + [p for _, p in proj]:
        if p not in paths:
            paths.append(p)
    table = gu.build_table(docs, paths)
    sel = n1o.run(table, cond, [], [], has_group=False).selected.astype(np.int64) if cond else np.arange(len(docs), dtype=np.int64)
    return table, terms, order, proj, sel
