"""Cuts tests/golden/cases_arr.json out of the reference's array-function statements: data only — statements, inputs and
recorded results.

    python tests/golden/make_golden_arr.py /path/to/reference

From test/filestore/json/default/cases/case_func_array.json and test/multistore/test_cases/array_functions/
case_func_array.json, as (function, array, second argument, recorded result) rows, the statements whose function is one of
array_length / array_count / array_sum / array_avg / array_contains / array_position.  Where the statement builds its array
with something else (array_agg, array_range, array_min over a comprehension), the row holds the array that expression gives
over the keyspace's documents (tests/golden/data_*.json), written out here and checked against them.

From the two case_group_by_having.json files, the multistore statement `... GROUP BY orderlines HAVING
ARRAY_LENGTH(orderlines) >= 2 ORDER BY O` whole, in the layout of cases_any.json: its plan in expression.Stringer text, the
HAVING text, the post stages, the recorded results.  (Its filestore twin groups by details.director, which the catalog
documents of tests/golden do not carry as an array-valued path; tests/golden/omitted.json keeps listing both.)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FILESTORE = ("filestore/case_func_array.json", ("test", "filestore", "json", "default", "cases", "case_func_array.json"))
MULTISTORE = ("multistore/array_functions/case_func_array.json", ("test", "multistore", "test_cases", "array_functions", "case_func_array.json"))
HAVING = ("multistore/aggregate_functions/case_group_by_having.json", ("test", "multistore", "test_cases", "aggregate_functions", "case_group_by_having.json"))

SEVEN = [None, None, None, "append", "avg", None, "max"]
TITLE_LENGTHS = [7, 18, 16]  # array_agg(LENGTH(title)) over default:catalog
ARRAY_MINS = ["coffee01", "coffee01", "coffee01", "sugar22"]  # array_agg(array_min(ARRAY ol.productId FOR ol IN orderlines END)) over default:orders (ARRAY_AGG sorts, algebra/agg_array.go:107-114)

# (source, statement prefix to find it by) -> (function, array or the non-array value, second argument, alias of the result)
ROWS = [
    (MULTISTORE, "select ARRAY_LENGTH([null, null, null,", "array_length", SEVEN, None, "$1"),
    (FILESTORE, "select array_sum(array_range(-3,5))", "array_sum", list(range(-3, 5)), None, "sum"),
    (FILESTORE, "SELECT ARRAY_COUNT(array_agg(LENGTH(title)))", "array_count", TITLE_LENGTHS, None, "$1"),
    (FILESTORE, "SELECT array_avg(array_agg(LENGTH(title)))", "array_avg", TITLE_LENGTHS, None, "$1"),
    (FILESTORE, "SELECT ARRAY_CONTAINS(array_agg(LENGTH(title)), 7)", "array_contains", TITLE_LENGTHS, 7, "$1"),
    (FILESTORE, "SELECT ARRAY_AVG(LENGTH(title))", "array_avg", 7, None, "$1"),  # a non-array: LENGTH(title) is a number
    (FILESTORE, "select array_position(array_agg(array_min(", "array_position", ARRAY_MINS, "sugar22", "A"),
]


def load(reference, rel):
    with open(os.path.join(reference, *rel)) as fh:
        return json.load(fh)


def docs(keyspace):
    with open(os.path.join(HERE, "data_%s.json" % keyspace)) as fh:
        return [d["doc"] for d in json.load(fh)]


def main(reference):
    assert sorted(len(d["title"]) for d in docs("catalog")) == sorted(TITLE_LENGTHS)
    assert sorted(min(ol["productId"] for ol in d["orderlines"]) for d in docs("orders")) == ARRAY_MINS
    rows = []
    for (source, rel), prefix, fn, array, second, alias in ROWS:
        hits = [(i, c) for i, c in enumerate(load(reference, rel)) if c["statements"].strip().startswith(prefix)]
        assert len(hits) == 1, (source, prefix, len(hits))
        idx, c = hits[0]
        results = c["results"]
        assert all(r == results[0] for r in results)  # (the per-document statement gives the same value for every document)
        rows.append({"id": "%s#%d" % (source, idx), "source": source, "index": idx, "statement": c["statements"], "function": fn,
                     "array": array, "second": second, "result": results[0][alias]})
    (source, rel) = HAVING
    hits = [(i, c) for i, c in enumerate(load(reference, rel)) if "HAVING ARRAY_LENGTH(orderlines)" in c["statements"]]
    assert len(hits) == 1
    idx, c = hits[0]
    OL, TID = "(`orders`.`orderlines`)", "(`orders`.`test_id`)"
    having = {
        "id": "%s#%d" % (source, idx), "source": source, "index": idx, "statement": c["statements"], "keyspace": "ms_orders",
        "columns": [OL, TID],
        "plan": {"condition": "(any `ord` in %s satisfies ((`ord`.`productId`) = \"tea111\") end and (%s = \"agg_func\"))" % (OL, TID),
                 "group_keys": [OL], "aggregates": ["count(*)"]},
        "having_text": "(2 <= array_length(%s))" % OL,
        "post": {"order": [[{"key": 0}, "asc"]], "project": [{"key": 0, "as": "O"}, {"agg": 0, "as": "count"}]},
        "results": c["results"],
    }
    about = ("The reference's statements over array_length / array_count / array_sum / array_avg / array_contains / array_position: "
             "(function, array, second argument, recorded result) rows, and the multistore HAVING ARRAY_LENGTH statement whole.  "
             "Written by tests/golden/make_golden_arr.py.")
    with open(os.path.join(HERE, "cases_arr.json"), "w") as fh:
        json.dump({"about": about, "rows": rows, "cases": [having]}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
