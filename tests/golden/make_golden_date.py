"""Cuts tests/golden/cases_date.json out of the reference's date-function statements: data only — statements, inputs and
recorded results.

    python tests/golden/make_golden_date.py /path/to/reference

From test/filestore/json/default/cases/case_func_date.json and test/multistore/test_cases/date_functions/case_func_date.json,
the statements whose functions are date_part_millis / date_trunc_millis / date_add_millis / str_to_millis (alias millis) /
date_part_str over constants, with no now_* / clock_* in them, as (function, arguments, recorded result) rows — one row per
call of a statement that selects several.  Both files hold most of them; a statement is taken once, from the multistore
file where it is there.

One statement wraps an in-scope call in a function that is not: MILLIS_TO_UTC(DATE_TRUNC_MILLIS(1.453505233e+12, "day"))
records "2016-01-22T00:00:00Z".  Its row holds the inner call and, as the result, that instant in milliseconds, written out
below (16822 days after 1970-01-01) and kept beside the recorded string.

The multistore statement over the orders documents of insert.json (test_id "datefunc") is kept as a column case: the
`shipped-on` values of the four documents — one MISSING, written {"$missing": true} — and the recorded rows.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
MULTISTORE = ("multistore/date_functions/case_func_date.json", ("test", "multistore", "test_cases", "date_functions", "case_func_date.json"))
FILESTORE = ("filestore/case_func_date.json", ("test", "filestore", "json", "default", "cases", "case_func_date.json"))
INSERT = ("test", "multistore", "test_cases", "date_functions", "insert.json")

D1, D2, D3 = "2004-07-09", "11:42:01Z", "2004-07-09T11:42:01Z"
# statement prefix -> [(function, arguments, alias of the result)]
ROWS = [
    ('SELECT DATE_PART_STR("2004-07-09", "year") AS year', [("date_part_str", [D1, p], p) for p in ("year", "month", "day")]),
    ('SELECT DATE_PART_STR("11:42:01Z","hour") AS hour', [("date_part_str", [D2, p], p) for p in ("hour", "minute", "second")]),
    ('SELECT DATE_PART_STR("2004-07-09T11:42:01Z", "year") AS year',
     [("date_part_str", [D3, p], p) for p in ("year", "month", "day", "hour", "minute", "second")]),
    ('SELECT DATE_PART_MILLIS(1.412243464575684768e+12, "millisecond")', [("date_part_millis", [1.412243464575684768e+12, "millisecond"], "ms")]),
    ('select STR_TO_MILLIS("2015-01-01T16:00:00-08:00")', [("str_to_millis", ["2015-01-01T16:00:00-08:00"], "$1")]),
    (' select MILLIS("2015-01-01T16:00:00-08:00")', [("str_to_millis", ["2015-01-01T16:00:00-08:00"], "$1")]),
    ("select date_part_millis(1463284740000,'day','UTC')", [("date_part_millis", [1463284740000, "day", "UTC"], "$1")]),
    ("select date_part_Str('2016-09-26T11:33:16.209-04:00','timezone')", [("date_part_str", ["2016-09-26T11:33:16.209-04:00", "timezone"], "$1")]),
    ("select date_part_Str('2016-09-26T11:33:16.209-07:00','timezone')", [("date_part_str", ["2016-09-26T11:33:16.209-07:00", "timezone"], "$1")]),
    ("select str_to_millis('2016-12-03T08:00:00Z'), str_to_millis('2015-12-03T08:00:00Z')",
     [("str_to_millis", ["2016-12-03T08:00:00Z"], "$1"), ("str_to_millis", ["2015-12-03T08:00:00Z"], "$2")]),
]
WRAPPED = ('select MILLIS_TO_UTC(DATE_TRUNC_MILLIS(1.453505233e+12,"day"))', ("date_trunc_millis", [1.453505233e+12, "day"], "$1"),
           "2016-01-22T00:00:00Z", 16822 * 86400000)
COLUMN = 'select DATE_PART_STR(`shipped-on`,"month") as a from orders where test_id = "datefunc" order by a'


def load(reference, rel):
    with open(os.path.join(reference, *rel)) as fh:
        return json.load(fh)


def find(cases, prefix):
    hits = [(i, c) for i, c in enumerate(cases) if c["statements"].startswith(prefix)]
    assert len(hits) == 1, (prefix, len(hits))
    return hits[0]


def main(reference):
    (source, rel) = MULTISTORE
    cases = load(reference, rel)
    twin = load(reference, FILESTORE[1])
    rows = []
    for prefix, calls in ROWS:
        idx, c = find(cases, prefix)
        _tidx, t = find(twin, prefix)
        (result,) = c["results"]
        assert t["results"] == c["results"]  # (1420156800000.0 in one file, 1420156800000 in the other: equal)
        for k, (fn, args, alias) in enumerate(calls):
            rows.append({"id": "%s#%d.%d" % (source, idx, k), "source": source, "index": idx, "statement": c["statements"], "function": fn,
                         "args": args, "result": result[alias]})
    prefix, (fn, args, alias), recorded, millis = WRAPPED
    idx, c = find(cases, prefix)
    assert c["results"] == [{alias: recorded}]
    rows.append({"id": "%s#%d.0" % (source, idx), "source": source, "index": idx, "statement": c["statements"], "function": fn, "args": args,
                 "result": millis, "recorded": recorded})
    idx, c = find(cases, COLUMN)
    inputs = []
    for ins in load(reference, INSERT):
        s = ins["statements"]
        if '"datefunc"' not in s:
            continue
        doc = json.loads(s[s.index("{"):s.rindex("}") + 1])
        inputs.append(doc["shipped-on"] if "shipped-on" in doc else {"$missing": True})
    assert len(inputs) == 4
    column = {"id": "%s#%d" % (source, idx), "source": source, "index": idx, "statement": c["statements"], "function": "date_part_str",
              "part": "month", "alias": "a", "inputs": inputs, "results": c["results"]}
    about = ("The reference's statements over date_part_millis / date_trunc_millis / date_add_millis / str_to_millis / date_part_str "
             "without now_* / clock_*: (function, arguments, recorded result) rows, and the statement over the `shipped-on` values of "
             "the datefunc documents as a column case.  Written by tests/golden/make_golden_date.py.")
    with open(os.path.join(HERE, "cases_date.json"), "w") as fh:
        json.dump({"about": about, "rows": rows, "columns": [column]}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
