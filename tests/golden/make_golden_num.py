"""Cuts tests/golden/cases_num.json out of the reference's test/filestore/json/default/cases/case_func_num.json: the
trigonometric, exponential, logarithmic and power statements, the constants and the NaN / Inf argument cases — the ones
tests/golden/make_golden.py leaves out (its G7 block holds the other 23).  Statement and results verbatim; the plan in the
`exprs` / `row_expr` shapes of cases.json, the expression in expression.Stringer text.

    python tests/golden/make_golden_num.py /path/to/reference

Indices 38 and 39 (`random`) stay out: with a seed it is Go's generator, without one no function of the row.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = "filestore/case_func_num.json"
SC = "(`game`.`score`)"

# index -> (shape, expression text, exact?)   exact: tag and payload; otherwise numeric within the float tolerance
EXPRS = {
    2: ("exprs", "acos(1.0)", False), 3: ("exprs", "acos(-1.0)", False), 4: ("exprs", "acos(3)", True),
    5: ("row_expr", "asin((%s / 10))" % SC, False), 6: ("row_expr", "atan((%s / 10))" % SC, False),
    7: ("row_expr", "atan2(%s, 10)" % SC, False),
    8: ("exprs", "cos((pi() / 2))", False), 9: ("exprs", "cos(pi())", False), 10: ("exprs", "sin((pi() / 2))", False),
    11: ("exprs", "sin(pi())", False), 12: ("exprs", "tan((pi() / 2))", False), 13: ("exprs", "tan(pi())", False),
    14: ("row_expr", "tan(%s)" % SC, False), 15: ("row_expr", "cos(%s)" % SC, False), 16: ("row_expr", "sin(%s)" % SC, False),
    19: ("exprs", "pi()", True), 20: ("exprs", "e()", True), 21: ("exprs", "power(e(), 2)", False),
    22: ("exprs", "ln(power(e(), 2))", False), 23: ("exprs", "exp(2)", False), 24: ("exprs", "ln(exp(2))", False),
    25: ("exprs", "log(exp(10))", False), 26: ("exprs", "log(power(10, 34))", False),
    27: ("exprs", "degrees(pi())", True), 28: ("exprs", "degrees((pi() / 2))", True), 29: ("exprs", "degrees(((-pi()) / 2))", True),
    30: ("exprs", "radians(90)", True), 31: ("exprs", "radians(-180)", True), 32: ("exprs", "radians(pi())", True),
    35: ("exprs", "power(12, 2)", False), 36: ("row_expr", "power(%s, 2)" % SC, False), 37: ("row_expr", "power(%s, 10)" % SC, False),
    52: ("exprs", "sign(nan())", True), 53: ("exprs", "sign(posinf())", True), 54: ("exprs", "sign(neginf())", True),
}


def main(reference):
    with open(os.path.join(reference, "test", "filestore", "json", "default", "cases", "case_func_num.json")) as fh:
        src = json.load(fh)
    cases = []
    for idx in sorted(EXPRS):
        shape, text, exact = EXPRS[idx]
        c = src[idx]
        alias = list(c["results"][0].keys())[0]
        plan = {"exprs": [[alias, text]]} if shape == "exprs" else {"row_expr": [alias, text]}
        cases.append({"id": "%s#%d" % (SOURCE, idx), "source": SOURCE, "index": idx, "statement": c["statements"], "keyspace": "game",
                      "plan": plan, "exact": exact, "results": c["results"]})
    assert len(cases) == 35
    with open(os.path.join(HERE, "cases_num.json"), "w") as fh:
        json.dump({"cases": cases}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
