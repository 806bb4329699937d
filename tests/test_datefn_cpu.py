"""DATE_PART_MILLIS / DATE_TRUNC_MILLIS / DATE_ADD_MILLIS and STR_TO_MILLIS / DATE_PART_STR as values, without a GPU: the yardstick
(tests/datefn_util.py) against a hand-written table, `datetime` and the reference's recorded results; what n1k_create accepts
and refuses; the host evaluator (n1k_datefn_eval) bit for bit against the yardstick over the edge pools; a compile-only build
of the fused shapes for gfx950; every plan tests/test_gpu_datefn.py pushes."""
import ctypes as C
import datetime
import json
import os

import numpy as np
import pytest

import datefn_util as du
import golden_util as gu
import query_amd
from query_amd import _ffi, plan

M = du.MISSING
D = du.D
T, S, K = D("t"), D("s"), D("k")
ms_of = du.ms_of

with open(os.path.join(gu.GOLDEN, "cases_date.json")) as _fh:
    GOLDEN = json.load(_fh)


def create(condition, keys, aggs, **kw):
    return query_amd.GpuFilterGroup(plan.filter_group_plan(condition, keys, aggs, **kw))


def paths_of(condition, keys, aggs, **kw):
    op = create(condition, keys, aggs, **kw)
    try:
        return op.column_paths
    finally:
        op.done()


def refusal(condition, keys, aggs, **kw):
    with pytest.raises(query_amd.N1kError) as ei:
        create(condition, keys, aggs, **kw).done()
    return ei.value


def P(part):
    return json.dumps(part)


# ---------------------------------------------------------------- the yardstick

BASE = ms_of(2016, 5, 15, 3, 59, 0)  # 1463284740000, a Sunday
assert BASE == 1463284740000
# (function, arguments with the part last, expected value) — written down by hand from a calendar and the Go documentation
HAND = [
    ("date_part_millis", [0, "year"], 1970), ("date_part_millis", [0, "dow"], 4), ("date_part_millis", [0, "day_of_year"], 1),
    ("date_part_millis", [0, "iso_week"], 1), ("date_part_millis", [0, "iso_year"], 1970), ("date_part_millis", [0, "week"], 1),
    ("date_part_millis", [0, "decade"], 197), ("date_part_millis", [0, "century"], 20), ("date_part_millis", [0, "millennium"], 2),
    ("date_part_millis", [0, "timezone"], 0), ("date_part_millis", [0, "timezone_hour"], 0), ("date_part_millis", [0, "timezone_minute"], 0),
    ("date_part_millis", [BASE, "year"], 2016), ("date_part_millis", [BASE, "month"], 5), ("date_part_millis", [BASE, "day"], 15),
    ("date_part_millis", [BASE, "hour"], 3), ("date_part_millis", [BASE, "minute"], 59), ("date_part_millis", [BASE, "second"], 0),
    ("date_part_millis", [BASE, "day_of_week"], 0), ("date_part_millis", [BASE, "iso_dow"], 7), ("date_part_millis", [BASE, "doy"], 136),
    ("date_part_millis", [BASE, "week"], 20), ("date_part_millis", [BASE, "iso_week"], 19), ("date_part_millis", [BASE, "quarter"], 2),
    ("date_part_millis", [BASE, "DAY"], 15), ("date_part_millis", [BASE, "day", "UTC"], 15),
    ("date_part_millis", [ms_of(2021, 1, 3), "iso_year"], 2020), ("date_part_millis", [ms_of(2021, 1, 3), "iso_week"], 53),
    ("date_part_millis", [ms_of(2018, 12, 31), "iso_year"], 2019), ("date_part_millis", [ms_of(2018, 12, 31), "iso_week"], 1),
    ("date_part_millis", [ms_of(2010, 1, 3), "iso_year"], 2009), ("date_part_millis", [ms_of(2010, 1, 3), "iso_week"], 53),
    ("date_part_millis", [-1, "year"], 1969), ("date_part_millis", [-1, "millisecond"], 999), ("date_part_millis", [-1, "second"], 59),
    ("date_part_millis", [1.412243464575684768e+12, "millisecond"], 575),
    ("date_part_millis", [du.MIN_MILLIS, "year"], 1), ("date_part_millis", [du.MAX_MILLIS, "year"], 9999), ("date_part_millis", [du.MAX_MILLIS, "millisecond"], 999),
    ("date_part_millis", [du.MIN_MILLIS - 1, "year"], du.RAISE), ("date_part_millis", [du.MAX_MILLIS + 1, "year"], du.RAISE),
    ("date_part_millis", [du.NAN, "year"], du.RAISE), ("date_part_millis", [du.PINF, "year"], du.RAISE), ("date_part_millis", [du.NINF, "day"], du.RAISE),
    ("date_part_millis", [M, "year"], M), ("date_part_millis", [None, "year"], None), ("date_part_millis", ["2016-01-01", "year"], None),
    ("date_part_millis", [True, "year"], None),
    ("date_trunc_millis", [1.453505233e+12, "day"], 1453420800000), ("date_trunc_millis", [1.453505233e+12, "month"], 1451606400000),
    ("date_trunc_millis", [1.453505233e+12, "quarter"], 1451606400000), ("date_trunc_millis", [1.453505233e+12, "year"], 1451606400000),
    ("date_trunc_millis", [1.453505233e+12, "decade"], 1262304000000), ("date_trunc_millis", [1.453505233e+12, "century"], 946684800000),
    ("date_trunc_millis", [1.453505233e+12, "millennium"], 946684800000), ("date_trunc_millis", [BASE + 59999, "minute"], BASE),
    ("date_trunc_millis", [BASE + 59999, "hour"], BASE - 59 * 60000), ("date_trunc_millis", [ms_of(2016, 8, 20, 1), "quarter"], ms_of(2016, 7, 1)),
    ("date_trunc_millis", [-1, "day"], -86400000), ("date_trunc_millis", [-1, "second"], -1000), ("date_trunc_millis", [-0.5, "millisecond"], -1),
    ("date_trunc_millis", [ms_of(999, 6, 15), "millennium"], du.RAISE), ("date_trunc_millis", [ms_of(99, 6, 15), "century"], du.RAISE),
    ("date_trunc_millis", [ms_of(9, 6, 15), "decade"], du.RAISE), ("date_trunc_millis", [ms_of(999, 6, 15), "century"], ms_of(900, 1, 1)),
    ("date_trunc_millis", [M, "day"], M), ("date_trunc_millis", ["a", "day"], None),
    # AddDate's normalisation: Jan 31 + 1 month is early March; Feb 29 + 1 year is March 1
    ("date_add_millis", [ms_of(2016, 1, 31, 10), 1, "month"], ms_of(2016, 3, 2, 10)), ("date_add_millis", [ms_of(2015, 1, 31, 10), 1, "month"], ms_of(2015, 3, 3, 10)),
    ("date_add_millis", [ms_of(2016, 1, 31, 10), -13, "month"], ms_of(2014, 12, 31, 10)), ("date_add_millis", [ms_of(2016, 1, 31), 13, "month"], ms_of(2017, 3, 3)),
    ("date_add_millis", [ms_of(2024, 2, 29), 1, "year"], ms_of(2025, 3, 1)), ("date_add_millis", [ms_of(2024, 2, 29), 4, "year"], ms_of(2028, 2, 29)),
    ("date_add_millis", [BASE, 1, "quarter"], ms_of(2016, 8, 15, 3, 59)), ("date_add_millis", [BASE, 1, "week"], BASE + 7 * 86400000),
    ("date_add_millis", [BASE, -1, "day"], BASE - 86400000), ("date_add_millis", [BASE, 1, "decade"], ms_of(2026, 5, 15, 3, 59)),
    ("date_add_millis", [BASE, 1, "century"], ms_of(2116, 5, 15, 3, 59)), ("date_add_millis", [BASE, 1, "millennium"], ms_of(3016, 5, 15, 3, 59)),
    ("date_add_millis", [BASE, 3, "hour"], BASE + 3 * 3600000), ("date_add_millis", [BASE, -61, "minute"], BASE - 61 * 60000),
    ("date_add_millis", [BASE, 2 ** 31, "millisecond"], BASE + 2 ** 31), ("date_add_millis", [BASE, 5, "second"], BASE + 5000),
    ("date_add_millis", [BASE, 2.5, "month"], None), ("date_add_millis", [BASE, 3.0, "day"], BASE + 3 * 86400000), ("date_add_millis", [BASE, du.NAN, "day"], None),
    ("date_add_millis", [BASE, M, "day"], M), ("date_add_millis", [M, None, "day"], M), ("date_add_millis", [None, M, "day"], M), ("date_add_millis", [BASE, "3", "day"], None),
    ("date_add_millis", [du.NAN, 2.5, "day"], None),  # (the non-integral n is tested before the millis are read)
    ("date_add_millis", [BASE, 2 ** 31 + 1, "millisecond"], du.RAISE), ("date_add_millis", [BASE, du.PINF, "day"], du.RAISE),
    ("date_add_millis", [BASE, 2562048, "hour"], du.RAISE),  # 2562048 h * 3.6e12 ns > 2^63
    ("date_add_millis", [BASE, 2562047, "hour"], BASE + 2562047 * 3600000),  # ... and 2562047 h, 292 years, fit
    ("date_add_millis", [BASE, 153722868, "minute"], du.RAISE), ("date_add_millis", [BASE, 8000, "year"], du.RAISE), ("date_add_millis", [BASE, -2016, "year"], du.RAISE),
    ("date_add_millis", [BASE, -2015, "year"], ms_of(1, 5, 15, 3, 59)),
    # the rounding of .9996 s carries into the next second and is lost (timeToMillis reads the seconds of the unrounded time)
    ("date_add_millis", [BASE + 999.6, 0, "day"], BASE), ("date_trunc_millis", [BASE + 999.6, "millisecond"], BASE + 999),
    ("str_to_millis", ["2015-01-01T16:00:00-08:00"], 1420156800000), ("str_to_millis", ["1970-01-01"], 0), ("str_to_millis", ["1970-01-01T00:00:00.0005Z"], 1),
    ("str_to_millis", ["1970-01-01T00:00:00.0004999Z"], 0), ("str_to_millis", ["1969-12-31T23:59:59.9995Z"], -1000),  # (the lost carry)
    ("str_to_millis", ["00:00:00"], ms_of(0, 1, 1)), ("str_to_millis", ["0000-01-01"], -62167219200000), ("str_to_millis", ["2006-01-02 15:04:05+07:00"], ms_of(2006, 1, 2, 8, 4, 5)),
    ("str_to_millis", ["2012/01/02"], None), ("str_to_millis", [M], M), ("str_to_millis", [None], None), ("str_to_millis", [5], None), ("str_to_millis", ["5:04:05"], du.RAISE),
    ("date_part_str", ["2016-09-26T11:33:16.209-04:00", "hour"], 11), ("date_part_str", ["2016-09-26T11:33:16.209-04:00", "timezone"], -14400),
    ("date_part_str", ["2016-09-26T11:33:16.209-04:00", "timezone_hour"], -4), ("date_part_str", ["2016-02-29 12:30:45.5+05:30", "timezone_minute"], 30),
    ("date_part_str", ["2016-02-29 12:30:45.5-05:30", "timezone_minute"], -30), ("date_part_str", ["2016-09-26T11:33:16.209-04:00", "millisecond"], 209),
    ("date_part_str", ["11:42:01Z", "year"], 0), ("date_part_str", ["11:42:01Z", "millennium"], 1), ("date_part_str", ["2021-01-03", "iso_year"], 2020),
    ("date_part_str", ["2006-01-00", "day"], du.RAISE), ("date_part_str", ["2006-01-32", "day"], None), ("date_part_str", [M, "day"], M), ("date_part_str", [7, "day"], None),
]


@pytest.mark.parametrize("i", range(len(HAND)))
def test_the_yardstick_gives_the_hand_written_table(i):
    fn, args, want = HAND[i]
    got = du.apply(fn, args)
    assert (got if got == du.RAISE else du.result_value(got)) is want or (got != du.RAISE and du.result_value(got) == want and type(du.result_value(got)) is type(want)), (fn, args, got, want)


@pytest.mark.parametrize("row", GOLDEN["rows"], ids=[r["id"] for r in GOLDEN["rows"]])
def test_the_yardstick_gives_the_references_recorded_results(row):
    got = du.apply(row["function"], row["args"])
    assert got == du.r_int(row["result"]), (row["statement"], got)


def test_the_yardstick_gives_the_recorded_rows_of_the_column_statement():
    (c,) = GOLDEN["columns"]
    got = [du.result_value(du.apply(c["function"], [M if isinstance(v, dict) else v, c["part"]])) for v in c["inputs"]]
    rows = [{} if v is M else {c["alias"]: v} for v in got]
    key = lambda r: (0,) if not r else (1,) if r[c["alias"]] is None else (2, r[c["alias"]])  # noqa: E731  (ORDER BY: MISSING, NULL, numbers)
    assert sorted(rows, key=key) == c["results"]


def test_the_calendar_agrees_with_datetime():
    """the cross-check: every part datetime knows, over the integral in-range millis of the edge pool and a sweep of days"""
    epoch = datetime.datetime(1970, 1, 1)
    pool = [int(v) for v in du.MILLIS_EDGES if du.is_number(v) and v == v and du.MIN_MILLIS <= v <= du.MAX_MILLIS and v == int(v)]
    pool += [ms_of(1, 1, 1) + k * 86400000 * 9973 + k * 3599999 for k in range(365)]  # ~ every 27 years' offset, to year 9971
    for m in pool:
        dt = epoch + datetime.timedelta(milliseconds=m)
        iso = dt.isocalendar()
        want = {"year": dt.year, "month": dt.month, "day": dt.day, "hour": dt.hour, "minute": dt.minute, "second": dt.second,
                "millisecond": dt.microsecond // 1000, "doy": dt.timetuple().tm_yday, "dow": (dt.weekday() + 1) % 7, "iso_dow": dt.isoweekday(),
                "iso_year": iso[0], "iso_week": iso[1], "quarter": (dt.month + 2) // 3, "week": -(-dt.timetuple().tm_yday // 7)}
        for part, w in want.items():
            assert du.apply_millis("date_part_millis", m, part) == du.r_int(w), (m, part, w)
        assert du.apply_millis("date_trunc_millis", m, "month") == du.r_int(int((dt.replace(day=1, hour=0, minute=0, second=0, microsecond=0) - epoch).total_seconds()) * 1000)
        assert du.ms_of(dt.year, dt.month, dt.day, dt.hour, dt.minute, dt.second, dt.microsecond // 1000) == m


def test_the_classifier_on_its_three_classes():
    for s in du.VALUE_STRINGS:
        assert du.classify(s.encode())[0] == "value", s
    for why, strings in du.UNSURE_STRINGS.items():
        for s in strings:
            assert du.classify(s.encode()) == ("unsure",), (why, s)
    for s in du.NULL_STRINGS:
        assert du.classify(s.encode()) == ("null",), s
    assert len(du.LAYOUT_STRINGS) == 19 and max(len(s) for s in du.VALUE_STRINGS) == 35
    assert du.classify(b"2016-09-26T11:33:16.209-04:00") == ("value", 2016, 9, 26, 11, 33, 16, 209000000, -14400)
    assert du.classify(b"15:04:05.25Z") == ("value", 0, 1, 1, 15, 4, 5, 250000000, 0)


# ---------------------------------------------------------------- n1k_create

def millis_call(fn, first=T, part="day", n=D("g")):
    return du.call_text(fn, first, part) if fn != "date_add_millis" else plan.date_fn(fn, first, n, P(part))


@pytest.mark.parametrize("fn", du.MILLIS_FUNCTIONS)
def test_the_millis_functions_stand_wherever_round_does(fn):
    f = millis_call(fn)
    c = [T] + ([D("g")] if fn == "date_add_millis" else [])
    assert paths_of("(%s < 2)" % f, [K], ["count(*)"]) == c + [K]
    assert paths_of(None, [f], ["count(*)"]) == c
    assert paths_of(None, [K], ["sum(%s)" % f]) == [K] + c
    assert paths_of(None, [K], ["max((%s + 1))" % f]) == [K] + c
    assert paths_of(None, [K], ["min(round((%s / 1000), 2))" % f]) == [K] + c
    assert paths_of("(0 < %s)" % f, [], [], filter_only=True) == c
    # over arithmetic and over one another
    inner = millis_call("date_trunc_millis", "(%s + 1)" % T, "month")
    assert paths_of(None, [millis_call(fn, inner)], ["count(*)"]) == c
    # HAVING and a projection over the groups, through its alias an ORDER BY term
    over = millis_call(fn, "max(%s)" % T, n="2")
    assert paths_of(None, [K], ["max(%s)" % T], having="(%s < 5)" % over) == [K, T]
    assert paths_of(None, [K], ["max(%s)" % T], project=[(over, "v"), (K, None)], order=[("`v`", False)]) == [K, T]


@pytest.mark.parametrize("fn", du.STRING_FUNCTIONS)
def test_the_string_functions_stand_wherever_round_does(fn):
    f = du.call_text(fn, S, *(["month"] if fn == "date_part_str" else []))
    assert paths_of("(%s < 2)" % f, [K], ["count(*)"]) == [S, K]
    assert paths_of(None, [f], ["count(*)"]) == [S]
    assert paths_of(None, [K], ["sum(%s)" % f]) == [K, S]
    assert paths_of(None, [K], ["max((%s + 1))" % f]) == [K, S]
    assert paths_of(None, [millis_call("date_part_millis", f, "year")], ["count(*)"]) == [S]
    assert paths_of("((0 < %s) and (%s < 9))" % (f, f), [f], ["count(*)"]) == [S]  # (the same term thrice: one column)
    over_key = du.call_text(fn, S, *(["month"] if fn == "date_part_str" else []))
    assert paths_of(None, [S], ["count(*)"], having="(%s < 5)" % over_key) == [S]
    over_min = du.call_text(fn, "min(%s)" % S, *(["month"] if fn == "date_part_str" else []))
    assert paths_of(None, [K], ["min(%s)" % S], project=[(over_min, "v"), (K, None)], order=[("`v`", True)]) == [K, S]


def test_every_part_name_in_either_case_and_a_missing_part():
    for part in du.PART_NAMES:
        assert paths_of(None, [du.call_text("date_part_millis", T, part.upper())], ["count(*)"]) == [T]
        assert paths_of(None, [du.call_text("date_part_str", S, part.title())], ["count(*)"]) == [S]
    for part in du.ADD_PARTS:
        assert paths_of(None, [plan.date_fn("date_add_millis", T, "1", P(part))], ["count(*)"]) == [T]
    for part in du.TRUNC_PARTS:
        assert paths_of(None, [du.call_text("date_trunc_millis", T, part)], ["count(*)"]) == [T]
    # a MISSING part makes the call the constant MISSING: no column is read for it
    assert paths_of(None, [K, plan.date_fn("date_trunc_millis", T, "missing")], ["count(*)"]) == [K, T]


def test_a_call_of_constants_folds_at_create():
    """no column, no node: the golden statements run this way"""
    for row in GOLDEN["rows"]:
        text = plan.date_fn(row["function"], *[du.const_text(a) for a in row["args"]])
        assert paths_of(None, [text], ["count(*)"]) == [], text
    assert paths_of("(%s < %s)" % (T, du.call_text("str_to_millis", P("2016-01-01"))), [], ["count(*)"]) == [T]


FIVE = [du.call_text("date_part_str", S, p) for p in ("year", "month", "day", "hour")] + [du.call_text("str_to_millis", S)]
REFUSED = {
    "an unknown part": (None, [du.call_text("date_part_millis", T, "fortnight")], ["count(*)"], {}, "fortnight"),
    "week under trunc": (None, [du.call_text("date_trunc_millis", T, "week")], ["count(*)"], {}, "week"),
    "doy under add": (None, [plan.date_fn("date_add_millis", T, "1", P("doy"))], ["count(*)"], {}, "doy"),
    "an unknown part of a string": (None, [du.call_text("date_part_str", S, "era")], ["count(*)"], {}, "era"),
    "a part that is a path": (None, [plan.date_fn("date_part_millis", T, K)], ["count(*)"], {}, "date_part_millis: the date part must be a STRING constant"),
    "a part that is a number": (None, [plan.date_fn("date_trunc_millis", T, "5")], ["count(*)"], {}, "date_trunc_millis: the date part must be a STRING constant"),
    "a part of a string that is a path": (None, [plan.date_fn("date_part_str", S, K)], ["count(*)"], {}, "date_part_str: the date part must be a STRING constant"),
    "another time zone": (None, [du.call_text("date_part_millis", T, "day", "US/Eastern")], ["count(*)"], {}, "date_part_millis: a time zone other than the constant \"UTC\""),
    "a time zone that is a path": (None, [plan.date_fn("date_part_millis", T, P("day"), K)], ["count(*)"], {}, "time zone"),
    "str_to_millis over a function": (None, [plan.date_fn("str_to_millis", "lower(%s)" % S)], ["count(*)"], {}, "str_to_millis over"),
    "date_part_str over arithmetic": (None, [plan.date_fn("date_part_str", "(%s + 1)" % S, P("day"))], ["count(*)"], {}, "date_part_str over"),
    "inside SATISFIES": ("any `v` in %s satisfies (date_part_millis(`v`, \"year\") < 2000) end" % D("a"), [], ["count(*)"], {}, "date_part_millis"),
    "a string function inside SATISFIES": ("any `v` in %s satisfies (str_to_millis(`v`) < 2000) end" % D("a"), [], ["count(*)"], {}, "str_to_millis"),
    "a sort term": ("(0 < %s)" % T, [], [], {"filter_only": True, "order": [(du.call_text("date_trunc_millis", T, "day"), False)]}, "date_trunc_millis("),
    "a DISTINCT term": ("(0 < %s)" % T, [], [], {"filter_only": True, "distinct": [(du.call_text("date_part_str", S, "day"), "x")]}, "date_part_str("),
    "inside CASE": (None, [plan.case_when([("(%s < 1)" % T, du.call_text("date_part_millis", T, "day"))], "0")], ["count(*)"], {}, "'date_part_millis' inside CASE"),
    "inside a conditional function": (None, [plan.cond_fn("ifnull", du.call_text("str_to_millis", S), "0")], ["count(*)"], {}, "'str_to_millis' inside CASE"),
    "a WHEN over one": (None, [plan.case_when([("(%s < 1)" % plan.date_fn("date_add_millis", T, "1", P("day")), "1")], "0")], ["count(*)"], {}, "'date_add_millis' inside CASE"),
    "a fifth string term": (None, FIVE[:4], ["max(%s)" % FIVE[4]], {}, "more than 4 distinct str_to_millis / date_part_str terms"),
    "constants outside the range": (None, [du.call_text("date_part_millis", "253402300800000", "year")], ["count(*)"], {}, "date_part_millis over constants"),
    "an UNSURE constant": (None, [du.call_text("str_to_millis", P("5:04:05"))], ["count(*)"], {}, "str_to_millis over the constant"),
}
OTHERS = ["date_diff_millis(%s, 0, \"day\")" % T, "date_diff_str(%s, %s, \"day\")" % (S, S), "date_add_str(%s, 1, \"day\")" % S, "date_trunc_str(%s, \"day\")" % S,
          "millis_to_str(%s)" % T, "millis_to_utc(%s)" % T, "millis_to_zone_name(%s, \"UTC\")" % T, "millis_to_local(%s)" % T, "millis_to_tz(%s, \"UTC\")" % T,
          "date_format_str(%s, \"2006-01-02\")" % S, "weekday_millis(%s)" % T, "weekday_str(%s)" % S, "date_range_millis(%s, 0, \"day\")" % T,
          "date_range_str(%s, %s, \"day\")" % (S, S), "now_millis()", "now_str()", "now_utc()", "now_local()", "now_tz(\"UTC\")", "clock_millis()", "clock_str()",
          "clock_utc()", "clock_local()", "clock_tz(\"UTC\")", "str_to_utc(%s)" % S, "str_to_zone_name(%s, \"UTC\")" % S, "str_to_tz(%s, \"UTC\")" % S,
          "str_to_duration(%s)" % S, "duration_to_str(%s)" % T, "millis(%s)" % S]


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_each_refusal_is_unsupported_and_names_its_construct(what):
    condition, keys, aggs, kw, names = REFUSED[what]
    e = refusal(condition, keys, aggs, **kw)
    assert e.status == _ffi.UNSUPPORTED, (e.status, e.message)
    assert names in e.message, e.message


@pytest.mark.parametrize("text", OTHERS, ids=[t.split("(")[0] for t in OTHERS])
def test_every_other_date_function_is_refused_by_its_name(text):
    e = refusal(None, [K], ["max(%s)" % text])
    assert e.status == _ffi.UNSUPPORTED, (e.status, e.message)
    assert "date function '%s'" % text.split("(")[0] in e.message, e.message


MALFORMED = ["date_part_millis(%s)" % T, "date_part_millis(%s, \"day\", \"UTC\", 1)" % T, "date_trunc_millis(%s)" % T, "date_trunc_millis(%s, \"day\", 1)" % T,
             "date_add_millis(%s, \"day\")" % T, "date_add_millis(%s, 1, \"day\", 2)" % T, "str_to_millis()", "str_to_millis(%s, \"x\")" % S,
             "date_part_str(%s)" % S, "date_part_str(%s, \"day\", 1)" % S, "date_part_millis(%s, \"day\"" % T]


@pytest.mark.parametrize("text", MALFORMED)
def test_a_wrong_argument_count_is_invalid(text):
    e = refusal(None, [text], ["count(*)"])
    assert e.status == _ffi.INVALID, (e.status, e.message)


def test_date_fn_writes_the_stringers_text_and_checks_its_arguments():
    assert plan.date_fn("DATE_TRUNC_MILLIS", T, plan.date_part("day")) == 'date_trunc_millis(%s, "day")' % T
    assert plan.date_fn("str_to_millis", S) == "str_to_millis(%s)" % S
    with pytest.raises(ValueError):
        plan.date_fn("date_diff_millis", T, T, '"day"')
    with pytest.raises(ValueError):
        plan.date_fn("date_add_millis", T, '"day"')
    with pytest.raises(ValueError):
        plan.date_part("fortnight")


# ---------------------------------------------------------------- the host evaluator

def parts_of(fn):
    return du.PART_NAMES if fn in ("date_part_millis", "date_part_str") else du.ADD_PARTS if fn == "date_add_millis" else du.TRUNC_PARTS


@pytest.mark.parametrize("fn", du.MILLIS_FUNCTIONS)
def test_the_host_evaluator_is_the_yardstick_over_the_millis_edges(fn):
    """every part name x the edge pool (x every n): tag and payload bit for bit, and the same rows raise"""
    raised = values = 0
    for part in parts_of(fn):
        for n in (du.ADD_NS if fn == "date_add_millis" else [None]):
            if isinstance(n, float) and (n != n or n in (du.PINF, du.NINF)):
                continue  # (NaN and the infinities have no constant text: tests/test_gpu_datefn.py brings them in a column)
            text = plan.date_fn(fn, T, du.const_text(n), P(part)) if fn == "date_add_millis" else du.call_text(fn, T, part)
            st, got, _ = du.eval_call(text, du.MILLIS_EDGES)
            assert st == _ffi.OK, text
            want = [du.apply_millis(fn, v, part, n=n) for v in du.MILLIS_EDGES]
            assert got == want, [(text, v, g, w) for v, g, w in zip(du.MILLIS_EDGES, got, want) if g != w][:4]
            raised += want.count(du.RAISE)
            values += sum(w != du.RAISE and w[0] == du.T_INT for w in want)
    assert raised > 10 and values > 100
    st, got, _ = du.eval_call(du.call_text("date_part_millis", T, "day", "UTC"), [BASE])
    assert st == _ffi.OK and got == [du.r_int(15)]


@pytest.mark.parametrize("fn", du.STRING_FUNCTIONS)
def test_the_host_evaluator_is_the_yardstick_over_the_string_pool(fn):
    pool = du.VALUE_STRINGS + du.NULL_STRINGS + [s for v in du.UNSURE_STRINGS.values() for s in v] + [M, None, 5, 2.5, True, [1], "x" * 64, "x" * 65, "2006-01-02" + " " * 60]
    for part in (parts_of(fn) if fn == "date_part_str" else [None]):
        text = du.call_text(fn, S, *([part] if part else []))
        st, got, _ = du.eval_call(text, pool)
        assert st == _ffi.OK, text
        want = [du.apply_string(fn, v, part) for v in pool]
        assert got == want, [(text, v, g, w) for v, g, w in zip(pool, got, want) if g != w][:4]
    assert want.count(du.RAISE) == sum(len(v) for v in du.UNSURE_STRINGS.values())


@pytest.mark.parametrize("row", GOLDEN["rows"], ids=[r["id"] for r in GOLDEN["rows"]])
def test_the_host_evaluator_gives_the_references_recorded_results(row):
    text = plan.date_fn(row["function"], T, *[du.const_text(a) for a in row["args"][1:]])
    st, got, _ = du.eval_call(text, [row["args"][0]])
    assert st == _ffi.OK and got == [du.r_int(row["result"])], (row["statement"], got)


def test_the_evaluator_refuses_what_create_refuses():
    assert du.eval_call(du.call_text("date_part_millis", T, "fortnight"), [0])[0] == _ffi.UNSUPPORTED
    assert du.eval_call(du.call_text("date_part_millis", T, "day", "US/Eastern"), [0])[0] == _ffi.UNSUPPORTED
    assert du.eval_call("date_diff_millis(%s, 0, \"day\")" % T, [0])[0] == _ffi.UNSUPPORTED
    assert du.eval_call("round(%s)" % T, [0])[0] == _ffi.INVALID
    assert du.eval_call(du.call_text("date_trunc_millis", "5", "day"), [0])[0] == _ffi.INVALID  # (the first argument stands for the value: a path)
    st, got, _ = du.eval_call(plan.date_fn("date_trunc_millis", T, "missing"), [0, None, M])
    assert st == _ffi.OK and got == [du.R_MISSING] * 3


# ---------------------------------------------------------------- what the GPU tests push

def test_the_library_takes_every_plan_of_the_gpu_differential():
    """tests/test_gpu_datefn.py counts a refusal as a failure: every plan it draws is created here, device side and oracle side
    alike; every function and every placement turns up; no drawn value raises (draw_plan evaluates them all)."""
    places, names = set(), set()
    for seed in range(du.NSEEDS):
        p = du.draw_plan(seed)
        places.add(p["place"])
        names.update(f for f in du.MILLIS_FUNCTIONS + du.STRING_FUNCTIONS if "'%s'" % f in repr(p["node"]))
        if p["place"] in ("having", "project"):
            keys, aggs = p["base"]
            if p["place"] == "having":
                paths = paths_of(None, keys, aggs, having="(%s %s 5)" % (p["over"], p["op"]))
            else:
                paths = paths_of(None, keys, aggs, project=[(keys[0], "k"), (p["over"], "p")])
        else:
            dcond, dkeys, daggs = p["device"]
            paths = paths_of(dcond, dkeys, daggs)
            ocond, okeys, oaggs = p["oracle"]
            assert D("h") in paths_of(ocond, okeys, oaggs)
        assert set(paths) <= {D(c) for c in ("t", "s", "k", "g", "x")}, (seed, paths)
    assert places == set(du.PLACEMENTS) and names == set(du.MILLIS_FUNCTIONS + du.STRING_FUNCTIONS)


def test_the_fused_shapes_compile_without_a_gpu():
    """date_apply<OP> inside the run-time-built scan: the shapes tests/test_gpu_datefn.py runs fused are instantiated through
    hiprtc (compile only, gfx950)."""
    import test_gpu_datefn as tg
    for name, (cond, keys, aggs) in sorted(tg.FUSED_SHAPES.items()):
        if name == "trunc-key":  # (a NUMBER-valued group key: its shape is fixed from device state, which needs a GPU)
            continue
        op = create(cond, keys, aggs)
        try:
            kinds = np.array([_ffi.COL_DICT32 if p == tg.CAT else _ffi.COL_TAGGED64 for p in op.column_paths], dtype=np.uint32)
            log = C.create_string_buffer(8192)
            st = _ffi.lib().n1k_jit_check(op._h, kinds.ctypes.data, len(kinds), log, 8192)
            assert st == _ffi.OK, (name, log.value.decode(errors="replace"))
        finally:
            op.done()
