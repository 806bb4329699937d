"""The date functions as values: the yardstick of tests/test_datefn_cpu.py and tests/test_gpu_datefn.py.

A pure-integer Python restatement of the reference's date arithmetic (expression/func_date.go) with time.Local = UTC:
  * millisToTime (:2395-2397) with time.Unix's normalisation, timeToMillis (:2403-2405) with Time.Round's half-up rule and the
    lost carry, value.NewValue's fold of an integral float to INT;
  * datePart (:2440-2498), dateAdd (:2504-2535, Time.AddDate / Time.Add), dateTrunc (:2541-2605, Time.Truncate / monthTrunc /
    yearTrunc), and the argument tests of DatePartMillis / DateTruncMillis / DateAddMillis / StrToMillis / DatePartStr .Apply;
  * the classifier of date strings this project fixes ("Date functions"): VALUE / UNSURE / NULL.
The calendar is counted here from a table of month lengths and the 400-year rule — not the closed forms the device uses — and
`datetime` is used by nothing in this file (tests/test_datefn_cpu.py cross-checks against it).

A result is (tag, payload) — the N1K_T_* tag and the 64 payload bits, compared bit for bit — or RAISE: the row raises
ERR_UNSUPPORTED_VALUE (Go's answer would depend on wrapped or out-of-range arithmetic, or on the toolchain's version).

Expressions of the plan generator:  ("col", name) | ("const", v) | ("arith", "+" | "-" | "*", x, y)
                                    | ("date", function, [args])     the part (and "UTC") as ("const", "day")
"""
from __future__ import annotations

import ctypes as C
import json
import math
import random
import re
import struct

import numpy as np

import cond_util as cn
from oracle import n1o
from query_amd import _ffi, plan

MISSING = cn.MISSING
T_MISSING, T_NULL, T_INT, T_FLOAT, T_STRING = n1o.T_MISSING, n1o.T_NULL, n1o.T_INT, n1o.T_FLOAT, n1o.T_STRING
R_MISSING, R_NULL = (T_MISSING, 0), (T_NULL, 0)
RAISE = "raise"

MILLIS_FUNCTIONS = ("date_part_millis", "date_trunc_millis", "date_add_millis")
STRING_FUNCTIONS = ("str_to_millis", "date_part_str")
PART_NAMES = ("millennium", "century", "decade", "year", "quarter", "month", "week", "day", "hour", "minute", "second", "millisecond",
              "day_of_year", "doy", "day_of_week", "dow", "iso_week", "iso_year", "iso_dow", "timezone", "timezone_hour", "timezone_minute")
ADD_PARTS = PART_NAMES[:12]
TRUNC_PARTS = tuple(p for p in ADD_PARTS if p != "week")
MIN_MILLIS, MAX_MILLIS = -62135596800000, 253402300799999  # 0001-01-01T00:00:00Z .. 9999-12-31T23:59:59.999Z
MIN_SEC, MAX_SEC = -62135596800, 253402300799
MAX_TERMS = 4      # kDateStrMaxTerms
DEV_MAX_LEN = 64   # bytes of a string datestr_table_kernel takes


def r_int(v: int):
    return (T_INT, v & 0xFFFFFFFFFFFFFFFF)


def f64_bits(f: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", f))[0]


def is_number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def new_value(f: float):
    """value.NewValue(float64): an integral value inside int64 IS the int (value/value.go:377-382)"""
    if f == f and not math.isinf(f) and -9223372036854775808.0 <= f < 9223372036854775808.0 and f == int(f):
        return r_int(int(f))
    return (T_FLOAT, f64_bits(f))


# ---------------------------------------------------------------- the calendar, from a table

MONTH_DAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)


def is_leap(y: int) -> bool:
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def days_before_year(y: int) -> int:
    """days from 1970-01-01 to y-01-01 (proleptic Gregorian; Python's // floors, so years before 1 work)"""
    y1 = y - 1
    return 365 * y1 + y1 // 4 - y1 // 100 + y1 // 400 - 719162  # (719162 days from 0001-01-01 to 1970-01-01)


def month_len(y: int, m: int) -> int:
    return 29 if m == 2 and is_leap(y) else MONTH_DAYS[m - 1]


def days_of(y: int, m: int, d: int) -> int:
    """days from 1970-01-01 to y-m-d, m in 1..12, d any integer (counted on from the first of the month)"""
    return days_before_year(y) + sum(month_len(y, k) for k in range(1, m)) + d - 1


def civil(days: int):
    """(year, month, day, yearday) of a day count"""
    y = 1970 + days // 366
    while days_before_year(y + 1) <= days:
        y += 1
    while days_before_year(y) > days:
        y -= 1
    yday = days - days_before_year(y) + 1
    m, rest = 1, yday
    while rest > month_len(y, m):
        rest -= month_len(y, m)
        m += 1
    return y, m, rest, yday


def go_div(a: int, b: int) -> int:
    """Go's integer division: truncated"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def go_mod(a: int, b: int) -> int:
    return a - go_div(a, b) * b


# ---------------------------------------------------------------- the millis functions

def millis_to_time(m: float):
    """time.Unix(int64(m / 1000), int64(math.Mod(m, 1000) * 1000000.0)) as (sec, nsec), or RAISE"""
    if m != m or math.isinf(m) or not MIN_MILLIS <= m <= MAX_MILLIS:
        return RAISE
    sec = int(m / 1000.0)
    nsec = int(math.fmod(m, 1000.0) * 1000000.0)
    if nsec < 0 or nsec >= 10 ** 9:  # time.Unix
        n = go_div(nsec, 10 ** 9)
        sec += n
        nsec -= n * 10 ** 9
        if nsec < 0:
            nsec += 10 ** 9
            sec -= 1
    if not MIN_SEC <= sec <= MAX_SEC:  # (the quotient rounded across the first second of year 1)
        return RAISE
    return sec, nsec


def time_to_millis(sec: int, nsec: int) -> float:
    """float64(t.Unix() * 1000) + float64(t.Round(time.Millisecond).Nanosecond()) / 1000000"""
    r = nsec % 10 ** 6
    rounded = nsec - r if r + r < 10 ** 6 else nsec + 10 ** 6 - r
    if rounded >= 10 ** 9:  # the carry goes into a second nobody reads
        rounded -= 10 ** 9
    return float(sec * 1000) + float(rounded) / 1000000.0


def canon_part(part: str) -> str:
    p = part.lower()
    return {"doy": "day_of_year", "dow": "day_of_week"}.get(p, p)


def date_part(wall: int, nsec: int, zone: int, part: str) -> int:
    """datePart over the wall clock `wall` seconds (counted in the time's own zone, `zone` seconds east of UTC)"""
    p = canon_part(part)
    days, sod = wall // 86400, wall % 86400
    y, m, d, yday = civil(days)
    wd = (days + 4) % 7  # Sunday = 0; 1970-01-01 was a Thursday
    if p in ("iso_week", "iso_year"):
        thursday = days - (wd + 6) % 7 + 3  # of the same Monday-based week
        iy, _m, _d, iyday = civil(thursday)
        return iy if p == "iso_year" else (iyday - 1) // 7 + 1
    return {"millennium": go_div(y, 1000) + 1, "century": go_div(y, 100) + 1, "decade": go_div(y, 10), "year": y, "quarter": (m + 2) // 3,
            "month": m, "day": d, "hour": sod // 3600, "minute": sod // 60 % 60, "second": sod % 60, "millisecond": nsec // 10 ** 6,
            "week": -(-yday // 7), "day_of_year": yday, "day_of_week": wd, "iso_dow": wd or 7, "timezone": zone,
            "timezone_hour": go_div(zone, 3600), "timezone_minute": go_div(zone - go_div(zone, 3600) * 3600, 60)}[p]


def date_trunc(sec: int, nsec: int, part: str):
    p = canon_part(part)
    if p == "millisecond":
        return sec, nsec - nsec % 10 ** 6
    if p in ("second", "minute", "hour", "day"):
        unit = {"second": 1, "minute": 60, "hour": 3600, "day": 86400}[p]
        return sec - sec % unit, 0  # Time.Truncate counts from 0001-01-01T00:00:00Z, a multiple of every unit
    y, m, _d, _yd = civil(sec // 86400)
    if p == "quarter":
        m -= (m - 1) % 3
    elif p != "month":
        m = 1
        y -= {"year": 0, "decade": y % 10, "century": y % 100, "millennium": y % 1000}[p]
    if y < 1:
        return RAISE
    return days_of(y, m, 1) * 86400, 0


def date_add(sec: int, nsec: int, n: int, part: str):
    p = canon_part(part)
    if p in ("hour", "minute", "second", "millisecond"):
        dur = n * {"hour": 3600 * 10 ** 9, "minute": 60 * 10 ** 9, "second": 10 ** 9, "millisecond": 10 ** 6}[p]
        if not -2 ** 63 <= dur < 2 ** 63:  # time.Duration(n) * unit wraps
            return RAISE
        sec, nsec = sec + go_div(dur, 10 ** 9), nsec + go_mod(dur, 10 ** 9)
        if nsec >= 10 ** 9:
            sec, nsec = sec + 1, nsec - 10 ** 9
        elif nsec < 0:
            sec, nsec = sec - 1, nsec + 10 ** 9
    else:
        y, m, d, _yd = civil(sec // 86400)
        sod = sec % 86400
        years, months, days = {"millennium": (1000 * n, 0, 0), "century": (100 * n, 0, 0), "decade": (10 * n, 0, 0), "year": (n, 0, 0),
                               "quarter": (0, 3 * n, 0), "month": (0, n, 0), "week": (0, 0, 7 * n), "day": (0, 0, n)}[p]
        # time.Date(year + years, month + months, day + days, ...): the months carry into the year, the days are counted on
        m0 = m - 1 + months
        y, m0 = y + years + m0 // 12, m0 % 12
        sec = (days_of(y, m0 + 1, 1) + d - 1 + days) * 86400 + sod
    if not MIN_SEC <= sec <= MAX_SEC:
        return RAISE
    return sec, nsec


def apply_millis(fn: str, x, part: str, n=None, zone=None):
    """DatePartMillis / DateTruncMillis / DateAddMillis .Apply over Python values (MISSING, None, bool, int, float, str, list,
    dict), the part a valid name.  zone: date_part_millis's third argument, "UTC" or None."""
    args = [x] + ([n] if fn == "date_add_millis" else [])
    if any(a is MISSING for a in args):
        return R_MISSING
    if not all(is_number(a) for a in args):
        return R_NULL
    if fn == "date_add_millis":
        nf = float(n)
        if nf != nf or (not math.isinf(nf) and nf != math.trunc(nf)):
            return R_NULL
    t = millis_to_time(float(x))
    if t == RAISE:
        return RAISE
    if fn == "date_part_millis":
        return r_int(date_part(t[0], t[1], 0, part))
    if fn == "date_add_millis":
        if math.isinf(nf) or abs(nf) > 2 ** 31:
            return RAISE
        t = date_add(t[0], t[1], int(nf), part)
    else:
        t = date_trunc(t[0], t[1], part)
    return RAISE if t == RAISE else new_value(time_to_millis(*t))


# ---------------------------------------------------------------- date strings

_DATE = rb"(\d{4})-(\d{2})-(\d{2})"
_TIME = rb"(\d{1,2}):(\d{2}):(\d{2})(?:([.,])(\d+))?(?:(Z)|([+-])(\d{2}):(\d{2}))?"
_WITH_DATE = re.compile(_DATE + rb"(?:[T ]" + _TIME + rb")?")
_TIME_ONLY = re.compile(_TIME)


def classify(s: bytes):
    """("null",) | ("unsure",) | ("value", year, month, day, hour, minute, second, nsec, zone seconds)"""
    m = _WITH_DATE.fullmatch(s)
    if m:
        y, mo, d = int(m.group(1)), int(m.group(2)), int(m.group(3))
        rest = m.groups()[3:]
    else:
        m = _TIME_ONLY.fullmatch(s)
        if not m:
            return ("null",)
        y, mo, d = 0, 1, 1
        rest = m.groups()
    unsure = False
    if not 1 <= mo <= 12 or d > month_len(y, mo):
        return ("null",)
    if d == 0:
        unsure = True
    hh, mi, ss, sep, frac, z, sign, zh, zm = rest
    h = minute = sec = nsec = zone = 0
    if hh is not None:
        h, minute, sec = int(hh), int(mi), int(ss)
        if h > 23 or minute > 59 or sec > 59:
            return ("null",)
        if len(hh) == 1:
            unsure = True
        if frac is not None:
            if sep == b"," or len(frac) > 9:
                unsure = True
            nsec = int(frac[:9].ljust(9, b"0"))
        if sign is not None:
            if int(zh) > 23 or int(zm) > 59:
                unsure = True
            zone = (int(zh) * 3600 + int(zm) * 60) * (-1 if sign == b"-" else 1)
    return ("unsure",) if unsure else ("value", y, mo, d, h, minute, sec, nsec, zone)


def apply_string(fn: str, s, part=None):
    """StrToMillis / DatePartStr .Apply over a Python value: a str or bytes is a STRING"""
    if s is MISSING:
        return R_MISSING
    if not isinstance(s, (str, bytes)):
        return R_NULL
    c = classify(s.encode() if isinstance(s, str) else s)
    if c[0] == "null":
        return R_NULL
    if c[0] == "unsure":
        return RAISE
    _k, y, mo, d, h, mi, sec, nsec, zone = c
    wall = days_of(y, mo, d) * 86400 + h * 3600 + mi * 60 + sec
    if fn == "date_part_str":
        return r_int(date_part(wall, nsec, zone, part))
    return new_value(time_to_millis(wall - zone, nsec))


def apply(fn: str, args):
    """one call over evaluated arguments, the part (and zone) among them as Python strings"""
    if fn == "date_add_millis":
        return apply_millis(fn, args[0], args[2], n=args[1])
    if fn in MILLIS_FUNCTIONS:
        return apply_millis(fn, args[0], args[1], zone=args[2] if len(args) > 2 else None)
    return apply_string(fn, args[0], args[1] if fn == "date_part_str" else None)


def result_value(r):
    """(tag, payload) -> the Python value a decoded result holds"""
    if r == R_MISSING:
        return MISSING
    if r == R_NULL:
        return None
    tag, p = r
    return p - 2 ** 64 if tag == T_INT and p >= 2 ** 63 else p if tag == T_INT else struct.unpack("<d", struct.pack("<Q", p))[0]


# ---------------------------------------------------------------- the pools

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")


def ms_of(y, mo, d, h=0, mi=0, s=0, ms=0):
    return (days_of(y, mo, d) * 86400 + h * 3600 + mi * 60 + s) * 1000 + ms


MILLIS_EDGES = [
    MIN_MILLIS, MIN_MILLIS - 1, MAX_MILLIS, MAX_MILLIS + 1, float(MIN_MILLIS) + 0.5, float(MAX_MILLIS) + 0.5, 0, -1, 1, 0.5, -0.5, -0.0,
    ms_of(1999, 12, 31, 23, 59, 59, 999), ms_of(2000, 1, 1), ms_of(2016, 12, 31, 23, 59, 59, 999), ms_of(1, 12, 31, 23, 59, 59, 999),
    ms_of(1900, 2, 28), ms_of(1900, 2, 28, 23, 59, 59, 999), ms_of(1900, 3, 1), ms_of(2000, 2, 28), ms_of(2000, 2, 29, 12), ms_of(2000, 3, 1),
    ms_of(2024, 2, 28, 23), ms_of(2024, 2, 29), ms_of(2024, 3, 1) - 1, ms_of(2023, 2, 28, 23, 59, 59, 999),
    # the rounding of the nanoseconds carries into the next second (and is lost): .9996 s, before and after 1970
    ms_of(2016, 5, 15, 3, 59, 0) + 999.6, float(ms_of(1960, 1, 1)) - 0.4, 1.412243464575684768e+12, 1463284740000, 1.453505233e+12,
    ms_of(2016, 1, 31, 10), ms_of(2015, 12, 31), ms_of(2021, 1, 3), ms_of(2020, 12, 28), ms_of(2018, 12, 31), ms_of(2010, 1, 3, 23, 59, 59, 999),
    ms_of(999, 6, 15), ms_of(99, 6, 15), ms_of(9, 6, 15), ms_of(9999, 1, 1), ms_of(9990, 6, 30, 1, 2, 3, 4), ms_of(1969, 12, 31, 23, 59, 59, 999),
    ms_of(1582, 10, 10), ms_of(1, 1, 1, 0, 0, 0, 1), 86399999.75, 1e15, -1e15, 2 ** 53 + 1, NAN, PINF, NINF,
    MISSING, None, True, "2016-01-01", [1], {"a": 1},
]
ADD_NS = [0, 1, -1, 13, -13, 2.5, 12, -12, 3, 400, -400, 1000, 2 ** 31, -(2 ** 31), 2 ** 31 + 1, -(2 ** 31) - 1, 2562047, 2562048, -2562048,
          153722867, 153722868, -153722868, 1e300, NAN, PINF, MISSING, None, "3", 30, 31, 366, 3.0]

LAYOUT_STRINGS = [  # every layout of _DATE_FORMATS, with and without a fraction where it has seconds
    "2006-01-02T15:04:05.999+07:00", "2006-01-02T15:04:05+07:00", "2006-01-02T15:04:05.5Z", "2006-01-02T15:04:05Z",
    "2006-01-02T15:04:05.999", "2006-01-02T15:04:05", "2006-01-02 15:04:05.999-07:00", "2006-01-02 15:04:05-07:00",
    "2006-01-02 15:04:05.123456789Z", "2006-01-02 15:04:05Z", "2006-01-02 15:04:05.999", "2006-01-02 15:04:05", "2006-01-02",
    "15:04:05.999+07:00", "15:04:05+07:00", "15:04:05.25Z", "15:04:05Z", "15:04:05.999", "15:04:05",
]
VALUE_STRINGS = LAYOUT_STRINGS + [
    "2016-09-26T11:33:16.209-04:00", "2016-09-26T11:33:16.209-07:00", "2015-01-01T16:00:00-08:00", "2004-07-09", "11:42:01Z", "2004-07-09T11:42:01Z",
    "0000-01-01", "0000-12-31T23:59:59.999999999Z", "9999-12-31T23:59:59.999999999-23:59", "0001-01-01T00:00:00+23:59", "2000-02-29", "2024-02-29T00:00:00Z",
    "1900-02-28T23:59:59.9996Z", "1969-12-31T23:59:59.9995Z", "1970-01-01T00:00:00.0004999Z", "2016-12-31T23:59:59Z",
    "2021-01-03", "2020-12-28", "2010-01-03T10:00:00+00:00", "00:00:00", "23:59:59.999999999-00:01", "2006-01-02T15:04:05.1", "2006-01-02T15:04:05.12",
    "2006-01-02T15:04:05.000000001Z", "2016-02-29 12:30:45.5+05:30", "1999-12-31T23:59:59.999Z",
]
UNSURE_STRINGS = {
    "hour of one digit": ["2006-01-02T5:04:05Z", "5:04:05", "2006-01-02 5:04:05.5+01:00"],
    "day 00": ["2006-01-00", "2006-02-00T15:04:05Z"],
    "zone beyond 23:59": ["2006-01-02T15:04:05+24:00", "15:04:05-07:60", "2006-01-02 15:04:05.5+99:99"],
    "fraction over 9 digits": ["2006-01-02T15:04:05.1234567890Z", "15:04:05.0000000001"],
    "comma for the point": ["2006-01-02T15:04:05,999Z", "15:04:05,5"],
}
NULL_STRINGS = [
    "", "x", "2006-01-02x", "x2006-01-02", " 2006-01-02", "2006-01-02 ", "2006-01-02t15:04:05Z", "2006-01-02T15:04:05z", "2006-1-02", "2006-01-2",
    "12006-01-02", "206-01-02", "2006-13-02", "2006-00-02", "2006-02-30", "2006-04-31", "1900-02-29", "2023-02-29", "2006-01-32", "2006/01/02", "2012/01/02",
    "2006-01-02T24:04:05", "2006-01-02T15:60:05", "2006-01-02T15:04:60", "2006-01-02T15:4:05", "2006-01-02T15:04:5", "2006-01-02T15:04", "2006-01-02T",
    "2006-01-02  15:04:05", "2006-01-02T15:04:05.", "2006-01-02T15:04:05.Z", "2006-01-02T15:04:05+0700", "2006-01-02T15:04:05+07", "2006-01-02T15:04:05+7:00",
    "2006-01-02T15:04:05 +07:00", "2006-01-02T15:04:05ZZ", "2006-01-02T15:04:05Z+07:00", "2006-01-02Z", "2006-01-02+07:00", "15:04", "15:04:05 ", "115:04:05",
    "not a date", "1463284740000", "2006-01-02T15:04:05.999+07:00 ", "٢٠٠٦-٠١-٠٢", "2006-01-02T15:04:05.9x", "2006-01-00x", "-006-01-02", "2006-01-02T-5:04:05",
    "[1,2]", "{}", "2006-01-02T15:04:05+07:0", "2006-01-02T15:04:05-07:000",
]


# ---------------------------------------------------------------- text

D = cn.D


def const_text(v) -> str:
    if v is MISSING:
        return "missing"
    if is_number(v) and v < 0:
        return "(-%s)" % json.dumps(-v)  # (the stringer writes a negative constant as a negation)
    return json.dumps(v)


def call_text(fn: str, first: str, *rest) -> str:
    """date_add_millis((`d`.`t`), 3, "month"): `first` is expression text, the other arguments Python constants"""
    return plan.date_fn(fn, first, *[const_text(a) for a in rest])


def value_text(e, col=D) -> str:
    k = e[0]
    if k == "col":
        return col(e[1])
    if k == "const":
        return const_text(e[1])
    if k == "arith":
        return "(%s %s %s)" % (value_text(e[2], col), e[1], value_text(e[3], col))
    assert k == "date", e
    return plan.date_fn(e[1], *[value_text(a, col) for a in e[2]])


class Raised(Exception):
    """the row raises ERR_UNSUPPORTED_VALUE"""


def eval_value(e, row):
    k = e[0]
    if k == "col":
        return row[e[1]]
    if k == "const":
        return e[1]
    if k == "arith":
        return cn.arith(e[1], eval_value(e[2], row), eval_value(e[3], row))
    assert k == "date", e
    r = apply(e[1], [eval_value(a, row) for a in e[2]])
    if r == RAISE:
        raise Raised(value_text(e))
    return result_value(r)


# ---------------------------------------------------------------- the evaluators behind the C ABI

def _marshal(values):
    """Python values -> (tags, payload, offsets, bytes): a str / bytes is a STRING with its text in the block"""
    n = len(values)
    tags, pay, off = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n + 1, np.uint64)
    blob = bytearray()
    for i, v in enumerate(values):
        if v is MISSING:
            tags[i] = T_MISSING
        elif v is None:
            tags[i] = T_NULL
        elif isinstance(v, bool):
            tags[i] = n1o.T_TRUE if v else n1o.T_FALSE
        elif isinstance(v, int):
            tags[i], pay[i] = T_INT, v & 0xFFFFFFFFFFFFFFFF
        elif isinstance(v, float):
            tags[i], pay[i] = T_FLOAT, f64_bits(v)
        elif isinstance(v, (str, bytes)):
            tags[i] = T_STRING
            blob += v.encode() if isinstance(v, str) else v
        else:
            tags[i] = n1o.T_ARRAY if isinstance(v, list) else n1o.T_OBJECT
        off[i + 1] = len(blob)
    return tags, pay, off, bytes(blob) + b"\0"


def eval_call(text: str, values, device=None):
    """n1k_datefn_eval (device None) or n1k_datefn_eval_device over Python values.  Returns (status, results, extra):
    results[i] is (tag, payload) or RAISE; extra = {"any_raise", "left"} on the device."""
    L = _ffi.lib()
    tags, pay, off, blob = _marshal(values)
    n = len(values)
    ot, op, orr = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint8)
    t = text.encode()
    args = [t, len(t), n, tags.ctypes.data, pay.ctypes.data, off.ctypes.data, blob, ot.ctypes.data, op.ctypes.data, orr.ctypes.data]
    extra = {}
    if device is None:
        st = L.n1k_datefn_eval(*args)
    else:
        anyr, left = C.c_uint32(0), C.c_uint64(0)
        st = L.n1k_datefn_eval_device(device, *args, C.byref(anyr), C.byref(left))
        extra = {"any_raise": int(anyr.value), "left": int(left.value)}
    res = [RAISE if orr[i] else (int(ot[i]), int(op[i])) for i in range(n)]
    return int(st), res, extra


# ---------------------------------------------------------------- tables for the plans

def date_table(rows, names_tagged=("t", "x", "g"), names_dict=("s", "k"), dictionary=None, tagged_strings=()):
    """rows of Python values -> an oracle / device table.  names_tagged: TAGGED64 columns of numbers (and any non-string);
    names_dict: DICT32 columns of strings; tagged_strings: TAGGED64 columns that hold strings too.  The dictionary is built
    from the strings in order of first appearance unless given."""
    words, code = [], {}
    if dictionary is not None:
        words = [w if isinstance(w, bytes) else w.encode() for w in dictionary]
        code = {w: i for i, w in enumerate(words)}

    def code_of(v):
        b = v.encode() if isinstance(v, str) else v
        if b not in code:
            code[b] = len(words)
            words.append(b)
        return code[b]

    cols = []
    for name in list(names_tagged) + list(tagged_strings):
        if not rows or name not in rows[0]:
            continue
        vals = [r[name] for r in rows]
        tags, pay, _off, _blob = _marshal([None if isinstance(v, (str, bytes, list, dict)) else v for v in vals])
        for i, v in enumerate(vals):
            if isinstance(v, (str, bytes)):
                tags[i], pay[i] = T_STRING, code_of(v)
            elif isinstance(v, (list, dict)):
                tags[i], pay[i] = (n1o.T_ARRAY if isinstance(v, list) else n1o.T_OBJECT), code_of(json.dumps(v, separators=(",", ":")))
        cols.append(n1o.Column(D(name), n1o.COL_TAGGED64, tags=tags, payload=pay))
    for name in names_dict:
        if not rows or name not in rows[0]:
            continue
        codes = np.array([0xFFFFFFFF if r[name] is MISSING else 0xFFFFFFFE if r[name] is None else code_of(r[name]) for r in rows], np.uint32)
        cols.append(n1o.Column(D(name), n1o.COL_DICT32, codes=codes))
    return n1o.Table(cols, list(words))


def helper_column(name, values):
    """the yardstick's values of a node as a TAGGED64 column the oracle reads (numbers, NULL, MISSING only)"""
    tags, pay, _off, _blob = _marshal(values)
    assert not any(isinstance(v, (str, bytes, list, dict)) for v in values)
    return n1o.Column(D(name), n1o.COL_TAGGED64, tags=tags, payload=pay)


# ---------------------------------------------------------------- the seeded generator
#
# Rows: t a millis inside years 1971 .. 2037 (ints, some with a fraction k / 8, some NULL / MISSING / a string), s a date
# string of SEED_STRINGS (VALUE strings, some that are NULL to the classifier, NULL, MISSING; no UNSURE one), k key strings,
# g ints 0 .. 6, x small numbers.  No drawn call can raise: the millis stay far inside the range under every n drawn.

SEED_STRINGS = [s for s in VALUE_STRINGS if not s.startswith(("0000", "9999", "0001"))] + ["not a date", "2012/01/02", "", "2006-1-02"]
KEYS = ["cat_1", "cat_2", "cat_3", "zz"]
PLACEMENTS = ["key", "agg", "filter", "having", "project"]
NSEEDS = 120


def make_rows(rng, n):
    rows = []
    base = ms_of(1971, 1, 1)
    span = ms_of(2037, 1, 1) - base
    for i in range(n):
        r = rng.random()
        t = MISSING if r < 0.04 else None if r < 0.08 else "a" if r < 0.1 else base + rng.randrange(span) + (rng.randrange(8) / 8.0 if r < 0.3 else 0)
        if isinstance(t, float) and t == int(t):
            t = int(t)
        r = rng.random()
        s = MISSING if r < 0.05 else None if r < 0.1 else rng.choice(SEED_STRINGS)
        rows.append({"t": t, "s": s, "k": rng.choice(KEYS), "g": rng.randrange(7), "x": rng.randrange(100), "id": i})
    return rows


def draw_call(rng, tail=False):
    """one call over the row's columns; tail: over `t` or `s` alone (the column then stands for a group key or an aggregate)"""
    t, g = ("col", "t"), ("col", "g")
    r = rng.random()
    if r < 0.3:
        first = t if tail else rng.choice([t, t, ("arith", "+", t, ("const", 86400000)), ("arith", "-", t, ("arith", "*", g, ("const", 3600000)))])
        args = [first, ("const", rng.choice(PART_NAMES))] + ([("const", "UTC")] if rng.random() < 0.2 else [])
        return ("date", "date_part_millis", args)
    if r < 0.5:
        return ("date", "date_trunc_millis", [t, ("const", rng.choice(TRUNC_PARTS))])
    if r < 0.7:
        part = rng.choice(ADD_PARTS)
        n = ("const", rng.choice([0, 1, 13, 2.5, 40]))
        if not tail:
            n = rng.choice([n, g, ("arith", "-", g, ("const", 3))])
        if part in ("millennium", "century"):
            n = ("const", rng.choice([0, 1, 2.5]))
        return ("date", "date_add_millis", [t, n, ("const", part)])
    if r < 0.85:
        return ("date", "str_to_millis", [("col", "s")])
    return ("date", "date_part_str", [("col", "s"), ("const", rng.choice(PART_NAMES))])


def uses_column(e, name):
    if isinstance(e, tuple):
        return (e[0] == "col" and e[1] == name) or any(uses_column(x, name) for x in e[1:])
    return isinstance(e, list) and any(uses_column(x, name) for x in e)


def draw_plan(seed):
    """One plan of the differential: the rows, the node, its placement.
    key / agg / filter: the device's and the oracle's (condition, keys, aggregates); the oracle reads helper column `h`, the
    yardstick's value of the node for every row, where the device evaluates the node.
    having / project: the node stands over a group key (`s`) or over MIN / MAX of `t` / `s`: "source" is that key's or
    aggregate's text, "base" the (keys, aggregates) both sides group by, "over" the node's text over the source, "op" and
    "const" HAVING's comparison (the constant is chosen once the groups are known)."""
    rng = random.Random(770_000 + seed)
    rows = make_rows(rng, rng.randint(1, 1500))
    place = PLACEMENTS[seed % len(PLACEMENTS)]
    tail = place in ("having", "project")
    node = draw_call(rng, tail)
    if rng.random() < 0.3 and node[1] in ("date_trunc_millis", "date_add_millis"):  # a two-node chain: a part of a truncated / added time
        node = ("date", "date_part_millis", [node, ("const", rng.choice(PART_NAMES))])
    if rng.random() < 0.2:
        node = ("arith", "+", node, ("const", 1))
    out = {"rows": rows, "node": node, "place": place}
    K, X = D("k"), D("x")
    if tail:
        col = "s" if uses_column(node, "s") else "t"
        how = rng.choice(["key", "min", "max"]) if col == "s" else rng.choice(["min", "min", "max"])  # (MAX(t) is often the string among them)
        source = D(col) if how == "key" else "%s(%s)" % (how, D(col))
        out.update(col=col, how=how, source=source, over=value_text(node, lambda name: source), op=rng.choice(["<", "<="]),
                   base=([D(col)] if how == "key" else [K], sorted(["count(*)"] + ([] if how == "key" else [source]))))
        return out
    values = [eval_value(node, r) for r in rows]  # (Raised here would be a generator bug)
    text, h = value_text(node), D("h")
    out["values"] = values
    if place == "key":
        out["device"], out["oracle"] = (None, [text, K], ["count(*)", "sum(%s)" % X]), (None, [h, K], ["count(*)", "sum(%s)" % X])
    elif place == "agg":
        f = rng.choice(["min(%s)", "max(%s)", "sum(%s)", "count(%s)", "avg(%s)"])
        out["device"], out["oracle"] = (None, [K], [f % text, "count(*)"]), (None, [K], [f % h, "count(*)"])
    else:
        nums = sorted(v for v in values if is_number(v))
        c = nums[len(nums) // 2] if nums else 0
        op = rng.choice(["<", "<=", "="])
        ct = const_text(c)
        out["device"], out["oracle"] = ("(%s %s %s)" % (text, op, ct), [K], ["count(*)"]), ("(%s %s %s)" % (h, op, ct), [K], ["count(*)"])
    return out
