"""The aggregate yardstick (tests/agg_util.py) checked without a GPU: against a hand-written table of the reference's branches,
against the C oracle (one thread, rows in order) over every group the GPU tests draw, and for the condition those tests
rest on: every group of the pools is well defined."""
import math

import pytest

import agg_util as ag
from agg_util import F, I, S, FALSE, MISSING, NULL, TRUE
from oracle import n1o

NAN, PINF, NINF, MIN64, MAX64 = ag.NAN, ag.PINF, ag.NINF, ag.MIN64, ag.MAX64

# (operands, kind, expected): written down from the Go text, not from the yardstick.  An expected int is an INT, an expected
# float a FLOAT, None is NULL, "nan" any NaN; strings are bytes, booleans themselves.
HAND = [
    # Count / Countn (agg_count.go:102-116, agg_countn.go:84-97)
    ([I(1), NULL, MISSING, S(b""), TRUE, F(NAN)], "count", 4), ([I(1), NULL, MISSING, S(b""), TRUE, F(NAN)], "countn", 2),
    ([NULL, MISSING], "count", 0), ([NULL, MISSING], "countn", 0), ([FALSE], "count", 1), ([FALSE], "countn", 0),
    # Sum: NUMBERs only, Default() NULL; intValue.Add keeps the int for one sign and no overflow (integer.go:266-277)
    ([NULL, S(b"m"), TRUE], "sum", None), ([], "sum", None), ([I(2), I(3)], "sum", 5), ([I(-2), I(-3)], "sum", -5),
    ([I(5), I(-3)], "sum", 2.0), ([I(5), I(-7), I(2)], "sum", 0.0), ([I(MAX64 - 1), I(1)], "sum", MAX64), ([I(MAX64), I(1)], "sum", 2.0 ** 63),
    ([I(MIN64 + 1), I(-1)], "sum", MIN64), ([I(MIN64), I(-1)], "sum", -(2.0 ** 63)), ([I(0)], "sum", 0), ([I(MIN64)], "sum", MIN64),
    ([I(1), F(0.5)], "sum", 1.5), ([F(0.5), F(0.5)], "sum", 1.0), ([F(-0.0)], "sum", -0.0), ([F(PINF), F(NINF)], "sum", "nan"),
    ([F(NAN), I(1)], "sum", "nan"), ([F(PINF), I(1), NULL], "sum", PINF), ([F(1e308), F(1e308)], "sum", PINF),
    ([I(2 ** 40), I(2 ** 40 - 1)], "sum", 2 ** 41 - 1),
    # deviation (iii): mixed signs beyond 2^53 — the device converts the exact total (the reference: 2^53 - 1, see below)
    ([I(2 ** 53 + 1), I(-1)], "sum", 2.0 ** 53),
    # Avg (agg_avg.go:111-129): float64(sum) / float64(count), NewValue folds an integral quotient
    ([I(1), I(2)], "avg", 1.5), ([I(1), I(3)], "avg", 2), ([I(2 ** 53 + 1)], "avg", 2 ** 53), ([I(MAX64)], "avg", 2.0 ** 63),
    ([I(MIN64)], "avg", MIN64), ([F(-0.0)], "avg", 0), ([F(0.5), NULL], "avg", 0.5), ([NULL], "avg", None), ([F(NAN)], "avg", "nan"),
    ([F(PINF), I(1)], "avg", PINF), ([I(5), I(-7), I(2)], "avg", 0),
    # Min / Max (agg_min.go:117-127): type order false < true < numbers < strings; NaN first among the numbers; ints exactly
    ([S(b"m"), I(3), TRUE, NULL], "min", True), ([S(b"m"), I(3), TRUE, NULL], "max", b"m"), ([TRUE, FALSE], "min", False),
    ([TRUE, FALSE], "max", True), ([NULL, MISSING], "min", None), ([NULL, MISSING], "max", None),
    ([F(NAN), F(NINF)], "min", "nan"), ([F(NAN), F(NINF)], "max", NINF), ([F(NAN)], "max", "nan"), ([I(1), F(PINF)], "max", PINF),
    ([I(2 ** 53), I(2 ** 53 + 1)], "max", 2 ** 53 + 1), ([I(-(2 ** 53)), I(-(2 ** 53 + 1))], "min", -(2 ** 53 + 1)),
    ([I(MAX64)], "min", MAX64), ([I(MIN64)], "max", MIN64), ([I(MAX64), F(1e308)], "min", MAX64), ([I(MIN64), F(-1e308)], "max", MIN64),
    ([S(b""), S(b"m")], "min", b""), ([S(b"")], "max", b""), ([F(-0.0)], "min", -0.0), ([F(5e-324), I(0)], "max", 5e-324),
]


def _as_pair(e):
    if e is None:
        return ag.NULL
    if e == "nan":
        return F(NAN)
    if isinstance(e, bool):
        return TRUE if e else FALSE
    if isinstance(e, int):
        return I(e)
    if isinstance(e, float):
        return F(e)
    return S(e)


@pytest.mark.parametrize("ops,kind,expected", HAND, ids=["%s-%d" % (h[1], i) for i, h in enumerate(HAND)])
def test_the_yardstick_against_the_hand_table(ops, kind, expected):
    got = ag.yardstick(ops)[kind]
    assert ag.same_bits(got, _as_pair(expected)), (ops, kind, got, expected)


def test_the_reference_chain_where_the_device_documents_a_deviation():
    """value/integer.go:266-277 over rows in order: what the oracle has to give, and where the yardstick says otherwise"""
    assert ag.reference_sum([I(2 ** 53 + 1), I(-1)]) == F(2.0 ** 53 - 1) and ag.deviates([I(2 ** 53 + 1), I(-1)])
    t = ag.DIRECTED["transient-overflow-mixed"]  # deviation (ii)
    assert ag.reference_sum(t) == F(0.0) and ag.yardstick(t)["sum"] == F(1.0) and ag.deviates(t)
    q = ag.Q
    # same sign: the chain overflows for good, float64 from there on; the total does not fit either: no deviation
    assert ag.reference_sum([I(q)] * 4) == F(2.0 ** 63) and not ag.deviates([I(q)] * 4)
    assert ag.reference_sum([I(5), I(-3)]) == F(2.0) and not ag.deviates([I(5), I(-3)])
    assert ag.reference_sum([NULL, S(b"m")]) == ag.NULL and ag.reference_avg([I(1), I(2)]) == F(1.5)


def test_comparison_rule():
    y = ag.yardstick([F(1e16), F(1.0), F(-1e16)])
    assert y["sum"] == F(1.0) and y["float_part"] and y["bound"] == 3 * 2.0 ** -53 * (2e16 + 1.0)
    assert ag.same_value("sum", F(0.0), y["sum"], y) and ag.same_value("sum", F(2.0), y["sum"], y)  # (either order of the adds)
    assert not ag.same_value("sum", F(16.0), y["sum"], y) and not ag.same_value("sum", F(NAN), y["sum"], y)
    assert not ag.same_value("sum", I(1), y["sum"], y)  # Add of a float is a floatValue
    y = ag.yardstick([F(PINF), I(1)])
    assert y["special"] and ag.same_value("sum", F(PINF), y["sum"], y) and not ag.same_value("sum", F(1e308), y["sum"], y)
    y = ag.yardstick([F(NAN), I(1)])
    assert ag.same_value("sum", F(NAN), y["sum"], y) and not ag.same_value("sum", F(PINF), y["sum"], y)
    y = ag.yardstick([F(-0.0)])  # value/float.go:41-43: both zeros print 0
    assert ag.text_of(F(-0.0)) == ag.text_of(F(0.0)) == "0"
    assert ag.same_value("sum", F(0.0), y["sum"], y) and ag.same_value("min", F(-0.0), y["min"], y)
    assert not ag.same_value("min", I(0), y["min"], y) and not ag.same_value("min", F(5e-324), y["min"], y)
    y = ag.yardstick([I(2 ** 53 + 1)])
    assert not ag.same_value("max", I(2 ** 53), y["max"], y) and not ag.same_value("max", F(2.0 ** 53), y["max"], y)


def test_order_dependent_groups_are_reported():
    for ops in ([I(0), F(0.0)], [F(0.0), F(-0.0)], [I(0), F(-0.0)], [I(7), F(7.0), F(8.5)], [I(2 ** 53 + 1), F(2.0 ** 53)],
                [I(2 ** 53 + 1), I(2 ** 53), F(2.0 ** 53), I(5)], [F(1e308), F(1e308), F(-1e308)]):
        assert not ag.yardstick(ops)["well_defined"], ops
    for ops in ([I(0), F(0.5)], [F(NAN), F(NAN)], [I(2 ** 53 + 1), F(2.0 ** 53 + 2)], [I(2 ** 53 + 1), I(2 ** 53)], [F(1e308), F(1e308)]):
        assert ag.yardstick(ops)["well_defined"], ops


def test_every_group_of_the_pools_is_well_defined():
    """the condition of tests/test_gpu_agg_edges.py: it leaves out no case, because none of these is order dependent"""
    groups = ag.all_groups()
    assert len(ag.SINGLETONS) == 31 and len(ag.DIRECTED) >= 25
    for name, ops in groups:
        assert ag.yardstick(ops)["well_defined"], (name, ops)
    # of the 625 ordered pairs only ties (an int and its float, the zeros) are left out
    left_out = [(a, b) for a in ag.NUMERIC for b in ag.NUMERIC if not ag.yardstick([a, b])["well_defined"]]
    assert len(ag.NUMERIC) == 25 and len(ag.pair_groups()) + len(left_out) == 625
    for a, b in left_out:
        zeros = a[1] == 0 and b[1] == 0 and not ag.same_bits(a, b)
        images = {a[0], b[0]} == {ag.T_INT, ag.T_FLOAT} and float(a[1]) == float(b[1])
        assert zeros or images, (a, b)
    assert len(left_out) == 6 and ag.yardstick([F(1e308), F(-1e308)])["sum"] == F(0.0), left_out
    y = ag.yardstick(ag.ARRAY_GROUP)
    assert y["min"] == ag.UNSUPPORTED and y["max"] == ag.UNSUPPORTED


def test_the_yardstick_against_the_oracle_on_every_group():
    """One oracle run, one thread, group after group in row order.  SUM / AVG: the oracle IS the reference's chain of Add,
    bit for bit, floats included; the yardstick agrees wherever no documented deviation applies, and those groups are
    mixed-sign ints beyond 2^53.  COUNT / COUNTN / MIN / MAX: the yardstick everywhere."""
    names = [n for n, _ in ag.all_groups()]
    groups = [g for _, g in ag.all_groups()]
    ora = ag.by_group(n1o.run(ag.table(groups, interleave=False), None, [ag.G], ag.AGGS, threads=1), len(groups))
    bad, deviating = [], []
    for name, ops, got in zip(names, groups, ora):
        y = ag.yardstick(ops)
        if not ag.same_bits(got["sum"], ag.reference_sum(ops)) or not ag.same_bits(got["avg"], ag.reference_avg(ops)):
            bad.append((name, ops, "chain", got["sum"], ag.reference_sum(ops), got["avg"], ag.reference_avg(ops)))
        dev = ag.deviates(ops, y)
        if dev:
            deviating.append(name)
            ints = [v for t, v in ops if t == ag.T_INT]
            assert min(ints) < 0 <= max(ints) and max(abs(v) for v in ints) > 2 ** 53, (name, ops)
        kinds = [k for k in ag.KINDS if not (dev and k in ("sum", "avg"))]
        for d in ag.differences(ops, got, y, kinds):
            bad.append((name, ops) + d)
    assert not bad, (len(bad), bad[:10])
    assert "transient-overflow-mixed" in deviating and len(deviating) < len(groups) // 4, deviating
