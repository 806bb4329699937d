"""Every tuning option of n1k_set_option has an oracle check: a value table in geometry_util.GEOMETRY (run by
test_gpu_geometries.py), an existing test that sets it (COVERED), or a stated reason (EXEMPT).  CPU only."""
import os
import re

import pytest

import geometry_util as gu
import query_amd
from query_amd import _ffi, plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def engine_option_names(src=None):
    """The option names n1k_set_option compares against (query_amd/csrc/n1k_engine.cpp)."""
    if src is None:
        src = open(os.path.join(ROOT, "query_amd", "csrc", "n1k_engine.cpp")).read()
    start = src.index("n1k_status n1k_set_option(")
    end = src.index("unknown option", start)
    return re.findall(r'\bn\s*==\s*"([A-Za-z0-9_]+)"', src[start:end])


def test_option_parser_sees_the_engine():
    names = engine_option_names()
    assert len(names) == len(set(names)) and len(names) >= 40
    assert {"block", "rec_block", "dedupe_block", "part_block", "device"} <= set(names)
    probe = 'n1k_status n1k_set_option(\n    else if (n == "x_probe") h->opt_x = value;\n    return fail(h, N1K_INVALID, "unknown option %s", name);'
    assert engine_option_names(probe) == ["x_probe"]


def test_every_option_has_an_oracle_check():
    names = set(engine_option_names())
    tables = [set(gu.GEOMETRY), set(gu.COVERED), set(gu.EXEMPT)]
    missing = names - set().union(*tables)
    assert not missing, "tuning options without an oracle check (add them to tests/geometry_util.py): %s" % sorted(missing)
    stale = set().union(*tables) - names
    assert not stale, "geometry_util.py names options the engine does not have: %s" % sorted(stale)
    for i, a in enumerate(tables):
        for b in tables[i + 1:]:
            assert not a & b, "an option in two tables: %s" % sorted(a & b)
    assert all(len(r.strip()) > 10 for r in gu.EXEMPT.values())


@pytest.mark.parametrize("option", sorted(gu.COVERED))
def test_covered_options_name_a_test_that_sets_them(option):
    path, _, name = gu.COVERED[option].partition("::")
    src = open(os.path.join(ROOT, path)).read()
    assert re.search(r"^def %s\(" % re.escape(name), src, re.M), gu.COVERED[option]
    assert re.search(r"""["']%s["']|\b%s=""" % (option, option), src), "%s does not set %s" % (path, option)


def _handle():
    D = gu.D
    return query_amd.GpuFilterGroup(plan.filter_group_plan("(50 < %s)" % D("price"), [D("cat")], ["sum(%s)" % D("price")]))


@pytest.mark.parametrize("option", sorted(gu.GEOMETRY))
def test_geometry_values_are_accepted(option):
    op = _handle()
    try:
        for v in gu.GEOMETRY[option]:
            op.set_option(option, v)
    finally:
        op.done()


@pytest.mark.parametrize("option,value", sorted(gu.REFUSED.items()))
def test_documented_bad_values_are_refused(option, value):
    op = _handle()
    try:
        with pytest.raises(query_amd.N1kError) as ei:
            op.set_option(option, value)
        assert ei.value.status == _ffi.INVALID
    finally:
        op.done()
