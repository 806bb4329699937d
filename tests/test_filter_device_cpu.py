"""Filter-only plans on the device, the part that needs no GPU: the three entry points exist, and every argument and plan
check of n1k_filter_device_batch / n1k_selected_to_host32 / n1k_gather_selected answers before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import query_amd
from query_amd import _ffi, plan

D = lambda *n: plan.field_path("default", *n)
COND = "(50 < %s)" % D("price")
NEW = ["n1k_filter_device_batch", "n1k_selected_to_host32", "n1k_gather_selected"]


def _filter_op():
    return query_amd.GpuFilterGroup(plan.filter_group_plan(COND, [], [], filter_only=True))


def _host_batch(op, n):
    """A batch that validates (one TAGGED64 column of n rows).  The arrays are host memory: only calls that stop at their
    checks, or at the missing device, may be given it."""
    tags = np.full(max(n, 1), _ffi.T_INT, dtype=np.uint8)
    pay = np.arange(max(n, 1), dtype=np.uint64)
    b = op.make_device_batch(n, [(_ffi.COL_TAGGED64, tags.ctypes.data, pay.ctypes.data, None)])
    return b, (tags, pay)


def test_symbols_resolve():
    L = _ffi.lib()
    for s in NEW:
        assert s in _ffi.SYMBOLS
        assert hasattr(L, s), "libn1k.so does not export " + s
    assert L.n1k_abi_version() == 3  # new entry points only


def test_plan_with_a_group_is_invalid():
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(COND, [D("cat")], ["count(*)"]))
    tags = np.zeros(4, np.uint8)
    pay = np.zeros(4, np.uint64)
    codes = np.zeros(4, np.uint32)
    b = op.make_device_batch(4, [(_ffi.COL_TAGGED64, tags.ctypes.data, pay.ctypes.data, None),
                                 (_ffi.COL_DICT32, None, None, codes.ctypes.data)])
    with pytest.raises(query_amd.N1kError) as ei:
        op.filter_device_batch(b)
    assert ei.value.status == _ffi.INVALID and "group" in ei.value.message
    op.done()


def test_null_arguments_are_invalid():
    op = _filter_op()
    L = _ffi.lib()
    sel = _ffi.Selection()
    assert L.n1k_filter_device_batch(op._h, None, C.byref(sel)) == _ffi.INVALID
    assert b"batch" in L.n1k_last_error(op._h)
    b, keep = _host_batch(op, 4)
    assert L.n1k_filter_device_batch(op._h, C.byref(b[0]), None) == _ffi.INVALID
    assert L.n1k_filter_device_batch(None, C.byref(b[0]), C.byref(sel)) == _ffi.INVALID
    op.done()


def test_four_giga_rows_are_invalid():
    op = _filter_op()
    b, keep = _host_batch(op, 4)
    b[0].nrows = 1 << 32  # (refused on the count alone: no row is read)
    with pytest.raises(query_amd.N1kError) as ei:
        op.filter_device_batch(b)
    assert ei.value.status == _ffi.INVALID and "2^32" in ei.value.message
    op.done()


def test_batch_that_does_not_validate_is_invalid():
    op = _filter_op()
    b = op.make_device_batch(4, [(_ffi.COL_TAGGED64, None, None, None)])
    with pytest.raises(query_amd.N1kError) as ei:
        op.filter_device_batch(b)
    assert ei.value.status == _ffi.INVALID
    b2 = op.make_device_batch(4, [])  # the plan names one column
    with pytest.raises(query_amd.N1kError) as ei:
        op.filter_device_batch(b2)
    assert ei.value.status == _ffi.INVALID
    op.done()


def test_fresh_handle_has_no_selection():
    op = _filter_op()
    out = np.zeros(8, np.uint32)
    with pytest.raises(query_amd.N1kError) as ei:
        op.selected_host32(out)
    assert ei.value.status == _ffi.INVALID and "selection" in ei.value.message
    b, keep = _host_batch(op, 4)
    with pytest.raises(query_amd.N1kError) as ei:
        op.gather_selected(b, 4, [(_ffi.COL_TAGGED64, keep[0].ctypes.data, keep[1].ctypes.data, None)])
    assert ei.value.status == _ffi.INVALID and "selection" in ei.value.message
    op.done()


def test_stop_is_observed_before_the_device():
    op = _filter_op()
    b, keep = _host_batch(op, 4)
    op.send_stop()
    with pytest.raises(query_amd.N1kError) as ei:
        op.filter_device_batch(b)
    assert ei.value.status == _ffi.STOPPED
    op.done()


def test_no_cpu_fallback_without_device():
    if query_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    op = _filter_op()
    b, keep = _host_batch(op, 4)
    with pytest.raises(query_amd.N1kError) as ei:
        op.filter_device_batch(b)
    assert ei.value.status == _ffi.DEVICE_ERROR
    with pytest.raises(query_amd.N1kError) as ei:  # and it left no selection behind
        op.selected_host32(np.zeros(4, np.uint32))
    assert ei.value.status == _ffi.INVALID
    op.done()
