#!/usr/bin/env python3
"""String functions in a condition on the GPU box: what the term costs in the scan, and where the host and the device route
of its predicate cross.

  scan     config-2 columns, variants alternating round by round in one process, per variant the best and the median HIP-event
           query_ms and the spread (max - min) over the rounds:
             WHERE lower(cat) = "cat_1" AND price > 50 GROUP BY cat, SUM(price)   against   cat LIKE "cat_1" in its place
           (the same survivors, the same groups, the same row test: the expectation is "within the run-to-run spread").
  matcher  N distinct strings of 29 bytes under `lower(trim(s)) like "%_0001%z"`: n1k_strfn_eval on one thread against
           n1k_strfn_eval_device end to end (upload + kernel + results back), for 1 Ki to 16 Ki strings.
  route    the handle's own route (ensure_match_table: buffers kept): N new dictionary strings interned, then the first push
           of a one-row batch timed against a second push that brings no new string.  N below kStrFnDeviceThreshold goes
           through the host evaluator, N from it on through the kernel.

usage: exp_strfn.py [scan|matcher|route|all] [rows] [route sizes, comma separated]   — prints one JSON line per measurement."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
import query_amd  # noqa: E402
import bench  # noqa: E402
from query_amd import _ffi, plan  # noqa: E402

SIZES = (1 << 10, 1 << 11, 1 << 12, 1 << 13, 1 << 14)
TERM = '(lower(trim(%s)) like "%%_0001%%z")'


def scan(rows, kcat=1000, rounds=9):
    D = bench.D
    cols = bench.DeviceColumns(rows, kcat, False, 0, rows, 0)
    gt = "(50 < %s)" % D("price")
    variants = [
        ("like cat", "((%s like \"cat_1\") and %s)" % (D("cat"), gt)),
        ("lower(cat) =", "((lower(%s) = \"cat_1\") and %s)" % (D("cat"), gt)),
    ]
    ops = []
    for name, cond in variants:
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [D("cat")], ["sum(%s)" % D("price")]))
        op.intern(bench.synth_dictionary(kcat))
        ops.append((name, op, [cols.by_path[p] for p in op.column_paths]))
    times = {name: [] for name, _, _ in ops}
    last = {}
    for rnd in range(rounds + 2):  # two warm-up rounds (run-time compilation, allocations)
        for name, op, batch in ops:
            op.reopen()
            torch.cuda.synchronize()
            op.process_device_items(rows, batch)
            op.after_items_raw()
            st = op.stats()
            last[name] = st
            if rnd >= 2:
                times[name].append(st["query_ms"] or st["device_ms"])
    assert len({last[name]["rows_selected"] for name, _, _ in ops}) == 1, last  # the same survivors
    for name, op, _ in ops:
        t = sorted(times[name])
        print(json.dumps({"exp": "strfn_scan", "variant": name, "rows": rows, "query_ms_best": round(t[0], 4), "query_ms_median": round(t[len(t) // 2], 4),
                          "spread_ms": round(t[-1] - t[0], 4), "rows_selected": last[name]["rows_selected"], "spec_kernel": last[name]["spec_kernel"],
                          "strfn": op.strfn_stats(), "like": op.like_stats()}), flush=True)
        op.done()


def _strings(rng, n):
    return [b"item_%09d-%s" % (i, bytes(rng.integers(97, 123, 14).astype(np.uint8))) for i in range(n)]  # 29 bytes


def matcher():
    rng = np.random.default_rng(1)
    lib = _ffi.lib()
    text = (TERM % bench.D("s")).encode()
    for count in SIZES:
        strings = _strings(rng, count)
        offs = np.zeros(count + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
        blob = b"".join(strings) + b"\0"
        out_h, out_d = np.zeros(count, dtype=np.uint8), np.zeros(count, dtype=np.uint8)
        left = C.c_uint64(0)
        th = td = 1e9
        for rep in range(4):
            t0 = time.perf_counter()
            assert lib.n1k_strfn_eval(text, len(text), count, offs.ctypes.data, blob, out_h.ctypes.data) == _ffi.OK
            if rep:
                th = min(th, time.perf_counter() - t0)
            t0 = time.perf_counter()
            assert lib.n1k_strfn_eval_device(0, text, len(text), count, offs.ctypes.data, blob, out_d.ctypes.data, C.byref(left)) == _ffi.OK
            if rep:
                td = min(td, time.perf_counter() - t0)
        assert np.array_equal(out_h, out_d) and left.value == 0
        print(json.dumps({"exp": "strfn_matcher", "strings": count, "bytes_per_string": round(float(offs[-1]) / count, 1), "hits": int(out_h.sum()),
                          "host_ms": round(th * 1e3, 3), "device_ms": round(td * 1e3, 3), "note": "the device figure allocates its scratch per call"}), flush=True)


def route(sizes=None):
    D = bench.D
    rng = np.random.default_rng(2)
    probe = query_amd.GpuFilterGroup(plan.filter_group_plan(TERM % D("s"), [], ["count(*)"]))
    thr = probe.strfn_stats()["device_threshold"]
    probe.done()

    class Col:
        kind = _ffi.COL_DICT32
        codes = np.zeros(1, dtype=np.uint32)

    for n in sizes or (thr // 4, thr - 1) + SIZES + (1 << 16,):
        best_first, best_again, stats = 1e9, 1e9, None
        for rep in range(4):
            strings = _strings(rng, n)
            pj = plan.filter_group_plan(TERM % D("s"), [], ["count(*)"])
            op = query_amd.GpuFilterGroup(pj)
            op.process_items([Col], None)  # device, stream, staging buffers: not what is measured
            op.sync()
            op.intern(strings)
            t0 = time.perf_counter()
            op.process_items([Col], None)
            op.sync()
            t1 = time.perf_counter()
            op.process_items([Col], None)
            op.sync()
            t2 = time.perf_counter()
            stats = op.strfn_stats()
            op.done()
            if rep:
                best_first, best_again = min(best_first, t1 - t0), min(best_again, t2 - t1)
        print(json.dumps({"exp": "strfn_route", "new_strings": n, "route": "device" if stats["device_strings"] else "host",
                          "first_push_ms": round(best_first * 1e3, 3), "push_without_new_strings_ms": round(best_again * 1e3, 3),
                          "table_ms": round((best_first - best_again) * 1e3, 3), "strfn": stats}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    if what in ("scan", "all"):
        scan(rows)
    if what in ("matcher", "all"):
        matcher()
    if what in ("route", "all"):
        route([int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else None)
