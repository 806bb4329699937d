#!/usr/bin/env python3
"""IN over a constant list on the GPU box: what the term costs in the scan, and where the host and the device route of the
list's strings cross.

  scan     config-2 columns, variants alternating round by round in one process, per variant the best and the median HIP-event
           query_ms and the spread (max - min) over the rounds:
             WHERE cat IN ["cat_1", "cat_3"] AND price > 50 GROUP BY cat, SUM(price)   against   cat = "cat_1" in its place
             WHERE region_id IN [<16 ints>] AND price > 50 GROUP BY cat, SUM(price)    against   region_id = <int> in its place
           (an IN passes more rows than the `=` beside it: the rows selected are printed with the times).
  matcher  N distinct strings of 29 bytes against a list of 1000 strings, half of them present: n1k_in_match on one thread
           against n1k_in_match_device end to end (upload + kernel + results back), for 1 Ki, 4 Ki, 64 Ki and 1 Mi strings.
  route    the handle's own route (ensure_match_table: buffers kept, the list's table uploaded once): N new dictionary strings
           interned, then the first push of a one-row batch timed against a second push that brings no new string.  N just
           below kInDeviceThreshold goes through the host matcher, N from it on through the kernel.

usage: exp_in.py [scan|matcher|route|all] [rows] [route sizes, comma separated]   — prints one JSON line per measurement."""
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

SIZES = (1 << 10, 1 << 12, 1 << 16, 1 << 20)


def scan(rows, kcat=1000, rounds=9):
    D = bench.D
    cols = bench.DeviceColumns(rows, kcat, False, 0, rows, 0)
    gt = "(50 < %s)" % D("price")
    regions = list(range(3, 3 + 32, 2))  # 16 ints
    variants = [
        ("eq cat", "((%s = \"cat_1\") and %s)" % (D("cat"), gt)),
        ("in cat x2", "(%s and %s)" % (plan.in_list(D("cat"), ["cat_1", "cat_3"]), gt)),
        ("eq region_id", "((%s = 3) and %s)" % (D("region_id"), gt)),
        ("in region_id x16", "(%s and %s)" % (plan.in_list(D("region_id"), regions), gt)),
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
    for name, op, _ in ops:
        t = sorted(times[name])
        print(json.dumps({"exp": "in_scan", "variant": name, "rows": rows, "query_ms_best": round(t[0], 4), "query_ms_median": round(t[len(t) // 2], 4),
                          "spread_ms": round(t[-1] - t[0], 4), "rows_selected": last[name]["rows_selected"], "spec_kernel": last[name]["spec_kernel"],
                          "in": op.in_stats()}), flush=True)
        op.done()


def _strings(rng, n):
    return [b"item_%09d-%s" % (i, bytes(rng.integers(97, 123, 14).astype(np.uint8))) for i in range(n)]  # 29 bytes


def _list_of(strings, k=1000):
    step = max(1, len(strings) // (k // 2))
    present = [s.decode() for s in strings[::step][:k // 2]]
    return present + ["absent_%09d-xxxxxxxxxxxxx" % i for i in range(k - len(present))]


def matcher():
    rng = np.random.default_rng(1)
    lib = _ffi.lib()
    for count in SIZES:
        strings = _strings(rng, count)
        text = ("[%s]" % ", ".join(json.dumps(s) for s in _list_of(strings))).encode()
        offs = np.zeros(count + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
        blob = b"".join(strings) + b"\0"
        out_h, out_d = np.zeros(count, dtype=np.uint8), np.zeros(count, dtype=np.uint8)
        left = C.c_uint64(0)
        th = td = 1e9
        for rep in range(4):
            t0 = time.perf_counter()
            assert lib.n1k_in_match(text, len(text), count, offs.ctypes.data, blob, out_h.ctypes.data) == _ffi.OK
            if rep:
                th = min(th, time.perf_counter() - t0)
            t0 = time.perf_counter()
            assert lib.n1k_in_match_device(0, text, len(text), count, offs.ctypes.data, blob, out_d.ctypes.data, C.byref(left)) == _ffi.OK
            if rep:
                td = min(td, time.perf_counter() - t0)
        assert np.array_equal(out_h, out_d) and left.value == 0 and 0 < int(out_h.sum()) <= 500
        print(json.dumps({"exp": "in_matcher", "strings": count, "bytes_per_string": round(float(offs[-1]) / count, 1), "list": 1000,
                          "host_ms": round(th * 1e3, 3), "device_ms": round(td * 1e3, 3), "note": "both parse the list and build its table per call"}), flush=True)


def route(sizes=None):
    D = bench.D
    rng = np.random.default_rng(2)
    probe = query_amd.GpuFilterGroup(plan.filter_group_plan(plan.in_list(D("s"), ["a"]), [], ["count(*)"]))
    thr = probe.in_stats()["device_threshold"]
    probe.done()

    class Col:
        kind = _ffi.COL_DICT32
        codes = np.zeros(1, dtype=np.uint32)

    for n in sizes or (thr // 4, thr - 1) + SIZES:
        best_first, best_again, stats = 1e9, 1e9, None
        for rep in range(4):
            strings = _strings(rng, n)
            pj = plan.filter_group_plan(plan.in_list(D("s"), _list_of(strings)), [], ["count(*)"])
            op = query_amd.GpuFilterGroup(pj)
            op.process_items([Col], None)  # device, stream, staging buffers, the list's table: not what is measured
            op.sync()
            op.intern(strings)
            t0 = time.perf_counter()
            op.process_items([Col], None)
            op.sync()
            t1 = time.perf_counter()
            op.process_items([Col], None)
            op.sync()
            t2 = time.perf_counter()
            stats = op.in_stats()
            op.done()
            if rep:
                best_first, best_again = min(best_first, t1 - t0), min(best_again, t2 - t1)
        print(json.dumps({"exp": "in_route", "new_strings": n, "route": "device" if stats["device_strings"] else "host",
                          "first_push_ms": round(best_first * 1e3, 3), "push_without_new_strings_ms": round(best_again * 1e3, 3),
                          "table_ms": round((best_first - best_again) * 1e3, 3), "in": stats}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    if what in ("scan", "all"):
        scan(rows)
    if what in ("matcher", "all"):
        matcher()
    if what in ("route", "all"):
        route([int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else None)
