#!/usr/bin/env python3
"""LIKE on the GPU box: what the term costs in the scan, and where the host and the device matcher cross.

  scan     config-2 columns: WHERE cat LIKE "cat_1" AND price > 50 GROUP BY cat, SUM(price) against the same plan with
           cat = "cat_1" (same columns, same survivors, same groups — asserted — so the difference is the term);
           "cat_1%" (11 % of the rows pass) and the Filter-only forms beside it.  Variants alternate, round by round;
           per variant the best HIP-event query_ms and wall step time.
  matcher  N distinct strings of about 30 bytes, three patterns: n1k_like_match on one thread against the device route
           end to end (upload + kernel + results back), strings per second each, for several block sizes: the crossover
           is what kLikeDeviceThreshold (n1k_like.h) is set from.

  route    the handle's own route (ensure_match_table: buffers kept, ONE upload and one launch for all patterns of the plan): a
           plan with three patterns, N new dictionary strings interned, then the first push of a one-row batch timed
           against a second push that brings no new string.  N just below kLikeDeviceThreshold goes through the host
           matcher, N at it through the kernel: both routes measured where they are meant to cross.

usage: exp_like.py [scan|matcher|route|all] [rows] [strings] [route sizes, comma separated]   — prints one JSON line per
measurement."""
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
from query_amd import _ffi  # noqa: E402


def scan(rows, kcat=1000, rounds=7):
    D = bench.D
    cols = bench.DeviceColumns(rows, kcat, False, 0, rows, 0)
    gt = "(50 < %s)" % D("price")
    variants = [
        ("eq  cat_1  group", "((%s = \"cat_1\") and %s)" % (D("cat"), gt), False),
        ("like cat_1  group", "((%s like \"cat_1\") and %s)" % (D("cat"), gt), False),
        ("like cat_1% group", "((%s like \"cat_1%%\") and %s)" % (D("cat"), gt), False),
        ("eq  cat_1  filter", "((%s = \"cat_1\") and %s)" % (D("cat"), gt), True),
        ("like cat_1  filter", "((%s like \"cat_1\") and %s)" % (D("cat"), gt), True),
        ("like cat_1% filter", "((%s like \"cat_1%%\") and %s)" % (D("cat"), gt), True),
    ]
    ops = []
    for name, cond, fo in variants:
        pj = query_amd.plan.filter_group_plan(cond, [] if fo else [D("cat")], [] if fo else ["sum(%s)" % D("price")], filter_only=fo)
        op = query_amd.GpuFilterGroup(pj)
        op.intern(bench.synth_dictionary(kcat))
        ops.append((name, op, [cols.by_path[p] for p in op.column_paths]))
    best = {name: [1e9, 1e9] for name, _, _ in ops}
    results = {}
    for rnd in range(rounds + 2):  # two warm-up rounds (run-time compilation, allocations)
        for name, op, batch in ops:
            op.reopen()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            op.process_device_items(rows, batch)
            r = op.after_items_raw()
            wall = (time.perf_counter() - t0) * 1e3
            st = op.stats()
            results[name] = (r, st)
            if rnd >= 2:
                best[name][0] = min(best[name][0], st["query_ms"] or st["device_ms"])
                best[name][1] = min(best[name][1], wall)
    # same survivors, same groups: the difference is the term
    for a, b in (("eq  cat_1  group", "like cat_1  group"), ("eq  cat_1  filter", "like cat_1  filter")):
        ra, rb = results[a][0], results[b][0]
        assert results[a][1]["rows_selected"] == results[b][1]["rows_selected"], (a, b)
        assert ra["ngroups"] == rb["ngroups"] and np.array_equal(ra["selected"], rb["selected"]), (a, b)
        if ra["ngroups"]:
            oa, ob = np.argsort(ra["keys"]["v"][:, 0]), np.argsort(rb["keys"]["v"][:, 0])
            assert np.array_equal(ra["keys"]["v"][oa], rb["keys"]["v"][ob]) and np.array_equal(ra["aggs"]["tag"][oa], rb["aggs"]["tag"][ob]), (a, b)
            va, vb, tg = ra["aggs"]["v"][oa], rb["aggs"]["v"][ob], ra["aggs"]["tag"][oa]
            flt = tg == 5  # T_FLOAT: a SUM of floats is the same sum in another order of additions (the project's 1e-9 relative)
            assert np.array_equal(va[~flt], vb[~flt]), (a, b)
            fa, fb = va[flt].view(np.float64), vb[flt].view(np.float64)
            rel = float(np.max(np.abs(fa - fb) / np.maximum(np.abs(fa), 1e-300))) if fa.size else 0.0
            assert rel <= 1e-9, (a, b, rel, fa[:4], fb[:4])
    for name, op, _ in ops:
        st = results[name][1]
        print(json.dumps({"exp": "like_scan", "variant": name, "rows": rows, "query_ms": round(best[name][0], 4), "wall_ms": round(best[name][1], 4),
                          "rows_selected": st["rows_selected"], "spec_kernel": st["spec_kernel"], "like": op.like_stats()}), flush=True)
        op.done()


def matcher(n):
    rng = np.random.default_rng(1)
    lib = _ffi.lib()
    patterns = [b"%1_3%", b"item\\_0%7", b"%-b_x%"]
    for count in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, n):
        count = min(count, n)
        strings = [b"item_%09d-%s" % (i, bytes(rng.integers(97, 123, 14).astype(np.uint8))) for i in range(count)]
        offs = np.zeros(count + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
        blob = b"".join(strings) + b"\0"
        out_h = np.zeros(count, dtype=np.uint8)
        out_d = np.zeros(count, dtype=np.uint8)
        left = C.c_uint64(0)
        th = td = 1e9
        for rep in range(4):
            t0 = time.perf_counter()
            for p in patterns:
                assert lib.n1k_like_match(p, len(p), count, offs.ctypes.data, blob, out_h.ctypes.data) == _ffi.OK
            if rep:
                th = min(th, time.perf_counter() - t0)
            t0 = time.perf_counter()
            for p in patterns:
                assert lib.n1k_like_match_device(0, p, len(p), count, offs.ctypes.data, blob, out_d.ctypes.data, C.byref(left)) == _ffi.OK
            if rep:
                td = min(td, time.perf_counter() - t0)
        assert np.array_equal(out_h, out_d) and left.value == 0
        print(json.dumps({"exp": "like_matcher", "strings": count, "bytes_per_string": round(float(offs[-1]) / count, 1), "patterns": len(patterns),
                          "host_1thread_Mstr_s": round(count / th / 1e6, 2), "device_route_Mstr_s": round(count / td / 1e6, 2),
                          "host_ms": round(th * 1e3, 3), "device_ms": round(td * 1e3, 3)}), flush=True)
        if count == n:
            break


def route(sizes=None):
    D = bench.D
    cond = "((%s like \"%%1_3%%\") or (%s like \"item\\\\_0%%7\") or (%s like \"%%-b_x%%\"))" % (D("s"), D("s"), D("s"))
    pj = query_amd.plan.filter_group_plan(cond, [], ["count(*)"])
    probe = query_amd.GpuFilterGroup(pj)
    thr = probe.like_stats()["device_threshold"]
    probe.done()
    rng = np.random.default_rng(2)

    class Col:
        kind = _ffi.COL_DICT32
        codes = np.zeros(1, dtype=np.uint32)

    for n in sizes or (thr // 4, thr // 2, thr - 1, thr, 2 * thr, 4 * thr, 16 * thr):
        best_first, best_again, stats = 1e9, 1e9, None
        for rep in range(5):
            strings = [b"item_%09d-%s" % (i, bytes(rng.integers(97, 123, 14).astype(np.uint8))) for i in range(n)]
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
            stats = op.like_stats()
            op.done()
            if rep:
                best_first, best_again = min(best_first, t1 - t0), min(best_again, t2 - t1)
        print(json.dumps({"exp": "like_route", "new_strings": n, "route": "device" if stats["device_strings"] else "host",
                          "first_push_ms": round(best_first * 1e3, 3), "push_without_new_strings_ms": round(best_again * 1e3, 3),
                          "table_ms": round((best_first - best_again) * 1e3, 3), "like": stats}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    nstr = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    if what in ("scan", "all"):
        scan(rows)
    if what in ("matcher", "all"):
        matcher(nstr)
    if what in ("route", "all"):
        route([int(x) for x in sys.argv[4].split(",")] if len(sys.argv) > 4 else None)
