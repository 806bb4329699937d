#!/usr/bin/env python3
"""ANY / EVERY on the GPU box: what the term costs in the scan, and where the host and the device evaluator cross.

  scan       config-2 columns plus `tags`, a TAGGED64 column of arrays (one distinct array per category, ["t_<i>", "x"]):
             WHERE ANY g IN tags SATISFIES g = "t_1" END AND price > 50 GROUP BY cat, SUM(price) against the same plan with
             cat = "cat_1" over the DICT32 column (the baseline: same survivors, same groups — asserted) and with
             cats = "cat_1" over a TAGGED64 string column (the same 9 B/row the array column costs, so that the bytes and
             the term can be told apart).  Variants alternate, round by round; per variant the best HIP-event query_ms and
             wall step time, and the spread of the baseline over the rounds.
  evaluator  N distinct arrays of about 30 bytes, one term: n1k_coll_eval on one thread against the device route end to
             end (upload + kernel + results back), arrays per second each, for several block sizes.
  route      the handle's own route (ensure_match_table): a plan with two collection predicates, N new dictionary entries interned,
             then the first push of a one-row batch timed against a second push that brings no new entry.
  mixed      route, with exp_like.py's three LIKE patterns over a string column in the same Filter: both kinds of term
             evaluated for every new entry, one table.

usage: exp_coll.py [scan|evaluator|route|mixed|all] [rows] [arrays] [route sizes, comma separated]   — prints one JSON line per
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

T_STRING, T_ARRAY = 6, 7


def scan(rows, kcat=1000, rounds=7):
    D = bench.D
    cols = bench.DeviceColumns(rows, kcat, False, 0, rows, 0)
    words = bench.synth_dictionary(kcat)
    arrays = [b'["t%s","x"]' % w[3:] for w in words]  # entry i of the arrays belongs to category i: "cat_1" -> ["t_1","x"]
    dictionary = words + arrays
    tags_t = torch.full((rows,), T_ARRAY, dtype=torch.uint8, device=cols.cat.device)
    tags_p = cols.cat.to(torch.int64) + len(words)
    cats_t = torch.full((rows,), T_STRING, dtype=torch.uint8, device=cols.cat.device)
    cats_p = cols.cat.to(torch.int64)
    by_path = dict(cols.by_path)
    by_path[D("tags")] = (_ffi.COL_TAGGED64, tags_t.data_ptr(), tags_p.data_ptr(), None)
    by_path[D("cats")] = (_ffi.COL_TAGGED64, cats_t.data_ptr(), cats_p.data_ptr(), None)
    gt = "(50 < %s)" % D("price")
    any_t1 = "any `g` in %s satisfies (`g` = \"t_1\") end" % D("tags")
    any_t1x = "any `g` in %s satisfies (`g` like \"t\\\\_1%%\") end" % D("tags")
    variants = [
        ("eq  dict32   group", "((%s = \"cat_1\") and %s)" % (D("cat"), gt), False),
        ("eq  tagged64 group", "((%s = \"cat_1\") and %s)" % (D("cats"), gt), False),
        ("any t_1      group", "(%s and %s)" % (any_t1, gt), False),
        ("any t_1%     group", "(%s and %s)" % (any_t1x, gt), False),
        ("eq  dict32   filter", "((%s = \"cat_1\") and %s)" % (D("cat"), gt), True),
        ("any t_1      filter", "(%s and %s)" % (any_t1, gt), True),
    ]
    ops = []
    for name, cond, fo in variants:
        pj = query_amd.plan.filter_group_plan(cond, [] if fo else [D("cat")], [] if fo else ["sum(%s)" % D("price")], filter_only=fo)
        op = query_amd.GpuFilterGroup(pj)
        op.intern(dictionary)
        ops.append((name, op, [by_path[p] for p in op.column_paths]))
    times = {name: [] for name, _, _ in ops}
    walls = {name: [] for name, _, _ in ops}
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
                times[name].append(st["query_ms"] or st["device_ms"])
                walls[name].append(wall)
    # same survivors, same groups: the difference is the term (and the bytes of its column)
    for a, b in (("eq  dict32   group", "any t_1      group"), ("eq  dict32   group", "eq  tagged64 group"), ("eq  dict32   filter", "any t_1      filter")):
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
            assert rel <= 1e-9, (a, b, rel)
    for name, op, _ in ops:
        st = results[name][1]
        q = sorted(times[name])
        print(json.dumps({"exp": "coll_scan", "variant": name, "rows": rows, "query_ms": round(q[0], 4), "query_ms_median": round(q[len(q) // 2], 4),
                          "query_ms_max": round(q[-1], 4), "wall_ms": round(min(walls[name]), 4), "rows_selected": st["rows_selected"],
                          "spec_kernel": st["spec_kernel"], "coll": op.coll_stats()}), flush=True)
        op.done()


def make_arrays(count, rng):
    letters = rng.integers(97, 123, (count, 6)).astype(np.uint8)
    return [b'["t_%d","%s",%d]' % (i % 1000, bytes(letters[i]), i) for i in range(count)]


def evaluator(n):
    rng = np.random.default_rng(1)
    lib = _ffi.lib()
    term = b'any `g` in (`d`.`tags`) satisfies ((`g` = "t_1") or (`g` like "%zz%")) end'
    for count in (1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 20, n):
        count = min(count, n)
        arrays = make_arrays(count, rng)
        offs = np.zeros(count + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in arrays], dtype=np.uint64)
        blob = b"".join(arrays) + b"\0"
        out_h = np.zeros(count, dtype=np.uint8)
        out_d = np.zeros(count, dtype=np.uint8)
        left = C.c_uint64(0)
        th = td = 1e9
        for rep in range(3):
            t0 = time.perf_counter()
            assert lib.n1k_coll_eval(term, len(term), count, offs.ctypes.data, blob, out_h.ctypes.data) == _ffi.OK
            if rep:
                th = min(th, time.perf_counter() - t0)
            t0 = time.perf_counter()
            assert lib.n1k_coll_eval_device(0, term, len(term), count, offs.ctypes.data, blob, out_d.ctypes.data, C.byref(left)) == _ffi.OK
            if rep:
                td = min(td, time.perf_counter() - t0)
        assert np.array_equal(out_h, out_d) and left.value == 0 and 0 < int(out_h.sum()) < count
        print(json.dumps({"exp": "coll_evaluator", "arrays": count, "bytes_per_array": round(float(offs[-1]) / count, 1),
                          "host_1thread_Marr_s": round(count / th / 1e6, 2), "device_route_Marr_s": round(count / td / 1e6, 2),
                          "host_ms": round(th * 1e3, 3), "device_ms": round(td * 1e3, 3)}), flush=True)
        if count == n:
            break


def route(sizes=None, mixed=False):
    D = bench.D
    cond = "(any `g` in %s satisfies (`g` = \"t_1\") end or every `g` in %s satisfies (`g` like \"%%zz%%\") end)" % (D("a"), D("a"))
    if mixed:
        cond = "(%s or (%s like \"%%1_3%%\") or (%s like \"item\\\\_0%%7\") or (%s like \"%%-b_x%%\"))" % (cond, D("s"), D("s"), D("s"))
    pj = query_amd.plan.filter_group_plan(cond, [], ["count(*)"])
    probe = query_amd.GpuFilterGroup(pj)
    thr = probe.coll_stats()["device_threshold"]
    probe.done()
    rng = np.random.default_rng(2)

    class Col:
        kind = _ffi.COL_TAGGED64
        tags = np.full(1, T_ARRAY, dtype=np.uint8)
        payload = np.zeros(1, dtype=np.uint64)

    class StrCol:
        kind = _ffi.COL_DICT32
        codes = np.zeros(1, dtype=np.uint32)

    by_path = {D("a"): Col, D("s"): StrCol}
    for n in sizes or (thr // 4, thr // 2, thr - 1, thr, 2 * thr, 4 * thr, 16 * thr):
        best_first, best_again, stats = 1e9, 1e9, None
        for rep in range(4):
            arrays = make_arrays(n, rng)
            op = query_amd.GpuFilterGroup(pj)
            cols = [by_path[p] for p in op.column_paths]
            op.intern([b"[]"])
            op.process_items(cols, None)  # device, stream, staging buffers: not what is measured
            op.sync()
            op.intern(arrays)
            t0 = time.perf_counter()
            op.process_items(cols, None)
            op.sync()
            t1 = time.perf_counter()
            op.process_items(cols, None)
            op.sync()
            t2 = time.perf_counter()
            stats, like = op.coll_stats(), op.like_stats()
            op.done()
            if rep:
                best_first, best_again = min(best_first, t1 - t0), min(best_again, t2 - t1)
        print(json.dumps({"exp": "coll_route_mixed" if mixed else "coll_route", "new_entries": n, "route": "device" if stats["device_arrays"] else "host",
                          "first_push_ms": round(best_first * 1e3, 3), "push_without_new_entries_ms": round(best_again * 1e3, 3),
                          "table_ms": round((best_first - best_again) * 1e3, 3), "coll": stats, **({"like": like} if mixed else {})}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    narr = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    if what in ("scan", "all"):
        scan(rows)
    if what in ("evaluator", "all"):
        evaluator(narr)
    sizes = [int(x) for x in sys.argv[4].split(",")] if len(sys.argv) > 4 else None
    if what in ("route", "all"):
        route(sizes)
    if what in ("mixed", "all"):
        route(sizes, mixed=True)
