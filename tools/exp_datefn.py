#!/usr/bin/env python3
"""The date functions on the GPU box: what datefn_kernel costs beside arith_kernel, what a query that buckets time costs fused
and materialised, where the host and the device route of the date strings' value table cross, and what their per-row lookup
costs beside the array functions'.

  query   config-2 columns plus `ts`, a TAGGED64 column of INT millis (one a second over 100 days from 2016-05-15):
          SELECT SUM(price) GROUP BY date_trunc_millis(ts, "day"), the node fused into the run-time-built scan and materialised
          (fuse_arith = 0: datefn_kernel<date_trunc>, then the scan over its derived column), SUM(price) GROUP BY
          date_part_millis(ts, "day_of_year") materialised, SELECT cat, SUM(date_part_millis(ts, "day_of_year")) GROUP BY cat
          fused and materialised, against SELECT cat, SUM(price * 1) GROUP BY cat with the node materialised (arith_kernel).  The three element-wise kernels read 9 B and write 9 B per row.  Their own times come
          from a kernel trace of this experiment, in a run of its own:
              rocprofv3 --kernel-trace --stats -- python tools/exp_datefn.py query
  route   the table build's two routes for N = 1 Ki, 4 Ki, 64 Ki, 1 Mi new date strings of 24 bytes, str_to_millis and
          date_part_str(s, "iso_week"): the host evaluator against upload + datestr_table_kernel + results back, through
          n1k_datefn_eval / n1k_datefn_eval_device — the driver ensure_datestr_table runs; best of three timed repetitions, the
          two terms added up.
  lookup  `day`, a DICT32 column of date strings (one per category), and `tags`, a TAGGED64 column of arrays (likewise):
          SELECT cat, SUM(date_part_str(day, "day")) GROUP BY cat (datestr_lookup_kernel) against
          SELECT cat, SUM(array_length(tags)) GROUP BY cat (arrfn_lookup_kernel).
The regression check of the prebuilt kernels is not a mode of this tool: it is bench.py itself (config 2, --steps 20 --warmup 3)
run alternately with this tree's library and with the parent commit's, loaded through N1K_LIB; DESIGN.md records both series.

usage: exp_datefn.py [query|route|lookup|all] [rows] [route sizes, comma separated]   — prints one JSON line per measurement."""
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

T_INT, T_STRING, T_ARRAY = 4, 6, 7
BASE_MS = 1463284740000  # 2016-05-15T03:59:00Z


def make_dates(count):
    """count DISTINCT 24-byte date strings: entry i is i minutes after 1971-01-01T00:00Z, its milliseconds i % 1000 (years of
    365 days and months of 28: every one a real date)"""
    out = []
    for i in range(count):
        d, rem = divmod(i, 1440)
        y, doy = 1971 + d // 336, d % 336
        out.append(b"%04d-%02d-%02dT%02d:%02d:00.%03dZ" % (y, 1 + doy // 28, 1 + doy % 28, rem // 60, rem % 60, i % 1000))
    assert len(set(out)) == count
    return out


def route(sizes=None):
    lib = _ffi.lib()
    terms = [b"str_to_millis((`d`.`s`))", b"date_part_str((`d`.`s`), \"iso_week\")"]
    for n in sizes or (1 << 10, 1 << 12, 1 << 16, 1 << 20):
        dates = make_dates(n)
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in dates], dtype=np.uint64)
        blob = b"".join(dates) + b"\0"
        tags, pay = np.full(n, T_STRING, np.uint8), np.zeros(n, np.uint64)
        th = td = 0.0
        anyr, left = C.c_uint32(0), C.c_uint64(0)
        for term in terms:
            ht, hp, hr = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint8)
            dt, dp, dr = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint8)
            bh = bd = 1e9
            for rep in range(4):
                t0 = time.perf_counter()
                assert lib.n1k_datefn_eval(term, len(term), n, tags.ctypes.data, pay.ctypes.data, offs.ctypes.data, blob, ht.ctypes.data,
                                           hp.ctypes.data, hr.ctypes.data) == _ffi.OK
                t1 = time.perf_counter()
                assert lib.n1k_datefn_eval_device(0, term, len(term), n, tags.ctypes.data, pay.ctypes.data, offs.ctypes.data, blob, dt.ctypes.data,
                                                  dp.ctypes.data, dr.ctypes.data, C.byref(anyr), C.byref(left)) == _ffi.OK
                t2 = time.perf_counter()
                if rep:
                    bh, bd = min(bh, t1 - t0), min(bd, t2 - t1)
            assert np.array_equal(ht, dt) and np.array_equal(hp, dp) and left.value == 0 and anyr.value == 0 and (ht == T_INT).all()
            th, td = th + bh, td + bd
        print(json.dumps({"exp": "datefn_route", "new_entries": n, "bytes_per_string": round(float(offs[-1]) / n, 1), "terms": len(terms),
                          "host_ms": round(th * 1e3, 3), "device_ms": round(td * 1e3, 3)}), flush=True)


def table(rows, kcat):
    D = bench.D
    cols = bench.DeviceColumns(rows, kcat, False, 0, rows, 0)
    words = bench.synth_dictionary(kcat)
    days = make_dates(kcat)
    arrays = [b'["t%s","x"]' % w[3:] for w in words]
    dev = cols.cat.device
    ts_t = torch.full((rows,), T_INT, dtype=torch.uint8, device=dev)
    ts_p = BASE_MS + (torch.arange(rows, dtype=torch.int64, device=dev) % (100 * 86400)) * 1000
    day = cols.cat + len(words)  # DICT32 codes of the date strings
    tags_t = torch.full((rows,), T_ARRAY, dtype=torch.uint8, device=dev)
    tags_p = cols.cat.to(torch.int64) + 2 * len(words)
    by_path = dict(cols.by_path)
    by_path[D("ts")] = (_ffi.COL_TAGGED64, ts_t.data_ptr(), ts_p.data_ptr(), None)
    by_path[D("day")] = (_ffi.COL_DICT32, None, None, day.data_ptr())
    by_path[D("tags")] = (_ffi.COL_TAGGED64, tags_t.data_ptr(), tags_p.data_ptr(), None)
    return by_path, words + days + arrays, (ts_t, ts_p, day, tags_t, tags_p, cols)


def run_variants(exp, rows, variants, kcat=1000, rounds=7):
    by_path, dictionary, keep = table(rows, kcat)
    ops = []
    for name, cond, keys, aggs, opts in variants:
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs), **opts)
        op.intern(dictionary)
        ops.append((name, op, [by_path[p] for p in op.column_paths]))
    times = {name: [] for name, _, _ in ops}
    last = {}
    for rnd in range(rounds + 2):  # two warm-up rounds (run-time compilation, allocations, the value table)
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
        print(json.dumps({"exp": exp, "variant": name, "rows": rows, "query_ms_best": round(t[0], 4), "query_ms_median": round(t[len(t) // 2], 4),
                          "spread_ms": round(t[-1] - t[0], 4), "rows_selected": last[name]["rows_selected"], "spec_kernel": last[name]["spec_kernel"],
                          "datefn": op.datefn_stats()}), flush=True)
        op.done()
    del keep


def query(rows):
    D = bench.D
    price = ["sum(%s)" % D("price")]
    trunc = plan.date_fn("date_trunc_millis", D("ts"), plan.date_part("day"))
    part = plan.date_fn("date_part_millis", D("ts"), plan.date_part("day_of_year"))
    run_variants("datefn_query", rows, [
        ("sum(price * 1) by cat, arith_kernel", None, [D("cat")], ["sum((%s * 1))" % D("price")], {"fuse_arith": 0}),
        ("sum(price) by date_trunc_millis(ts, day), datefn_kernel", None, [trunc], price, {"fuse_arith": 0}),
        ("sum(price) by date_trunc_millis(ts, day), fused", None, [trunc], price, {"jit": 2}),
        ("sum(price) by date_part_millis(ts, doy), datefn_kernel", None, [part], price, {"fuse_arith": 0}),
        ("sum(date_part_millis(ts, doy)) by cat, datefn_kernel", None, [D("cat")], ["sum(%s)" % part], {"fuse_arith": 0}),
        ("sum(date_part_millis(ts, doy)) by cat, fused", None, [D("cat")], ["sum(%s)" % part], {"jit": 2}),
    ])


def lookup(rows):
    D = bench.D
    cat = [D("cat")]
    run_variants("datefn_lookup", rows, [
        ("sum(array_length(tags)), arrfn_lookup_kernel", None, cat, ["sum(array_length(%s))" % D("tags")], {}),
        ("sum(date_part_str(day, day)), datestr_lookup_kernel", None, cat, ["sum(%s)" % plan.date_fn("date_part_str", D("day"), plan.date_part("day"))], {}),
    ])


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    sizes = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else None
    if what in ("route", "all"):
        route(sizes)
    if what in ("query", "all"):
        query(rows)
    if what in ("lookup", "all"):
        lookup(rows)
