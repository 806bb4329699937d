#!/usr/bin/env python3
"""The array functions on the GPU box: where the host and the device route of the value table cross, what the per-row
lookup costs beside an arithmetic node, and what a plan with array_length costs beside the same plan with ANY.

  route   the table build's two routes for N = 1 Ki, 4 Ki, 64 Ki, 1 Mi new arrays of about 30 bytes, array_length and array_sum:
          the host evaluator against upload + arrfn_table_kernel + results back, through n1k_arrfn_eval / n1k_arrfn_eval_device —
          the driver ensure_value_table runs (a handle takes one route per extension, by the threshold; here both are
          timed on the same block), best of three timed repetitions, the two terms added up.
  lookup  config-2 columns plus `tags`, a TAGGED64 column of arrays (one distinct array per category):
          SELECT cat, SUM(array_length(tags)) GROUP BY cat (arrfn_lookup_kernel, then the scan over its derived column) against
          SELECT cat, SUM(price * 1) GROUP BY cat with fuse_arith = 0 (arith_kernel, then the same scan).  Both nodes read 9 B
          and write 9 B per row; the lookup reads its table beside them.  The kernels' own times come from a kernel trace of
          this experiment, in a run of its own:   rocprofv3 --kernel-trace --stats -- python tools/exp_arrfn.py lookup
  scan    WHERE array_length(tags) > 1 AND price > 50 GROUP BY cat, SUM(price) against the same plan with
          ANY g IN tags SATISFIES g = "t_1" END in its place (one bit of the match table, tested inside the scan).

usage: exp_arrfn.py [route|lookup|scan|all] [rows] [route sizes, comma separated]   — prints one JSON line per measurement."""
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

T_ARRAY = 7


def make_arrays(count, rng):
    letters = rng.integers(97, 123, (count, 6)).astype(np.uint8)
    return [b'["t_%d","%s",%d]' % (i % 1000, bytes(letters[i]), i) for i in range(count)]


def route(sizes=None):
    """both routes of the ONE driver the handle's table build runs (arrfn_block), through the diagnostic entry points: the host
    evaluator over the block against upload + kernel + results back + the hand-overs"""
    lib = _ffi.lib()
    rng = np.random.default_rng(2)
    terms = [b"array_length((`d`.`a`))", b"array_sum((`d`.`a`))"]
    for n in sizes or (1 << 10, 1 << 12, 1 << 16, 1 << 20):
        arrays = make_arrays(n, rng)
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in arrays], dtype=np.uint64)
        blob = b"".join(arrays) + b"\0"
        th = td = 0.0
        left = C.c_uint64(0)
        for term in terms:
            ht, hp = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
            dt, dp = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
            bh = bd = 1e9
            for rep in range(4):
                t0 = time.perf_counter()
                assert lib.n1k_arrfn_eval(term, len(term), n, offs.ctypes.data, blob, ht.ctypes.data, hp.ctypes.data) == _ffi.OK
                t1 = time.perf_counter()
                assert lib.n1k_arrfn_eval_device(0, term, len(term), n, offs.ctypes.data, blob, dt.ctypes.data, dp.ctypes.data, C.byref(left)) == _ffi.OK
                t2 = time.perf_counter()
                if rep:
                    bh, bd = min(bh, t1 - t0), min(bd, t2 - t1)
            assert np.array_equal(ht, dt) and np.array_equal(hp, dp) and left.value == 0
            th, td = th + bh, td + bd
        print(json.dumps({"exp": "arrfn_route", "new_entries": n, "bytes_per_array": round(float(offs[-1]) / n, 1), "terms": len(terms),
                          "host_ms": round(th * 1e3, 3), "device_ms": round(td * 1e3, 3)}), flush=True)


def table_with_tags(rows, kcat):
    D = bench.D
    cols = bench.DeviceColumns(rows, kcat, False, 0, rows, 0)
    words = bench.synth_dictionary(kcat)
    arrays = [b'["t%s","x"]' % w[3:] for w in words]  # entry i of the arrays belongs to category i: "cat_1" -> ["t_1","x"]
    tags_t = torch.full((rows,), T_ARRAY, dtype=torch.uint8, device=cols.cat.device)
    tags_p = cols.cat.to(torch.int64) + len(words)
    by_path = dict(cols.by_path)
    by_path[D("tags")] = (_ffi.COL_TAGGED64, tags_t.data_ptr(), tags_p.data_ptr(), None)
    return by_path, words + arrays, (tags_t, tags_p, cols)


def run_variants(exp, rows, variants, kcat=1000, rounds=7):
    by_path, dictionary, keep = table_with_tags(rows, kcat)
    ops = []
    for name, cond, keys, aggs, opts in variants:
        op = query_amd.GpuFilterGroup(query_amd.plan.filter_group_plan(cond, keys, aggs), **opts)
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
                          "arrfn": op.arrfn_stats()}), flush=True)
        op.done()
    del keep


def lookup(rows):
    D = bench.D
    cat = [D("cat")]
    run_variants("arrfn_lookup", rows, [
        ("sum(price * 1), arith_kernel", None, cat, ["sum((%s * 1))" % D("price")], {"fuse_arith": 0}),
        ("sum(array_length(tags)), arrfn_lookup_kernel", None, cat, ["sum(array_length(%s))" % D("tags")], {}),
    ])


def scan(rows):
    D = bench.D
    cat, gt, aggs = [D("cat")], "(50 < %s)" % D("price"), ["sum(%s)" % D("price")]
    run_variants("arrfn_scan", rows, [
        ("any t_1", "(any `g` in %s satisfies (`g` = \"t_1\") end and %s)" % (D("tags"), gt), cat, aggs, {}),
        ("array_length(tags) > 1", "((1 < array_length(%s)) and %s)" % (D("tags"), gt), cat, aggs, {}),
    ])


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    sizes = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else None
    if what in ("route", "all"):
        route(sizes)
    if what in ("lookup", "all"):
        lookup(rows)
    if what in ("scan", "all"):
        scan(rows)
