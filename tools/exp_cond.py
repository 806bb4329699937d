#!/usr/bin/env python3
"""CASE and the conditional functions on the GPU box: what a conditional node costs beside an arithmetic node.

Four plans over the bench table (bench.DeviceColumns), alternating round by round in one process; per plan the best and the
median HIP-event query_ms and the spread (max - min) over 7 measured rounds behind 2 warm-up rounds:

  a  config 2 as it stands:  SELECT cat, SUM(price) WHERE price > 50 GROUP BY cat
  b  SELECT cat, SUM(CASE WHEN price > 50 THEN price ELSE 0 END) GROUP BY cat          (one cond_kernel launch per batch)
  c  SELECT cat, SUM(IFMISSING(price, 0)) GROUP BY cat                                 (idem)
  d  SELECT cat, SUM(price * 1) GROUP BY cat with fuse_arith = 0                       (one arith_kernel launch per batch)

b, c and d read the operand column once more than a (9 B per row) and write a derived TAGGED64 column (9 B per row), which
the scan then reads in the operand's place: the yardstick for cond_kernel is arith_kernel in d.  The kernels' own times come
from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/exp_cond.py 100000000 b,d), in a run of
its own.

usage: exp_cond.py [rows] [variants, comma separated: a,b,c,d]   — prints one JSON line per plan."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401
import query_amd  # noqa: E402
import bench  # noqa: E402
from query_amd import plan  # noqa: E402


def variants():
    D = bench.D
    price, cat = D("price"), [D("cat")]
    gt = "(50 < %s)" % price
    return {
        "a": ("config2", gt, cat, ["sum(%s)" % price], {}),
        "b": ("sum(case when price > 50 then price else 0 end)", None, cat, ["sum(%s)" % plan.case_when([(gt, price)], "0")], {}),
        "c": ("sum(ifmissing(price, 0))", None, cat, ["sum(%s)" % plan.cond_fn("ifmissing", price, "0")], {}),
        "d": ("sum(price * 1), derived column", None, cat, ["sum((%s * 1))" % price], {"fuse_arith": 0}),
    }


def scan(rows, which, kcat=1000, rounds=7):
    cols = bench.DeviceColumns(rows, kcat, False, 0, rows, 0)
    ops = []
    for v in which:
        name, cond, keys, aggs, opts = variants()[v]
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs), **opts)
        op.intern(bench.synth_dictionary(kcat))
        ops.append((v, name, op, [cols.by_path[p] for p in op.column_paths]))
    times = {v: [] for v, _, _, _ in ops}
    last = {}
    for rnd in range(rounds + 2):  # two warm-up rounds (run-time compilation, allocations)
        for v, name, op, batch in ops:
            op.reopen()
            torch.cuda.synchronize()
            op.process_device_items(rows, batch)
            op.after_items_raw()
            st = op.stats()
            last[v] = st
            if rnd >= 2:
                times[v].append(st["query_ms"] or st["device_ms"])
    for v, name, op, _ in ops:
        t = sorted(times[v])
        print(json.dumps({"exp": "cond_scan", "variant": v, "plan": name, "rows": rows, "query_ms_best": round(t[0], 4),
                          "query_ms_median": round(t[len(t) // 2], 4), "spread_ms": round(t[-1] - t[0], 4),
                          "rows_selected": last[v]["rows_selected"], "spec_kernel": last[v]["spec_kernel"]}), flush=True)
        op.done()


if __name__ == "__main__":
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    scan(rows, sys.argv[2].split(",") if len(sys.argv) > 2 else ["a", "b", "c", "d"])
