#!/usr/bin/env python3
"""The numeric library functions on the GPU box: what a library function costs beside an arithmetic node, materialised and
fused.

Seven plans over the bench table (bench.DeviceColumns), alternating round by round in one process; per plan the best and the
median HIP-event query_ms and the spread (max - min) over 7 measured rounds behind 2 warm-up rounds:

  a   SELECT cat, SUM(price * 1) GROUP BY cat, fuse_arith = 0          (one arith_kernel launch per batch: the yardstick)
  em  SELECT cat, SUM(exp(price / 100)) GROUP BY cat, fuse_arith = 0   (arith_kernel + mathfn_kernel<exp>)
  ef  the same, jit = 2                                                (both nodes in the scan's registers)
  pm  SELECT cat, SUM(power(price, 2)) GROUP BY cat, fuse_arith = 0    (mathfn_kernel<power>)
  pf  the same, jit = 2
  sm  SELECT cat, SUM(price) WHERE sin(price) > 0 GROUP BY cat, fuse_arith = 0   (mathfn_kernel<sin>)
  sf  the same, jit = 2

A materialised node reads its operand column (9 B per row) and writes a derived TAGGED64 column (9 B per row), which the scan
then reads: 18 B per row of traffic beside the plan without the node.  The kernels' own times — mathfn_kernel<...> against
arith_kernel for those same 18 B per row — come from a kernel trace of this script, in a run of its own:

    rocprofv3 --kernel-trace --stats -- python tools/exp_mathfn.py 100000000 a,em,pm,sm

usage: exp_mathfn.py [rows] [variants, comma separated]   — prints one JSON line per plan; spec_kernel 3 says that the nodes
were fused."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401
import query_amd  # noqa: E402
import bench  # noqa: E402
from query_amd import plan  # noqa: E402

ORDER = ["a", "em", "ef", "pm", "pf", "sm", "sf"]


def variants():
    D = bench.D
    price, cat = D("price"), [D("cat")]
    exp = "sum(%s)" % plan.num_fn("exp", "(%s / 100)" % price)
    power = "sum(%s)" % plan.num_fn("power", price, "2")
    sin = "(0 < %s)" % plan.num_fn("sin", price)
    mat, fus = {"fuse_arith": 0}, {"jit": 2}
    return {
        "a": ("sum(price * 1), derived column", None, cat, ["sum((%s * 1))" % price], mat),
        "em": ("sum(exp(price / 100)), derived columns", None, cat, [exp], mat),
        "ef": ("sum(exp(price / 100)), fused", None, cat, [exp], fus),
        "pm": ("sum(power(price, 2)), derived column", None, cat, [power], mat),
        "pf": ("sum(power(price, 2)), fused", None, cat, [power], fus),
        "sm": ("where sin(price) > 0, derived column", sin, cat, ["sum(%s)" % price], mat),
        "sf": ("where sin(price) > 0, fused", sin, cat, ["sum(%s)" % price], fus),
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
        print(json.dumps({"exp": "mathfn_scan", "variant": v, "plan": name, "rows": rows, "query_ms_best": round(t[0], 4),
                          "query_ms_median": round(t[len(t) // 2], 4), "spread_ms": round(t[-1] - t[0], 4),
                          "rows_selected": last[v]["rows_selected"], "spec_kernel": last[v]["spec_kernel"]}), flush=True)
        op.done()


if __name__ == "__main__":
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    scan(rows, sys.argv[2].split(",") if len(sys.argv) > 2 else ORDER)
