"""ORDER BY / LIMIT over the rows of a Filter-only plan, sorted on the device, on one box in one run (bench.py's `filter`
workload: `price > 50` over the synthetic columns):

  filter        no Order: n1k_filter_device_batch as it was (the control)
  by price      ORDER BY price
  by cat,price  ORDER BY cat, price DESC
  top 100       ORDER BY price DESC LIMIT 100 (the select route), and the same with the full sort forced (topk_min_groups beyond
                the selection) — the select route exists only to be cheaper than that

    python tools/exp_order.py [rows] [repetitions]

Kernel times are n1k_stats.device_ms (the Filter kernel and everything the ordering launches), wall times are per step around
the call (the best and the median of the repetitions); `passes` are the radix passes launched (n1k_stats.order_passes), each a
per-tile histogram, a scan and a scatter over (8 B key, 4 B position) pairs."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench, query_amd
from query_amd import plan

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
D = bench.D
COND = "(50 < %s)" % D("price")
cols = bench.DeviceColumns(rows, 1000, False, 0, rows, 0)


def step(name, order=None, limit=None, **options):
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(COND, [], [], filter_only=True, order=order, limit=limit), **options)
    try:
        op.intern(bench.synth_dictionary(1000))
        batch = op.make_device_batch(rows, [cols.by_path[p] for p in op.column_paths])
        wall, dev = [], []
        for i in range(reps + 1):  # (the first repetition allocates: not reported)
            t0 = time.perf_counter()
            nsel, _ = op.filter_device_batch(batch)
            t1 = time.perf_counter()
            if i:
                wall.append((t1 - t0) * 1e3)
                dev.append(op.stats()["device_ms"])
        st = op.stats()
        head = op.selected_host32()[:5]
        print("%-22s wall best %8.3f ms  median %8.3f ms | kernels (device_ms) best %8.3f ms  median %8.3f ms | %d rows out, %d passes, %d candidates, first ordinals %s"
              % (name, min(wall), statistics.median(wall), min(dev), statistics.median(dev), nsel, st["order_passes"], st["topk_candidates"], head.tolist()))
        return min(dev), st
    finally:
        op.done()


base, _ = step("filter")
full, st = step("by price", [(D("price"), False)])
print("    per pass: %.2f GB read + %.2f GB written at %d survivors (12 B pairs in and out, 8 B keys for the tile histograms)"
      % (st["rows_selected"] * 20 / 1e9, st["rows_selected"] * 12 / 1e9, st["rows_selected"]))
step("by cat, price desc", [(D("cat"), False), (D("price"), True)])
top, _ = step("top 100 (select)", [(D("price"), True)], limit=100)
forced, _ = step("top 100 (full sort)", [(D("price"), True)], limit=100, topk_min_groups=1 << 40)
print("select route %.3f ms against the full sort's %.3f ms for LIMIT 100: %s" % (top, forced, "cheaper" if top < forced else "NOT cheaper"))
