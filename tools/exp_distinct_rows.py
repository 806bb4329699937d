"""SELECT DISTINCT over the rows of a Filter-only plan, de-duplicated on the device, on one box in one run (bench.py's synthetic
columns, WHERE price > 50), each with the LDS pre-filter (rowdistinct_lds_slots = 2048) and without it (0), beside two yardsticks taken
in the same run: the plain Filter-only step, and the group path over the same keys (GROUP BY <terms>, count(*) through
n1k_run_device_batch — the spelling of DISTINCT that lands its groups on the host):

  cat               DISTINCT cat              1 000 keys   (K_cat = 1 000)
  cat, region_id    DISTINCT cat, region_id   6.4 M keys   (K_cat = 100 000, the columns of config 5)
  user_id           DISTINCT user_id          10 M keys

    python tools/exp_distinct_rows.py [rows] [repetitions]

Kernel times are n1k_stats.device_ms (the Filter kernel and everything the stage launches), wall times are per step around the
one call (the best and the median of the repetitions); `reached` are the rows that went to the global table
(n1k_rowdistinct_stats)."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, query_amd
from query_amd import plan

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
D = bench.D
COND = "(50 < %s)" % D("price")


def timed(call, stats):
    wall, dev = [], []
    for i in range(reps + 1):  # (the first repetition allocates: not reported)
        t0 = time.perf_counter()
        out = call()
        t1 = time.perf_counter()
        if i:
            wall.append((t1 - t0) * 1e3)
            dev.append(stats()["device_ms"])
    return out, "wall best %8.3f ms  median %8.3f ms | kernels (device_ms) best %8.3f ms  median %8.3f ms" % (
        min(wall), statistics.median(wall), min(dev), statistics.median(dev))


def rows_step(cols, k_cat, name, terms=None, **options):
    pj = plan.filter_group_plan(COND, [], [], filter_only=True, distinct=[(t, None) for t in terms] if terms else None)
    op = query_amd.GpuFilterGroup(pj, **options)
    try:
        op.intern(bench.synth_dictionary(k_cat))
        batch = op.make_device_batch(rows, [cols.by_path[p] for p in op.column_paths])
        (nsel, _), line = timed(lambda: op.filter_device_batch(batch), op.stats)
        rd = op.rowdistinct_stats()
        print("%-34s %s | %d rows out of %d survivors, %d reached the table of %d slots"
              % (name, line, nsel, rd["survivors"] if terms else nsel, rd["reached_table"], rd["table_slots"]), flush=True)
    finally:
        op.done()


def group_step(cols, k_cat, name, keys):
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(COND, keys, ["count(*)"]))
    try:
        op.intern(bench.synth_dictionary(k_cat))
        batch = op.make_device_batch(rows, [cols.by_path[p] for p in op.column_paths])
        res, line = timed(lambda: op.run_device_batch_raw(batch), op.stats)
        print("%-34s %s | %d groups on the host" % (name, line, res["ngroups"]), flush=True)
    finally:
        op.done()


for k_cat, cases in ((1000, [("cat", [D("cat")])]), (100_000, [("cat, region_id", [D("cat"), D("region_id")]), ("user_id", [D("user_id")])])):
    cols = bench.DeviceColumns(rows, k_cat, False, 0, rows, 0)
    rows_step(cols, k_cat, "filter alone (K_cat %d)" % k_cat)
    for name, terms in cases:
        rows_step(cols, k_cat, "DISTINCT " + name + ", LDS set of 2048", terms, rowdistinct_lds_slots=2048)
        rows_step(cols, k_cat, "DISTINCT " + name + ", no LDS set", terms, rowdistinct_lds_slots=0)
        group_step(cols, k_cat, "GROUP BY " + name + ", count(*)", terms)
    del cols
