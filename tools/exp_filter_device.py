"""Filter-only plans, the answer on the host against the answer on the device, on one box in one run (bench.py's `filter`
workload: `price > 50` over the synthetic columns):

  host64      the 64-bit step: n1k_run_device_batch (reset + push + finish; 8 B per survivor to a pageable host vector)
  device32    n1k_filter_device_batch (32-bit ordinals stay in HBM; the count comes back)
  +host32     n1k_filter_device_batch + n1k_selected_to_host32 into a pinned buffer (4 B per survivor)
  gather      n1k_gather_selected of three synthetic columns (cat DICT32, price and user_id TAGGED64) by the device selection

    python tools/exp_filter_device.py [rows] [repetitions]

Kernel times are n1k_stats.device_ms, wall times are per step around the calls (the best and the median of the repetitions)."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench, query_amd
from query_amd import _ffi, plan

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
D = bench.D
cols = bench.DeviceColumns(rows, 1000, False, 0, rows, 0)
op = query_amd.GpuFilterGroup(plan.filter_group_plan("(50 < %s)" % D("price"), [], [], filter_only=True))
op.intern(bench.synth_dictionary(1000))
batch = op.make_device_batch(rows, [cols.by_path[p] for p in op.column_paths])


def report(name, wall, dev, note=""):
    print("%-9s wall best %8.3f ms  median %8.3f ms | kernel (device_ms) best %6.3f ms  median %6.3f ms  %s" %
          (name, min(wall), statistics.median(wall), min(dev), statistics.median(dev), note))


def timed(fn):
    wall, dev = [], []
    for i in range(reps + 1):  # (the first repetition allocates: not reported)
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if i:
            wall.append((t1 - t0) * 1e3)
            dev.append(op.stats()["device_ms"])
    return wall, dev


sel64 = {}
wall, dev = timed(lambda: sel64.update(n=len(op.run_device_batch_raw(batch)["selected"])))
report("host64", wall, dev, "%d of %d rows selected" % (sel64["n"], rows))

nsel = op.filter_device_batch(batch)[0]
assert nsel == sel64["n"]
wall, dev = timed(lambda: op.filter_device_batch(batch))
report("device32", wall, dev, "%.2f G rows/s by the best wall time" % (rows / min(wall) / 1e6))

pinned = torch.empty(nsel, dtype=torch.int32).pin_memory()
landing = pinned.numpy().view(np.uint32)
wall, dev = timed(lambda: (op.filter_device_batch(batch), op.selected_host32(landing)))
report("+host32", wall, dev, "%.2f G rows/s by the best wall time" % (rows / min(wall) / 1e6))
ref = op.run_device_batch_raw(batch)["selected"]
op.filter_device_batch(batch)
assert np.array_equal(op.selected_host32(landing).astype(np.uint64), ref), "the two paths disagree"

paths = [D("cat"), D("price"), D("user_id")]
src = op.make_device_batch(rows, [cols.by_path[p] for p in paths])
o_cat = torch.empty(nsel, dtype=torch.int32, device="cuda")
o_tags = [torch.empty(nsel, dtype=torch.uint8, device="cuda") for _ in range(2)]
o_pay = [torch.empty(nsel, dtype=torch.int64, device="cuda") for _ in range(2)]
out = [(_ffi.COL_DICT32, None, None, o_cat.data_ptr())] + [(_ffi.COL_TAGGED64, o_tags[i].data_ptr(), o_pay[i].data_ptr(), None) for i in range(2)]
torch.cuda.synchronize()
wall, dev = [], []
for i in range(reps + 1):
    op.sync()
    before = op.stats()["device_ms"]
    t0 = time.perf_counter()
    op.gather_selected(src, nsel, out)
    op.sync()
    t1 = time.perf_counter()
    if i:
        wall.append((t1 - t0) * 1e3)
        dev.append(op.stats()["device_ms"] - before)
moved = nsel * (4 + 2 * (4 + 9 + 9))  # per survivor: its ordinal, 22 B read, 22 B written
report("gather", wall, dev, "%d rows x (4 + 22 + 22) B = %.2f GB: %.2f TB/s by the best kernel time; selectivity %.3f" %
       (nsel, moved / 1e9, moved / (min(dev) * 1e-3) / 1e12, nsel / rows))
idx = torch.from_numpy(landing[:nsel].astype(np.int64)).cuda()
assert torch.equal(o_cat, cols.cat[idx]) and torch.equal(o_pay[0], cols.price_p[idx]) and torch.equal(o_tags[1], cols.user_t[idx])
op.done()
