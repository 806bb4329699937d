"""Exchange regions at, over and across their capacities.

Every region of the multi-GPU exchange has a fixed capacity, and include/n1k.h ("Failures") promises what happens when one
is too small: N1K_REGION_FULL on every rank alike, nothing written outside a region, a retry in step with larger regions
that gives the right groups.  This module goes to those edges:

  1. the two direct entry points (n1k_partition_device_batch with both partition kernels, n1k_export_partials_device) with
     a capacity that is generous, exactly enough and one too small, into sentinel-filled buffers with a guard part behind
     the last — row multisets against the input columns and the oracle's selected ordinals, bit-exact;
  2. the protocol over the loopback transport: fixed capacities too small, a sub-region that fills below its region's
     capacity, automatic capacities with one hot owner, data that outgrows agreed capacities, one overflowing sender,
     partial groups beyond their regions and beyond the gather's slots, DISTINCT state across a voided step;
  3. a rank's failure in a step whose capacities differ from the step that sized the communicator's buffers.

Wall time on one MI355X (measured once, `pytest -m gpu`, both in one visit to the same box): this module's 220 tests take
22 s, the rest of the GPU suite — the tests the suite had before this module — 338 s.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import parity_util as pu
import query_amd
from oracle import n1o
from query_amd import _ffi, plan
from test_gpu_distributed import COND, D, KEYS, _device_cols, _paths, _run_ranks, _shards

pytestmark = pytest.mark.gpu

GUARD = 64  # slots behind the guard part (a capacity of 0 rows leaves the parts themselves empty)


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel level
# ---------------------------------------------------------------------------------------------------------------------

# (name, option jit, option part_block, rows of one tile).  The interpreting partition_kernel<4, 512> takes 2048 rows per
# tile (n1k_exchange.cpp run_partition: `ntiles = (n + 2047) / 2048`); the run-time-built kernel takes part_block threads x
# two loads of two adjacent rows per lane (`tiles = (n + pblock * 4 - 1) / (pblock * 4)`, same function).
KERNELS = [("interpreter", 0, 512, 2048), ("runtime-built-256", 2, 256, 1024), ("runtime-built-512", 2, 512, 2048)]
KEY_SHAPES = {"dict": [D("cat")], "float": [D("price")], "dict+int": [D("cat"), D("region_id")]}
MANY_TILES = 200
N_BIG = MANY_TILES * 2048 + 17 + 4096


def _aggs_for(keys):
    # (as test_partition_kernel_routes_every_survivor_once: at most 3 input columns, so that every shape has a run-time-built kernel)
    return sorted(["count(*)", "sum(%s)" % D("price"), "max(%s)" % D("user_id")]) if len(keys) == 1 else sorted(["count(*)", "sum(%s)" % D("price")])


@functools.lru_cache(maxsize=None)
def _big_table():
    """Zipf keys over few categories: one destination dominates, so that `cap = max(cnt)` fills the hottest part exactly and
    leaves room in the others.  Returns the table and the ordinal of its first row that passes COND."""
    t = n1o.synth_table(N_BIG, k_cat=29, zipf=True)
    sel = n1o.run(t, COND, [], [], has_group=False).selected
    return t, int(sel[0])


def _table_of(nrows):
    """`nrows` rows whose first one survives the Filter (so that even one row gives a survivor)."""
    t, lo = _big_table()
    assert lo + nrows <= N_BIG
    return t.slice(lo, lo + nrows)


def _word_columns(t, paths):
    """The copied columns as a list of (kind, uint64 array): DICT32 -> codes; TAGGED64 -> payload, tags."""
    by = {c.name: c for c in t.columns}
    out = []
    for p in paths:
        c = by[p]
        if c.kind == n1o.COL_DICT32:
            out.append(("codes", c.codes.astype(np.uint64)))
        else:
            out.append(("payload", c.payload.astype(np.uint64)))
            out.append(("tags", c.tags.astype(np.uint64)))
    return out


def _absent(values, start, limit):
    """A value below `limit` that `values` does not take."""
    taken = set(np.unique(values).tolist())
    v = start
    while v in taken:
        v = (v + 1) % limit
    return v


def _sorted_rows(mat):
    return mat[np.lexsort(mat.T[::-1])] if len(mat) else mat


def _row_counter(mat):
    from collections import Counter
    return Counter(np.ascontiguousarray(mat).view(np.dtype((np.void, 8 * mat.shape[1]))).ravel().tolist()) if len(mat) else Counter()


class _PartOut:
    """Output columns of one partition call: nparts parts of `cap` rows, one more part and GUARD slots behind them, every
    cell a sentinel."""

    def __init__(self, kinds, nparts, cap, sent):
        import torch
        self.size = (nparts + 1) * cap + GUARD
        self.cols = (_ffi.Col * len(kinds))()
        self.arrays = []  # in _word_columns order: (kind, tensor)
        for i, k in enumerate(kinds):
            self.cols[i].kind = k
            if k == _ffi.COL_DICT32:
                b = torch.from_numpy(np.full(self.size, sent["codes"], np.uint32).view(np.int32)).cuda()
                self.cols[i].codes = b.data_ptr()
                self.arrays.append(("codes", b))
            else:
                a = torch.from_numpy(np.full(self.size, sent["tags"], np.uint8)).cuda()
                b = torch.from_numpy(np.full(self.size, sent["payload"], np.uint64).view(np.int64)).cuda()
                self.cols[i].tags, self.cols[i].payload = a.data_ptr(), b.data_ptr()
                self.arrays += [("payload", b), ("tags", a)]
        torch.cuda.synchronize()

    def host(self):
        view = {"codes": np.uint32, "payload": np.uint64, "tags": np.uint8}
        return [(k, x.cpu().numpy().view(view[k]).astype(np.uint64)) for k, x in self.arrays]


def _check_parts(out, sent, nparts, cap, kept, ref_sorted, ref_counter):
    """Part d holds kept[d] rows of destination d's reference multiset in its first slots; every other cell of every column
    array — the rest of each part, the guard part, the slots behind it — is still the sentinel."""
    host = out.host()
    written = np.zeros(out.size, bool)
    for d in range(nparts):
        assert kept[d] <= cap
        written[d * cap: d * cap + kept[d]] = True
    for kind, arr in host:
        stray = np.flatnonzero((arr != sent[kind]) & ~written)
        assert stray.size == 0, "%s written outside a region: slots %r (capacity %d)" % (kind, stray[:8].tolist(), cap)
        holes = np.flatnonzero((arr == sent[kind]) & written)
        assert holes.size == 0, "%s slots below a part's row count were not written: %r" % (kind, holes[:8].tolist())
    for d in range(nparts):
        mat = np.stack([arr[d * cap: d * cap + kept[d]] for _k, arr in host], axis=1)
        if kept[d] == len(ref_sorted[d]):
            assert np.array_equal(_sorted_rows(mat), ref_sorted[d]), "part %d does not hold its destination's rows" % d
        else:
            over = _row_counter(mat) - ref_counter(d)
            assert not over, "part %d holds %d rows that are not its destination's" % (d, sum(over.values()))


@pytest.mark.parametrize("rows", ["1", "tile-1", "tile", "tile+1", "%d-tiles+17" % MANY_TILES])
@pytest.mark.parametrize("nparts", [1, 3, 8, 64])
@pytest.mark.parametrize("shape", list(KEY_SHAPES))
@pytest.mark.parametrize("kernel", KERNELS, ids=[k[0] for k in KERNELS])
def test_partition_at_exact_and_short_capacities(kernel, shape, nparts, rows):
    """n1k_partition_device_batch with `cap` = the fullest part's row count (OK, the same row multiset per destination as a
    generous run), one less and 1 (N1K_REGION_FULL, nothing written at or behind a part's end — not a tag, not a payload,
    not a code — and only the destination's own rows in front of it), and the same handle right again afterwards.  (A table
    of one row has a fullest part of one row: one short is then a capacity of 0 rows, which the entry point takes — nothing at
    all may be written.)"""
    import torch
    _name, jit, block, tile = kernel
    n = {"1": 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}.get(rows, MANY_TILES * tile + 17)
    keys = KEY_SHAPES[shape]
    aggs = _aggs_for(keys)
    t = _table_of(n)
    sender = query_amd.GpuFilterGroup(plan.filter_group_plan(COND, keys, aggs), jit=jit, part_block=block)
    sender.intern(list(t.dictionary))
    paths = sender.column_paths
    assert len(paths) <= 3
    dev, keep = _device_cols(t, paths)
    cols = [dev[p] for p in paths]
    batch, arr = sender._make_batch(n, cols)
    words = _word_columns(t, paths)
    inp = np.stack([w for _k, w in words], axis=1)
    # sentinels no cell of their kind takes
    sent = {"codes": _absent(np.concatenate([w for k, w in words if k == "codes"] or [np.zeros(0, np.uint64)]), 0xABABABAB, 1 << 32),
            "payload": _absent(np.concatenate([w for k, w in words if k == "payload"]), 0xDEADBEEFCAFEF00D, 1 << 64),
            "tags": _absent(np.concatenate([w for k, w in words if k == "tags"]), 0xEE, 1 << 8)}
    for k, w in words:
        assert not (w == sent[k]).any()
    sel = n1o.run(t, COND, [], [], has_group=False).selected
    assert len(sel) >= 1 and sel[0] == 0

    def partition(cap):
        out = _PartOut([c[0] for c in cols], nparts, cap, sent)
        counts = torch.full((nparts,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        st = sender._lib.n1k_partition_device_batch(sender._h, C.byref(batch), nparts, cap, out.cols, counts.data_ptr())
        return st, counts.cpu().numpy(), out

    good = 0

    def stats_are(k):
        s = sender.stats()
        assert (s["rows_in"], s["batches"]) == (k * n, k), (s["rows_in"], s["batches"], k)

    # the reference run: generous parts
    st, cnt, out = partition(n)
    assert st == _ffi.OK
    good += 1
    stats_are(good)
    assert (sender.stats()["spec_kernel"] != 0) == (jit == 2)
    assert int(cnt.sum()) == len(sel) and (cnt >= 0).all()
    host = out.host()
    ref_sorted = [_sorted_rows(np.stack([a[d * n: d * n + int(cnt[d])] for _k, a in host], axis=1)) for d in range(nparts)]
    counters = {}

    def ref_counter(d):
        if d not in counters:
            counters[d] = _row_counter(ref_sorted[d])
        return counters[d]

    _check_parts(out, sent, nparts, n, [int(x) for x in cnt], ref_sorted, ref_counter)
    # ... pinned itself: its parts together are the oracle's selected rows of the input columns, each once
    assert np.array_equal(_sorted_rows(np.concatenate(ref_sorted)), _sorted_rows(inp[sel]))
    most = int(cnt.max())
    assert most >= 1

    def again_generous():
        nonlocal good
        st2, cnt2, out2 = partition(n)
        assert st2 == _ffi.OK, "the handle kept something of the failed call: status %d" % st2
        good += 1
        stats_are(good)
        assert np.array_equal(cnt2, cnt)
        _check_parts(out2, sent, nparts, n, [int(x) for x in cnt], ref_sorted, ref_counter)

    # exact fit: the fullest part has not one slot to spare
    st, cnt_fit, out = partition(most)
    assert st == _ffi.OK, "a capacity of exactly the fullest part's %d rows was refused (status %d)" % (most, st)
    good += 1
    stats_are(good)
    assert np.array_equal(cnt_fit, cnt)
    _check_parts(out, sent, nparts, most, [int(x) for x in cnt], ref_sorted, ref_counter)
    # one short, and parts of one row: every part cut at its capacity
    for cap in sorted({most - 1, min(1, most - 1)}, reverse=True):
        st, _cnt_over, out = partition(cap)
        _check_parts(out, sent, nparts, cap, [min(int(x), cap) for x in cnt], ref_sorted, ref_counter)
        assert st == _ffi.REGION_FULL, "capacity %d for a part of %d rows: status %d" % (cap, most, st)
        stats_are(good)  # (only successful calls count)
        again_generous()
    sender.done()


# eight aggregates (the most a plan takes), each of the widest kind its operand gives: 3 x AVG (5 words), 3 x SUM (4),
# MIN and MAX (4 each)
WIDE_AGGS = sorted(["avg(%s)" % D(c) for c in ("price", "user_id", "region_id")] + ["sum(%s)" % D(c) for c in ("price", "user_id", "region_id")] +
                   ["min(%s)" % D("price"), "max(%s)" % D("user_id")])


@pytest.mark.parametrize("nparts", [1, 3, 8])
@pytest.mark.parametrize("shape", ["one-word", "widest"])
def test_export_partials_at_exact_and_short_capacities(shape, nparts):
    """n1k_export_partials_device with capacity_groups = the fullest region's group count (OK; merged into a fresh receiver
    the regions give the oracle's groups) and one less (N1K_REGION_FULL): header word 0 of every region is the count OFFERED
    to it (export_partials_kernel adds before it tests `pos >= cap`), word 1 is 1 in EVERY region (the overflow verdict),
    the key and accumulator slots from min(count, cap) on are still the zeros the export started from, and a
    sentinel-filled region behind the last is untouched.  Then the same handle exports correctly again."""
    import torch
    n = 60_000
    t = n1o.synth_table(n, k_cat=300)
    aggs = ["count(*)"] if shape == "one-word" else WIDE_AGGS
    ora = n1o.run(t, COND, KEYS, aggs)
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(COND, KEYS, aggs))
    op.intern(list(t.dictionary))
    lib = op._lib
    dev, keep = _device_cols(t, _paths(COND, KEYS, WIDE_AGGS))
    op.process_device_items(n, [dev[p] for p in op.column_paths])
    gw = int(lib.n1k_partial_words(op._h))
    assert gw == (1 if shape == "one-word" else 3 * 5 + 3 * 4 + 2 * 4)

    def export(cap, sentinel):
        words = 2 + cap * (1 + gw)
        assert int(lib.n1k_partial_region_bytes(op._h, cap)) == 8 * words
        buf = torch.from_numpy(np.full((nparts + 1) * words, sentinel, np.uint64).view(np.int64)).cuda()
        torch.cuda.synchronize()
        st = lib.n1k_export_partials_device(op._h, nparts, cap, buf.data_ptr())
        return st, buf, buf.cpu().numpy().view(np.uint64).reshape(nparts + 1, words)

    def check_regions(regions, cap, offered, verdict, sentinel, ref_keys):
        assert (regions[nparts] == sentinel).all(), "the region behind the last was written"
        for d in range(nparts):
            r = regions[d]
            assert (int(r[0]), int(r[1])) == (offered[d], verdict), (d, int(r[0]), int(r[1]))
            kept = min(offered[d], cap)
            keys_d, acc_d = r[2: 2 + cap], r[2 + cap:]
            assert not keys_d[kept:].any() and not acc_d[kept * gw:].any(), "region %d: a group behind its %d kept ones" % (d, kept)
            extra = set(keys_d[:kept].tolist()) - ref_keys[d]
            assert len(set(keys_d[:kept].tolist())) == kept and not extra, "region %d holds keys of another destination" % d

    def merged_equals_oracle(buf, cap):
        rcv = query_amd.GpuFilterGroup(plan.filter_group_plan(None, KEYS, aggs))
        rcv.intern(list(t.dictionary))
        rcv.process_device_items(0, [dev[p] for p in rcv.column_paths])  # (an empty batch: fixes the key layout)
        rcv._check(lib.n1k_merge_partials_device(rcv._h, nparts, cap, buf.data_ptr()))
        got = rcv.after_items()
        rcv.done()
        pu.assert_same_groups(got, ora, aggs=aggs)

    generous = 512
    st, buf, first = export(generous, 0x5E5E5E5E5E5E5E5E)
    assert st == _ffi.OK
    sentinel = _absent(first[:nparts].ravel(), 0x5E5E5E5E5E5E5E5E, 1 << 64)  # (no exported word takes it)
    st, buf, ref = export(generous, sentinel)
    assert st == _ffi.OK and not (ref[:nparts] == sentinel).any()
    offered = [int(ref[d][0]) for d in range(nparts)]
    assert sum(offered) == len(ora.keys) and max(offered) >= 2
    ref_keys = [set(ref[d][2: 2 + offered[d]].tolist()) for d in range(nparts)]
    check_regions(ref, generous, offered, 0, sentinel, ref_keys)
    merged_equals_oracle(buf, generous)
    most = max(offered)
    st, buf, fit = export(most, sentinel)
    assert st == _ffi.OK, "a capacity of exactly the fullest region's %d groups was refused (status %d)" % (most, st)
    check_regions(fit, most, offered, 0, sentinel, ref_keys)
    merged_equals_oracle(buf, most)
    st, buf, short = export(most - 1, sentinel)
    assert st == _ffi.REGION_FULL, st
    check_regions(short, most - 1, offered, 1, sentinel, ref_keys)
    st, buf, after = export(generous, sentinel)
    assert st == _ffi.OK, "the handle kept something of the failed export: status %d" % st
    check_regions(after, generous, offered, 0, sentinel, ref_keys)
    merged_equals_oracle(buf, generous)
    op.done()


# ---------------------------------------------------------------------------------------------------------------------
# 2. protocol level: overflow, retry and growth over the loopback transport
# ---------------------------------------------------------------------------------------------------------------------

QUANTUM = 128  # n1k_wire.h quantum: capacities are rounded up to kRowSubs sub-regions of whole 16-row groups


def _round_up(x, q=QUANTUM):
    return (int(x) + q - 1) // q * q


def _dest_counts(cond, keys, aggs, dictionary, rows_n, dev, world, lo=0, hi=None):
    """Rows [lo, hi) of a shard that pass the Filter, per destination of a `world`-way partition: counted by
    n1k_partition_device_batch with generous parts (both partition kernels send a key to the same destination)."""
    import torch
    hi = rows_n if hi is None else hi
    n = hi - lo
    h = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs), jit=0)
    h.intern(list(dictionary))
    cols = []
    for p in h.column_paths:
        kind, tags, payload, codes = dev[p]
        cols.append((kind, None if tags is None else tags + lo, None if payload is None else payload + 8 * lo, None if codes is None else codes + 4 * lo))
    batch, arr = h._make_batch(n, cols)
    out = (_ffi.Col * len(cols))()
    bufs = []
    for i, c in enumerate(cols):
        out[i].kind = c[0]
        if c[0] == _ffi.COL_DICT32:
            b = torch.zeros(n * world, dtype=torch.int32, device="cuda")
            out[i].codes = b.data_ptr()
            bufs.append(b)
        else:
            a = torch.zeros(n * world, dtype=torch.uint8, device="cuda")
            b = torch.zeros(n * world, dtype=torch.int64, device="cuda")
            out[i].tags, out[i].payload = a.data_ptr(), b.data_ptr()
            bufs += [a, b]
    counts = torch.zeros(world, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h._check(h._lib.n1k_partition_device_batch(h._h, C.byref(batch), world, n, out, counts.data_ptr()))
    h.done()
    return [int(x) for x in counts.cpu().numpy()]


def _groups(op, raw, nkeys, naggs):
    from query_amd.gpu_operator import GroupRows
    cache = {}
    return GroupRows(nkeys, naggs, op.merger._py_values(raw["keys"], cache), op.merger._py_values(raw["aggs"], cache), [])


def _step_report(op, st, worst, out):
    lib = op.sender._lib
    glob = {name for name, h in (("sender", op.sender), ("receiver", op.receiver)) if lib.n1k_failure_is_global(h._h)}
    msg = " | ".join((lib.n1k_last_error(h._h) or b"").decode(errors="replace") for h in (op.sender, op.receiver, op.merger))
    raw = op._result_dict(out) if st == _ffi.OK and worst == 0 else None
    return {"st": st, "worst": worst, "raw": raw, "global": glob, "msg": msg, "recv_rows": int(op.receiver.stats()["rows_selected"])}


def _rows_step(op, rows_n, dev, caps):
    """One n1k_rows_step_v with the capacities given, its status visible: (status, worst, groups or None, the handles on which
    n1k_failure_is_global is 1, the messages)."""
    lib = op.sender._lib
    batch = op._batch(rows_n, dev)
    arr = (C.c_uint64 * op.world)(*[int(c) for c in caps])
    out, worst = _ffi.Result(), C.c_int(0)
    st = int(lib.n1k_rows_step_v(op.comm._h, op.sender._h, C.byref(batch[0]), op.receiver._h, op.merger._h, arr, C.byref(out), C.byref(worst)))
    return _step_report(op, st, worst.value, out)


def _slices(t, bounds):
    """Shards of a table cut at the row ordinals given (uneven shards)."""
    return [t.slice(lo, hi) for lo, hi in zip(bounds[:-1], bounds[1:])]


def _uneven_shards(t, paths, bounds):
    shards, keep = [], []
    for sub in _slices(t, bounds):
        dev, k = _device_cols(sub, paths)
        keep.append(k)
        shards.append((sub.nrows, dev))
    return shards, keep


ROW_AGGS = sorted(["count(*)", "sum(%s)" % D("price")])
# (jit, part_subs): run_partition (n1k_exchange.cpp) writes sub-regions only from the run-time-built kernel with part_subs = 2
# (or >= 4096 tiles); every other combination writes dense runs that dense_to_segments_kernel cuts into segments
FORMS = {"interpreter-dense": (0, 1), "runtime-built-dense": (2, 1), "runtime-built-subregions": (2, 2)}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world,form", [(1, "interpreter-dense"), (1, "runtime-built-subregions"), (2, "interpreter-dense"), (2, "runtime-built-subregions"),
                                        (3, "runtime-built-dense"), (3, "runtime-built-subregions"), (8, "interpreter-dense"),
                                        (8, "runtime-built-subregions")])
def test_rows_with_a_fixed_capacity_too_small_retry_in_step(world, form):
    """op.row_capacity a quarter of the fullest region's rows: the first attempt overflows, every rank doubles alike
    (run_rows' fixed-capacity `* 2` branch) until the regions hold the rows, and the groups are the oracle's.  The sender's
    counters afterwards are one successful step's."""
    from query_amd import distributed as qd
    jit, subs = FORMS[form]
    n = 120_007
    t = n1o.synth_table(n, k_cat=61, zipf=True)
    ora = n1o.run(t, COND, KEYS, ROW_AGGS)
    comms = qd.Comm.loopback(world, 0)
    shards, keep = _shards(t, _paths(COND, KEYS, ROW_AGGS), world)
    counts = [_dest_counts(COND, KEYS, ROW_AGGS, t.dictionary, rows_n, dev, world) for rows_n, dev in shards]
    assert all(min(c) >= 1 for c in counts), counts  # every sender has rows for every owner
    most = max(max(c) for c in counts)
    cap0 = _round_up(max(1, most // 4))
    assert cap0 < most  # the first attempt must overflow
    doublings = 0
    while cap0 << doublings < most:
        doublings += 1

    def rank_body(r):
        op = qd.ShardedFilterGroup(COND, KEYS, ROW_AGGS, t.dictionary, r, world, 0, comm=comms[r])
        for h in (op.sender, op.receiver):
            h.set_option("jit", jit)
        op.sender.set_option("part_subs", subs)
        op.row_capacity = cap0
        rows_n, dev = shards[r]
        raw, info = op.run_rows(rows_n, dev)
        s = op.sender.stats()
        return _groups(op, raw, 1, len(ROW_AGGS)), info, (int(s["rows_in"]), int(s["batches"]), int(s["spec_kernel"]))

    outs = _run_ranks(world, rank_body)
    for r in range(world):
        rows, info, (rows_in, batches, spec) = outs[r]
        pu.assert_same_groups(rows, ora, aggs=ROW_AGGS)
        assert info["region_rows"] == outs[0][1]["region_rows"]  # one vector on every rank
        assert (spec != 0) == (jit == 2)
        assert (rows_in, batches) == (shards[r][0], 1)  # nothing of the voided attempts is left in the counters
    got = outs[0][1]["region_rows"]
    assert len(set(got)) == 1 and got[0] % cap0 == 0
    if subs == 2:  # (a sub-region may fill before its region does: at least the doublings the totals need)
        assert got[0] >= cap0 << doublings and got[0] // cap0 in (2, 4, 8, 16, 32, 64), (got, cap0)
    else:
        assert got[0] == cap0 << doublings, (got, cap0, doublings)
    assert sum(outs[r][1]["recv_rows"] for r in range(world)) == ora.rows_passed


@pytest.mark.timeout(600)
def test_a_sub_region_fills_while_its_region_has_room():
    """Two tiles per shard through the run-time-built kernel with sub-regions: workgroup b writes sub-region b % 8 of every
    destination (n1k_spec.h: `sub = blockIdx.x % nsub`; the grid is rounded up to a multiple of 8 and tile t is workgroup t's),
    so each destination's rows land in sub-regions 0 and 1 and the other six stay empty.  With a sub-region capacity of half
    the fullest (tile, destination) count — 16-row groups — the region as a whole (8 sub-regions) holds every sender's rows
    for its owner twice over, yet the step is N1K_REGION_FULL on every rank; the doubled capacity succeeds."""
    from query_amd import distributed as qd
    world, tile, tiles = 2, 2048, 2
    n = world * tile * tiles
    t = n1o.synth_table(n, k_cat=5)
    ora = n1o.run(t, COND, KEYS, ROW_AGGS)
    comms = qd.Comm.loopback(world, 0)
    shards, keep = _shards(t, _paths(COND, KEYS, ROW_AGGS), world)
    per_tile = [[_dest_counts(COND, KEYS, ROW_AGGS, t.dictionary, rows_n, dev, world, lo=k * tile, hi=(k + 1) * tile) for k in range(tiles)]
                for rows_n, dev in shards]
    fullest = max(max(c) for shard in per_tile for c in shard)
    total = max(sum(c[d] for c in shard) for shard in per_tile for d in range(world))
    sub = (fullest // 2 + 15) // 16 * 16
    cap = 8 * sub
    assert sub < fullest <= 2 * sub and total <= cap and cap % QUANTUM == 0, (fullest, total, sub)

    def rank_body(r):
        op = qd.ShardedFilterGroup(COND, KEYS, ROW_AGGS, t.dictionary, r, world, 0, comm=comms[r])
        for h in (op.sender, op.receiver):
            h.set_option("jit", 2)
        op.sender.set_option("part_subs", 2)
        op.sender.set_option("part_block", 512)  # (tiles of 2048 rows)
        rows_n, dev = shards[r]
        assert rows_n == tile * tiles
        first = _rows_step(op, rows_n, dev, [cap] * world)
        spec = int(op.sender.stats()["spec_kernel"])
        second = _rows_step(op, rows_n, dev, [2 * cap] * world)
        if second["raw"] is not None:
            second["rows"] = _groups(op, second["raw"], 1, len(ROW_AGGS))
        return first, second, spec

    outs = _run_ranks(world, rank_body)
    for first, second, spec in outs:
        assert spec != 0
        assert first["st"] == _ffi.REGION_FULL and "receiver" in first["global"], first
        assert (second["st"], second["worst"]) == (_ffi.OK, 0), second
        pu.assert_same_groups(second["rows"], ora, aggs=ROW_AGGS)
    assert sum(second["recv_rows"] for _f, second, _s in outs) == ora.rows_passed


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 4])
def test_automatic_capacities_with_one_hot_owner(world):
    """Every row has the same group key and passes: one owner receives every shard whole, and the first step's regions
    (_first_row_capacity = largest shard x 1.1 / world + 4096 rows) are smaller than a shard.  The step overflows on its own,
    every rank doubles alike (run_rows' automatic `* 2` branch), and the capacities agreed afterwards keep the hot owner's
    regions large and cut the others to the floor of 4096 rows."""
    from query_amd import distributed as qd
    per_shard = 20_000
    n = per_shard * world
    t = n1o.synth_table(n, k_cat=1)
    ora = n1o.run(t, None, KEYS, ROW_AGGS)
    assert len(ora.keys) == 1
    comms = qd.Comm.loopback(world, 0)
    shards, keep = _shards(t, _paths(None, KEYS, ROW_AGGS), world)
    first_cap = max(4096, int(per_shard * 1.1 / world) + 4096)
    assert first_cap < per_shard
    counts = _dest_counts(None, KEYS, ROW_AGGS, t.dictionary, shards[0][0], shards[0][1], world)
    hot = counts.index(per_shard)  # (all of a shard's rows go to one owner)

    def rank_body(r):
        op = qd.ShardedFilterGroup(None, KEYS, ROW_AGGS, t.dictionary, r, world, 0, comm=comms[r])
        rows_n, dev = shards[r]
        steps = []
        for _ in range(2):
            raw, info = op.run_rows(rows_n, dev)
            steps.append((_groups(op, raw, 1, len(ROW_AGGS)), info))
        return steps

    outs = _run_ranks(world, rank_body)
    doubled = first_cap
    while _round_up(doubled) < per_shard:
        doubled *= 2
    for r in range(world):
        for rows, info in outs[r]:
            pu.assert_same_groups(rows, ora, aggs=ROW_AGGS)
        assert outs[r][0][1]["region_rows"] == [doubled] * world  # the same doublings on every rank
        second = outs[r][1][1]["region_rows"]
        assert second[hot] >= per_shard and all(second[d] == 4096 for d in range(world) if d != hot), second
    for step in range(2):
        assert sum(outs[r][step][1]["recv_rows"] for r in range(world)) == n


@pytest.mark.timeout(600)
def test_data_that_outgrows_the_agreed_capacities():
    """Step 1 over a short prefix of every shard: the ranks agree on small per-destination capacities.  Step 2 over data whose
    survivors exceed them on rank 0 only: every rank retries (run_rows' `* 2` on the agreed capacities) and ends with the
    oracle's groups of step 2's data; step 3 repeats step 2 without a retry — the grown capacities were kept."""
    from query_amd import distributed as qd
    world, big, small = 2, 40_000, 2_000
    t = n1o.synth_table(big + small, k_cat=61)
    ora = n1o.run(t, COND, KEYS, ROW_AGGS)
    comms = qd.Comm.loopback(world, 0)
    shards, keep = _uneven_shards(t, _paths(COND, KEYS, ROW_AGGS), [0, big, big + small])
    prefix = [_dest_counts(COND, KEYS, ROW_AGGS, t.dictionary, small, dev, world) for _n, dev in shards]
    whole = [_dest_counts(COND, KEYS, ROW_AGGS, t.dictionary, rows_n, dev, world) for rows_n, dev in shards]
    agreed = [max(4096, int(max(prefix[r][d] for r in range(world)) * 1.1) + 4096) for d in range(world)]  # (run_rows, after step 1)
    assert max(whole[0]) > _round_up(max(agreed)) and max(whole[1]) <= min(agreed), (whole, agreed)

    def rank_body(r):
        op = qd.ShardedFilterGroup(COND, KEYS, ROW_AGGS, t.dictionary, r, world, 0, comm=comms[r])
        rows_n, dev = shards[r]
        _raw, info1 = op.run_rows(small, dev)
        caps1 = list(op._caps)
        raw2, info2 = op.run_rows(rows_n, dev)
        rows2 = _groups(op, raw2, 1, len(ROW_AGGS))
        raw3, info3 = op.run_rows(rows_n, dev)
        return caps1, info2, rows2, info3, _groups(op, raw3, 1, len(ROW_AGGS))

    outs = _run_ranks(world, rank_body)
    for caps1, info2, rows2, info3, rows3 in outs:
        assert caps1 == agreed
        grown = info2["region_rows"]
        assert all(g % a == 0 and g > a for g, a in zip(grown, agreed)), (grown, agreed)  # doubled, every destination alike
        assert grown == outs[0][1]["region_rows"] and max(whole[0]) <= max(grown)
        assert info3["region_rows"] == grown  # no further retry
        pu.assert_same_groups(rows2, ora, aggs=ROW_AGGS)
        pu.assert_same_groups(rows3, ora, aggs=ROW_AGGS)
    assert sum(o[1]["recv_rows"] for o in outs) == ora.rows_passed and sum(o[3]["recv_rows"] for o in outs) == ora.rows_passed


@pytest.mark.timeout(600)
def test_one_senders_overflow_voids_the_step_on_every_rank():
    """Three shards of which only rank 1's is large, Zipf keys: with a capacity between the two fullest (sender, destination)
    counts exactly ONE sender overflows ONE destination.  Every rank's step is N1K_REGION_FULL, learnt from the headers
    (n1k_failure_is_global on the receiver), nobody entered the gather, and no receiver aggregated a single row — also not
    from the regions of the senders that did not overflow.  The step repeated with room gives the oracle's groups."""
    from query_amd import distributed as qd
    world = 3
    bounds = [0, 3_000, 33_000, 36_000]
    t = n1o.synth_table(bounds[-1], k_cat=29, zipf=True)
    ora = n1o.run(t, COND, KEYS, ROW_AGGS)
    comms = qd.Comm.loopback(world, 0)
    shards, keep = _uneven_shards(t, _paths(COND, KEYS, ROW_AGGS), bounds)
    counts = [_dest_counts(COND, KEYS, ROW_AGGS, t.dictionary, rows_n, dev, world) for rows_n, dev in shards]
    flat = sorted((c, r, d) for r in range(world) for d, c in enumerate(counts[r]))
    cap = _round_up(flat[-2][0])
    assert flat[-1][0] > cap and flat[-1][1] == 1 and sum(c > cap for c, _r, _d in flat) == 1, flat
    room = _round_up(flat[-1][0])

    def rank_body(r):
        op = qd.ShardedFilterGroup(COND, KEYS, ROW_AGGS, t.dictionary, r, world, 0, comm=comms[r])
        for h in (op.sender, op.receiver):
            h.set_option("jit", 0)
        rows_n, dev = shards[r]
        first = _rows_step(op, rows_n, dev, [cap] * world)
        second = _rows_step(op, rows_n, dev, [room] * world)
        if second["raw"] is not None:
            second["rows"] = _groups(op, second["raw"], 1, len(ROW_AGGS))
        return first, second

    outs = _run_ranks(world, rank_body)
    for first, second in outs:
        assert first["st"] == _ffi.REGION_FULL and first["global"] == {"receiver"}, first
        assert first["recv_rows"] == 0, "a receiver aggregated %d rows of a voided step" % first["recv_rows"]
        assert (second["st"], second["worst"]) == (_ffi.OK, 0), second
        pu.assert_same_groups(second["rows"], ora, aggs=ROW_AGGS)
    assert sum(second["recv_rows"] for _f, second in outs) == ora.rows_passed


def _partial_counts(cond, keys, aggs, dictionary, rows_n, dev, world):
    """Groups of a shard per destination of a `world`-way export (header word 0 of a generous export's regions)."""
    import torch
    h = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs))
    h.intern(list(dictionary))
    h.process_device_items(rows_n, [dev[p] for p in h.column_paths])
    h.sync()
    cap = max(1, int(h.stats()["groups_out"]))
    words = int(h._lib.n1k_partial_region_bytes(h._h, cap)) // 8
    buf = torch.zeros(world * words, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h._check(h._lib.n1k_export_partials_device(h._h, world, cap, buf.data_ptr()))
    got = [int(buf[d * words].item()) for d in range(world)]
    h.done()
    return got


@pytest.mark.timeout(600)
@pytest.mark.parametrize("start", ["one", "fullest-1"])
@pytest.mark.parametrize("world", [2, 3])
def test_partials_with_a_capacity_too_small_retry_in_step(world, start):
    """op.partial_capacity preset to 1 group, and to one less than the fullest region needs: every rank multiplies by 4 alike
    (run_partials' retry) until the regions hold the groups; each owner then finishes more groups than the 1024 records a
    gather slot starts with, so n1k_gather_groups_status grows its slots too.  The result is the oracle's."""
    from query_amd import distributed as qd
    n = 60_000
    t = n1o.synth_table(n, k_cat=5000)
    ora = n1o.run(t, COND, KEYS, ROW_AGGS)
    assert len(ora.keys) > 1024 * world  # some owner finishes more than one gather slot of groups
    comms = qd.Comm.loopback(world, 0)
    shards, keep = _shards(t, _paths(COND, KEYS, ROW_AGGS), world)
    fullest = max(max(_partial_counts(COND, KEYS, ROW_AGGS, t.dictionary, rows_n, dev, world)) for rows_n, dev in shards)
    cap0 = 1 if start == "one" else fullest - 1
    assert 1 <= cap0 < fullest
    want = cap0
    while want < fullest:
        want *= 4

    def rank_body(r):
        op = qd.ShardedFilterGroup(COND, KEYS, ROW_AGGS, t.dictionary, r, world, 0, comm=comms[r])
        op.partial_capacity = cap0
        rows_n, dev = shards[r]
        raw, info = op.run_partials(rows_n, dev)
        return _groups(op, raw, 1, len(ROW_AGGS)), info, op.partial_capacity

    outs = _run_ranks(world, rank_body)
    for rows, info, cap in outs:
        assert info["mode"] == "partials" and cap == want, (info, cap, want)
        assert len(rows.keys) == len(ora.keys)
        pu.assert_same_groups(rows, ora, aggs=ROW_AGGS)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 3])
def test_distinct_counts_survive_a_voided_step(world):
    """Config 3's aggregates (COUNT(DISTINCT user_id), AVG(price)) through the row exchange with regions too small at first:
    the voided attempt must leave nothing in the owner's DISTINCT sets — a member counted twice would show in the counts."""
    from query_amd import distributed as qd
    aggs = sorted(["count(distinct %s)" % D("user_id"), "avg(%s)" % D("price")])
    n = 90_000
    t = n1o.synth_table(n, k_cat=53)
    ora = n1o.run(t, None, KEYS, aggs)
    comms = qd.Comm.loopback(world, 0)
    shards, keep = _shards(t, _paths(None, KEYS, aggs), world)
    counts = [_dest_counts(None, KEYS, aggs, t.dictionary, rows_n, dev, world) for rows_n, dev in shards]
    most = max(max(c) for c in counts)
    cap0 = _round_up(most // 2)
    assert cap0 < most <= 2 * cap0

    def rank_body(r):
        op = qd.ShardedFilterGroup(None, KEYS, aggs, t.dictionary, r, world, 0, comm=comms[r])
        assert op.has_distinct
        op.row_capacity = cap0
        rows_n, dev = shards[r]
        raw, info = op.run_rows(rows_n, dev)
        return _groups(op, raw, 1, len(aggs)), info

    outs = _run_ranks(world, rank_body)
    for rows, info in outs:
        assert info["region_rows"] == [2 * cap0] * world  # one overflow, one doubling
        pu.assert_same_groups(rows, ora, aggs=aggs)
    assert sum(info["recv_rows"] for _rows, info in outs) == n


# ---------------------------------------------------------------------------------------------------------------------
# 3. a rank's failure in a step whose capacities changed
# ---------------------------------------------------------------------------------------------------------------------

def _manual_rows_step(op, rows_n, dev, caps, stop):
    """What n1k_rows_step_v does, call by call — so that a stop can be placed behind the resets (n1k_reset clears the stop flag):
    n1k_reset x 2, n1k_stop on the faulty sender, n1k_exchange_rows_v, n1k_finish, and the gather only where the failure is not
    global."""
    lib = op.sender._lib
    snd, rcv = op.sender, op.receiver
    batch = op._batch(rows_n, dev)
    arr = (C.c_uint64 * op.world)(*[int(c) for c in caps])
    out, worst, local = _ffi.Result(), C.c_int(0), _ffi.Result()

    def report(st):
        return _step_report(op, st, worst.value, out)

    assert lib.n1k_reset(rcv._h) == _ffi.OK and lib.n1k_reset(snd._h) == _ffi.OK
    if stop:
        snd.send_stop()
    st = int(lib.n1k_exchange_rows_v(op.comm._h, snd._h, C.byref(batch[0]), rcv._h, arr))
    if st != _ffi.OK and lib.n1k_failure_is_global(snd._h):
        return report(st)  # this rank's own failure, told to every peer in the headers: no gather anywhere
    fs = int(lib.n1k_finish(rcv._h, C.byref(local)))
    if fs != _ffi.OK and lib.n1k_failure_is_global(rcv._h):
        return report(fs)  # learnt from the headers, by every rank alike: no gather anywhere
    if st == _ffi.OK:
        st = fs
    gs = int(lib.n1k_gather_groups_status(op.comm._h, op.merger._h, C.byref(local) if st == _ffi.OK else None, st, C.byref(out), C.byref(worst)))
    return report(gs if gs != _ffi.OK else st)


# steps of a scenario: (capacity in units of C, or "small" / "small x 2"; fault in this step?; what every rank must return)
SCENARIOS = {
    "good-C-then-fault-at-2C": [("C", False, "ok"), ("2C", True, "fault"), ("2C", False, "ok")],
    "good-C-then-fault-at-4C": [("C", False, "ok"), ("4C", True, "fault"), ("4C", False, "ok")],
    "good-4C-then-fault-at-C": [("4C", False, "ok"), ("C", True, "fault"), ("C", False, "ok")],
    "overflow-then-fault-in-the-doubled-retry": [("small", False, "full"), ("small x 2", True, "fault"), ("C", False, "ok")],
    "good-4C-then-overflow-then-fault-in-the-doubled-retry": [("4C", False, "ok"), ("small", False, "full"), ("small x 2", True, "fault"),
                                                               ("C", False, "ok")],
}
FAULTS = {"buffers": _ffi.OOM, "null-tags-batch": _ffi.INVALID, "stopped-sender": _ffi.STOPPED}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fault", list(FAULTS))
@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_a_ranks_failure_in_a_step_of_other_capacities_reaches_every_rank(scenario, fault):
    """World 3, row exchange, rank 1 faulty in ONE step whose capacities differ from those of the step that sized the
    communicator's buffers — larger (the failing rank's usual buffers do not hold three regions of this step's stride: it
    ships one scratch region to every peer), smaller (they do), or those of the doubled retry after an overflow.  The fault:
    the exchange's buffers cannot be had (option inject_failure = 1, N1K_OOM), a batch whose tag pointer is null
    (N1K_INVALID), or a sender stopped behind its reset (N1K_STOPPED).  Every rank returns the faulty rank's status from that
    step — the peers' messages name the peer's status — nobody hangs, and the next step, without the fault, gives the oracle's
    groups on every rank."""
    from query_amd import distributed as qd
    world, bad = 3, 1
    n = 60_003
    t = n1o.synth_table(n, k_cat=37)
    ora = n1o.run(t, COND, KEYS, ROW_AGGS)
    comms = qd.Comm.loopback(world, 0)
    shards, keep = _shards(t, _paths(COND, KEYS, ROW_AGGS), world)
    counts = [_dest_counts(COND, KEYS, ROW_AGGS, t.dictionary, rows_n, dev, world) for rows_n, dev in shards]
    most = max(max(c) for c in counts)
    unit = _round_up(most)  # C: the fullest region fits
    small = _round_up(most // 4)
    assert QUANTUM <= small < most <= unit
    capacity = {"C": unit, "2C": 2 * unit, "4C": 4 * unit, "small": small, "small x 2": 2 * small}
    want = FAULTS[fault]

    def rank_body(r):
        op = qd.ShardedFilterGroup(COND, KEYS, ROW_AGGS, t.dictionary, r, world, 0, comm=comms[r])
        rows_n, dev = shards[r]
        seen = []
        for cap, faulty_step, _expect in SCENARIOS[scenario]:
            faulty = faulty_step and r == bad
            caps = [capacity[cap]] * world
            saved = None
            if faulty and fault == "buffers":
                op.sender.set_option("inject_failure", 1)
            if faulty and fault == "null-tags-batch":
                good = op._batch(rows_n, dev)
                which = [i for i in range(len(op.send_paths)) if good[0].cols[i].kind == _ffi.COL_TAGGED64][0]
                saved, good[0].cols[which].tags = good[0].cols[which].tags, None
            if faulty_step and fault == "stopped-sender":
                res = _manual_rows_step(op, rows_n, dev, caps, stop=faulty)
            else:
                res = _rows_step(op, rows_n, dev, caps)
            if saved is not None:
                good[0].cols[which].tags = saved
            if res["raw"] is not None:
                res["rows"] = _groups(op, res["raw"], 1, len(ROW_AGGS))
            seen.append(res)
        return seen

    outs = _run_ranks(world, rank_body)
    for r in range(world):
        for (cap, _faulty_step, expect), res in zip(SCENARIOS[scenario], outs[r]):
            where = "rank %d, step at %s: %r" % (r, cap, {k: v for k, v in res.items() if k not in ("raw", "rows")})
            if expect == "ok":
                assert (res["st"], res["worst"]) == (_ffi.OK, 0), where
                pu.assert_same_groups(res["rows"], ora, aggs=ROW_AGGS)
            elif expect == "full":
                assert res["st"] == _ffi.REGION_FULL and "receiver" in res["global"], where
            else:
                assert res["st"] == want, where
                assert ("sender" if r == bad else "receiver") in res["global"], where
                if r != bad:
                    assert "its status: %d" % want in res["msg"], where
    for i, (_cap, _f, expect) in enumerate(SCENARIOS[scenario]):
        if expect == "ok":
            assert sum(outs[r][i]["recv_rows"] for r in range(world)) == ora.rows_passed
