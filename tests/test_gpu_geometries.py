"""Every kernel geometry the tuning options select (geometry_util.GEOMETRY), checked against the oracle.

Each case runs one option value at a row count where it takes effect (the clamps are cited next to the cases), compares
the groups with the oracle, and asserts from stats() that the named path really ran.  Row counts sit where tails break:
1, tile - 1, tile, tile + 1 and 2 * grid * tile +- 1, with the tile derived from the kernel's launch.  MI355X has 256 CUs;
the grid formulas below are evaluated with that number.
"""
import ctypes as C

import numpy as np
import pytest

import geometry_util as gu
import parity_util as pu
import query_amd
from geometry_util import D
from oracle import n1o
from query_amd import _ffi, plan

pytestmark = pytest.mark.gpu

G = gu.GEOMETRY
NCUS = 256

_tables, _oracles = {}, {}


def table(kind, n, **kw):
    """Tables are built once per module: slices of one table per (kind, parameters) share its rows."""
    key = (kind, n, tuple(sorted(kw.items())))
    if key not in _tables:
        if kind == "synth":
            _tables[key] = n1o.synth_table(n, **kw)
        elif kind == "records":
            _tables[key] = gu.records_table(n, **kw)
        else:
            _tables[key] = gu.distinct_table(n, **kw)
    return _tables[key]


def oracle(tkey, t, cond, keys, aggs):
    key = (tkey, cond, tuple(keys), tuple(aggs))
    if key not in _oracles:
        _oracles[key] = n1o.run(t, cond, keys, aggs, threads=4)
    return _oracles[key]


def selected(tkey, t, cond):
    key = (tkey, cond, "selected")
    if key not in _oracles:
        _oracles[key] = np.arange(t.nrows) if cond is None else n1o.run(t, cond, [], [], has_group=False).selected
    return _oracles[key]


def check(t, tkey, cond, keys, aggs, gpu, stats, val=None):
    ora = oracle(tkey, t, cond, keys, aggs)
    pu.assert_same_groups(gpu, ora, aggs=aggs)
    assert stats["rows_selected"] == ora.rows_passed
    if val and any(a.startswith(("sum(", "avg(")) for a in aggs):
        exact = gu.exact_sums(t, selected(tkey, t, cond), keys[0], val)
        assert gu.assert_float_sums_exact(gpu, exact, aggs, val) > 0 or not exact
    return ora


# --------------------------------------------------------------------------------------------------------------- scan path
PRICE = D("price")
SCAN_SHAPES = {
    # prebuilt Spec_gt_sum, DIRECT: 1002 slots x 4 LDS words (key + kLdsWordsSum) = 32 KB >= 4096: slabs on when automatic
    "direct": ("(50 < %s)" % PRICE, [D("cat")], ["sum(%s)" % PRICE], dict(k_cat=1000, zipf=True)),
    # the same shape over 37 categories: 1.2 KB, slabs off when automatic (choose_scan's use_slabs)
    "direct-small": ("(50 < %s)" % PRICE, [D("cat")], ["sum(%s)" % PRICE], dict(k_cat=37, zipf=True)),
    # prebuilt Spec_ik_sum, HASHED: user_id in [0, 100 000) gives ~63 k groups, more than the 2048 LDS slots
    "hashed": (None, [D("user_id")], ["sum(%s)" % PRICE], dict(k_cat=37, total_rows=1_000_000)),
    # no prebuilt kernel (built at run time); 1 + 4 + 4 LDS words per slot: 1024 bytes hold 14 slots, fewer than the 16
    # build_fast_args needs of a hashed table
    "hashed-jit": (None, [D("user_id")], sorted(["avg(%s)" % PRICE, "max(%s)" % PRICE]), dict(k_cat=37, total_rows=1_000_000)),
    "direct-jit": ("(%s < 30)" % PRICE, [D("cat")], sorted(["count(*)", "min(%s)" % PRICE]), dict(k_cat=1000, zipf=True)),
}
DIRECT, HASH = 2, 1  # N1K_MODE_LDS_DIRECT, N1K_MODE_LDS_HASH (include/n1k.h)
N_SCAN = 100_001  # odd: the WIDE form's last pair has one row


def _scan_cases():
    cases = []
    add = lambda shape, opts, mode, spec: cases.append(pytest.param(shape, opts, mode, spec, id="%s-%s" % (
        shape, "-".join("%s=%s" % kv for kv in opts.items()) or "default")))
    mode = {"direct": DIRECT, "direct-small": DIRECT, "hashed": HASH}
    for s in ("direct", "hashed"):
        # default options reach both tails of the speculative FinalGroup (n1k_finish.cpp small_tail_layout): "direct" (2048
        # table slots) finalize_small_kernel, "hashed" (262 144 slots) finalize_kernel + publish_counters_kernel
        add(s, {}, mode[s], 1)
        for b in G["block"]:  # the interpreter at every workgroup size (tile block x rows per lane; 4 below 1024)
            add(s, {"fast": 0, "block": b}, mode[s], 0)
        for b in (512, 1024):  # the specialised kernel's two sizes (256 is not one of them: auto, choose_scan's fblock)
            add(s, {"block": b}, mode[s], 1)
        for r in G["rows_per_lane"]:  # rows per lane: the interpreter at 1024 threads (choose_scan's rpl)
            add(s, {"fast": 0, "block": 1024, "rows_per_lane": r}, mode[s], 0)
        # grid_blocks: the grid itself, clipped to the tiles (launch_chunk, run_interpreter); 100 000 exceeds the 25 / 49 tiles
        for g in G["grid_blocks"]:
            add(s, {"grid_blocks": g}, mode[s], 1)
            add(s, {"fast": 0, "grid_blocks": g}, mode[s], 0)
        for rep in G["rep_row"]:  # representative rows: the interpreter only (build_fast_args refuses want_rep_row)
            add(s, {"rep_row": rep}, mode[s], 0 if rep else 1)
    for r in G["rows_per_lane"]:  # the bounded-shape kernel (spec off): tile 512 threads x rows per lane
        add("direct", {"spec": 0, "rows_per_lane": r}, DIRECT, 0)
    for sl in G["slabs"]:  # 0 off, 1 from 4096 table bytes on, 2 always (option slabs, choose_scan's use_slabs)
        add("direct", {"slabs": sl}, DIRECT, 1)
        add("direct", {"spec": 0, "slabs": sl}, DIRECT, 0)
    add("direct-small", {"slabs": 2}, DIRECT, 1)  # forced where the automatic choice is off
    for m in G["merge_chunks"]:  # merge_slabs_kernel rows per block (0: from the grid), with slabs on
        add("direct", {"slabs": 2, "merge_chunks": m}, DIRECT, 1)
        add("direct-small", {"slabs": 2, "merge_chunks": m, "grid_blocks": 3}, DIRECT, 1)
    for lb in G["lds_bytes"]:
        # 32 .. 2048 slots of 32 bytes.  163840 is clamped to 64 KiB (n1k_set_option): it used to ask the prebuilt kernel for
        # a 160 KiB table on top of its own LDS, and the launch failed
        add("hashed", {"lds_bytes": lb}, HASH, 1)
        # 1024: 14 slots of 72 bytes, the interpreter (build_fast_args: fewer than 16 slots)
        add("hashed-jit", {"jit": 2, "lds_bytes": lb}, HASH, 0 if lb == 1024 else 2)
        # the interpreter's DIRECT table takes 1002 x 32 bytes: below that the key domain does not fit, HASHED
        add("direct", {"fast": 0, "lds_bytes": lb}, DIRECT if lb >= 1002 * 32 else HASH, 0)
    for jm in G["jit_min_rows"]:  # jit=1: built at run time from jit_min_rows rows on (shape_kernel)
        add("direct-jit", {"jit": 1, "jit_min_rows": jm}, DIRECT, 2 if jm <= N_SCAN else 0)
        add("hashed-jit", {"jit": 1, "jit_min_rows": jm}, HASH, 2 if jm <= N_SCAN else 0)
    return cases


@pytest.mark.parametrize("shape,opts,mode,spec", _scan_cases())
def test_scan_geometry(shape, opts, mode, spec):
    cond, keys, aggs, kw = SCAN_SHAPES[shape]
    tkey = ("synth", N_SCAN, tuple(sorted(kw.items())))
    t = table("synth", N_SCAN, **kw)
    gpu, stats = pu.run_gpu(t, cond, keys, aggs, device_resident=True, **opts)
    ora = check(t, tkey, cond, keys, aggs, gpu, stats, val=PRICE)
    if shape.startswith("hashed"):
        assert len(ora.keys) > 8192  # more groups than any of the LDS tables holds
    assert stats["agg_mode"] == mode
    assert stats["spec_kernel"] == spec
    if opts.get("rep_row"):
        _check_rep_rows(t, tkey, cond, keys, gpu)


def _check_rep_rows(t, tkey, cond, keys, gpu):
    """The representative row of a group is its smallest passing row ordinal (execution/group_initial.go:69-72)."""
    sel = np.asarray(selected(tkey, t, cond), dtype=np.int64)
    by = {c.name: c for c in t.columns}
    kc = by[keys[0]]
    first = {}
    for r in sel.tolist():
        k = pu._canon_key((gu._key_of(kc, t.dictionary, r),))
        if k not in first:
            first[k] = r
    assert gpu.rep_row is not None and len(gpu.rep_row) == len(gpu.keys)
    for k, r in zip(gpu.keys, gpu.rep_row):
        assert first[pu._canon_key(k)] == int(r), (k, int(r))


# Tails.  The specialised scan's tile is BLOCK x R items, two rows per item in the WIDE form (n1k_kernels.hip launch_spec:
# R = 2): 2048 rows at 512 threads, 4096 at 1024; the bounded-shape kernel's 512 x 4 rows, the interpreter's 1024 x 4.  At
# grid_blocks = 3 the rows 2 * 3 * tile +- 1 put the second in-flight tile just past / just before the end (issued
# unconditionally and dropped, n1k_spec.h:266, :505).
TAIL_GEOMS = {
    "spec512": ("direct", {"block": 512, "grid_blocks": 3}, 2048, 1),
    "spec1024": ("direct", {"block": 1024, "grid_blocks": 3}, 4096, 1),
    "spec-hashed": ("hashed", {"grid_blocks": 3}, 2048, 1),
    "bounded": ("direct", {"spec": 0, "grid_blocks": 3}, 2048, 0),
    "interp": ("direct", {"fast": 0, "block": 1024, "grid_blocks": 3}, 4096, 0),
    "jit": ("direct-jit", {"jit": 2, "grid_blocks": 3}, 2048, 2),
}


def _tail_sizes(tile, grid=3):
    return [1, tile - 1, tile, tile + 1, 2 * grid * tile - 1, 2 * grid * tile + 1]


@pytest.mark.parametrize("geom,n", [(g, n) for g in TAIL_GEOMS for n in _tail_sizes(TAIL_GEOMS[g][2])])
def test_scan_tails(geom, n):
    shape, opts, _, spec = TAIL_GEOMS[geom]
    cond, keys, aggs, kw = SCAN_SHAPES[shape]
    big = table("synth", 30_000, **kw)
    t = big.slice(0, n)
    tkey = ("synth-slice", n, tuple(sorted(kw.items())))
    gpu, stats = pu.run_gpu(t, cond, keys, aggs, device_resident=True, **opts)
    check(t, tkey, cond, keys, aggs, gpu, stats, val=PRICE)
    assert stats["spec_kernel"] == spec


@pytest.mark.parametrize("geom", ["spec512", "bounded"])
def test_scan_tails_unaligned_columns(geom):
    """Columns that start one row into their allocation: no 16-byte loads (the scalar form), at 2 * grid * tile + 1 rows."""
    import torch
    shape, opts, tile, _ = TAIL_GEOMS[geom]
    cond, keys, aggs, kw = SCAN_SHAPES[shape]
    n = 2 * 3 * tile + 1
    big = table("synth", 30_000, **kw)
    t = big.slice(1, n + 1)
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs), **opts)
    try:
        op.intern(list(big.dictionary))
        by = {c.name: c for c in big.columns}
        keep, dev = [], []
        for p in op.column_paths:
            c = by[p]
            if c.kind == n1o.COL_DICT32:
                x = torch.from_numpy(np.ascontiguousarray(c.codes[:n + 1]).view(np.int32)).cuda()
                keep.append(x)
                dev.append((_ffi.COL_DICT32, None, None, x.data_ptr() + 4))
            else:
                a = torch.from_numpy(np.ascontiguousarray(c.tags[:n + 1])).cuda()
                b = torch.from_numpy(np.ascontiguousarray(c.payload[:n + 1]).view(np.int64)).cuda()
                keep += [a, b]
                dev.append((_ffi.COL_TAGGED64, a.data_ptr() + 1, b.data_ptr() + 8, None))
        torch.cuda.synchronize()
        op.process_device_items(n, dev)
        gpu = op.after_items()
        stats = op.stats()
    finally:
        op.done()
    check(t, ("synth-unaligned", n, tuple(sorted(kw.items()))), cond, keys, aggs, gpu, stats, val=PRICE)


# Filter-only plans: here grid_blocks is a factor per CU, not a grid — the one-comparison kernel runs
# min(tiles, CUs x grid_blocks) workgroups of 8192-row tiles (filter_stream_grid).  At 2.2 M rows there are 269 tiles: 1 gives
# 256 workgroups where the default 5 gives 269; 3 and 100 000 are clipped to the tiles.
@pytest.mark.parametrize("gb", G["grid_blocks"])
def test_filter_only_grid_blocks_is_per_cu(gb):
    n = 2_200_001
    t = table("synth", n, k_cat=37)
    cond = "(50 < %s)" % PRICE
    gpu, stats = pu.run_gpu(t, cond, [], [], filter_only=True, grid_blocks=gb)
    sel = selected(("synth", n, (("k_cat", 37),)), t, cond)
    assert stats["spec_kernel"] == 1  # the one-comparison kernel
    assert stats["rows_selected"] == len(sel)
    assert np.array_equal(np.asarray(gpu.selected, dtype=np.uint64), np.asarray(sel, dtype=np.uint64))


# ------------------------------------------------------------------------------------------------ records path (agg_mode 4)
V = D("v")
REC_KEYS = [D("k")]
REC_KINDS = {  # each single aggregate kind fixed at compile time in agg_bins16_kernel, and the generic kernel (KIND -1)
    "sum": ["sum(%s)" % V], "avg": ["avg(%s)" % V], "count": ["count(%s)" % V], "countn": ["countn(%s)" % V],
    "min": ["min(%s)" % V], "max": ["max(%s)" % V], "generic": sorted(["count(*)", "max(%s)" % V, "sum(%s)" % V]),
}
REC_MULTI = REC_KINDS["generic"]
N_REC = 300_000


def _run_records(t, tkey, aggs, cond=None, **opts):
    gpu, stats = pu.run_gpu(t, cond, REC_KEYS, aggs, agg_mode=4, jit=2, **opts)
    check(t, tkey, cond, REC_KEYS, aggs, gpu, stats, val=V if t.nrows <= N_REC else None)
    assert stats["agg_mode"] == 4
    assert stats["spec_kernel"] != 0, "the records path fell back to the exact partitioned path"
    return stats


# all 28 instantiations agg_bins16_kernel<BLOCK, U, KIND> (n1k_bins.hip:436-452).  rec_bins = 1: 256 bins of ~1170 records,
# against chunks of BLOCK x U = 512 .. 2048 records — every bin ends in a partial chunk, at a different place in it.
@pytest.mark.parametrize("kind", sorted(REC_KINDS))
@pytest.mark.parametrize("unroll", G["rec_unroll"])
@pytest.mark.parametrize("block", G["rec_block"])
def test_records_agg_bins16_instantiations(block, unroll, kind):
    aggs = REC_KINDS[kind]
    t = table("records", N_REC)
    _run_records(t, ("records", N_REC), aggs, rec_block=block, rec_unroll=unroll, rec_bins=1,
                 **({"agg_spec": 0} if kind == "generic" else {}))


# Bins per region: automatic at 300 000 rows is 4 (groups = rows, want_bins = n / (slots / 2) + 1 = 586 with 512 slots,
# n1k_partitioned.cpp:242-246); every value here differs from it.
@pytest.mark.parametrize("bins", G["rec_bins"])
def test_records_bins_per_region(bins):
    t = table("records", N_REC)
    _run_records(t, ("records", N_REC), REC_MULTI, rec_bins=bins)


# Workgroups per region of radix_scatter_sub_kernel: min(value, region_tiles) with region_tiles = (n / 256 + 4095) / 4096 + 8
# = 9 at 300 000 rows (n1k_partitioned.cpp:299-303), so 1, 3 and 9 all take effect.  The automatic choice is 8 below ~19 M
# rows (every default case runs it); 9 is more workgroups than sub-regions, what the automatic choice gives past that.
@pytest.mark.parametrize("slices", G["rec_slices"])
def test_records_slices_per_region(slices):
    t = table("records", N_REC)
    _run_records(t, ("records", N_REC), REC_MULTI, rec_slices=slices)


# The records scan's grid: min(CUs x per_cu, tiles of 2048 rows) rounded up to 8 (n1k_partitioned.cpp:233-235).  At 1.6 M
# rows (782 tiles) 1, 3 and 8 give 256, 768 and 784 workgroups, the default 2 gives 512.  Regions of ~6250 records are
# more than one 4096-record tile of the radix scatter: with one workgroup per region it walks the second tile's tail.
N_REC_BIG = 1_600_001


@pytest.mark.parametrize("per_cu,slices", [(p, 0) for p in G["rec_scan_per_cu"]] + [(0, 1)])
def test_records_scan_grid_and_scatter_tiles(per_cu, slices):
    t = table("records", N_REC_BIG)
    _run_records(t, ("records", N_REC_BIG), ["sum(%s)" % V], rec_scan_per_cu=per_cu, rec_slices=slices)


# Per-bin LDS slots: halved while slots x LDS words x 8 > 64 KB (n1k_partitioned.cpp:239-241).  COUNT(*) has 2 words per slot:
# 64 and 256 stay, 8192 becomes 4096; the default is 1024.
@pytest.mark.parametrize("slots", G["rec_slots"])
def test_records_lds_slots(slots):
    t = table("records", N_REC)
    _run_records(t, ("records", N_REC), ["count(*)"], rec_slots=slots)


# The records scan's tile: 512 threads x 2 items x 2 rows = 2048 rows (n1k_kernels.hip launch_spec_records).  With one
# workgroup per CU the grid is 256 (a multiple of 8): 2 x 256 x 2048 +- 1 rows put its second in-flight tile past the end.
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 2 * 256 * 2048 - 1, 2 * 256 * 2048 + 1])
def test_records_scan_tails(n):
    big = table("records", 2 * 256 * 2048 + 1)
    t = big.slice(0, n)
    _run_records(t, ("records-slice", n), REC_MULTI, rec_scan_per_cu=1)


def test_records_skewed_table_falls_back_exactly():
    """One key holds 35 % of the rows: its hash region overflows, the batch takes the exact partitioned path, and the
    survivor count the records scan had added is undone (n1k_partitioned.cpp:264, :348) — exactly the oracle's."""
    cond = "(10 < %s)" % D("k")
    plain = table("records", 200_000, big_ints=False)
    _run_records(plain, ("records", 200_000, "plain"), REC_MULTI, cond=cond)  # control: the records path takes this shape
    t = table("records", 200_000, big_ints=False, hot_share=0.35)
    gpu, stats = pu.run_gpu(t, cond, REC_KEYS, REC_MULTI, agg_mode=4, jit=2)
    check(t, ("records", 200_000, "hot"), cond, REC_KEYS, REC_MULTI, gpu, stats, val=V)
    assert stats["agg_mode"] == 4 and stats["spec_kernel"] == 0  # the exact path ran


def test_records_batch_sequence_on_one_handle():
    """A batch whose records region is kept pending, an overflowing batch, a batch of one row, an empty batch."""
    a = gu.records_table(100_000, seed=1, big_ints=False)
    b = gu.records_table(100_000, seed=2, big_ints=False, hot_share=0.35)
    c = gu.records_table(6, seed=3, big_ints=False).slice(0, 1)
    e = a.slice(0, 0)
    whole = gu.concat([a, b, c])
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(None, REC_KEYS, REC_MULTI), agg_mode=4, jit=2)
    try:
        spec = []
        for part in (a, b, c, e):
            by = {x.name: x for x in part.columns}
            op.process_items([by[p] for p in op.column_paths], part.dictionary, rows=part.nrows)
            spec.append(op.stats()["spec_kernel"])
        gpu = op.after_items()
        stats = op.stats()
    finally:
        op.done()
    assert spec[0] != 0 and spec[1] == 0, spec  # records path, then the overflow's fall-back
    check(whole, ("records-seq",), None, REC_KEYS, REC_MULTI, gpu, stats, val=V)


# --------------------------------------------------------------------------------------------------------- COUNT(DISTINCT)
DISTINCT_SHAPES = {"one-pass": dict(n=120_000, nvals=40_000, ngroups=7), "two-pass": dict(n=900_000, nvals=700_000, ngroups=50)}
DISTINCT_AGGS = sorted(["count(distinct %s)" % V, "count(%s)" % V])


def _run_distinct(shape, **opts):
    kw = DISTINCT_SHAPES[shape]
    t = table("distinct", kw["n"], nvals=kw["nvals"], ngroups=kw["ngroups"])
    gpu, stats = pu.run_gpu(t, None, [D("g")], DISTINCT_AGGS, batches=2, **opts)
    check(t, ("distinct", shape), None, [D("g")], DISTINCT_AGGS, gpu, stats)
    assert stats["distinct_path"] & 2  # radix partition + per-bin LDS sets: distinct_dedupe_kernel ran


# distinct_dedupe_kernel<B, U, TOGETHER> (n1k_kernels.hip:3225-3228): 256 -> <256, 8>, 512 -> <512, 4>, 1024 -> <1024, 2> or
# <1024, 4> with dedupe_unroll = 4; +1 probes word by word (TOGETHER = false).  The 12 pairs reach all 8 instantiations.
@pytest.mark.parametrize("unroll", G["dedupe_unroll"])
@pytest.mark.parametrize("block", G["dedupe_block"])
@pytest.mark.parametrize("shape", sorted(DISTINCT_SHAPES))
def test_distinct_dedupe_instantiations(shape, block, unroll):
    _run_distinct(shape, dedupe_block=block, dedupe_unroll=unroll)


# A final bin's expected words in % of the 8192 slots (n1k_distinct.cpp:36): 1 % (81 words) adds a partition pass to both
# shapes, 75 % lets bins fill to three quarters.
@pytest.mark.parametrize("pct", G["distinct_fill_pct"])
@pytest.mark.parametrize("shape", sorted(DISTINCT_SHAPES))
def test_distinct_fill_pct(shape, pct):
    _run_distinct(shape, distinct_fill_pct=pct)


# ----------------------------------------------------------------------------------------------- row-exchange partition
# The run-time-built partition kernel: 256-thread workgroups (tiles of 1024 rows) or 512 (2048 rows), min(CUs x per_cu,
# tiles) of them (n1k_exchange.cpp:55-57).  At 2.2 M rows: 2149 / 1075 tiles, so 1, 2 and 8 per CU give 256, 512 and 2048 /
# 1075 workgroups (defaults: 6 per CU at 256, 2 at 512).
N_PART = 2_200_001
PART_COND = "(50 < %s)" % PRICE
PART_AGGS = sorted(["count(*)", "sum(%s)" % PRICE, "max(%s)" % D("user_id")])


@pytest.mark.parametrize("per_cu", G["part_per_cu"])
@pytest.mark.parametrize("block", G["part_block"])
def test_partition_kernel_geometry(block, per_cu):
    import torch
    nparts = 3
    keys = [D("cat")]
    t = table("synth", N_PART, k_cat=29, zipf=True)
    tkey = ("synth", N_PART, (("k_cat", 29), ("zipf", True)))
    sender = query_amd.GpuFilterGroup(plan.filter_group_plan(PART_COND, keys, PART_AGGS), jit=2, part_block=block, part_per_cu=per_cu)
    try:
        sender.intern(list(t.dictionary))
        paths = sender.column_paths
        by = {c.name: c for c in t.columns}
        keep, cols = [], []
        for p in paths:
            c = by[p]
            if c.kind == n1o.COL_DICT32:
                x = torch.from_numpy(c.codes.view(np.int32)).cuda()
                keep.append(x)
                cols.append((_ffi.COL_DICT32, None, None, x.data_ptr()))
            else:
                a = torch.from_numpy(c.tags).cuda()
                b = torch.from_numpy(c.payload.view(np.int64)).cuda()
                keep += [a, b]
                cols.append((_ffi.COL_TAGGED64, a.data_ptr(), b.data_ptr(), None))
        n = t.nrows
        batch, arr = sender._make_batch(n, cols)
        out = (_ffi.Col * len(cols))()
        bufs = []
        for i, c in enumerate(cols):
            out[i].kind = c[0]
            if c[0] == _ffi.COL_DICT32:
                b = torch.zeros(n * nparts, dtype=torch.int32, device="cuda")
                out[i].codes = b.data_ptr()
                bufs.append((b,))
            else:
                a = torch.zeros(n * nparts, dtype=torch.uint8, device="cuda")
                b = torch.zeros(n * nparts, dtype=torch.int64, device="cuda")
                out[i].tags, out[i].payload = a.data_ptr(), b.data_ptr()
                bufs.append((a, b))
        counts = torch.zeros(nparts, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        sender._check(sender._lib.n1k_partition_device_batch(sender._h, C.byref(batch), nparts, n, out, counts.data_ptr()))
        assert sender.stats()["spec_kernel"] != 0  # the run-time-built kernel, not the interpreting one
        cnt = counts.cpu().numpy()
        assert int(cnt.sum()) == len(selected(tkey, t, PART_COND))  # every survivor exactly once
        seen, mk, ma = {}, [], []
        for d in range(nparts):
            recv = query_amd.GpuFilterGroup(plan.filter_group_plan(None, keys, PART_AGGS))
            try:
                recv.intern(list(t.dictionary))
                rcols = []
                for p in recv.column_paths:
                    i = paths.index(p)
                    if cols[i][0] == _ffi.COL_DICT32:
                        rcols.append((_ffi.COL_DICT32, None, None, bufs[i][0].data_ptr() + 4 * d * n))
                    else:
                        rcols.append((_ffi.COL_TAGGED64, bufs[i][0].data_ptr() + d * n, bufs[i][1].data_ptr() + 8 * d * n, None))
                recv.process_device_items(int(cnt[d]), rcols)
                rows = recv.after_items()
            finally:
                recv.done()
            for k, a in zip(rows.keys, rows.aggs):
                assert k not in seen, "group %r landed in two parts" % (k,)
                seen[k] = d
                mk.append(k)
                ma.append(a)
    finally:
        sender.done()
    from query_amd.gpu_operator import GroupRows
    pu.assert_same_groups(GroupRows(len(keys), len(PART_AGGS), mk, ma, []), oracle(tkey, t, PART_COND, keys, PART_AGGS),
                          aggs=PART_AGGS)
