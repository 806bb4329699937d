"""The tuning options of n1k_set_option (query_amd/csrc/n1k_engine.cpp) and where each one is checked against the oracle.

Every option name the engine accepts is in exactly one of three tables:
  GEOMETRY  option -> the values test_gpu_geometries.py runs (each one a kernel instantiation, launch geometry or path)
  COVERED   option -> the existing test that already sets it
  EXEMPT    option -> why no oracle check applies
test_options_cpu.py parses the engine and fails when a new option is in none of them.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import n1o
from query_amd import plan as qplan

GEOMETRY = {
    # scan (DIRECT / HASHED group tables, Filter-only plans)
    "block": (0, 256, 512, 1024),
    "rows_per_lane": (2, 4),
    "grid_blocks": (1, 3, 100_000),
    "slabs": (0, 1, 2),
    "merge_chunks": (0, 1, 3, 16),
    "lds_bytes": (1024, 4096, 65536, 163840),
    "jit_min_rows": (0, 1 << 40),
    "rep_row": (0, 1),
    # records / per-bin tables (agg_mode 4)
    "rec_block": (256, 512),
    "rec_unroll": (2, 4),
    "rec_bins": (1, 2, 16, 256),
    "rec_slices": (1, 3, 9),
    "rec_scan_per_cu": (1, 3, 8),
    "rec_slots": (64, 256, 8192),
    # COUNT(DISTINCT) de-duplication
    "dedupe_block": (256, 257, 512, 513, 1024, 1025),
    "dedupe_unroll": (0, 4),
    "distinct_fill_pct": (1, 25, 75),
    # row-exchange partition kernel
    "part_block": (256, 512),
    "part_per_cu": (1, 2, 8),
}

COVERED = {
    "agg_mode": "tests/test_gpu_parity.py::test_every_kernel_variant_agrees_with_the_oracle",
    "max_groups": "tests/test_gpu_parity.py::test_error_paths_are_reported_not_silent",
    "fast": "tests/test_gpu_parity.py::test_every_kernel_variant_agrees_with_the_oracle",
    "spec": "tests/test_gpu_parity.py::test_every_kernel_variant_agrees_with_the_oracle",
    "wide": "tests/test_gpu_parity.py::test_every_kernel_variant_agrees_with_the_oracle",
    "fuse_arith": "tests/test_gpu_parity.py::test_arithmetic_fused_into_the_runtime_built_scan",
    "lean_topk": "tests/test_gpu_parity.py::test_topk_over_the_partitioned_paths_kept_region",
    "topk_sample": "tests/test_gpu_parity.py::test_topk_threshold_from_a_sample",
    "topk_min_groups": "tests/test_gpu_parity.py::test_device_topk_filter_feeds_the_exact_order",
    "agg_spec": "tests/test_gpu_parity.py::test_per_bin_tables_over_16_byte_records",
    "records": "tests/test_gpu_fullsize.py::test_full_size_config5_own_query",
    "jit": "tests/test_gpu_parity.py::test_runtime_specialised_kernels_agree_with_the_oracle",
    "part_subs": "tests/test_gpu_distributed.py::test_rank_pipeline_world1_rccl",
    "distinct_words": "tests/test_gpu_parity.py::test_count_distinct_paths",
    "distinct_set_slots": "tests/test_gpu_parity.py::test_count_distinct_paths",
    "distinct_levels": "tests/test_gpu_parity.py::test_count_distinct_in_the_specialised_scan",
    "distinct_region_cap": "tests/test_gpu_parity.py::test_count_distinct_in_the_specialised_scan",
    "partition_min_rows": "tests/test_gpu_parity.py::test_partitioned_path_is_chosen_from_the_data",
    "partition_probe_rows": "tests/test_gpu_parity.py::test_partitioned_path_is_chosen_from_the_data",
    "partition_min_groups": "tests/test_gpu_parity.py::test_partitioned_path_is_chosen_from_the_data",
    "partition_levels": "tests/test_gpu_parity.py::test_partitioned_high_cardinality_group_by",
    "wide_values": "tests/test_gpu_parity.py::test_wide_key_value_table_overflow_is_reported",
    "json_device": "tests/test_gpu_parity.py::test_device_json_extractor_against_the_host_extractor",
    "json_device_left_pct": "tests/test_gpu_parity.py::test_device_json_extractor_against_the_host_extractor",
    "json_device_min_docs": "tests/test_gpu_parity.py::test_device_json_extractor_against_the_host_extractor",
    "json_threads": "tests/test_json_extract_cpu.py::test_threads_agree_and_share_one_dictionary",
}

EXEMPT = {
    "device": "picks the GPU; every test runs on device 0",
    "stream": "the caller's stream; no kernel or geometry of its own",
    "inject_failure": "fault injection of the row exchange, covered by its failure tests in test_gpu_distributed.py",
    "partition_sticky": "reuses the previous execution's probe decision; the path it picks is the partitioned one checked here",
}

# values the engine documents as refused (N1K_INVALID)
REFUSED = {"block": 128, "rows_per_lane": 3, "dedupe_block": 300}


def D(*names):
    return qplan.field_path("default", *names)


def records_table(n, seed=7, big_ints=True, key_range=None, hot_share=0.0):
    """(k, v): an int key with about six rows per group (`key_range` overrides) and ONE operand column holding every kind of
    value the per-bin tables meet: small ints, ints >= 2^40 (they leave the narrow LDS sum as partial groups of their own),
    floats, NULL / MISSING, a boolean and a string now and then.  `hot_share` of the rows get the largest key (a skewed table)."""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, key_range or max(1, n // 6), n).astype(np.int64)
    if hot_share:
        key[rng.random(n) < hot_share] = max(1, n // 6) - 1
    kind = rng.integers(0, 100, n)
    tags = np.full(n, n1o.T_INT, np.uint8)
    pay = rng.integers(-1000, 1000, n).astype(np.int64).view(np.uint64).copy()
    if big_ints:
        big = kind < 3
        pay[big] = (rng.integers(1, 1 << 20, big.sum()).astype(np.int64) << 41).view(np.uint64)
    fl = (kind >= 3) & (kind < 40)
    tags[fl] = n1o.T_FLOAT
    pay[fl] = np.round(rng.uniform(-50, 50, fl.sum()), 3).view(np.uint64)
    tags[(kind >= 40) & (kind < 45)] = n1o.T_NULL
    tags[(kind >= 45) & (kind < 50)] = n1o.T_MISSING
    tags[kind == 50] = n1o.T_TRUE
    st = kind == 51
    tags[st] = n1o.T_STRING
    pay[st] = rng.integers(0, 3, st.sum()).astype(np.uint64)
    pay[(tags == n1o.T_NULL) | (tags == n1o.T_MISSING) | (tags == n1o.T_TRUE)] = 0
    return n1o.Table([n1o.Column(D("k"), n1o.COL_TAGGED64, tags=np.full(n, n1o.T_INT, np.uint8), payload=key.view(np.uint64)),
                      n1o.Column(D("v"), n1o.COL_TAGGED64, tags=tags, payload=pay)], [b"a", b"b", b"c"])


def _key_of(col, dictionary, i):
    if col.kind == n1o.COL_DICT32:
        return (n1o.T_STRING, dictionary[int(col.codes[i])])
    tag = int(col.tags[i])
    if tag == n1o.T_INT:
        return (tag, int(col.payload[i:i + 1].view(np.int64)[0]))
    if tag == n1o.T_FLOAT:
        return (tag, float(col.payload[i:i + 1].view(np.float64)[0]))
    return (tag, int(col.payload[i]))


def exact_sums(table, selected, key_name, val_name):
    """Per group key (canonical, as parity_util compares keys): (math.fsum of the numeric operands, their count, sum of |x|)
    over the rows in `selected` — the exact reference a float SUM / AVG is bounded against."""
    import parity_util as pu
    by = {c.name: c for c in table.columns}
    kc, vc = by[key_name], by[val_name]
    sel = np.asarray(selected, dtype=np.int64)
    vt = vc.tags[sel]
    num = (vt == n1o.T_INT) | (vt == n1o.T_FLOAT)
    rows = sel[num]
    vals = np.where(vc.tags[rows] == n1o.T_INT, vc.payload[rows].view(np.int64).astype(object),
                    vc.payload[rows].view(np.float64).astype(object))
    groups = {}
    for r, x in zip(rows.tolist(), vals.tolist()):
        groups.setdefault(pu._canon_key((_key_of(kc, table.dictionary, r),)), []).append(x)
    return {k: (math.fsum(xs), len(xs), math.fsum(abs(x) for x in xs)) for k, xs in groups.items()}


def assert_float_sums_exact(gpu, exact, aggs, val_name):
    """Every SUM / AVG of the operand against the exact sum: |gpu - exact| <= n 2^-53 sum|x| (whatever order the kernel's
    geometry adds the n terms in; AVG: the same over n plus the division's rounding).  Holds where the data cancel and a
    relative tolerance means nothing."""
    import parity_util as pu
    checked = 0
    for i, a in enumerate(aggs):
        kind = a.split("(")[0]
        if kind not in ("sum", "avg") or val_name not in a:
            continue
        for k, ga in zip(gpu.keys, gpu.aggs):
            ck = pu._canon_key(k)
            if ck not in exact:  # (no numeric operand in the group: the oracle comparison checks its NULL)
                continue
            s, n, mag = exact[ck]
            tag, v = ga[i]
            assert tag in (n1o.T_INT, n1o.T_FLOAT), (a, k, ga[i])
            bound = n * 2.0 ** -53 * mag
            if kind == "sum":
                assert abs(float(v) - s) <= bound + (abs(s) * 2.0 ** -53), (a, k, v, s, bound)
            else:
                want = s / n
                assert abs(float(v) - want) <= bound / n + abs(want) * 2.0 ** -52, (a, k, v, want, bound)
            checked += 1
    return checked


def distinct_table(n, nvals, ngroups, seed=3, wide_share=0.1):
    """(g, v) for COUNT(DISTINCT v): v mostly small ints (one-word members), plus floats / huge ints / strings (two-word
    pairs) and NULLs — the data of test_gpu_parity.py::test_count_distinct_paths."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, ngroups, n).astype(np.uint64)
    tags = np.full(n, n1o.T_INT, np.uint8)
    pay = (rng.integers(0, nvals, n) - nvals // 3).astype(np.int64).view(np.uint64).copy()
    w = rng.random(n) < wide_share
    kind = rng.integers(0, 4, n)
    fl = w & (kind == 0)
    tags[fl] = n1o.T_FLOAT
    pay[fl] = (rng.integers(0, nvals, int(fl.sum())) + 0.5).view(np.uint64)
    big = w & (kind == 1)
    pay[big] = (rng.integers(0, 50, int(big.sum())).astype(np.int64) * np.int64(2 ** 55)).view(np.uint64)
    st = w & (kind == 2)
    tags[st] = n1o.T_STRING
    pay[st] = rng.integers(0, 3, int(st.sum())).astype(np.uint64)
    nul = w & (kind == 3)
    tags[nul] = n1o.T_NULL
    pay[nul] = 0
    return n1o.Table([n1o.Column(D("g"), n1o.COL_TAGGED64, tags=np.full(n, n1o.T_INT, np.uint8), payload=g),
                      n1o.Column(D("v"), n1o.COL_TAGGED64, tags=tags, payload=pay)], [b"x", b"y", b"z"])


def concat(tables):
    """Row-wise concatenation of tables with the same columns and dictionary."""
    cols = []
    for i, c in enumerate(tables[0].columns):
        parts = [t.columns[i] for t in tables]
        if c.kind == n1o.COL_DICT32:
            cols.append(n1o.Column(c.name, c.kind, codes=np.concatenate([p.codes for p in parts])))
        else:
            cols.append(n1o.Column(c.name, c.kind, tags=np.concatenate([p.tags for p in parts]),
                                   payload=np.concatenate([p.payload for p in parts])))
    return n1o.Table(cols, tables[0].dictionary)
