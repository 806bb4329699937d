"""Nothing is left behind: every owner of device memory in the host engine gives back exactly what it took.

n1k_device_bytes_live() is the library's own count of the device bytes it holds (added where it allocates, subtracted where
it frees; the device's free memory would move under other processes' work).  Each case records it, creates an operator,
runs one small query to its result through the path that owns a set of buffers — the plans and option settings are those
by which test_gpu_geometries.py, test_gpu_capacities.py and test_gpu_parity.py force the path at small sizes, and the
statistics say that it ran — requires the count to be ABOVE the recorded value while the operator lives (a count of nothing
would pass everything else), destroys the operator and requires the recorded value back, exactly.
"""
import ctypes as C
import gc
import threading

import numpy as np
import pytest

import coll_util as cu
import geometry_util as gu
import in_util as iu
import json_util as ju
import query_amd
import strfn_util as su
from geometry_util import D
from oracle import n1o
from query_amd import _ffi, plan

pytestmark = pytest.mark.gpu

PRICE = D("price")


def live() -> int:
    return int(_ffi.lib().n1k_device_bytes_live())


class Accounted:
    """with Accounted() as acc: ... acc.own(op) ...: `alive()` inside, while the operators exist; on exit they are destroyed
    (after a gc.collect()) and the count must be back where it was."""

    def __enter__(self):
        gc.collect()
        self.before = live()
        self.owned = []
        return self

    def own(self, x):
        self.owned.append(x)
        return x

    def alive(self):
        assert live() > self.before, "the operator holds device memory and the count does not show it"

    def __exit__(self, et, ev, tb):
        gc.collect()
        for x in self.owned:
            x.done()
        if et is None:
            assert live() == self.before, "device bytes left behind: %d" % (live() - self.before)
        return False


def push(op, t):
    by = {c.name: c for c in t.columns}
    op.process_items([by[p] for p in op.column_paths], t.dictionary, rows=t.nrows)


def run_host(acc, t, cond, keys, aggs, filter_only=False, batches=1, **kw):
    """One operator over host batches (the staging sets) to its result: (rows, stats), the operator still alive."""
    tail = {k: kw.pop(k) for k in ("order", "limit", "offset", "having", "project") if k in kw}
    op = acc.own(query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs, filter_only=filter_only, **tail), **kw))
    step = (t.nrows + batches - 1) // batches
    for lo in range(0, t.nrows, step):
        push(op, t.slice(lo, min(t.nrows, lo + step)))
    rows = op.after_items()
    acc.alive()
    return op, rows, op.stats()


def test_scan_group_by_with_slabs():
    t = n1o.synth_table(5_001, k_cat=1000, zipf=True)
    with Accounted() as acc:
        _, rows, st = run_host(acc, t, "(50 < %s)" % PRICE, [D("cat")], ["sum(%s)" % PRICE], slabs=2)
        assert st["agg_mode"] == 2 and st["spec_kernel"] == 1 and len(rows.keys) > 1


@pytest.mark.parametrize("opts,path", [({"jit": 2}, 3), ({"distinct_words": 0}, 1)], ids=["member-word-regions", "pair-log"])
def test_count_distinct(opts, path):
    t = gu.distinct_table(3_000, 50, 4)
    aggs = sorted(["count(distinct %s)" % D("v"), "count(%s)" % D("v")])
    with Accounted() as acc:
        _, rows, st = run_host(acc, t, None, [D("g")], aggs, batches=2, **opts)
        assert st["distinct_path"] == path and len(rows.keys) == 4
        if "jit" in opts:
            assert st["spec_kernel"] == 2  # the specialised scan: member words into the hash regions


@pytest.mark.parametrize("records", [1, 0])
def test_partitioned_group_by(records):
    t = gu.records_table(6_000, big_ints=False)
    with Accounted() as acc:
        _, rows, st = run_host(acc, t, None, [D("k")], sorted(["count(*)", "sum(%s)" % D("v")]), agg_mode=4, jit=2, records=records)
        assert st["agg_mode"] == 4 and len(rows.keys) > 500
        assert (st["spec_kernel"] != 0) == bool(records)  # the 16-byte records, or the three-array records of the exact path


def test_order_by_limit_through_the_device_topk():
    t = n1o.synth_table(8_000, k_cat=120)
    keys, aggs = [D("cat"), D("region_id")], sorted(["count(*)", "sum(%s)" % PRICE])
    with Accounted() as acc:
        _, rows, st = run_host(acc, t, None, keys, aggs, order=[("sum(%s)" % PRICE, True)], limit=10, topk_min_groups=1)
        assert len(rows.keys) == 10 and st["topk_candidates"] > 0


def test_having_and_projection_inner_handles():
    t = n1o.synth_table(4_000, k_cat=90)
    aggs = sorted(["count(*)", "sum(%s)" % PRICE])
    with Accounted() as acc:
        _, rows, _ = run_host(acc, t, None, [D("cat")], aggs, having="(1 < count(*))",
                              project=[(D("cat"), "c"), ("round(sum(%s), 1)" % PRICE, "s")])
        assert rows.proj and len(rows.proj) == len(rows.keys) > 0


def test_filter_only_plan():
    t = n1o.synth_table(5_001, k_cat=37)
    with Accounted() as acc:
        _, rows, st = run_host(acc, t, "(50 < %s)" % PRICE, [], [], filter_only=True)
        assert 0 < len(rows.selected) == st["rows_selected"] < t.nrows


def test_push_json_through_the_device_extractor():
    docs = [ju.padded_doc(i, 96) for i in range(300)]
    with Accounted() as acc:
        op = acc.own(query_amd.GpuFilterGroup(ju.Channel([("s",)], [("x", "y")]).plan, json_device=1, json_device_min_docs=1))
        op.process_json(docs)
        raw = op.after_items_raw()
        acc.alive()
        assert raw["ngroups"] == len(docs) and op.stats()["json_device_docs"] > 0


def test_match_table_through_its_device_route():
    """One LIKE, one ANY, one IN and one string-function term over new dictionary entries at the device threshold of each."""
    terms = ['(%s like "%%7")' % D("s"), iu.term(D("s"), ["s7", "s70", "nope"]),
             su.term_text(D("s"), ([("upper", None)], ("like", "S1%5"))),
             cu.term_text(cu.ANY, ("cmp", "=", [], "t_1", False), over=D("a"))]
    with Accounted() as acc:
        op = acc.own(query_amd.GpuFilterGroup(plan.filter_group_plan("(%s)" % " or ".join(terms), [], ["count(*)"])))
        T = max(op.like_stats()["device_threshold"], op.in_stats()["device_threshold"], op.strfn_stats()["device_threshold"],
                op.coll_stats()["device_threshold"], 1024)
        strings = [b"s%d" % i for i in range(T)]
        arrays = cu.texts_of([["w%d" % i] + (["t_1"] if i % 3 == 0 else []) for i in range(T)])
        rows = 4_000
        rng = np.random.default_rng(1)
        cols = {D("s"): n1o.Column(D("s"), n1o.COL_DICT32, codes=rng.integers(0, T, rows).astype(np.uint32)),
                D("a"): n1o.Column(D("a"), n1o.COL_TAGGED64, tags=np.full(rows, n1o.T_ARRAY, np.uint8),
                                   payload=rng.integers(T, 2 * T, rows).astype(np.uint64))}
        op.process_items([cols[p] for p in op.column_paths], strings + arrays)
        assert 0 < op.after_items().aggs[0][0][1] < rows
        acc.alive()
        assert op.like_stats()["device_strings"] > 0 and op.in_stats()["device_strings"] > 0
        assert op.strfn_stats()["device_strings"] > 0 and op.coll_stats()["device_arrays"] > 0


def test_export_then_merge_of_groups_between_two_operators():
    t = n1o.synth_table(4_000, k_cat=90)
    pj = plan.filter_group_plan(None, [D("cat")], sorted(["count(*)", "sum(%s)" % PRICE]))
    with Accounted() as acc:
        a, b = acc.own(query_amd.GpuFilterGroup(pj)), acc.own(query_amd.GpuFilterGroup(pj))
        push(a, t)
        push(b, t.slice(0, 1))  # (merge needs the key layout)
        blob, ln = C.c_void_p(), C.c_size_t()
        a._check(a._lib.n1k_export_groups(a._h, C.byref(blob), C.byref(ln)))
        b._check(b._lib.n1k_merge_groups(b._h, blob, ln))
        ra, rb = a.after_items(), b.after_items()
        acc.alive()
        assert len(ra.keys) == len(rb.keys) > 1
        assert sum(x[0][1] for x in rb.aggs) == t.nrows + 1  # count(*): a's groups and b's one row


def test_two_rank_loopback_row_exchange_and_gather():
    import torch
    from query_amd import distributed as qd
    world, n = 2, 6_000
    t = n1o.synth_table(n, k_cat=61, zipf=True)
    cond, keys, aggs = "(50 < %s)" % PRICE, [D("cat")], sorted(["count(*)", "sum(%s)" % PRICE])
    want = len(n1o.run(t, cond, keys, aggs).keys)
    with Accounted() as acc:
        comms = qd.Comm.loopback(world, 0)
        ranks = [acc.own(qd.ShardedFilterGroup(cond, keys, aggs, t.dictionary, r, world, 0, comm=comms[r])) for r in range(world)]
        keep, shards = [], []
        for r in range(world):
            sub = t.slice(n * r // world, n * (r + 1) // world)
            dev = {}
            for c in sub.columns:
                if c.kind == n1o.COL_DICT32:
                    x = torch.from_numpy(np.ascontiguousarray(c.codes).view(np.int32)).cuda()
                    keep.append(x)
                    dev[c.name] = (_ffi.COL_DICT32, None, None, x.data_ptr())
                else:
                    a = torch.from_numpy(np.ascontiguousarray(c.tags)).cuda()
                    b = torch.from_numpy(np.ascontiguousarray(c.payload).view(np.int64)).cuda()
                    keep += [a, b]
                    dev[c.name] = (_ffi.COL_TAGGED64, a.data_ptr(), b.data_ptr(), None)
            shards.append((sub.nrows, dev))
        torch.cuda.synchronize()
        outs, errs = [None] * world, [None] * world

        def body(r):
            try:
                outs[r] = ranks[r].run_rows(*shards[r])
            except BaseException as e:  # noqa: BLE001 - raised below
                errs[r] = e

        ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
        for x in ts:
            x.start()
        for x in ts:
            x.join(timeout=60)
        for e in errs:
            if e is not None:
                raise e
        assert not any(x.is_alive() for x in ts), "a rank is stuck in a collective"
        acc.alive()
        assert all(o[0]["ngroups"] == want and o[1]["mode"] == "rows" for o in outs)


def test_destroy_after_push_without_finish():
    t = n1o.synth_table(5_001, k_cat=1000, zipf=True)
    with Accounted() as acc:
        op = acc.own(query_amd.GpuFilterGroup(plan.filter_group_plan("(50 < %s)" % PRICE, [D("cat")], ["sum(%s)" % PRICE])))
        push(op, t)
        acc.alive()
