"""SELECT DISTINCT over the rows of a Filter-only plan, de-duplicated on the device: the ordinals n1k_filter_device_batch
returns for such a plan against tests/distinct_util.py (the smallest surviving ordinal per distinct row of the result terms),
then tests/order_util.py for the tail — exactly: ordinals, not values, no tolerance.

Survivor counts sit at the edges of the kernels (wave = 64, tile T = 1024 survivors), with the optional LDS set ahead of the
table and without it; keys make a tile's LDS set hold one key, a key per row, more keys than it has slots, and put a key's
duplicate into another tile than its smallest ordinal; the table is forced full and one slot short.  Device memory comes from torch, the selection from the oracle."""
import numpy as np
import pytest
import torch

import distinct_util as du
import golden_util as gu
import order_util as ou
import query_amd
import test_gpu_random_plans as rp
from oracle import n1o
from query_amd import _ffi, plan

pytestmark = pytest.mark.gpu

D = lambda *n: plan.field_path("d", *n)
F, K, V, W, X, S = D("f"), D("k"), D("v"), D("w"), D("x"), D("s")
COND = "(0 < %s)" % F
T = 1024  # kRdTile
I = lambda x: (n1o.T_INT, int(x))
FL = lambda x: (n1o.T_FLOAT, float(x))

_state = {}


class Tab:
    """A table (column F = the Filter's flag, and named columns), its device copy, the oracle's selections by row count.  A
    column is a list of (tag, python value) pairs, an int64 array (INT values; distinct_util's vectorised form) or a uint32 array
    (DICT32 codes)."""

    def __init__(self, flags, cols, dictionary=()):
        n = len(flags)
        self.n, self.dictionary = n, [bytes(s) for s in dictionary]
        self.cols = {F: n1o.Column(F, n1o.COL_TAGGED64, tags=np.full(n, n1o.T_INT, np.uint8), payload=np.asarray(flags).astype(np.uint64))}
        self.values = {}
        for name, c in cols.items():
            if isinstance(c, np.ndarray) and c.dtype == np.int64:
                self.cols[name] = n1o.Column(name, n1o.COL_TAGGED64, tags=np.full(n, n1o.T_INT, np.uint8), payload=c.view(np.uint64).copy())
                self.values[name] = c
            elif isinstance(c, np.ndarray):
                self.cols[name] = n1o.Column(name, n1o.COL_DICT32, codes=c.astype(np.uint32))
                self.values[name] = ou.codes_values(c, self.dictionary)
            else:
                code = {s: i for i, s in enumerate(self.dictionary)}
                tags = np.array([v[0] for v in c], dtype=np.uint8)
                pay = np.zeros(n, dtype=np.uint64)
                for i, (t, x) in enumerate(c):
                    if t == n1o.T_INT:
                        pay[i] = x & 0xFFFFFFFFFFFFFFFF
                    elif t == n1o.T_FLOAT:
                        pay[i] = np.float64(x).view(np.uint64)
                    elif t >= n1o.T_STRING:
                        pay[i] = code[x]
                self.cols[name] = n1o.Column(name, n1o.COL_TAGGED64, tags=tags, payload=pay)
                self.values[name] = list(c)
        self.table = n1o.Table(list(self.cols.values()), self.dictionary)
        self.dev = {}
        for name, c in self.cols.items():
            if c.kind == n1o.COL_DICT32:
                self.dev[name] = (torch.from_numpy(np.ascontiguousarray(c.codes).view(np.int32)).cuda(),)
            else:
                self.dev[name] = (torch.from_numpy(np.ascontiguousarray(c.tags)).cuda(), torch.from_numpy(np.ascontiguousarray(c.payload).view(np.int64)).cuda())
        torch.cuda.synchronize()
        self._sel = {}

    def selected(self, n=None, cond=COND):
        n = self.n if n is None else n
        if cond is None:
            return np.arange(n, dtype=np.int64)
        if (n, cond) not in self._sel:
            self._sel[n, cond] = n1o.run(self.table.slice(0, n), cond, [], [], has_group=False).selected.astype(np.int64)
        return self._sel[n, cond]

    def spec(self, name):
        d = self.dev[name]
        return (_ffi.COL_DICT32, None, None, d[0].data_ptr()) if len(d) == 1 else (_ffi.COL_TAGGED64, d[0].data_ptr(), d[1].data_ptr(), None)

    def batch(self, op, n=None, names=None):
        return op.make_device_batch(self.n if n is None else n, [self.spec(p) for p in (op.column_paths if names is None else names)])


def make_op(tab, terms, order=None, offset=None, limit=None, cond=COND, **options):
    pj = plan.filter_group_plan(cond, [], [], filter_only=True, distinct=[t if isinstance(t, tuple) else (t, None) for t in terms],
                                order=order, offset=offset, limit=limit)
    op = query_amd.GpuFilterGroup(pj, **options)
    if tab.dictionary:
        codes = op.intern(tab.dictionary)
        assert np.array_equal(codes, np.arange(len(codes), dtype=np.uint32))
    return op


def answer(op, tab, n=None):
    nsel, addr = op.filter_device_batch(tab.batch(op, n))
    st = op.stats()
    assert (addr is None) == (nsel == 0) and st["rows_selected"] == nsel and st["rows_in"] == (tab.n if n is None else n)
    got = op.selected_host32()
    assert got.dtype == np.uint32 and len(got) == nsel
    return got


def run(tab, terms, order=None, offset=None, limit=None, n=None, cond=COND, **options):
    """(the returned ordinals, n1k_rowdistinct_stats) of one n1k_filter_device_batch over the table's first n rows."""
    op = make_op(tab, terms, order, offset, limit, cond, **options)
    try:
        return answer(op, tab, n), op.rowdistinct_stats()
    finally:
        op.done()


def paths_of(terms):
    return [t[0] if isinstance(t, tuple) else t for t in terms]


def expected(tab, terms, order=None, offset=None, limit=None, n=None, cond=COND):
    """(the representatives, ascending; the answer: they ordered by `order` — given by paths — and cut)."""
    reps = du.representatives([tab.values[p] for p in paths_of(terms)], tab.selected(n, cond))
    if order:
        return reps, ou.expected([tab.values[p] for p, _ in order], [d for _, d in order], offset or 0, limit, sel=reps)
    first = min(len(reps), offset or 0)
    return reps, reps[first:len(reps) if limit is None else first + limit]


def check(tab, terms, got, rd=None, **kw):
    reps, want = expected(tab, terms, **kw)
    assert np.array_equal(got, want), (len(got), len(want), got[:20], want[:20])
    if rd is not None:
        nsel = len(tab.selected(kw.get("n"), kw.get("cond", COND)))
        assert rd["survivors"] == nsel and rd["distinct_rows"] == len(reps) and rd["reached_table"] <= nsel
        assert (rd["table_slots"] >= len(reps)) or nsel == 0
        assert rd["reached_table"] >= len(reps)  # every representative went through the table


def small(key, build):
    if key not in _state:
        _state[key] = build()
    return _state[key]


# ------------------------------------------------------------------------------------------------ 1. survivor counts
COUNTS = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]


def counted(count, shape):
    """`count` survivors among count + count // 5 + 3 rows; survivor j has key: one for all / j / min(j, count - 1 - j) (key i
    again at count - 1 - i: beyond a tile's worth, a key's smallest ordinal and its duplicate lie in different tiles)."""
    rng = np.random.default_rng(count * 3 + len(shape))
    n = count + count // 5 + 3
    flags = np.zeros(n, np.uint64)
    flags[np.sort(rng.choice(n, count, replace=False))] = 1
    j = np.cumsum(flags).astype(np.int64) - 1  # (rows that are not selected repeat a neighbour's key: they must not count)
    keys = {"equal": np.full(n, 7, np.int64), "different": np.maximum(j, 0), "mirrored": np.maximum(np.minimum(j, count - 1 - j), 0)}[shape]
    return Tab(flags, {K: keys})


@pytest.mark.parametrize("shape", ["equal", "different", "mirrored"])
@pytest.mark.parametrize("count", COUNTS)
def test_survivor_counts_at_the_edges_of_the_tile(count, shape):
    tab = counted(count, shape)
    assert len(tab.selected()) == count
    for lds in (0, 2048):
        got, rd = run(tab, [K], rowdistinct_lds_slots=lds)
        assert len(got) == {"equal": min(count, 1), "different": count, "mirrored": (count + 1) // 2}[shape]
        check(tab, [K], got, rd)
        if shape == "equal":  # without the LDS set every survivor goes to the table, with it one row per tile (= workgroup)
            assert rd["reached_table"] == (count if lds == 0 else (count + T - 1) // T)


# ------------------------------------------------------------------------------------------------ 2. value classes, DICT32, terms
NAN2 = float(np.uint64(0xFFF8000000000001).view(np.float64))
POOL = [(n1o.T_MISSING, None), (n1o.T_NULL, None), (n1o.T_FALSE, None), (n1o.T_TRUE, None), I(0), FL(-0.0), FL(0.0), FL(0.5), I(2), FL(2.0),
        I(2 ** 53 + 1), FL(2.0 ** 53), I(2 ** 53), I(2 ** 63 - 1), FL(2.0 ** 63), I(-2 ** 63), FL(-2.0 ** 63), FL(float("nan")), FL(NAN2),
        FL(float("inf")), FL(float("-inf")), (n1o.T_STRING, b"[5]"), (n1o.T_ARRAY, b"[5]"), (n1o.T_OBJECT, b"[5]"), (n1o.T_STRING, b"NaN"),
        (n1o.T_STRING, b"+Infinity"), I(-1), FL(-1.0), FL(1e300), FL(5e-324)]
N_CLASSES = 23  # distinct values of POOL under the rules of n1k.h


def mixed():
    rng = np.random.default_rng(0xD157)
    n = 3 * T + 77
    dictionary = [b"zero", b"[5]", b"NaN", b"+Infinity", b"x", b"y"]
    classes = [POOL[i] for i in rng.integers(0, len(POOL), n)]
    codes = rng.integers(0, 3, n).astype(np.uint32)
    codes[rng.integers(0, n, 300)] = _ffi.CODE_MISSING
    codes[rng.integers(0, n, 300)] = _ffi.CODE_NULL
    a, b = rng.integers(0, 4, n), rng.integers(0, 4, n)
    a[:4], b[:4] = [1, 2, 1, 1], [2, 1, 2, 3]  # (a, b) against (b, a); rows that differ in the last term only
    last = [POOL[i] for i in rng.integers(4, 10, n)]
    return Tab((rng.random(n) < 0.9).astype(np.uint64), {V: classes, S: codes, K: a.astype(np.int64), W: b.astype(np.int64), X: last}, dictionary)


def test_every_value_class_in_one_tagged_column():
    tab = small("mixed", mixed)
    assert len({du.normalise(v) for v in POOL}) == N_CLASSES
    got, rd = run(tab, [V])
    assert len(got) == N_CLASSES
    check(tab, [V], got, rd)
    # the pairs of the equality list, one by one, as two-row tables (the second row falls iff the values are equal)
    for a, b in [(POOL[4], POOL[5]), (POOL[8], POOL[9]), (POOL[10], POOL[11]), (POOL[11], POOL[12]), (POOL[13], POOL[14]), (POOL[17], POOL[18]),
                 (POOL[0], POOL[1]), (POOL[21], POOL[22]), (POOL[22], POOL[23]), (POOL[17], POOL[24]), (POOL[19], POOL[25]), (POOL[15], POOL[16])]:
        two = Tab(np.ones(2, np.uint64), {V: [a, b]}, tab.dictionary)
        got, _ = run(two, [V])
        assert list(got) == ([0] if du.normalise(a) == du.normalise(b) else [0, 1]), (a, b)


def test_a_dict32_column_with_missing_and_null_codes():
    tab = small("mixed", mixed)
    got, rd = run(tab, [S])
    assert len(got) == 5  # three strings, MISSING, NULL
    check(tab, [S], got, rd)


@pytest.mark.parametrize("terms", [[K, W], [W, K], [K, X], [S, K, W, X], [X, W, K, V]], ids=["ab", "ba", "a-last", "4a", "4b"])
def test_two_and_four_terms(terms):
    tab = small("mixed", mixed)
    got, rd = run(tab, terms)
    check(tab, terms, got, rd)
    assert len(got) > len(run(tab, terms[:-1])[0])  # the last term tells rows apart


# ------------------------------------------------------------------------------------------------ 3. the LDS set, the table
def tiles(lds):
    """Three tiles of survivors (every row passes) holding lds - 1, lds and lds + 1 distinct keys, some shared between tiles."""
    rng = np.random.default_rng(lds)
    keys = np.concatenate([rng.integers(0, lds - 1, T), rng.integers(3, 3 + lds, T), rng.integers(5, 6 + lds, T)]).astype(np.int64)
    for t, d in enumerate((lds - 1, lds, lds + 1)):
        assert len(np.unique(keys[t * T:(t + 1) * T])) == d
    return Tab(np.ones(3 * T, np.uint64), {K: keys})


@pytest.mark.parametrize("lds", [8, 64])
def test_tiles_at_under_and_over_the_lds_sets_size(lds):
    tab = small(("tiles", lds), lambda: tiles(lds))
    answers = []
    for slots in (lds, 0, 2048, 1):
        got, rd = run(tab, [K], rowdistinct_lds_slots=slots)
        check(tab, [K], got, rd)
        answers.append(got)
        if slots == 0:
            assert rd["reached_table"] == 3 * T  # no pre-filter: every survivor goes to the table
        if slots == 2048:
            assert rd["reached_table"] == 3 * lds  # room for every key: one row per key and tile
    assert all(np.array_equal(answers[0], a) for a in answers[1:])


def test_a_full_table_wraps_and_a_table_one_slot_short_is_oom_and_the_handle_goes_on():
    tab = small("mixed", mixed)
    terms = [K, W]
    reps, _ = expected(tab, terms)
    d = len(reps)
    assert d == 16
    got, rd = run(tab, terms, rowdistinct_slots=d)
    check(tab, terms, got, rd)
    assert rd["table_slots"] == d
    for lds in (2048, 0):
        op = make_op(tab, terms, rowdistinct_slots=d - 1, rowdistinct_lds_slots=lds)
        try:
            with pytest.raises(query_amd.N1kError) as ei:
                op.filter_device_batch(tab.batch(op))
            assert ei.value.status == _ffi.OOM and "rowdistinct_slots" in ei.value.message
            with pytest.raises(query_amd.N1kError) as ei:  # and no selection is left
                op.selected_host32()
            assert ei.value.status == _ffi.INVALID
            op.set_option("rowdistinct_slots", 0)
            assert np.array_equal(answer(op, tab), reps)
            assert op.rowdistinct_stats()["table_slots"] >= 2 * len(tab.selected())
        finally:
            op.done()


def test_two_calls_on_one_handle_carry_nothing_over():
    a, b = small("mixed", mixed), small(("tiles", 8), lambda: tiles(8))
    other = Tab(np.ones(700, np.uint64), {K: (np.arange(700, dtype=np.int64) % 300) + 1000})  # keys the first call never saw, and its own
    op = make_op(a, [K])
    try:
        for tab in (a, other, b, a):
            got = answer(op, tab)
            assert np.array_equal(got, expected(tab, [K])[0])
            assert op.rowdistinct_stats()["survivors"] == len(tab.selected())
    finally:
        op.done()


# ------------------------------------------------------------------------------------------------ 4. the tail
FULL, SELECT = {"topk_min_groups": 1 << 40}, {"topk_min_groups": 1}


@pytest.mark.parametrize("route", [FULL, SELECT], ids=["full", "select"])
@pytest.mark.parametrize("order,kw", [([(K, False)], {}), ([(W, True), (K, False)], {}), ([(K, True)], {"offset": 1, "limit": 2}),
                                      ([(X, False), (K, True)], {"limit": 3}), ([(W, False), (K, True)], {"offset": 5, "limit": 6})])
def test_order_offset_limit_over_the_representatives(order, kw, route):
    tab = small("mixed", mixed)
    terms = [K, W, X]
    got, rd = run(tab, terms, order, **kw, **route)
    reps, want = expected(tab, terms, order, **kw)
    assert np.array_equal(got, want) and rd["distinct_rows"] == len(reps) > len(got) - (0 if kw else 1)


def test_an_alias_sort_term_orders_by_its_terms_column():
    tab = small("mixed", mixed)
    terms = [(K, "first"), (W, None)]
    got, _ = run(tab, terms, [("`first`", True), ("`w`", False)])
    check(tab, terms, got, order=[(K, True), (W, False)])


@pytest.mark.parametrize("offset,limit", [(None, 3), (4, None), (4, 5), (7, 100), (0, 0), (16, 1)])
def test_offset_and_limit_without_order_cut_the_ascending_representatives(offset, limit):
    tab = small("mixed", mixed)
    got, rd = run(tab, [K, W], offset=offset, limit=limit)
    check(tab, [K, W], got, offset=offset, limit=limit)
    assert rd["distinct_rows"] == 16


def test_gather_after_it_returns_the_terms_columns_without_a_duplicate_row():
    tab = small("mixed", mixed)
    terms = [S, V]
    op = make_op(tab, terms, [(S, True)])
    try:
        got = answer(op, tab)
        nsel = len(got)
        check(tab, terms, got, order=[(S, True)])
        o_codes = torch.zeros(nsel, dtype=torch.int32, device="cuda")
        o_tags = torch.zeros(nsel, dtype=torch.uint8, device="cuda")
        o_pay = torch.zeros(nsel, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        op.gather_selected(tab.batch(op, names=terms), nsel, [(_ffi.COL_DICT32, None, None, o_codes.data_ptr()),
                                                              (_ffi.COL_TAGGED64, o_tags.data_ptr(), o_pay.data_ptr(), None)])
        op.sync()
        ix = got.astype(np.int64)
        assert np.array_equal(o_codes.cpu().numpy().view(np.uint32), tab.cols[S].codes[ix])
        assert np.array_equal(o_tags.cpu().numpy(), tab.cols[V].tags[ix])
        assert np.array_equal(o_pay.cpu().numpy().view(np.uint64), tab.cols[V].payload[ix])
        rows = list(zip(ou.codes_values(o_codes.cpu().numpy().view(np.uint32), tab.dictionary),
                        ou.column_values(o_tags.cpu().numpy(), o_pay.cpu().numpy().view(np.uint64), tab.dictionary)))
        assert len({(du.normalise(s), du.normalise(v)) for s, v in rows}) == nsel
    finally:
        op.done()


def test_an_array_as_a_sort_value_is_unsupported_data_and_the_handle_goes_on():
    n = 200
    vals = [I(i % 17) for i in range(n)]
    vals[150] = (n1o.T_ARRAY, b"[1]")
    tab = Tab(np.ones(n, np.uint64), {V: vals, K: (np.arange(n, dtype=np.int64) % 5)}, [b"[1]"])
    op = make_op(tab, [V, K], [(K, False), (V, True)])
    try:
        with pytest.raises(query_amd.N1kError) as ei:
            op.filter_device_batch(tab.batch(op))
        assert ei.value.status == _ffi.UNSUPPORTED_DATA
        got = answer(op, tab, 150)  # the rows before the array: the handle goes on working
        check(tab, [V, K], got, order=[(K, False), (V, True)], n=150)
    finally:
        op.done()
    got, _ = run(tab, [V, K])  # as a term it is a value like any other: de-duplicated by its code
    check(tab, [V, K], got)


# ------------------------------------------------------------------------------------------------ 5. no Filter, lifetime
@pytest.mark.parametrize("order", [None, [(W, True), (K, False)]])
def test_a_plan_without_filter_takes_every_row(order):
    tab = small("mixed", mixed)
    op = make_op(tab, [K, W], order, cond=None)
    try:
        assert op.column_paths == [K, W]
        got = answer(op, tab)
        check(tab, [K, W], got, op.rowdistinct_stats(), order=order, cond=None)
        assert op.rowdistinct_stats()["survivors"] == tab.n
        assert len(answer(op, tab, 0)) == 0
    finally:
        op.done()


def test_stop_before_the_call_and_device_memory_after_destroy():
    tab = small("mixed", mixed)
    base = int(_ffi.lib().n1k_device_bytes_live())
    op = make_op(tab, [K], [(K, False)])
    try:
        answer(op, tab)
        assert int(_ffi.lib().n1k_device_bytes_live()) > base
        op.send_stop()
        with pytest.raises(query_amd.N1kError) as ei:
            op.filter_device_batch(tab.batch(op))
        assert ei.value.status == _ffi.STOPPED
        op.reopen()
        assert len(answer(op, tab)) == 4
    finally:
        op.done()
    assert int(_ffi.lib().n1k_device_bytes_live()) == base


# ------------------------------------------------------------------------------------------------ 6. one size up
def big():
    rng = np.random.default_rng(0xB16)
    n = 1 << 20
    return Tab((rng.random(n) < 0.95).astype(np.uint64), {K: rng.integers(0, 40, n), W: rng.integers(0, 25, n),
                                                          V: rng.integers(0, 800, n), X: rng.integers(0, 900, n)})


@pytest.mark.parametrize("terms,about", [([K, W], 1000), ([V, X], 500_000)], ids=["1000-keys", "500000-keys"])
def test_a_million_rows_with_few_and_with_many_distinct_rows(terms, about):
    tab = small("big", big)
    got, rd = run(tab, terms)
    check(tab, terms, got, rd)
    assert about * 0.8 <= len(got) <= about * 1.2
    assert rd["table_slots"] == 1 << 21 and rd["reached_table"] <= rd["survivors"]
    # fewer workgroups than tiles: a workgroup's LDS set goes from tile to tile, and a key it has met falls there
    few, rd_few = run(tab, terms, grid_blocks=1, rowdistinct_lds_slots=2048)
    assert np.array_equal(few, got) and rd_few["distinct_rows"] == rd["distinct_rows"]
    if about == 1000:
        assert rd_few["reached_table"] < rd["survivors"] // 2


# ------------------------------------------------------------------------------------------------ 7. seeded random plans
def random_columns(t):
    by = {c.name: c for c in t.columns}
    return {name: (ou.codes_values(c.codes, t.dictionary) if c.kind == n1o.COL_DICT32 else ou.column_values(c.tags, c.payload, t.dictionary))
            for name, c in by.items()}


def rand_leaf(rng):
    """One leaf comparison of test_gpu_random_plans.rand_cond over a column and a constant."""
    col = rp.D(["a", "b", "f", "s"][rng.integers(0, 4)])
    r = rng.integers(0, 10)
    if r < 6:
        const = ["3", "-2", "2.5", "0", "\"ab\"", "100"][rng.integers(0, 6)]
        a, b = (col, const) if rng.random() < 0.5 else (const, col)
        return "(%s %s %s)" % (a, ["<", "<=", "="][rng.integers(0, 3)], b)
    if r < 7:
        return "(%s between %s and %s)" % (col, ["-1", "0", "1.5"][rng.integers(0, 3)], ["4", "7.25", "\"b\""][rng.integers(0, 3)])
    return "(%s is %s)" % (col, ["null", "not null", "missing", "not missing", "valued", "not valued"][rng.integers(0, 6)])


@pytest.mark.parametrize("seed", range(100))
def test_random_plans_agree_with_the_reference(seed):
    rng = np.random.default_rng(0xD15 * 1000 + seed)
    t = rp.make_table(rng, int(rng.integers(1, 5000)))
    names = [rp.D(c) for c in "abfs"]
    terms = [names[i] for i in rng.choice(4, int(rng.integers(1, 5)), replace=rng.random() < 0.2)][:4]
    cond = rand_leaf(rng) if rng.random() < 0.85 else None
    order = [(names[i], bool(rng.random() < 0.5)) for i in rng.choice(4, int(rng.integers(1, 4)), replace=False)] if rng.random() < 0.6 else None
    offset = int(rng.integers(0, 30)) if rng.random() < 0.4 else None
    limit = int(rng.integers(0, 60)) if rng.random() < 0.5 else None
    opts = {}
    if rng.random() < 0.5:
        opts["rowdistinct_lds_slots"] = int([0, 1, 5, 64, 4096][rng.integers(0, 5)])
    if rng.random() < 0.3:
        opts["topk_min_groups"] = 1
    values = random_columns(t)
    sel = n1o.run(t, cond, [], [], has_group=False).selected.astype(np.int64) if cond else np.arange(t.nrows, dtype=np.int64)
    reps = du.representatives([values[p] for p in terms], sel)
    if order:
        want = ou.expected([values[p] for p, _ in order], [d for _, d in order], offset or 0, limit, sel=reps)
    else:
        first = min(len(reps), offset or 0)
        want = reps[first:len(reps) if limit is None else first + limit]
    by = {c.name: c for c in t.columns}
    dev = {}
    for name, c in by.items():
        if c.kind == n1o.COL_DICT32:
            dev[name] = (torch.from_numpy(np.ascontiguousarray(c.codes).view(np.int32)).cuda(),)
        else:
            dev[name] = (torch.from_numpy(np.ascontiguousarray(c.tags)).cuda(), torch.from_numpy(np.ascontiguousarray(c.payload).view(np.int64)).cuda())
    torch.cuda.synchronize()
    spec = lambda p: (_ffi.COL_DICT32, None, None, dev[p][0].data_ptr()) if len(dev[p]) == 1 else (_ffi.COL_TAGGED64, dev[p][0].data_ptr(), dev[p][1].data_ptr(), None)
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], [], filter_only=True, distinct=[(p, None) for p in terms], order=order,
                                                         offset=offset, limit=limit), **opts)
    try:
        op.intern(list(t.dictionary))
        nsel, _ = op.filter_device_batch(op.make_device_batch(t.nrows, [spec(p) for p in op.column_paths]))
        got = op.selected_host32()
        rd = op.rowdistinct_stats()
        assert np.array_equal(got, want), (cond, terms, order, offset, limit, opts, got[:10], want[:10])
        assert nsel == len(want) and rd["survivors"] == len(sel) and rd["distinct_rows"] == len(reps)
    finally:
        op.done()


# ------------------------------------------------------------------------------------------------ 8. the golden cases, end to end
@pytest.mark.parametrize("case", du.golden_cases(), ids=[c["id"] for c in du.golden_cases()])
def test_golden_distinct_cases_end_to_end(case):
    """Filter? + Distinct + Order on the device, the result terms by n1k_gather_selected: the reference's `results`."""
    table, terms, order, proj, sel = du.golden_setup(case)
    by = {c.name: c for c in table.columns}
    dev = {p: (torch.from_numpy(np.ascontiguousarray(c.tags)).cuda(), torch.from_numpy(np.ascontiguousarray(c.payload).view(np.int64)).cuda())
           for p, c in by.items()}
    torch.cuda.synchronize()
    spec = lambda p: (_ffi.COL_TAGGED64, dev[p][0].data_ptr(), dev[p][1].data_ptr(), None)
    # (the sort term as the planner leaves it: the projection's alias)
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(case["plan"]["condition"], [], [], filter_only=True, distinct=terms,
                                                         order=[("`%s`" % proj[0][0], d) for _, d in order]))
    try:
        assert op.column_paths == [c.name for c in table.columns]
        op.intern(list(table.dictionary))
        n = table.nrows
        nsel, _ = op.filter_device_batch(op.make_device_batch(n, [spec(p) for p in op.column_paths]))
        assert nsel == len(case["results"]) and op.rowdistinct_stats()["survivors"] == len(sel)
        out = [(torch.zeros(nsel, dtype=torch.uint8, device="cuda"), torch.zeros(nsel, dtype=torch.int64, device="cuda")) for _ in proj]
        torch.cuda.synchronize()
        op.gather_selected(op.make_device_batch(n, [spec(p) for _, p in proj]), nsel, [(_ffi.COL_TAGGED64, t.data_ptr(), p.data_ptr(), None) for t, p in out])
        op.sync()
        cols = [(t.cpu().numpy()[:nsel], p.cpu().numpy().view(np.uint64)[:nsel]) for t, p in out]
        rows = ou.golden_rows(table, proj, list(range(nsel)), columns=cols)
        assert rows == case["results"] and gu.same_json(rows, case["results"]), (rows, case["results"])
    finally:
        op.done()
