"""ORDER BY / OFFSET / LIMIT over the rows of a Filter-only plan, sorted on the device: the ordinals n1k_filter_device_batch
returns for such a plan against tests/order_util.py — exactly: ordinals, not values, no tolerance.

Survivor counts sit at the edges of the sort (wave = 64, tile T = 4096 elements, more tiles than the 256 workgroups of
grid_blocks = 1); key shapes make every digit pass run, none, or single ones; the select route (radix select of the first
offset + limit rows, then the sort of the candidates) and the full sort are forced through topk_min_groups and must agree.
Device memory comes from torch, the selection from the oracle."""
import numpy as np
import pytest
import torch

import golden_util as gu
import order_util as ou
import query_amd
import topk_util as tk
from oracle import n1o
from query_amd import _ffi, plan

pytestmark = pytest.mark.gpu

D = lambda *n: plan.field_path("d", *n)
F, V, W, X, Y, S = D("f"), D("v"), D("w"), D("x"), D("y"), D("s")
COND = "(0 < %s)" % F
T = 4096
N_BIG = 257 * T + 1  # survivors: one tile more than a grid_blocks = 1 grid has workgroups, and a row
FULL, SELECT = {"topk_min_groups": 1 << 40}, {"topk_min_groups": 1}

_state = {}


class Tab:
    """A table (column F = the Filter's flag, and named sort columns), its device copy, the oracle's selections by row count."""

    def __init__(self, flags, cols, dictionary=()):
        n = len(flags)
        self.n, self.dictionary = n, [bytes(s) for s in dictionary]
        self.cols = {F: n1o.Column(F, n1o.COL_TAGGED64, tags=np.full(n, n1o.T_INT, np.uint8), payload=np.asarray(flags).astype(np.uint64))}
        self.values = {}
        for name, c in cols.items():
            if isinstance(c, np.ndarray) and c.dtype == np.float64:  # FLOAT values, kept as the array (order_util's vectorised form)
                self.cols[name] = n1o.Column(name, n1o.COL_TAGGED64, tags=np.full(n, n1o.T_FLOAT, np.uint8), payload=c.view(np.uint64).copy())
                self.values[name] = c
            elif isinstance(c, np.ndarray):  # DICT32 codes
                self.cols[name] = n1o.Column(name, n1o.COL_DICT32, codes=c.astype(np.uint32))
                self.values[name] = ou.codes_values(c, self.dictionary)
            else:  # (tag, python value) pairs
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

    def selected(self, n=None):
        n = self.n if n is None else n
        if n not in self._sel:
            self._sel[n] = n1o.run(self.table.slice(0, n), COND, [], [], has_group=False).selected.astype(np.int64)
        return self._sel[n]

    def spec(self, name):
        d = self.dev[name]
        return (_ffi.COL_DICT32, None, None, d[0].data_ptr()) if len(d) == 1 else (_ffi.COL_TAGGED64, d[0].data_ptr(), d[1].data_ptr(), None)

    def batch(self, op, n=None, names=None):
        return op.make_device_batch(self.n if n is None else n, [self.spec(p) for p in (op.column_paths if names is None else names)])


def make_op(tab, order=None, offset=None, limit=None, **options):
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(COND, [], [], filter_only=True, order=order, offset=offset, limit=limit), **options)
    if tab.dictionary:
        codes = op.intern(tab.dictionary)
        assert np.array_equal(codes, np.arange(len(codes), dtype=np.uint32))
    return op


def run(tab, order=None, offset=None, limit=None, n=None, **options):
    """(the returned ordinals, the stats) of one n1k_filter_device_batch over the table's first n rows."""
    op = make_op(tab, order, offset, limit, **options)
    try:
        nsel, addr = op.filter_device_batch(tab.batch(op, n))
        st = op.stats()
        assert (addr is None) == (nsel == 0) and st["rows_selected"] == nsel and st["rows_in"] == (tab.n if n is None else n)
        got = op.selected_host32()
        assert got.dtype == np.uint32 and len(got) == nsel
        return got, st
    finally:
        op.done()


def check(tab, order, got, offset=None, limit=None, n=None):
    sel = tab.selected(n)
    values, desc = [tab.values[p] for p, _ in order], [d for _, d in order]
    if len(sel) <= ou.MAX_SORTED:
        want = ou.expected(values, desc, offset or 0, limit, sel=sel)
        assert np.array_equal(got, want), (got[:20], want[:20])
    ou.check_sorted(values, got, desc, offset or 0, limit, sel=sel)


def random_doubles(rng, n):
    """Random bit patterns that are no NaN / infinity: every one of the key's 8 digits is live."""
    bits = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    bits = np.where((bits >> np.uint64(52)) & np.uint64(0x7FF) == np.uint64(0x7FF), bits & ~np.uint64(1 << 62), bits)
    return bits.view(np.float64).copy()


def big():
    """1.1 M rows, ~ 97 % of them selected (row 0 is not), a column of random doubles and one of a few hundred distinct ones."""
    if "big" not in _state:
        rng = np.random.default_rng(0x0DE7)
        n = N_BIG + 40_000
        flags = (rng.random(n) < 0.97).astype(np.uint64)
        flags[0] = 0
        v = random_doubles(rng, n)
        w = rng.integers(0, 300, n).astype(np.float64) / 4.0
        _state["big"] = Tab(flags, {V: v, W: w})
        assert len(_state["big"].selected()) >= N_BIG
    return _state["big"]


def rows_for(tab, count):
    """The shortest prefix of the table that holds `count` survivors."""
    sel = tab.selected()
    return int(sel[count - 1]) + 1 if count else int(sel[0])


def small(key, build):
    if key not in _state:
        _state[key] = build()
    return _state[key]


N_SMALL = 10_000


def flags_small(rng, n=N_SMALL):
    return (rng.random(n) < 0.9).astype(np.uint64)


# ------------------------------------------------------------------------------------------------ 1. survivor counts
@pytest.mark.parametrize("count", [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, N_BIG])
def test_survivor_counts_at_the_edges_of_the_sort(count):
    tab = big()
    n = rows_for(tab, count)
    assert len(tab.selected(n)) == count
    opts = dict(FULL, **({"grid_blocks": 1} if count == N_BIG else {}))
    got, st = run(tab, [(V, False)], n=n, **opts)
    assert len(got) == count and st["topk_candidates"] == 0
    check(tab, [(V, False)], got, n=n)


def test_descending_and_a_second_term_over_a_million_rows():
    tab = big()
    order = [(W, True), (V, False)]
    got, _ = run(tab, order, **FULL)
    check(tab, order, got)


# ------------------------------------------------------------------------------------------------ 2. key shapes
def shapes():
    rng = np.random.default_rng(0x5A9E)
    n = N_SMALL
    low = (np.uint64(0x3FF0000000000000) | rng.integers(0, 256, n, dtype=np.uint64)).view(np.float64).copy()
    high = ((rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x0010000000000000)).view(np.float64).copy()
    assert not np.isnan(high).any() and len(np.unique(high)) > 200
    return Tab(flags_small(rng), {V: np.full(n, 2.5), W: np.array([1.5, -3.0, 7.25])[rng.integers(0, 3, n)], X: low, Y: high})


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("col", [V, W, X, Y])
def test_key_shapes(col, desc):
    tab = small("shapes", shapes)
    got, _ = run(tab, [(col, desc)])
    check(tab, [(col, desc)], got)
    if col == V:  # one distinct value: every pass is skipped and the ascending selection comes back
        assert np.array_equal(got, tab.selected().astype(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. classes, big ints, strings
def mixed():
    rng = np.random.default_rng(0xC1A5)
    n = N_SMALL
    strings = sorted(tk.STRINGS)
    dictionary = [strings[i] for i in rng.permutation(len(strings))] + [b"~never used"]
    pool = [tk.MISSING] + list(tk.POOL.values())
    classes = [pool[i] for i in rng.integers(0, len(pool), n)]
    ints = [tk.I(2 ** 53), tk.I(2 ** 53 + 1), tk.I(2 ** 53 - 1), tk.I(-2 ** 53), tk.I(-2 ** 53 - 1), tk.I(-2 ** 53 + 1), tk.F(9007199254740992.0),
            tk.F(-9007199254740992.0), tk.I(2 ** 63 - 1), tk.I(-2 ** 63), tk.F(9.223372036854775808e18), tk.F(-9.223372036854775808e18),
            tk.I(2 ** 63 - 1025), tk.I(2 ** 62 + 257), tk.I(-2 ** 63 + 1), tk.F(tk.INF), tk.F(-tk.INF), tk.I(0), tk.F(-0.0), tk.F(0.0)]
    floats = random_doubles(rng, n)
    bigint = [ints[i] if i < len(ints) else tk.F(float(floats[k])) for k, i in enumerate(rng.integers(0, 3 * len(ints), n))]
    codes = rng.integers(0, len(strings), n).astype(np.uint32)  # DICT32: the dictionary is shuffled, a code is no rank
    codes[rng.integers(0, n, 300)] = _ffi.CODE_MISSING
    codes[rng.integers(0, n, 300)] = _ffi.CODE_NULL
    few = [tk.I(int(i)) for i in rng.integers(0, 4, n)]
    return Tab(flags_small(rng), {V: classes, W: bigint, S: codes, X: few, Y: random_doubles(rng, n)}, dictionary)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("col", [V, W, S], ids=["classes", "big-ints", "dict32-strings"])
def test_classes_big_ints_and_strings(col, desc):
    tab = small("mixed", mixed)
    got, _ = run(tab, [(col, desc)])
    check(tab, [(col, desc)], got)


@pytest.mark.parametrize("order", [[(X, False), (Y, True)], [(X, True), (S, False)], [(X, False), (S, True), (V, False), (Y, True)],
                                   [(X, True), (V, True), (W, False), (S, False)]], ids=["2a", "2b", "4a", "4b"])
def test_two_and_four_terms_with_mixed_directions(order):
    tab = small("mixed", mixed)
    got, _ = run(tab, order)
    check(tab, order, got)


# ------------------------------------------------------------------------------------------------ 4. offset / limit
@pytest.mark.parametrize("route", [FULL, SELECT], ids=["full", "select"])
@pytest.mark.parametrize("offset,limit", [(0, 0), (0, 1), (1, 1), (0, -1), (1, -1), (0, None), (5, 0), (None, -2), (3, -3), (-1, 5), (None, 1 << 40),
                                          (0, 100), (1234, 777)])
def test_offset_and_limit(offset, limit, route):
    """limit < 0 stands for nselected + limit + 1 (so -1 is nselected, -2 is nselected - 1), offset -1 for nselected: keep =
    nselected - 1, nselected and beyond, an offset at nselected (empty)."""
    tab = small("mixed", mixed)
    nsel = len(tab.selected())
    offset = nsel if offset == -1 else offset
    limit = nsel + limit + 1 if limit is not None and limit < 0 else limit
    order = [(X, False), (Y, True)]
    got, st = run(tab, order, offset=offset, limit=limit, **route)
    check(tab, order, got, offset=offset, limit=limit)
    keep = (offset or 0) + (limit if limit is not None else nsel)
    ran = route is SELECT and limit is not None and 0 < keep < nsel
    assert (st["topk_candidates"] > 0) == ran and (not ran or keep <= st["topk_candidates"] <= nsel)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("keep", [1, 700, 2500])
def test_ties_at_the_cut_resolve_by_ordinal_on_both_routes(keep, desc):
    """Three values over ~ 9 000 survivors: the threshold value is shared by thousands of rows."""
    tab = small("shapes", shapes)
    answers = []
    for route in (FULL, SELECT):
        got, st = run(tab, [(W, desc)], offset=keep // 2, limit=keep - keep // 2, **route)
        check(tab, [(W, desc)], got, offset=keep // 2, limit=keep - keep // 2)
        answers.append(got)
        assert (st["topk_candidates"] > 0) == (route is SELECT)
    assert np.array_equal(answers[0], answers[1])


@pytest.mark.parametrize("order", [[(V, True)], [(W, False), (V, False)]], ids=["one-term", "two-terms"])
def test_limit_100_over_a_million_rows_selects_from_a_sample(order):
    """The default topk_min_groups: a million survivors take the select route, its threshold from a sample."""
    tab = big()
    got, st = run(tab, order, limit=100)
    assert len(got) == 100 and 100 <= st["topk_candidates"] < len(tab.selected())
    check(tab, order, got, limit=100)
    full, st = run(tab, order, limit=100, **FULL)
    assert st["topk_candidates"] == 0 and np.array_equal(got, full)


@pytest.mark.parametrize("offset,limit", [(None, 10), (7, None), (7, 10), (8, 10), (0, 0), (-1, 3), (5, 1 << 40)])
def test_offset_and_limit_without_order_cut_the_ascending_selection(offset, limit):
    tab = small("shapes", shapes)
    sel = tab.selected()
    offset = len(sel) if offset == -1 else offset
    got, _ = run(tab, None, offset=offset, limit=limit)
    first = min(len(sel), offset or 0)
    assert np.array_equal(got, sel[first:len(sel) if limit is None else first + limit].astype(np.uint32))


# ------------------------------------------------------------------------------------------------ 5. what follows, errors
@pytest.mark.parametrize("offset", [None, 3])
def test_gather_after_an_ordered_selection_returns_the_sort_column_in_order(offset):
    tab = small("mixed", mixed)
    order = [(W, True)]
    op = make_op(tab, order, offset=offset, limit=500)
    try:
        nsel, _ = op.filter_device_batch(tab.batch(op))
        assert nsel == 500
        got = op.selected_host32()
        check(tab, order, got, offset=offset, limit=500)
        o_tags = torch.zeros(nsel, dtype=torch.uint8, device="cuda")
        o_pay = torch.zeros(nsel, dtype=torch.int64, device="cuda")
        o_codes = torch.zeros(nsel, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        op.gather_selected(tab.batch(op, names=[W, S]), nsel, [(_ffi.COL_TAGGED64, o_tags.data_ptr(), o_pay.data_ptr(), None),
                                                              (_ffi.COL_DICT32, None, None, o_codes.data_ptr())])
        op.sync()
        ix = got.astype(np.int64)
        assert np.array_equal(o_tags.cpu().numpy(), tab.cols[W].tags[ix])
        assert np.array_equal(o_pay.cpu().numpy().view(np.uint64), tab.cols[W].payload[ix])
        assert np.array_equal(o_codes.cpu().numpy().view(np.uint32), tab.cols[S].codes[ix])
        vals = ou.column_values(o_tags.cpu().numpy(), o_pay.cpu().numpy().view(np.uint64), tab.dictionary)
        assert all(tk.collate_exact(a, b) >= 0 for a, b in zip(vals, vals[1:]))  # descending
    finally:
        op.done()


@pytest.mark.parametrize("route", [FULL, SELECT], ids=["full", "select"])
def test_an_array_as_a_sort_value_is_unsupported_data_and_the_handle_goes_on(route):
    n = 200
    vals = [tk.I(i % 17) for i in range(n)]
    vals[150] = (n1o.T_ARRAY, b"[1]")
    tab = Tab(np.ones(n, np.uint64), {V: vals, W: [tk.I(i % 5) for i in range(n)]}, [b"[1]"])
    for order in ([(V, False)], [(W, False), (V, True)]):  # as the first term and as a later one
        op = make_op(tab, order, limit=10, **route)
        try:
            with pytest.raises(query_amd.N1kError) as ei:
                op.filter_device_batch(tab.batch(op))
            assert ei.value.status == _ffi.UNSUPPORTED_DATA
            with pytest.raises(query_amd.N1kError) as ei:  # and no selection is left
                op.selected_host32()
            assert ei.value.status == _ffi.INVALID
            nsel, _ = op.filter_device_batch(tab.batch(op, 150))  # the rows before the array: the handle goes on working
            assert nsel == 10
            check(tab, order, op.selected_host32(), limit=10, n=150)
        finally:
            op.done()


def test_a_plan_without_order_after_an_ordered_one_returns_ascending_ordinals():
    tab = small("shapes", shapes)
    got, _ = run(tab, [(Y, True)], limit=50)
    check(tab, [(Y, True)], got, limit=50)
    plain, st = run(tab)
    assert np.array_equal(plain, tab.selected().astype(np.uint32)) and st["topk_candidates"] == 0


# ------------------------------------------------------------------------------------------------ 6. the golden cases, end to end
GOLDEN = ou.golden_sortable_cases()


@pytest.mark.parametrize("case", GOLDEN, ids=[c["id"] for c in GOLDEN])
def test_golden_order_by_cases_end_to_end(case):
    """Filter + Order on the device, the result terms by n1k_gather_selected: the reference's `results`, no host ordering."""
    table, terms, proj, sel = ou.golden_setup(case)
    by = {c.name: c for c in table.columns}
    dev = {p: (torch.from_numpy(np.ascontiguousarray(c.tags)).cuda(), torch.from_numpy(np.ascontiguousarray(c.payload).view(np.int64)).cuda())
           for p, c in by.items()}
    torch.cuda.synchronize()
    spec = lambda p: (_ffi.COL_TAGGED64, dev[p][0].data_ptr(), dev[p][1].data_ptr(), None)
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(case["plan"]["condition"], [], [], filter_only=True, order=terms))
    try:
        op.intern(list(table.dictionary))
        n = table.nrows
        nsel, _ = op.filter_device_batch(op.make_device_batch(n, [spec(p) for p in op.column_paths]))
        assert nsel == len(sel)
        out = [(torch.zeros(max(nsel, 1), dtype=torch.uint8, device="cuda"), torch.zeros(max(nsel, 1), dtype=torch.int64, device="cuda")) for _ in proj]
        torch.cuda.synchronize()
        if nsel:
            op.gather_selected(op.make_device_batch(n, [spec(p) for _, p in proj]), nsel,
                               [(_ffi.COL_TAGGED64, t.data_ptr(), p.data_ptr(), None) for t, p in out])
            op.sync()
        cols = [(t.cpu().numpy()[:nsel], p.cpu().numpy().view(np.uint64)[:nsel]) for t, p in out]
        rows = ou.golden_rows(table, proj, list(range(nsel)), columns=cols)
        assert gu.same_json(rows, case["results"]), (rows, case["results"])
    finally:
        op.done()
