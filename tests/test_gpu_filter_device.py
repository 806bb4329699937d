"""Filter-only plans whose answer stays on the device: n1k_filter_device_batch (32-bit batch-local ordinals in the handle's
memory), n1k_selected_to_host32 and n1k_gather_selected, against the oracle's selection.

Row counts sit at the edges of filter_stream_kernel (tile = 8192 rows, look-back window = 64 tiles, two rows per lane in the
FAST variant) and of gather_rows_kernel (four rows per lane, 1024 per workgroup).  Device memory comes from torch; one synthetic
table and its device copy serve every row count (a batch is the table's first n rows)."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity_util as pu
import query_amd
from oracle import n1o
from query_amd import _ffi, plan

pytestmark = pytest.mark.gpu

D = lambda *n: plan.field_path("default", *n)
PRICE, CAT = D("price"), D("cat")
N_BIG = 2_200_001  # 269 tiles: more than the 256 workgroups of grid_blocks = 1 (one per CU), so a workgroup takes a second tile
TILE = 8192
ROWS = [0, 1, 2, 3, TILE - 1, TILE, TILE + 1, 65 * TILE + 1, N_BIG]
FAST = "(50 < %s)" % PRICE
INTERP = "((50 < %s) or (%s = \"cat_3\"))" % (PRICE, CAT)
NONE = "((%s is missing) and (%s is not missing))" % (PRICE, PRICE)
ALL = "((%s is missing) or (%s is not missing))" % (PRICE, PRICE)

_state = {}


def big():
    """The table, its device copy (price payload twice: as allocated, and one element into a larger tensor: 8-byte but not
    16-byte aligned) — built once."""
    if not _state:
        t = n1o.synth_table(N_BIG, k_cat=37)
        by = {c.name: c for c in t.columns}
        pay = np.ascontiguousarray(by[PRICE].payload).view(np.int64)
        shifted = torch.zeros(N_BIG + 1, dtype=torch.int64, device="cuda")
        shifted[1:] = torch.from_numpy(pay).cuda()
        _state.update(table=t, sel={},
                      cat=torch.from_numpy(np.ascontiguousarray(by[CAT].codes).view(np.int32)).cuda(),
                      tags=torch.from_numpy(np.ascontiguousarray(by[PRICE].tags)).cuda(),
                      pay=torch.from_numpy(pay).cuda(), pay_shifted=shifted[1:])
        assert _state["pay"].data_ptr() % 16 == 0 and _state["pay_shifted"].data_ptr() % 16 == 8
        torch.cuda.synchronize()
    return _state


def oracle_selected(n, cond):
    s = big()
    if (n, cond) not in s["sel"]:
        s["sel"][(n, cond)] = n1o.run(s["table"].slice(0, n), cond, [], [], has_group=False).selected
    return s["sel"][(n, cond)]


def filter_op(cond, **options):
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], [], filter_only=True), **options)
    codes = op.intern(list(big()["table"].dictionary))
    assert np.array_equal(codes, np.arange(len(codes), dtype=np.uint32))
    return op


def big_batch(op, n, shifted=False):
    s = big()
    cols = {PRICE: (_ffi.COL_TAGGED64, s["tags"].data_ptr(), (s["pay_shifted"] if shifted else s["pay"]).data_ptr(), None),
            CAT: (_ffi.COL_DICT32, None, None, s["cat"].data_ptr())}
    return op.make_device_batch(n, [cols[p] for p in op.column_paths])


def device_u32(addr, n):
    """n uint32 words of device memory at `addr`, read through torch (n1k_selected_to_host32 is checked against it, so the
    selection is read here without it)."""
    if not n:
        return np.zeros(0, np.uint32)

    class View:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (int(addr), False), "version": 2}

    return torch.as_tensor(View(), device="cuda").cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. ordinals
@pytest.mark.parametrize("mode", ["fast", "interpreter", "unaligned"])
@pytest.mark.parametrize("n", ROWS)
def test_ordinals_equal_the_oracles(n, mode):
    cond = INTERP if mode == "interpreter" else FAST
    want = oracle_selected(n, cond)
    op = filter_op(cond, **({"grid_blocks": 1} if n == N_BIG else {}))
    try:
        nsel, addr = op.filter_device_batch(big_batch(op, n, shifted=mode == "unaligned"))
        st = op.stats()
        print("n=%d mode=%s nselected=%d oracle=%d spec_kernel=%d device_ms=%.3f" % (n, mode, nsel, len(want), st["spec_kernel"], st["device_ms"]))
        assert nsel == len(want)
        assert (addr is None) == (nsel == 0)
        if n:  # (no rows: no launch, no kernel to name)
            assert st["spec_kernel"] == (1 if mode == "fast" else 0)
        assert st["rows_in"] == n and st["rows_selected"] == nsel and st["batches"] == 1
        got = op.selected_host32()
        assert got.dtype == np.uint32 and np.array_equal(got, want.astype(np.uint32))
        assert np.array_equal(want.astype(np.uint32).astype(np.uint64), want)  # (the oracle's ordinals fit)
        assert np.array_equal(device_u32(addr, nsel), got)  # the returned device pointer is that selection
        assert op.after_items().selected.size == 0  # otherwise as after a reset: a following finish has nothing
    finally:
        op.done()


@pytest.mark.parametrize("cond,count", [(NONE, 0), (ALL, None)])
@pytest.mark.parametrize("n", [3, TILE + 1, 65 * TILE + 1])
def test_nothing_and_everything_passes(n, cond, count):
    want = oracle_selected(n, cond)
    assert len(want) == (n if count is None else count)
    op = filter_op(cond)
    try:
        nsel, addr = op.filter_device_batch(big_batch(op, n))
        assert nsel == len(want) and (addr is None) == (nsel == 0)
        assert np.array_equal(op.selected_host32(), want.astype(np.uint32))
        if nsel:
            into = np.full(nsel + 5, 0xFFFFFFFF, dtype=np.uint32)  # a caller's buffer with room to spare
            assert np.array_equal(op.selected_host32(into), want.astype(np.uint32)) and (into[nsel:] == 0xFFFFFFFF).all()
            with pytest.raises(query_amd.N1kError) as ei:
                op.selected_host32(np.zeros(nsel - 1, np.uint32))
            assert ei.value.status == _ffi.INVALID
    finally:
        op.done()


# ------------------------------------------------------------------------------------------------ 2. the existing paths
@pytest.mark.parametrize("cond", [FAST, INTERP])
def test_same_ordinals_as_the_host_path_and_one_selection_per_call(cond):
    n1, n2 = 100_003, 30_001
    op = filter_op(cond)
    try:
        b1, b2 = big_batch(op, n1), big_batch(op, n2)
        nsel, _ = op.filter_device_batch(b1)
        got32 = op.selected_host32()
        dev_stats = op.stats()
        raw = op.run_device_batch_raw(b1)  # the same handle, the 64-bit host ordinals
        assert raw["selected"].dtype == np.uint64 and np.array_equal(raw["selected"], got32.astype(np.uint64))
        assert op.stats()["rows_selected"] == dev_stats["rows_selected"] == nsel == len(oracle_selected(n1, cond))
        with pytest.raises(query_amd.N1kError) as ei:  # that path's reset took the device selection with it
            op.selected_host32()
        assert ei.value.status == _ffi.INVALID
        # twice in a row: the second batch's selection alone
        op.filter_device_batch(b1)
        nsel2, _ = op.filter_device_batch(b2)
        assert nsel2 == len(oracle_selected(n2, cond)) and op.stats()["rows_in"] == n2
        assert np.array_equal(op.selected_host32(), oracle_selected(n2, cond).astype(np.uint32))
    finally:
        op.done()


# ------------------------------------------------------------------------------------------------ 3. gather
N_SRC = 5000  # survivors of `x < K`: K rows scattered over the batch (x is a permutation of 0 .. N_SRC - 1)
X = D("x")
TAGS_SENTINEL, PAY_SENTINEL, CODE_SENTINEL = 0xEE, 0x5E5E5E5E5E5E5E5E, 0xABABABAB
PAD = 8  # elements in front of and behind every output array's rows


def gather_source():
    if "src" not in _state:
        big()
        rng = np.random.default_rng(0x6A7)
        x = rng.permutation(N_SRC).astype(np.uint64)
        kinds = np.array([n1o.T_MISSING, n1o.T_NULL, n1o.T_FALSE, n1o.T_TRUE, n1o.T_INT, n1o.T_FLOAT, n1o.T_STRING], dtype=np.uint8)
        host = {"x_tags": np.full(N_SRC, n1o.T_INT, np.uint8), "x_pay": x,
                "a_tags": kinds[rng.integers(0, len(kinds), N_SRC)], "a_pay": rng.integers(0, 2 ** 64, N_SRC, dtype=np.uint64),
                "b_tags": kinds[np.arange(N_SRC) % len(kinds)], "b_pay": rng.integers(0, 2 ** 64, N_SRC, dtype=np.uint64),
                "c_codes": rng.integers(0, 1000, N_SRC).astype(np.uint32)}
        host["c_codes"][rng.integers(0, N_SRC, 400)] = _ffi.CODE_MISSING
        host["c_codes"][rng.integers(0, N_SRC, 400)] = _ffi.CODE_NULL
        assert set(host["a_tags"]) == set(kinds) and (host["c_codes"] == _ffi.CODE_MISSING).any() and (host["c_codes"] == _ffi.CODE_NULL).any()
        signed = {"x_pay": np.int64, "a_pay": np.int64, "b_pay": np.int64, "c_codes": np.int32}
        dev = {k: torch.from_numpy(v.view(signed.get(k, v.dtype))).cuda() for k, v in host.items()}
        torch.cuda.synchronize()
        t = n1o.Table([n1o.Column(X, n1o.COL_TAGGED64, tags=host["x_tags"], payload=host["x_pay"])], [])
        _state["src"] = (host, dev, t, {})
    return _state["src"]


def gather_case(K):
    """The Filter handle with the selection of `x < K` in it, the oracle's ordinals, the source batch (a, b TAGGED64; c DICT32)."""
    host, dev, t, sels = gather_source()
    cond = "(%s < %d)" % (X, K)
    if K not in sels:
        sels[K] = n1o.run(t, cond, [], [], has_group=False).selected
    want = sels[K]
    assert len(want) == K
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], [], filter_only=True))
    nsel, _ = op.filter_device_batch(op.make_device_batch(N_SRC, [(_ffi.COL_TAGGED64, dev["x_tags"].data_ptr(), dev["x_pay"].data_ptr(), None)]))
    assert nsel == K
    src = op.make_device_batch(N_SRC, [(_ffi.COL_TAGGED64, dev["a_tags"].data_ptr(), dev["a_pay"].data_ptr(), None),
                                       (_ffi.COL_DICT32, None, None, dev["c_codes"].data_ptr()),
                                       (_ffi.COL_TAGGED64, dev["b_tags"].data_ptr(), dev["b_pay"].data_ptr(), None)])
    return op, want, src


class Out:
    """Output arrays inside larger sentinel-filled tensors: tags / payloads / codes start `o` / `o` / `o` elements behind a
    PAD that torch aligned to 256 bytes, so o = 0..3 gives tags every offset in a word, payloads 16-byte (even o) and 8-byte
    (odd o) alignment, codes 16-byte (o = 0) and 4-byte alignment.  The second TAGGED64 column sits one element further."""

    def __init__(self, rows, o):
        self.rows, self.o = rows, o
        self.off = {"a": o, "b": (o + 1) % 4, "c": o}
        size = PAD + 4 + rows + PAD
        self.t = {k: torch.full((size,), TAGS_SENTINEL, dtype=torch.uint8, device="cuda") for k in "ab"}
        self.p = {k: torch.full((size,), PAY_SENTINEL, dtype=torch.int64, device="cuda") for k in "ab"}
        self.c = torch.full((size,), CODE_SENTINEL - 2 ** 32, dtype=torch.int32, device="cuda")
        for k in "ab":
            assert self.t[k].data_ptr() % 16 == 0 and self.p[k].data_ptr() % 16 == 0
        assert self.c.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def start(self, k):
        return PAD + self.off[k]

    def cols(self):
        tg = lambda k: self.t[k].data_ptr() + self.start(k)
        py = lambda k: self.p[k].data_ptr() + 8 * self.start(k)
        return [(_ffi.COL_TAGGED64, tg("a"), py("a"), None), (_ffi.COL_DICT32, None, None, self.c.data_ptr() + 4 * self.start("c")),
                (_ffi.COL_TAGGED64, tg("b"), py("b"), None)]

    def check(self, host, want):
        """Rows [0, len(want)) are the source's rows `want`, bit for bit; everything around them is the sentinel."""
        n = len(want)
        for k in "ab":
            t, p, s = self.t[k].cpu().numpy(), self.p[k].cpu().numpy().view(np.uint64), self.start(k)
            assert np.array_equal(t[s:s + n], host[k + "_tags"][want]) and np.array_equal(p[s:s + n], host[k + "_pay"][want])
            assert (t[:s] == TAGS_SENTINEL).all() and (t[s + n:] == TAGS_SENTINEL).all()
            assert (p[:s] == PAY_SENTINEL).all() and (p[s + n:] == PAY_SENTINEL).all()
        c, s = self.c.cpu().numpy().view(np.uint32), self.start("c")
        assert np.array_equal(c[s:s + n], host["c_codes"][want])
        assert (c[:s] == CODE_SENTINEL).all() and (c[s + n:] == CODE_SENTINEL).all()


@pytest.mark.parametrize("o", [0, 1, 2, 3])
@pytest.mark.parametrize("K", [3000, 3001, 3002, 3003, 3, 1024, 1025])  # K % 4 = 0, 1, 2, 3; a tail alone; one workgroup, and a row more
def test_gather_is_numpy_indexing_by_the_oracles_ordinals(K, o):
    op, want, src = gather_case(K)
    try:
        assert K % 4 == {3000: 0, 3001: 1, 3002: 2, 3003: 3, 3: 3, 1024: 0, 1025: 1}[K]
        out = Out(K + 3, o)
        op.gather_selected(src, K + 3, out.cols())
        op.sync()
        out.check(gather_source()[0], want.astype(np.int64))
    finally:
        op.done()


def test_gather_refuses_what_does_not_fit():
    K = 3001
    op, want, src = gather_case(K)
    host, dev, _, _ = gather_source()
    try:
        out = Out(K, 0)
        good = out.cols()
        with pytest.raises(query_amd.N1kError) as ei:  # capacity
            op.gather_selected(src, K - 1, good)
        assert ei.value.status == _ffi.INVALID
        swapped = [good[1], good[0], good[2]]  # kinds
        with pytest.raises(query_amd.N1kError) as ei:
            op.gather_selected(src, K, swapped)
        assert ei.value.status == _ffi.INVALID
        a = (_ffi.COL_TAGGED64, dev["a_tags"].data_ptr(), dev["a_pay"].data_ptr(), None)  # 17 columns
        with pytest.raises(query_amd.N1kError) as ei:
            op.gather_selected(op.make_device_batch(N_SRC, [a] * 17), K, [good[0]] * 17)
        assert ei.value.status == _ffi.INVALID
        short = op.make_device_batch(N_SRC - 1, [a])  # not the filtered batch's row count
        with pytest.raises(query_amd.N1kError) as ei:
            op.gather_selected(short, K, [good[0]])
        assert ei.value.status == _ffi.INVALID
        with pytest.raises(query_amd.N1kError) as ei:  # a NULL array
            op.gather_selected(src, K, [good[0], (_ffi.COL_DICT32, None, None, None), good[2]])
        assert ei.value.status == _ffi.INVALID
        op.sync()
        out.check(host, want[:0].astype(np.int64))  # untouched: the sentinel everywhere
        op.gather_selected(op.make_device_batch(N_SRC, [a] * 16), K, [good[0]] * 16)  # 16 columns are fine
        op.sync()
    finally:
        op.done()


# ------------------------------------------------------------------------------------------------ 4. chain
def test_filter_gather_group_chain():
    """Filter handle -> gather of the plan's key and operand columns -> n1k_push_device_batch of the gathered batch into a
    handle built from the same query's InitialGroup without its Filter -> n1k_finish."""
    n = 100_003
    s = big()
    keys, aggs = [CAT], sorted(["sum(%s)" % PRICE, "count(*)", "min(%s)" % PRICE])
    ora = n1o.run(s["table"].slice(0, n), FAST, keys, aggs)
    f = filter_op(FAST)
    g = query_amd.GpuFilterGroup(plan.filter_group_plan(None, keys, aggs))
    try:
        g.intern(list(s["table"].dictionary))
        nsel, _ = f.filter_device_batch(big_batch(f, n))
        assert nsel == ora.rows_passed
        src_cols = {PRICE: (_ffi.COL_TAGGED64, s["tags"].data_ptr(), s["pay"].data_ptr(), None), CAT: (_ffi.COL_DICT32, None, None, s["cat"].data_ptr())}
        o_tags = torch.empty(nsel, dtype=torch.uint8, device="cuda")
        o_pay = torch.empty(nsel, dtype=torch.int64, device="cuda")
        o_cat = torch.empty(nsel, dtype=torch.int32, device="cuda")
        out_cols = {PRICE: (_ffi.COL_TAGGED64, o_tags.data_ptr(), o_pay.data_ptr(), None), CAT: (_ffi.COL_DICT32, None, None, o_cat.data_ptr())}
        torch.cuda.synchronize()
        f.gather_selected(f.make_device_batch(n, [src_cols[p] for p in g.column_paths]), nsel, [out_cols[p] for p in g.column_paths])
        f.sync()  # (the two handles have streams of their own)
        g.process_device_items(nsel, [out_cols[p] for p in g.column_paths])
        pu.assert_same_groups(g.after_items(), ora, aggs=aggs)
        assert g.stats()["rows_in"] == nsel
    finally:
        f.done()
        g.done()


# ------------------------------------------------------------------------------------------------ 5. errors, life cycle
def test_unsupported_data_stop_and_device_bytes():
    """`a < b` over two arrays that differ has no order on the device (ERR_UNSUPPORTED_VALUE): N1K_UNSUPPORTED_DATA through the
    three-call path and through the new call alike.  A stop before the call answers it.  Every byte goes with the handles."""
    L = _ffi.lib()
    big()
    live0 = L.n1k_device_bytes_live()
    A, B = D("a"), D("b")
    cond = "(%s < %s)" % (A, B)
    n = 10
    tags = np.full(n, n1o.T_INT, np.uint8)
    a, b = np.arange(n, dtype=np.uint64), np.arange(n, dtype=np.uint64)[::-1].copy()
    tags_a, tags_b = tags.copy(), tags.copy()
    tags_a[4] = tags_b[4] = n1o.T_ARRAY
    a[4], b[4] = 0, 1  # codes of "[1]" and "[2]"
    t = n1o.Table([n1o.Column(A, n1o.COL_TAGGED64, tags=tags_a, payload=a), n1o.Column(B, n1o.COL_TAGGED64, tags=tags_b, payload=b)], [b"[1]", b"[2]"])
    with pytest.raises(query_amd.N1kError) as ei:
        pu.run_gpu(t, cond, [], [], filter_only=True, device_resident=True)
    assert ei.value.status == _ffi.UNSUPPORTED_DATA
    dev = [torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda() for x in (tags_a, a, tags_b, b)]
    torch.cuda.synchronize()
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], [], filter_only=True))
    try:
        op.intern(list(t.dictionary))
        cols = {A: (_ffi.COL_TAGGED64, dev[0].data_ptr(), dev[1].data_ptr(), None), B: (_ffi.COL_TAGGED64, dev[2].data_ptr(), dev[3].data_ptr(), None)}
        batch = op.make_device_batch(n, [cols[p] for p in op.column_paths])
        with pytest.raises(query_amd.N1kError) as ei:
            op.filter_device_batch(batch)
        assert ei.value.status == _ffi.UNSUPPORTED_DATA
        with pytest.raises(query_amd.N1kError) as ei:  # and no selection is left
            op.selected_host32()
        assert ei.value.status == _ffi.INVALID
        # the same rows without the array pair: the handle goes on working
        nsel, _ = op.filter_device_batch(op.make_device_batch(4, [cols[p] for p in op.column_paths]))
        assert nsel == len(n1o.run(t.slice(0, 4), cond, [], [], has_group=False).selected)
        op.send_stop()
        with pytest.raises(query_amd.N1kError) as ei:
            op.filter_device_batch(batch)
        assert ei.value.status == _ffi.STOPPED
        op.reopen()  # reopen() forgets the stop
        assert op.filter_device_batch(op.make_device_batch(4, [cols[p] for p in op.column_paths]))[0] == nsel
        assert L.n1k_device_bytes_live() > live0
    finally:
        op.done()
    assert L.n1k_device_bytes_live() == live0
