"""String functions in Filter and HAVING on the device: the device evaluator against the host evaluator and the mirror,
and a differential against the oracle BY SUBSTITUTION — the oracle has no string functions, but it evaluates a bare path
inside AND / OR / NOT with the full 4-valued logic, so every string-function term of the device's plan becomes, for the
oracle, a helper column that holds the mirror's TRUE / FALSE / NULL / MISSING of that row (tests/strfn_util.py)."""
import os

import numpy as np
import pytest

import parity_util as pu
import query_amd
import strfn_util as su
from oracle import n1o
from query_amd import _ffi, plan

pytestmark = pytest.mark.gpu

D = su.D
DEV_MAX_LEN = su.DEV_MAX_LEN


# ------------------------------------------------------------------ the evaluators

def test_device_evaluator_equals_host_evaluator_and_mirror_on_the_cpu_tests_pairs():
    """`left` counts exactly what the rules send to the host: one of the four runes under the matching case step, bytes that
    are not valid UTF-8 under LIKE (no string here is beyond the length limit)."""
    total_left = 0
    for term, strings in su.random_pairs(20261018):
        text = su.term_text(D("s"), term)
        dev, left = su.device_eval(text, strings)
        host = su.host_eval(text, strings)
        want = np.array([su.strfn_mirror(s, term) for s in strings], dtype=np.uint8)
        assert np.array_equal(dev, host) and np.array_equal(dev, want), (text, strings)
        assert left == sum(su.left_to_host(s, term) for s in strings), (text, left, strings)
        total_left += left
    assert total_left > 200


LENGTH_TERMS = [([("lower", None), ("trim", None)], ("like", "%ab%a")), ([("upper", None)], ("contains", "ABBA")), ([], ("pos", "pos1", "bb", "<", 100, False)),
                ([("rtrim", "ab"), ("lower", None)], ("cmp", "<", "ab b", False)), ([("trim", "b \n"), ("upper", None)], ("between", "A", "AB"))]


def test_device_evaluator_on_every_length_at_every_alignment():
    """Lengths 0 to 130 bytes, 150 strings of each: the running offset puts every length at every alignment within a word.
    The entries of 128 bytes are taken, those from 129 on left to the host."""
    rng = np.random.default_rng(12)
    lens = np.tile(np.arange(0, 131), 150)
    rng.shuffle(lens)
    letters = np.frombuffer(b"abAB \n", np.uint8)
    strings = [bytes(rng.choice(letters, int(n))) for n in lens]
    offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
    assert len(strings) == 19650 and all(len({int(o) % 4 for o, n in zip(offs, lens) if n == k}) == 4 for k in (1, 127, 128, 129))
    excluded = int((lens > DEV_MAX_LEN).sum())
    assert excluded == 300
    for term in LENGTH_TERMS:
        text = su.term_text(D("s"), term)
        dev, left = su.device_eval(text, strings)
        host = su.host_eval(text, strings)
        want = np.array([su.strfn_mirror(s, term) for s in strings], dtype=np.uint8)
        assert left == excluded, (text, left)
        assert np.array_equal(dev, host) and np.array_equal(dev, want), text
        assert 0 < int(want[lens == 128].sum()) < 150 or term[1][0] == "pos", text  # (a mixed answer at the last length the kernel takes)


def test_device_evaluator_when_a_waves_strings_span_more_than_its_slab():
    """Runs of consecutive long strings with short ones in between: the 64 strings of such a wave span more than the 8 KiB
    LDS slab, and its lanes read the strings the kernel does take straight from global memory."""
    rng = np.random.default_rng(3)
    strings = []
    for block in range(200):
        for i in range(64):
            if block % 2 == 0 and i % 8 != 7:  # 56 strings of 150-260 B, every eighth one short: 64 strings span > 8 KiB
                n = int(rng.integers(150, 260))
            else:
                n = int(rng.integers(0, 20))
            t = "".join(rng.choice(list("aabBA_ \né"), n))
            if block % 2 == 0 and i % 16 == 3:
                t = "aB" * 50  # within the limit (100 B) inside a long run
            strings.append(t.encode())
    spans = [sum(len(s) for s in strings[w:w + 64]) for w in range(0, len(strings), 64)]
    assert max(spans) > 8192 and min(spans) < 8192
    excluded = sum(1 for s in strings if len(s) > DEV_MAX_LEN)
    taken_in_wide_waves = sum(1 for w in range(0, len(strings), 64) if spans[w // 64] > 8192 for s in strings[w:w + 64] if len(s) <= DEV_MAX_LEN)
    assert taken_in_wide_waves > 500
    for term in LENGTH_TERMS[:3] + [([("lower", None)], ("like", "ab%ab"))]:
        text = su.term_text(D("s"), term)
        dev, left = su.device_eval(text, strings)
        host = su.host_eval(text, strings)
        want = np.array([su.strfn_mirror(s, term) for s in strings], dtype=np.uint8)
        assert left == excluded and np.array_equal(dev, host) and np.array_equal(dev, want), text


BLOCK_EDGES = [1, 63, 64, 65, 255, 256, 257]  # the last lane's clamp, a full wave, a wave of one lane, a second workgroup of one string


def test_device_evaluator_at_the_edges_of_a_block():
    """Blocks that end inside a wave, on a wave and one string into the next workgroup; strings of 0 to 40 bytes.  Once more
    with a last string of 10 KB: the final wave then spans more than its slab and reads what it takes from global memory."""
    rng = np.random.default_rng(11)
    pool = ["".join(rng.choice(list("aabBA_ \néK"), int(rng.integers(0, 41)))).encode()[:40] for _ in range(max(BLOCK_EDGES))]
    pool[5] = pool[5][:3] + b"\xff"
    huge = b"aB" * 5000
    term = ([("lower", None), ("trim", None)], ("like", "%ab%"))
    text = su.term_text(D("s"), term)
    for n in BLOCK_EDGES:
        for last in (None, huge):
            strings = pool[:n] if last is None else pool[:n - 1] + [last]
            dev, left = su.device_eval(text, strings)
            host = su.host_eval(text, strings)
            want = np.array([su.strfn_mirror(s, term) for s in strings], dtype=np.uint8)
            assert np.array_equal(dev, host) and np.array_equal(dev, want), (n, last is None, np.nonzero(dev != host))
            assert left == sum(su.left_to_host(s, term) for s in strings), (n, last is None, left)
        assert n < 64 or 0 < int(host.sum()) < n


def _strings_table(strings, dictionary, groups=None):
    n = len(strings)
    index = {x: i for i, x in enumerate(dictionary)}
    codes = np.array([index[x] for x in strings], dtype=np.uint32)
    g = np.array(groups if groups is not None else [0] * n, dtype=np.uint64)
    return n1o.Table([n1o.Column(D("s"), n1o.COL_DICT32, codes=codes),
                      n1o.Column(D("g"), n1o.COL_TAGGED64, tags=np.full(n, n1o.T_INT, np.uint8), payload=g)], dictionary)


def test_eight_predicates_at_once_on_both_routes():
    """Eight distinct string-function predicates fill the byte; a condition that pairs each with the negation of the next
    is TRUE for the rows the mirror says, so no predicate reads another's bit.  2000 dictionary strings: the device route;
    200: the host route."""
    terms = [([("lower", None)], ("cmp", "=", "ab", False)), ([("upper", None)], ("contains", "B")), ([("trim", None)], ("cmp", "<", "b", False)),
             ([], ("contains", "a")), ([("lower", None), ("trim", "a")], ("like", "b%")), ([], ("pos", "position", "b", "=", 1, False)),
             ([("rtrim", None)], ("cmp", "=", "ab", False)), ([("upper", None)], ("like", "%A"))]
    texts = [su.term_text(D("s"), t) for t in terms]
    cond = "(%s)" % " or ".join("(%s and (not %s))" % (texts[i], texts[i + 1]) for i in range(0, 8, 2))
    for n in (2000, 200):
        rng = np.random.default_rng(n)
        dictionary = sorted({bytes(rng.choice(np.frombuffer(b"abAB  ", np.uint8), int(rng.integers(0, 7)))) for _ in range(8 * n)})[:n]
        dictionary[7] = "İab".encode()  # the host's, under lower, on either route
        assert len(dictionary) == n
        codes = rng.integers(0, n, 50_000).astype(np.uint32)
        t = n1o.Table([n1o.Column(D("s"), n1o.COL_DICT32, codes=codes)], dictionary)
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], ["count(*)"]))
        op.process_items(t.columns, dictionary)
        rows = op.after_items()
        stats = op.strfn_stats()
        op.done()
        hit = np.array([any(su.strfn_mirror(s, terms[i]) and not su.strfn_mirror(s, terms[i + 1]) for i in range(0, 8, 2)) for s in dictionary])
        assert 0 < hit.sum() < n and rows.aggs[0][0][1] == int(hit[codes].sum()), (n, rows.aggs)
        assert stats["predicates"] == 8
        if n == 2000:
            assert stats["device_strings"] == n - 1 and stats["host_strings"] == 1, stats
        else:
            assert stats["device_strings"] == 0 and stats["host_strings"] == n, stats


# ------------------------------------------------------------------ differential by substitution

# NOTE: tests/test_strfn_cpu.py (test_the_bounded_family_takes_the_gpu_differentials_bounded_plans) re-derives the bounded
# plans of this test through the same su.draw_plan, to check without a GPU that the bounded family takes them.
@pytest.mark.parametrize("seed", range(int(os.environ.get("N1K_STRFN_SEEDS", str(su.SEEDS)))))
def test_strfn_plans_agree_with_the_oracle_by_substitution(seed):
    t, (opts, bounded, kernel), (sub, dcond, ocond, keys, aggs), batches = su.draw_plan(seed)
    what = "device %r oracle %r keys %r aggs %r opts %r batches %d" % (dcond, ocond, keys, aggs, opts, batches)
    ot = sub.oracle_table()
    # Filter-only: the selected row ordinals (a skip or N1K_UNSUPPORTED is a failure: the generator draws supported constructs)
    gsel, _ = pu.run_gpu(t, dcond, [], [], filter_only=True, batches=batches)
    osel = n1o.run(ot, ocond, [], [], has_group=False)
    assert np.array_equal(np.asarray(gsel.selected, dtype=np.uint64), osel.selected), what  # ordered row ordinals, as they come
    # grouped
    gpu, st = pu.run_gpu(t, dcond, keys, aggs, batches=batches, **opts)
    ora = n1o.run(ot, ocond, keys, aggs, threads=2)
    try:
        pu.assert_same_groups(gpu, ora, aggs=aggs)
    except AssertionError as e:
        raise AssertionError("%s | %s" % (e, what))
    assert st["spec_kernel"] == kernel, (st["spec_kernel"], what)
    assert st["rows_selected"] == ora.rows_passed, what


# ------------------------------------------------------------------ the match table's life

def test_strfn_when_the_dictionary_grows_between_batches():
    """Strings interned after the first push — some of which hold — are seen by the later batches: the table is extended
    for the new codes only.  n1k_reset keeps it."""
    cond, keys, aggs = '(lower(trim(%s)) like "new%%")' % D("s"), [D("g")], ["count(*)"]
    d1 = [b"old", b"NEWer"]
    d2 = [b"old", b"NEWer", b" New ", b"news\n", b"renew", b"x\nnEw"]
    b1 = _strings_table([b"old", b"NEWer", b"old"], d1, [0, 0, 1])
    b2 = _strings_table([b" New ", b"news\n", b"renew", b"x\nnEw", b"old", b"NEWer"], d2, [0, 1, 1, 2, 2, 2])
    want = {0: 2, 1: 1, 2: 2}
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs))
    for round_ in range(2):
        for b in (b1, b2):
            op.process_items([{c.name: c for c in b.columns}[p] for p in op.column_paths], b.dictionary)
        rows = op.after_items()
        assert {k[0][1]: a[0][1] for k, a in zip(rows.keys, rows.aggs)} == want
        stats = op.strfn_stats()
        # every dictionary string (the batches' and the three a TAGGED64 key column makes the handle intern: NaN, ±Infinity)
        # evaluated exactly once — also after the reset, which keeps the table
        ndict = int(_ffi.lib().n1k_dict_size(op._h))
        assert ndict >= len(d2) and stats["host_strings"] == ndict and stats["device_strings"] == 0, (stats, ndict)
        op.reopen()
    op.done()


def test_a_large_dictionary_takes_the_device_route_and_a_small_one_the_host_route():
    probe = query_amd.GpuFilterGroup(plan.filter_group_plan('(lower(%s) = "a")' % D("s"), [], ["count(*)"]))
    threshold = probe.strfn_stats()["device_threshold"]
    probe.done()
    assert threshold == 1024
    terms = [([("upper", None)], ("like", "%7_")), ([("lower", None), ("ltrim", "s")], ("like", "1%5"))]
    cond = "(%s or %s)" % tuple(su.term_text(D("s"), x) for x in terms)
    for n, route in ((threshold, "device"), (threshold - 1, "host")):
        texts = [("s%d" if i % 2 else "S%d") % i for i in range(n)]
        texts[3] = "x" * 300 + "75"  # beyond the kernel's limit: the host evaluator's, on either route
        dictionary = [x.encode() for x in texts]
        rng = np.random.default_rng(n)
        codes = rng.integers(0, n, 100_000).astype(np.uint32)
        t = n1o.Table([n1o.Column(D("s"), n1o.COL_DICT32, codes=codes)], dictionary)
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], ["count(*)"]))
        op.process_items(t.columns, dictionary)
        rows = op.after_items()
        stats = op.strfn_stats()
        op.done()
        hit = np.array([su.strfn_mirror(x, terms[0]) or su.strfn_mirror(x, terms[1]) for x in dictionary])
        assert 0 < hit.sum() < n and rows.aggs[0][0][1] == int(hit[codes].sum())
        if route == "device":
            assert stats["device_strings"] == n - 1 and stats["host_strings"] == 1, stats
        else:
            assert stats["device_strings"] == 0 and stats["host_strings"] == n, stats


@pytest.mark.parametrize("nwords", [4095, 4097])
def test_strfn_term_on_both_sides_of_the_lds_switch(nwords):
    """The bounded and the run-time-built kernels stage a match table of at most 4096 entries in LDS and read a larger one
    from global memory: one entry below and one above, DICT32 and TAGGED64 string column, against the oracle by
    substitution."""
    rng = np.random.default_rng(nwords)
    words = [("w%dA%sb" if i % 2 else "W%da%sB ") % (i, "x" * (i % 3)) for i in range(nwords)]
    n = 30_000
    sc = rng.integers(0, nwords, n).astype(np.uint32)
    sc[:2] = [0, nwords - 1]
    sc[rng.random(n) < 0.03] = 0xFFFFFFFE
    mt = np.full(n, n1o.T_STRING, np.uint8)
    mp = rng.integers(0, nwords, n).astype(np.uint64)
    mp[:2] = [nwords - 1, 0]
    mt[rng.random(n) < 0.05] = n1o.T_NULL
    xt = np.full(n, n1o.T_INT, np.uint8)
    xp = rng.integers(0, 100, n).astype(np.int64).view(np.uint64).copy()
    term = ([("lower", None), ("rtrim", None)], ("like", "w%7a_b"))
    holds = {w: su.strfn_mirror(w.encode(), term) for w in words}
    for col, scol in (("s", n1o.Column(D("s"), n1o.COL_DICT32, codes=sc)), ("m", n1o.Column(D("m"), n1o.COL_TAGGED64, tags=mt, payload=mp))):
        vals = [None if (c == 0xFFFFFFFE if col == "s" else tg == n1o.T_NULL) else words[int(c)]
                for c, tg in zip((sc if col == "s" else mp).tolist(), mt.tolist())]
        ht = np.array([n1o.T_NULL if v is None else (n1o.T_TRUE if holds[v] else n1o.T_FALSE) for v in vals], np.uint8)
        cols = [scol, n1o.Column(D("x"), n1o.COL_TAGGED64, tags=xt, payload=xp)]
        t = n1o.Table(cols, [w.encode() for w in words])
        ot = n1o.Table(cols + [n1o.Column(D("h"), n1o.COL_TAGGED64, tags=ht, payload=np.zeros(n, np.uint64))], t.dictionary)
        dcond = "(%s and (10 < %s))" % (su.term_text(D(col), term), D("x"))
        ocond = "(%s and (10 < %s))" % (D("h"), D("x"))
        aggs = sorted(["count(*)", "sum(%s)" % D("x")])
        ora = n1o.run(ot, ocond, [], aggs)
        assert 0 < ora.rows_passed < n // 2
        for opts, kernel in (({"jit": 2}, 2), ({"spec": 0}, 0), ({"fast": 0}, 0)):
            gpu, st = pu.run_gpu(t, dcond, [], aggs, batches=2, **opts)
            pu.assert_same_groups(gpu, ora, aggs=aggs)
            assert st["spec_kernel"] == kernel and st["rows_selected"] == ora.rows_passed, (nwords, col, opts, st)


# ------------------------------------------------------------------ HAVING and the exchange

def test_having_strfn_over_a_string_group_key():
    rng = np.random.default_rng(9)
    t = su.make_table(rng, 4000)
    keys, aggs = [D("k")], ["count(*)"]
    ora = n1o.run(t, None, keys, aggs)
    term = ([("lower", None)], ("like", "cat\\_1%"))
    text = 'lower(%s) like "cat\\\\_1%%"' % D("k")
    for having, keep in [("(%s)" % text, lambda v: v is True), ("(not (%s))" % text, lambda v: v is False)]:
        gpu, _ = pu.run_gpu(t, None, keys, aggs, having=having)

        def val(k):
            return su.MISSING if k[0] == n1o.T_MISSING else (None if k[0] != n1o.T_STRING else k[1])
        want = sorted((k[0], a[0][1]) for k, a in zip(ora.keys, ora.aggs) if keep(su.strfn4(val(k[0]), term)))
        got = sorted((k[0], a[0][1]) for k, a in zip(gpu.keys, gpu.aggs))
        assert got == want and len(want) >= 2 and len(want) < len(ora.keys), (having, got, want)
    # the key is NULL / MISSING in some groups: the negation keeps neither (NULL / MISSING are not TRUE)
    assert any(k[0][0] == n1o.T_NULL for k in ora.keys) and any(k[0][0] == n1o.T_MISSING for k in ora.keys)


@pytest.mark.timeout(600)
def test_strfn_across_two_ranks_over_the_loopback_transport():
    """World size 2, row exchange: the sender evaluates the Filter — the string-function term through its own handle's table —
    and every rank ends with the substituted oracle's groups."""
    from query_amd import distributed as qd
    from query_amd.gpu_operator import GroupRows
    from test_gpu_distributed import _device_cols, _run_ranks
    world, n, jit = 2, 60_011, 2
    rng = np.random.default_rng(33)
    t = su.make_table(rng, n)
    sub = su.Substitution(t)
    d, o = sub.strfn("s", ([("lower", None), ("trim", None)], ("like", "%ab%")))
    dcond, ocond = "(%s and (10 < %s))" % (d, D("x")), "(%s and (10 < %s))" % (o, D("x"))
    keys, aggs = [D("k")], sorted(["count(*)", "sum(%s)" % D("x")])
    ora = n1o.run(sub.oracle_table(), ocond, keys, aggs)
    assert 0 < ora.rows_passed < n
    comms = qd.Comm.loopback(world, 0)
    probe = query_amd.GpuFilterGroup(plan.filter_group_plan(dcond, keys, aggs))
    paths = probe.column_paths
    probe.done()
    shards, keep = [], []
    for r in range(world):
        dev, k = _device_cols(t.slice(n * r // world, n * (r + 1) // world), paths)
        keep.append(k)
        shards.append((n * (r + 1) // world - n * r // world, dev))

    def rank_body(r):
        op = qd.ShardedFilterGroup(dcond, keys, aggs, t.dictionary, r, world, 0, comm=comms[r])
        for h in (op.sender, op.receiver):
            h.set_option("jit", jit)
        op.row_capacity = 2 * n
        raw, info = op.run_rows(*shards[r])
        info["sender_kernel"] = op.sender.stats()["spec_kernel"]
        cache = {}
        return GroupRows(1, len(aggs), op.merger._py_values(raw["keys"], cache), op.merger._py_values(raw["aggs"], cache), []), info

    outs = _run_ranks(world, rank_body)
    for rows, info in outs:
        pu.assert_same_groups(rows, ora, aggs=aggs)
        assert info["mode"] == "rows"
        assert info["sender_kernel"] != 0, info  # scan_spec_partition_body saw the string-function term
    assert sum(info["recv_rows"] for _, info in outs) == ora.rows_passed
