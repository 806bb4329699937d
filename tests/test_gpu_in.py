"""IN / NOT IN over a constant list on the device: the device matcher of the list's strings against the host matcher and
python's set, and a differential against the oracle BY EXPANSION — the oracle has no IN, but for a non-empty list the term
equals the 4-valued `((x = c1) or (x = c2) or ...)`, which it evaluates (tests/in_util.py; tests/test_in_cpu.py checks the
yardstick).  Lists too long to expand reach the oracle by substitution: a helper column of in4's results."""
import functools

import numpy as np
import pytest

import in_util as iu
import parity_util as pu
import query_amd
from oracle import n1o
from query_amd import _ffi, plan

pytestmark = pytest.mark.gpu

MISSING = iu.MISSING


def D(name):
    return plan.field_path("default", name)


# ------------------------------------------------------------------ the matchers

BLOCK_EDGES = [1, 63, 64, 65, 255, 256, 257]  # the last lane's clamp, a full wave, a wave of one lane, a second workgroup of one string
LIST_SIZES = [1, 3, 1000, iu.IN_MAX_STRINGS]


def _pool(rng, n, lo=0, hi=25):
    """n distinct byte strings of lo..hi-1 bytes, any byte values (the empty string at most once)"""
    seen, out = set(), []
    while len(out) < n:
        s = rng.integers(0, 256, int(rng.integers(lo, hi)), dtype=np.uint8).tobytes()
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def _list_for(rng, strings, size):
    """`size` distinct constants, about half of them present in `strings`"""
    present = list(dict.fromkeys(strings))
    take = [present[i] for i in rng.choice(len(present), min(size // 2 + size % 2, len(present)), replace=False)]
    have = set(strings)
    while len(take) < size:
        s = rng.integers(0, 256, int(rng.integers(1, 30)), dtype=np.uint8).tobytes()
        if s not in have:
            have.add(s)
            take.append(s)
    return take


def _check(strings, consts, what):
    text = iu.list_text(consts)
    dev, left = iu.device_match(text, strings)
    host = iu.host_match(text, strings)
    cs = set(consts)
    want = np.fromiter((s in cs for s in strings), dtype=np.uint8, count=len(strings))
    assert left == sum(1 for s in strings if len(s) > iu.DEV_MAX_LEN), (what, left)  # exact: the documented limit and nothing else
    assert np.array_equal(dev, host) and np.array_equal(dev, want), (what, np.nonzero(dev != want)[0][:8])
    return int(want.sum())


def test_device_matcher_at_the_edges_of_a_block():
    """Blocks that end inside a wave, on a wave and one string into the next workgroup.  Once more with a last string of
    10 KB: the final wave then spans more than its slab and reads what it takes from global memory."""
    rng = np.random.default_rng(11)
    pool = _pool(rng, max(BLOCK_EDGES), 0, 41)
    huge = b"ab" * 5000
    consts = _list_for(rng, pool[:60], 40) + [huge]
    for n in BLOCK_EDGES:
        for last in (None, huge):
            strings = pool[:n] if last is None else pool[:n - 1] + [last]
            hits = _check(strings, consts, (n, last is None))
            assert n < 64 or 0 < hits < n


@functools.lru_cache(maxsize=1)
def _two_hundred_thousand():
    rng = np.random.default_rng(77)
    n = 200_000
    lens = rng.integers(0, 25, n)
    long_ix = rng.choice(n, 3000, replace=False)
    lens[long_ix] = rng.integers(120, 169, 3000)
    raw = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8).tobytes()
    cuts = np.concatenate([[0], np.cumsum(lens)])
    strings = [raw[cuts[i]:cuts[i + 1]] for i in range(n)]
    strings[::1000] = [b"dup"] * len(strings[::1000])  # the same string many times in one block
    assert min(len(s) for s in strings) == 0 and sum(1 for s in strings if len(s) > iu.DEV_MAX_LEN) > 1000
    return strings, [strings[i] for i in long_ix[:50]]


@pytest.mark.parametrize("size", LIST_SIZES)
def test_device_matcher_on_two_hundred_thousand_strings(size):
    """One block of strings of 0-24 bytes of any value with 3 000 of 120-168 bytes among them; about half the list's
    constants are in the block.  out_left_to_host counts exactly the strings over 128 bytes."""
    strings, some_long = _two_hundred_thousand()
    consts = _list_for(np.random.default_rng(size), some_long + strings[:20000], size)
    hits = _check(strings, consts, size)
    assert 0 < hits < len(strings)


def test_device_matcher_when_a_waves_strings_span_more_than_its_slab():
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
            s = rng.integers(97, 101, n, dtype=np.uint8).tobytes()
            if block % 2 == 0 and i % 16 == 3:
                s = b"ab" * 50  # within the limit (100 B) inside a long run
            strings.append(s)
    spans = [sum(len(s) for s in strings[w:w + 64]) for w in range(0, len(strings), 64)]
    assert max(spans) > 8192 and min(spans) < 8192
    consts = [b"ab" * 50, b"", b"a", b"ab", b"abc", strings[0], b"nope"] + [s for s in strings[64:128] if s][:20]
    consts = list(dict.fromkeys(consts))
    hits = _check(strings, consts, "slab")
    assert 0 < hits < len(strings)


# ------------------------------------------------------------------ differential by expansion

WORDS = ["", "a", "ab", "abc", "b", "ba", "3", "3.0", "true", "null", "é", "a\U0001F600b", "a\\b", "x\ny", "cat_1", "cat_10", "cat_11", "cat_2", "zz"]
DICT = [w.encode() for w in WORDS] + [b"[1,2]", b"[\"ab\"]"]
ARR0 = len(WORDS)
FLOATS = [0.0, 1.0, 2.5, 3.0, 3.5, 7.0, -0.0, 9.25, -2.0]
CONSTS = ["a", "ab", "b", "3", "true", "é", "cat_1", "cat_11", "zz", "nope", "", "x\ny", 0, 1, 3, 3.0, -2, 2.5, 3.5, 9.25, 7, 50, -0.5, True, False]


def make_table(rng, n):
    """s: DICT32 strings with NULL / MISSING; m: TAGGED64 of every class (strings, INTs, FLOATs, booleans, NULL, MISSING,
    arrays); x: numbers, INT and FLOAT with equal values (3 and 3.0, 0 and -0.0); k: DICT32 key; g: small ints."""
    sc = rng.integers(0, len(WORDS), n).astype(np.uint32)
    sc[rng.random(n) < 0.05] = 0xFFFFFFFE
    sc[rng.random(n) < 0.05] = 0xFFFFFFFF
    mt = np.zeros(n, np.uint8)
    mp = np.zeros(n, np.uint64)
    r = rng.integers(0, 100, n)
    st = r < 40
    mt[st] = n1o.T_STRING
    mp[st] = rng.integers(0, len(WORDS), int(st.sum())).astype(np.uint64)
    it = (r >= 40) & (r < 52)
    mt[it] = n1o.T_INT
    mp[it] = rng.integers(-3, 4, int(it.sum())).astype(np.int64).view(np.uint64)
    ft = (r >= 52) & (r < 64)
    mt[ft] = n1o.T_FLOAT
    mp[ft] = np.array(FLOATS)[rng.integers(0, len(FLOATS), int(ft.sum()))].view(np.uint64)
    mt[(r >= 64) & (r < 70)] = n1o.T_TRUE
    mt[(r >= 70) & (r < 76)] = n1o.T_FALSE
    mt[(r >= 76) & (r < 84)] = n1o.T_NULL
    mt[(r >= 84) & (r < 92)] = n1o.T_MISSING
    ar = r >= 92
    mt[ar] = n1o.T_ARRAY
    mp[ar] = (ARR0 + rng.integers(0, 2, int(ar.sum()))).astype(np.uint64)
    xt = np.full(n, n1o.T_FLOAT, np.uint8)
    xp = np.array(FLOATS)[rng.integers(0, len(FLOATS), n)].view(np.uint64).copy()
    ints = rng.random(n) < 0.5
    xt[ints] = n1o.T_INT
    xp[ints] = rng.integers(-2, 10, int(ints.sum())).astype(np.int64).view(np.uint64)
    xt[rng.random(n) < 0.03] = n1o.T_NULL
    kc = rng.integers(14, 19, n).astype(np.uint32)  # cat_1 .. zz
    kc[rng.random(n) < 0.04] = 0xFFFFFFFE
    kc[rng.random(n) < 0.03] = 0xFFFFFFFF
    gt = np.full(n, n1o.T_INT, np.uint8)
    gp = rng.integers(0, 7, n).astype(np.int64).view(np.uint64).copy()
    return n1o.Table([n1o.Column(D("s"), n1o.COL_DICT32, codes=sc), n1o.Column(D("m"), n1o.COL_TAGGED64, tags=mt, payload=mp),
                      n1o.Column(D("x"), n1o.COL_TAGGED64, tags=xt, payload=xp), n1o.Column(D("k"), n1o.COL_DICT32, codes=kc),
                      n1o.Column(D("g"), n1o.COL_TAGGED64, tags=gt, payload=gp)], list(DICT))


def column_values(t, name, words=WORDS):
    """The python values of a column: str, int, float, bool, None (NULL), MISSING, or a list for an ARRAY."""
    c = {c.name: c for c in t.columns}[D(name)]
    if c.kind == n1o.COL_DICT32:
        return [MISSING if x == 0xFFFFFFFF else (None if x == 0xFFFFFFFE else words[x]) for x in c.codes.tolist()]
    out = []
    fl = c.payload.view(np.float64)
    sg = c.payload.view(np.int64)
    for i, tg in enumerate(c.tags.tolist()):
        out.append(MISSING if tg == n1o.T_MISSING else None if tg == n1o.T_NULL else True if tg == n1o.T_TRUE else False if tg == n1o.T_FALSE
                   else int(sg[i]) if tg == n1o.T_INT else float(fl[i]) if tg == n1o.T_FLOAT else words[int(c.payload[i])] if tg == n1o.T_STRING else [])
    return out


def rand_list(rng, col):
    """1 to 6 constants, mixed; leaning to the classes the column holds; sometimes `null`, sometimes a duplicate"""
    n = int(rng.integers(1, 7))
    strs = [c for c in CONSTS if isinstance(c, str)]
    nums = [c for c in CONSTS if not isinstance(c, str)]
    out = []
    for _ in range(n):
        pool = CONSTS if rng.random() < 0.4 else (nums if col in ("x", "g") else strs if col in ("s", "k") else CONSTS)
        out.append(pool[int(rng.integers(0, len(pool)))])
    if rng.random() < 0.2:
        out[int(rng.integers(0, n))] = None
    return out


def in_pair(rng, col):
    consts = rand_list(rng, col)
    return iu.term(D(col), consts, folded=rng.random() < 0.3), iu.expand(D(col), consts)


def other_term(rng):
    r = rng.integers(0, 6)
    if r == 0: return "(%s < %s)" % (["1", "2.5", "7"][rng.integers(0, 3)], D("x"))
    if r == 1: return "(%s <= %s)" % (D("x"), ["3", "3.25"][rng.integers(0, 2)])
    if r == 2: return "(%s = %s)" % (D("s"), ["\"ab\"", "\"cat_1\""][rng.integers(0, 2)])
    if r == 3: return "(%s is %s)" % (D(["m", "s", "x"][rng.integers(0, 3)]), ["null", "not null", "missing", "valued"][rng.integers(0, 4)])
    if r == 4: return "(%s between 2 and 5)" % D("g")
    return "((%s + %s) < 8)" % (D("x"), D("g"))


def rand_tree(rng, budget, depth=0):
    """A condition with IN terms among the existing kinds: (device text, oracle text)."""
    r = rng.integers(0, 10)
    if depth < 2 and r < 4:
        op = ["and", "or"][rng.integers(0, 2)]
        parts = [rand_tree(rng, budget, depth + 1) for _ in range(int(rng.integers(2, 4)))]
        return "(%s)" % (" %s " % op).join(p[0] for p in parts), "(%s)" % (" %s " % op).join(p[1] for p in parts)
    if depth < 3 and r == 4:
        d, o = rand_tree(rng, budget, depth + 1)
        return "(not %s)" % d, "(not %s)" % o
    if budget[0] > 0 and (r < 8 or budget[1] == 0):
        budget[0] -= 1
        budget[1] += 1
        return in_pair(rng, ["s", "m", "x", "m"][rng.integers(0, 4)])
    t = other_term(rng)
    return t, t


def rand_in_plan(rng, bounded):
    if bounded:
        # the bounded family: an IN term over a column as one of <= 2 ANDed terms, <= 3 columns, dictionary key
        d, o = in_pair(rng, ["s", "m", "x"][rng.integers(0, 3)])
        if rng.random() < 0.75:
            second = ["(%s < %s)" % (["1", "2.5"][rng.integers(0, 2)], D("x")), "(%s is not null)" % D("x"), "(%s <= 7)" % D("x")][rng.integers(0, 3)]
            if rng.random() < 0.5:
                d, o = "(%s and %s)" % (d, second), "(%s and %s)" % (o, second)
            else:
                d, o = "(%s and %s)" % (second, d), "(%s and %s)" % (second, o)
        keys = [D("k")]
        aggs = sorted(set(["sum(%s)" % D("x")] + [["count(*)", "avg(%s)" % D("x"), "max(%s)" % D("x"), "count(%s)" % D("x")][i]
                                                   for i in rng.choice(4, int(rng.integers(0, 3)), replace=False)]))
        return d, o, keys, aggs
    budget = [int(rng.integers(1, 4)), 0]
    for _ in range(50):
        b = list(budget)
        d, o = rand_tree(rng, b)
        if 1 <= b[1] <= 3:
            break
    else:
        d, o = in_pair(rng, "s")
    keys = [[D("k")], [D("g")], [D("k"), D("g")], []][rng.integers(0, 4)]
    aggs = sorted(set(["count(*)"] + [["sum(%s)" % D("x"), "avg(%s)" % D("x"), "min(%s)" % D("s"), "max(%s)" % D("x"), "count(%s)" % D("m")][i]
                                      for i in rng.choice(5, int(rng.integers(1, 3)), replace=False)]))
    return d, o, keys, aggs


# NOTE: tests/test_in_cpu.py re-derives the plans of this test from FAMILIES, the seed base 616_000 and the order of the
# draws (table size, then rand_in_plan, then the batch count) to check without a GPU that every plan is accepted and that
# the bounded family takes the bounded ones: change those here and that test follows.
# (options, bounded shape, the kernel family stats["spec_kernel"] must report: 0 interpreter / bounded kernel, 2 run-time built)
FAMILIES = [({"fast": 0}, False, 0), ({}, False, 0), ({"fast": 0}, True, 0), ({"spec": 0}, True, 0), ({"jit": 2}, True, 2), ({"jit": 2}, True, 2)]
SEED_BASE = 616_000
SEEDS = 240


@pytest.mark.parametrize("seed", range(SEEDS))
def test_in_plans_agree_with_the_oracle_by_expansion(seed):
    rng = np.random.default_rng(SEED_BASE + seed)
    t = make_table(rng, int(rng.integers(1, 5000)))
    opts, bounded, kernel = FAMILIES[seed % len(FAMILIES)]
    dcond, ocond, keys, aggs = rand_in_plan(rng, bounded)
    batches = int(rng.integers(1, 4))
    what = "device %r oracle %r keys %r aggs %r opts %r batches %d" % (dcond, ocond, keys, aggs, opts, batches)
    # Filter-only: the selected row ordinals (a skip or N1K_UNSUPPORTED is a failure: the generator draws supported constructs)
    gsel, _ = pu.run_gpu(t, dcond, [], [], filter_only=True, batches=batches)
    osel = n1o.run(t, ocond, [], [], has_group=False)
    assert np.array_equal(np.asarray(gsel.selected, dtype=np.uint64), osel.selected), what  # ordered row ordinals, as they come
    # grouped
    gpu, st = pu.run_gpu(t, dcond, keys, aggs, batches=batches, **opts)
    ora = n1o.run(t, ocond, keys, aggs, threads=2)
    try:
        pu.assert_same_groups(gpu, ora, aggs=aggs)
    except AssertionError as e:
        raise AssertionError("%s | %s" % (e, what))
    assert st["spec_kernel"] == kernel, (st["spec_kernel"], what)
    assert st["rows_selected"] == ora.rows_passed, what


# ------------------------------------------------------------------ by substitution: what cannot be expanded

class Substitution:
    """The device sees the IN term, the oracle a helper column of in4's results for that row."""

    def __init__(self, table, words=WORDS):
        self.table, self.words, self.helpers = table, words, []

    def term(self, col, consts, folded=False):
        vals = column_values(self.table, col, self.words)
        f = iu.matcher(consts)
        tags = np.array([iu.tag_of(f(v), n1o) for v in vals], np.uint8)
        name = D("h%d" % len(self.helpers))
        self.helpers.append(n1o.Column(name, n1o.COL_TAGGED64, tags=tags, payload=np.zeros(len(vals), np.uint64)))
        return iu.term(D(col), consts, folded), name

    def oracle_table(self):
        return n1o.Table(list(self.table.columns) + self.helpers, self.table.dictionary)


def _int_col(name, values):
    v = np.asarray(values, dtype=np.int64)
    return n1o.Column(D(name), n1o.COL_TAGGED64, tags=np.full(len(v), n1o.T_INT, np.uint8), payload=v.view(np.uint64).copy())


@pytest.mark.parametrize("nwords", [3000, 6000])
def test_long_lists_on_both_sides_of_the_lds_switch(nwords):
    """A 1000-string list and a 1024-number list in one plan, over dictionaries of 3000 and of 6000 strings (the bounded and
    the run-time-built kernels stage a match table of at most 4096 entries in LDS and read a larger one from global memory),
    DICT32 and TAGGED64 string column, NOT IN through the interpreter."""
    rng = np.random.default_rng(nwords)
    words = ["w%da%sb" % (i, "x" * (i % 3)) for i in range(nwords)]
    n = 20_000
    sc = rng.integers(0, nwords, n).astype(np.uint32)
    sc[rng.random(n) < 0.03] = 0xFFFFFFFE
    sc[rng.random(n) < 0.02] = 0xFFFFFFFF
    mt = np.full(n, n1o.T_STRING, np.uint8)
    mp = rng.integers(0, nwords, n).astype(np.uint64)
    mt[rng.random(n) < 0.05] = n1o.T_NULL
    odd = rng.random(n) < 0.05
    mt[odd] = n1o.T_INT
    mp[odd] = 7
    xt = np.full(n, n1o.T_INT, np.uint8)
    xv = rng.integers(0, 4096, n).astype(np.int64)
    fl = rng.random(n) < 0.3
    xt[fl] = n1o.T_FLOAT
    xp = xv.view(np.uint64).copy()
    xp[fl] = (xv[fl] / 2.0).view(np.uint64)  # halves: integral ones equal INT constants, the others equal nothing
    cols = [n1o.Column(D("s"), n1o.COL_DICT32, codes=sc), n1o.Column(D("m"), n1o.COL_TAGGED64, tags=mt, payload=mp),
            n1o.Column(D("x"), n1o.COL_TAGGED64, tags=xt, payload=xp), _int_col("g", rng.integers(0, 5, n))]
    t = n1o.Table(cols, [w.encode() for w in words])
    strs = [words[i] for i in rng.choice(nwords, 700, replace=False)] + ["absent%d" % i for i in range(300)]
    nums = [int(v) for v in rng.choice(4096, iu.IN_MAX_NUMBERS, replace=False)]
    aggs = sorted(["count(*)", "sum(%s)" % D("x")])
    for col in ("s", "m"):
        sub = Substitution(t, words)
        ds, os_ = sub.term(col, strs)
        dn, on = sub.term("x", nums, folded=True)
        ot = sub.oracle_table()
        for dcond, ocond, families in (
                ("(%s and %s)" % (ds, dn), "(%s and %s)" % (os_, on), (({"jit": 2}, 2), ({"spec": 0}, 0), ({"fast": 0}, 0))),
                ("((not %s) or %s)" % (ds, dn), "((not %s) or %s)" % (os_, on), (({}, 0),))):
            for keys in ([], [D("g")]):
                ora = n1o.run(ot, ocond, keys, aggs)
                assert 0 < ora.rows_passed < n
                for opts, kernel in families:
                    gpu, st = pu.run_gpu(t, dcond, keys, aggs, batches=2, **opts)
                    pu.assert_same_groups(gpu, ora, aggs=aggs)
                    assert st["spec_kernel"] == kernel and st["rows_selected"] == ora.rows_passed, (nwords, col, keys, opts, st)


def test_numeric_edges():
    """INT 3 against 3.0 and FLOAT 3.0 against 3; -0.0 against 0; NaN equals nothing; INT 2^53 + 1 is not the constant
    2^53 although their doubles are equal; the first and the last constant of the sorted array and one past either end; two
    lists of one plan sharing the array; the empty list."""
    big = 1 << 53
    rows = [(n1o.T_INT, 3), (n1o.T_FLOAT, 3.0), (n1o.T_FLOAT, -0.0), (n1o.T_INT, 0), (n1o.T_FLOAT, float("nan")), (n1o.T_INT, big + 1),
            (n1o.T_INT, big), (n1o.T_FLOAT, float(big)), (n1o.T_INT, -big), (n1o.T_INT, -big - 1), (n1o.T_INT, 10), (n1o.T_INT, 11), (n1o.T_INT, 9),
            (n1o.T_INT, 20), (n1o.T_INT, 21), (n1o.T_FLOAT, 20.5), (n1o.T_FLOAT, 2.5), (n1o.T_FLOAT, 2.4999), (n1o.T_NULL, 0), (n1o.T_MISSING, 0),
            (n1o.T_TRUE, 0), (n1o.T_FALSE, 0), (n1o.T_FLOAT, float("inf")), (n1o.T_FLOAT, float("-inf")), (n1o.T_INT, -(1 << 63)), (n1o.T_INT, (1 << 63) - 1)]
    tags = np.array([r[0] for r in rows], np.uint8)
    pay = np.zeros(len(rows), np.uint64)
    vals = []
    for i, (tg, v) in enumerate(rows):
        if tg == n1o.T_INT:
            pay[i] = np.array([v], np.int64).view(np.uint64)[0]
        elif tg == n1o.T_FLOAT:
            pay[i] = np.array([v], np.float64).view(np.uint64)[0]
        vals.append(MISSING if tg == n1o.T_MISSING else None if tg == n1o.T_NULL else True if tg == n1o.T_TRUE else False if tg == n1o.T_FALSE else v)
    t = n1o.Table([n1o.Column(D("x"), n1o.COL_TAGGED64, tags=tags, payload=pay), _int_col("g", np.arange(len(rows)) % 3)], [])
    lists = [[3.0], [3], [0], [big], [-big], [10, 20], [10, 11, 20, 2.5], [20.5, 2.5, True], [False, None, 9], []]
    for consts in lists:
        for neg in (False, True):
            d = iu.term(D("x"), consts)
            want = [i for i, v in enumerate(vals) if (iu.in4(v, consts) is False if neg else iu.in4(v, consts) is True)]
            gsel, _ = pu.run_gpu(t, "(not %s)" % d if neg else d, [], [], filter_only=True)
            assert sorted(gsel.selected) == want, (consts, neg, sorted(gsel.selected), want)
    assert iu.in4(big + 1, [big]) is False and iu.in4(float(big), [big]) is True and iu.in4(3, [3.0]) is True and iu.in4(float("nan"), [0]) is False
    # two lists of one plan share the sorted array ([9, 10, 20] then [2.5, 11, 21]): each term searches its own range only
    a, b = [20, 10, 9], [21, 2.5, 11]
    dcond = "(%s and (not %s))" % (iu.term(D("x"), a + b), iu.term(D("x"), b, folded=True))
    want = [i for i, v in enumerate(vals) if iu.in4(v, a + b) is True and iu.in4(v, b) is False]
    for opts in ({"fast": 0}, {}):
        gsel, _ = pu.run_gpu(t, dcond, [], [], filter_only=True, **opts)
        assert sorted(gsel.selected) == want and len(want) == 3
    # and through the grouped kernels, bounded and run-time built: (x IN a) AND (x IN a + b)
    dcond = "(%s and %s)" % (iu.term(D("x"), a), iu.term(D("x"), a + b))
    for opts, kernel in (({"jit": 2}, 2), ({"spec": 0}, 0), ({"fast": 0}, 0)):
        gpu, st = pu.run_gpu(t, dcond, [], ["count(*)"], **opts)
        assert gpu.aggs[0][0][1] == 3 and st["spec_kernel"] == kernel, (opts, gpu.aggs, st)


# ------------------------------------------------------------------ the match table's life

def _table(strings, dictionary, groups=None):
    n = len(strings)
    codes = np.array([dictionary.index(x) for x in strings], dtype=np.uint32)
    return n1o.Table([n1o.Column(D("s"), n1o.COL_DICT32, codes=codes), _int_col("g", groups if groups is not None else [0] * n)], dictionary)


def test_in_when_the_dictionary_grows_between_batches():
    """Strings interned after the first push — some of which are in the list — are seen by the later batches: the table is
    extended for the new codes.  n1k_reset keeps it; in_stats shows every dictionary string looked up exactly once."""
    cond, keys, aggs = iu.term(D("s"), ["new", "newer", "x\nnew", 4]), [D("g")], ["count(*)"]
    d1 = [b"old", b"newer"]
    d2 = [b"old", b"newer", b"new", b"news\n", b"renew", b"x\nnew"]
    b1 = _table([b"old", b"newer", b"old"], d1, [0, 0, 1])
    b2 = _table([b"new", b"news\n", b"renew", b"x\nnew", b"old", b"newer"], d2, [0, 1, 1, 2, 2, 2])
    want = {0: 2, 2: 2}
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs))
    for round_ in range(2):
        for b in (b1, b2):
            op.process_items([{c.name: c for c in b.columns}[p] for p in op.column_paths], b.dictionary)
        rows = op.after_items()
        assert {k[0][1]: a[0][1] for k, a in zip(rows.keys, rows.aggs)} == want
        stats = op.in_stats()
        ndict = int(_ffi.lib().n1k_dict_size(op._h))
        assert stats["lists"] == 1 and ndict >= len(d2) and stats["host_strings"] == ndict and stats["device_strings"] == 0, (stats, ndict)
        op.reopen()
    op.done()


def test_a_large_dictionary_takes_the_device_route_and_a_small_one_the_host_route():
    probe = query_amd.GpuFilterGroup(plan.filter_group_plan(iu.term(D("s"), ["a"]), [], ["count(*)"]))
    threshold = probe.in_stats()["device_threshold"]
    probe.done()
    assert threshold * 4 <= 4_000_000, "a threshold that large means the kernel is not worth having"
    for n, route in ((4 * threshold, "device"), (100, "host")):
        texts = ["s%d" % i for i in range(n)]
        texts[3] = "x" * 300 + "75"  # beyond the kernel's limit: the host matcher's, on either route
        lists = [[texts[3], "s7", "s70", "nope"], ["s%d" % i for i in range(5, n, 9)], [1, 2]]
        cond = "(%s or %s or %s)" % tuple(iu.term(D("s"), l) for l in lists)
        dictionary = [x.encode() for x in texts]
        rng = np.random.default_rng(n)
        codes = rng.integers(0, n, 100_000).astype(np.uint32)
        t = n1o.Table([n1o.Column(D("s"), n1o.COL_DICT32, codes=codes)], dictionary)
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], ["count(*)"]))
        op.process_items(t.columns, dictionary)
        rows = op.after_items()
        stats = op.in_stats()
        op.done()
        member = set(lists[0]) | set(lists[1])
        hit = np.array([x in member for x in texts])
        assert rows.aggs[0][0][1] == int(hit[codes].sum()) and 0 < int(hit[codes].sum()) < len(codes)
        assert stats["lists"] == 3
        if route == "device":
            assert stats["device_strings"] == n - 1 and stats["host_strings"] == 1, stats
        else:
            assert stats["device_strings"] == 0 and stats["host_strings"] == n, stats


def test_eight_bits_shared_with_like_and_any_every():
    """Three IN lists with strings, three LIKE patterns and two collection predicates fill the eight bits of a table entry —
    and answer as the oracle does; number-only lists take no bit; a ninth bit is refused."""
    import coll_util as cu
    import like_util as lu
    rng = np.random.default_rng(8)
    t = make_table(rng, 3000)
    sub = Substitution(t)
    ins = [sub.term("s", ["a", "ab", 3]), sub.term("m", ["3", "true", True, None]), sub.term("s", ["zz", "é", "nope"])]
    vals = column_values(t, "s")
    likes = []
    for p in ("a%", "%b", "cat\\_1%"):
        tags = np.array([iu.tag_of(lu.like4(v, p), n1o) for v in vals], np.uint8)
        name = D("l%d" % len(likes))
        sub.helpers.append(n1o.Column(name, n1o.COL_TAGGED64, tags=tags, payload=np.zeros(len(vals), np.uint64)))
        likes.append(('(%s like "%s")' % (D("s"), p.replace("\\", "\\\\")), name))
    nums = (iu.term(D("x"), [3, 2.5]), iu.expand(D("x"), [3, 2.5]))
    parts = ins + likes + [nums]
    dcond = "(%s)" % " or ".join(("(not %s)" % p[0]) if i % 4 == 3 else p[0] for i, p in enumerate(parts))
    ocond = "(%s)" % " or ".join(("(not %s)" % p[1]) if i % 4 == 3 else p[1] for i, p in enumerate(parts))
    keys, aggs = [D("k")], ["count(*)"]
    gpu, st = pu.run_gpu(t, dcond, keys, aggs)
    ora = n1o.run(sub.oracle_table(), ocond, keys, aggs)
    pu.assert_same_groups(gpu, ora, aggs=aggs)
    assert st["rows_selected"] == ora.rows_passed and 0 < ora.rows_passed < 3000
    colls = [cu.term_text(cu.ANY, ("cmp", "=", [], w, False), over=D("m")) for w in ("ab", "zz", "q")]
    eight = "(%s or %s or %s)" % (dcond, colls[0], colls[1])
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(eight, keys, aggs))
    assert op.in_stats()["lists"] == 4 and op.like_stats()["patterns"] == 3 and op.coll_stats()["predicates"] == 2
    op.done()
    for ninth in (colls[2], iu.term(D("s"), ["other"]), '(%s like "q%%")' % D("s")):
        with pytest.raises(query_amd.N1kError) as ei:
            query_amd.GpuFilterGroup(plan.filter_group_plan("(%s or %s)" % (eight, ninth), keys, aggs))
        assert ei.value.status == _ffi.UNSUPPORTED and "more than 8" in ei.value.message


LIKE_MAX_LEN, COLL_MAX_LEN = 128, 192  # bytes of an entry like_match_kernel / coll_match_kernel takes (tests/test_gpu_coll.py)
LONG_PATTERN = "%" + "x" * 250 + "7"    # its program (a MANY and a literal of 251 bytes) is longer than the LIKE kernel takes
THREE_KIND_TAGS = ("s", "u", "v")


def three_kind_dictionary(n, tag):
    """n distinct entries marked with `tag`, strings then arrays, as tests/test_gpu_coll.py's mixed_dictionary builds them;
    from 16 entries on with what each kernel leaves to the host and what only looks like an array among them.  Returns
    (entries, texts of the strings as Go reads them, array values)."""
    import coll_util as cu
    ns = n - n // 2
    strings = [("%s%d" % (tag, i)).encode() for i in range(ns)]
    arrays = [[tag + "w%d" % i] + (["t_1"] if i % 3 == 0 else []) + ([i] if i % 2 else []) for i in range(n - ns)]
    if n >= 16:
        strings[1] = (tag + "x" * 300 + "7").encode()     # over 128 B: the host's for LIKE and IN; "%7", LONG_PATTERN and a list hold it
        strings[2] = b"ab\xffc" + tag.encode()            # not valid UTF-8: the host's for LIKE (the byte is one U+FFFD, which `_` takes)
        strings[3] = ("[looks like one " + tag).encode()  # a STRING that begins with '[': evaluated as array text; a list holds it
        arrays[1] = [tag + "w1"] * 60 + ["t_1"]           # over 192 B: the host's for ANY / EVERY and for IN
        arrays[2] = ['x"y', tag, "t_1"]                   # an escaped string FIRST, under both predicates: the host's for ANY / EVERY
    return strings + cu.texts_of(arrays), [s.decode("utf-8", errors="replace") for s in strings], arrays


def three_kind_counts(entries, like_dev, dev):
    """(LIKE device, host; ANY / EVERY device, host; IN device, host) of one extension of the table by `entries`, by the rules
    DESIGN.md §4 states.  LIKE and IN are evaluated for every entry, ANY / EVERY for one of at least 2 bytes that begins
    with '['.  On the device route the LIKE kernel leaves an entry over 128 B or not valid UTF-8, the ANY / EVERY kernel one
    over 192 B or with an escaped string where these predicates compare, the IN kernel one over 128 B."""
    def valid(b):
        try:
            b.decode("utf-8")
            return True
        except UnicodeDecodeError:
            return False
    n = len(entries)
    arr = [e for e in entries if len(e) >= 2 and e[:1] == b"["]
    like_left = sum(1 for e in entries if len(e) > LIKE_MAX_LEN or not valid(e)) if like_dev else n
    coll_left = sum(1 for e in arr if len(e) > COLL_MAX_LEN or b"\\" in e) if dev else len(arr)
    in_left = sum(1 for e in entries if len(e) > iu.DEV_MAX_LEN) if dev else n
    return n - like_left, like_left, len(arr) - coll_left, coll_left, n - in_left, in_left


@pytest.mark.parametrize("long_pattern", [False, True], ids=["every-kind-on-the-device", "like-stays-on-the-host"])
def test_a_plan_with_all_three_kinds_builds_one_table_on_both_routes(long_pattern):
    """Two LIKE patterns and three IN lists (two with strings, one of numbers) over a string column and an ANY and an EVERY
    over an array column in one Filter.  (a) T - 1 new entries go through the host matchers for every kind; (b) T more,
    from an odd entry on, through the three kernels (one upload, merged once) — or, when one pattern's program is longer
    than the LIKE kernel takes, through two kernels while LIKE stays with the host in the same extension; (c) 5 more through
    the host matchers again, onto a table the device built.  The old entries keep their bits throughout."""
    import json

    import coll_util as cu
    import like_util as lu
    patterns = ["%b_c%", LONG_PATTERN] if long_pattern else ["%7", "%b_c%"]
    preds = [(cu.ANY, ("cmp", "=", [], "t_1", False)), (cu.EVERY, ("like", [], "%w%4"))]
    lists = [[tag + "x" * 300 + "7" for tag in THREE_KIND_TAGS] + ["s7", "u17", "v1", "nope"],
             ["%s%d" % (tag, i) for tag in THREE_KIND_TAGS for i in range(5, 400, 9)] + ["[looks like one u"],
             [1, 2.5]]
    some = [b"a", b"", b"x" * 300 + b"7", b"ab\xffc", b"[1]", b"b7", b"abxc", b"7"]
    # (no device is asked: a program the kernel does not take sends every string to the host before anything is launched)
    assert [lu.device_match(p.encode(), some)[1] == len(some) for p in patterns] == [False, long_pattern]
    cond = "(%s)" % " or ".join(["(%s like %s)" % (D("s"), json.dumps(p)) for p in patterns] + [iu.term(D("s"), l) for l in lists] +
                                [cu.term_text(m, c, over=D("a")) for m, c in preds])
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], ["count(*)"]))
    T = op.like_stats()["device_threshold"]
    assert T == op.coll_stats()["device_threshold"] == op.in_stats()["device_threshold"] and T % 2 == 0
    in_fns = [iu.matcher(l) for l in lists]
    rng = np.random.default_rng(int(long_pattern))
    dictionary, str_hit, arr_hit, str_codes, arr_codes = [], [], [], [], []
    want_stats = np.zeros(6, np.int64)
    for tag, n in zip(THREE_KIND_TAGS, (T - 1, T, 5)):
        entries, texts, arrays = three_kind_dictionary(n, tag)
        base, ns = len(dictionary), len(texts)
        dictionary += entries
        str_codes += range(base, base + ns)
        arr_codes += range(base + ns, base + n)
        str_hit += [any(lu.like4(t, p) is True for p in patterns) or any(f(t) is True for f in in_fns) for t in texts]
        arr_hit += [any(cu.coll_mirror(m, c, a) is True for m, c in preds) for a in arrays]
        # rows over every entry interned so far (the old ones too), each special entry among them
        rows = 20_000
        si = np.concatenate([np.arange(len(str_codes)), rng.integers(0, len(str_codes), rows - len(str_codes))])
        ai = np.concatenate([rng.integers(0, len(arr_codes), rows - len(arr_codes)), np.arange(len(arr_codes))])
        cols = {D("s"): n1o.Column(D("s"), n1o.COL_DICT32, codes=np.array(str_codes, np.uint32)[si]),
                D("a"): n1o.Column(D("a"), n1o.COL_TAGGED64, tags=np.full(rows, n1o.T_ARRAY, np.uint8), payload=np.array(arr_codes, np.uint64)[ai])}
        op.process_items([cols[p] for p in op.column_paths], dictionary)
        got = op.after_items().aggs[0][0][1]
        assert int(_ffi.lib().n1k_dict_size(op._h)) == len(dictionary)  # (the handle interned nothing of its own: n new entries)
        want = int((np.array(str_hit)[si] | np.array(arr_hit)[ai]).sum())
        assert 0 < want < rows and got == want, (tag, got, want)
        want_stats += three_kind_counts(entries, like_dev=n >= T and not long_pattern, dev=n >= T)
        ls, cs, ins = op.like_stats(), op.coll_stats(), op.in_stats()
        got_stats = (ls["device_strings"], ls["host_strings"], cs["device_arrays"], cs["host_arrays"], ins["device_strings"], ins["host_strings"])
        assert got_stats == tuple(want_stats), (tag, got_stats, want_stats)
        assert ls["patterns"] == 2 and cs["predicates"] == 2 and ins["lists"] == 3
        op.reopen()  # (keeps the table)
    # both routes were taken, the kernels left their special entries to the host, every pattern and list selected something
    assert (want_stats[0] > 0) != long_pattern and want_stats[2] > 0 and want_stats[4] > 0
    assert want_stats[1] >= T + 4 + 3 and want_stats[3] >= 2 and want_stats[5] >= T + 4 + 2
    if long_pattern:
        assert ls["device_strings"] == 0 and cs["device_arrays"] > 0 and ins["device_strings"] > 0
    strings = [dictionary[c].decode("utf-8", errors="replace") for c in str_codes]
    assert all(any(f(t) is True for t in strings) for f in in_fns[:2]) and all(any(lu.like4(t, p) for t in strings) for p in patterns)
    op.done()


def test_having_in_over_an_aggregate_and_over_a_string_group_key():
    rng = np.random.default_rng(9)
    t = make_table(rng, 4000)
    keys, aggs = [D("k")], ["count(*)", "sum(%s)" % D("g")]
    ora = n1o.run(t, None, keys, aggs)
    sums = [a[1][1] for a in ora.aggs]
    assert len(set(sums)) == len(sums) >= 5 and all(isinstance(v, int) for v in sums)

    def key(k):
        return MISSING if k[0] == n1o.T_MISSING else (None if k[0] != n1o.T_STRING else k[1].decode())

    cases = [("sum(%s)" % D("g"), [sums[0], float(sums[2]), sums[1] + 0.5, -1], lambda k, a: a[1][1]),
             (D("k"), ["cat_1", "cat_11", "nope", 5], lambda k, a: key(k[0]))]
    for path, consts, value in cases:
        for neg, keep in ((False, lambda r: r is True), (True, lambda r: r is False)):
            having = iu.term(path, consts)
            gpu, _ = pu.run_gpu(t, None, keys, aggs, having="(not %s)" % having if neg else having)
            want = sorted((k[0], a[0][1]) for k, a in zip(ora.keys, ora.aggs) if keep(iu.in4(value(k, a), consts)))
            got = sorted((k[0], a[0][1]) for k, a in zip(gpu.keys, gpu.aggs))
            assert got == want and 1 <= len(want) < len(ora.keys), (having, neg, got, want)
    # the key is NULL / MISSING in some groups: NOT IN keeps neither (NULL / MISSING are not TRUE)
    assert any(k[0][0] == n1o.T_NULL for k in ora.keys) and any(k[0][0] == n1o.T_MISSING for k in ora.keys)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("jit", [0, 2], ids=["interpreter", "runtime-built"])
def test_in_across_two_ranks_over_the_loopback_transport(jit):
    """World size 2, row exchange: the sender evaluates the Filter — IN through its own handle's table and constants — and
    every rank ends with the expanded oracle's groups."""
    from query_amd import distributed as qd
    from query_amd.gpu_operator import GroupRows
    from test_gpu_distributed import _device_cols, _run_ranks
    world, n = 2, 60_011
    rng = np.random.default_rng(31 + jit)
    t = make_table(rng, n)
    consts = ["ab", "a", "zz", "nope", 3]
    dcond = "(%s and (1 < %s))" % (iu.term(D("s"), consts), D("x"))
    ocond = "(%s and (1 < %s))" % (iu.expand(D("s"), consts), D("x"))
    keys, aggs = [D("k")], sorted(["count(*)", "sum(%s)" % D("x")])
    ora = n1o.run(t, ocond, keys, aggs)
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
        assert (info["sender_kernel"] != 0) == (jit == 2), info  # scan_spec_partition_body saw the IN term, or partition_kernel did
    assert sum(info["recv_rows"] for _, info in outs) == ora.rows_passed
