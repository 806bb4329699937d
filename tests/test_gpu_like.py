"""LIKE / NOT LIKE on the device: the reference's statements, the device matcher against the host matcher and the
mirror, and a differential against the oracle BY SUBSTITUTION — the oracle has no LIKE, but it evaluates a bare path
inside AND / OR / NOT with the full 4-valued logic, so every `(p like "...")` of the device's plan becomes, for the
oracle, a helper column that holds the mirror's TRUE / FALSE / NULL / MISSING of that row (tests/like_util.py)."""
import json
import os

import numpy as np
import pytest

import golden_util as gu
import like_util as lu
import parity_util as pu
import query_amd
from oracle import n1o
from query_amd import _ffi, plan

pytestmark = pytest.mark.gpu


def D(name):
    return plan.field_path("default", name)


with open(os.path.join(gu.GOLDEN, "cases_like.json")) as fh:
    LIKE_CASES = json.load(fh)["cases"]


@pytest.mark.parametrize("case", LIKE_CASES, ids=[c["id"] for c in LIKE_CASES])
def test_the_references_like_statements(case):
    docs = gu.load_docs(case["keyspace"])
    table = gu.build_table(docs, gu.leaf_paths(case["plan"]))
    rows, _ = pu.run_gpu(table, case["plan"]["condition"], [], [], filter_only=True)
    got = gu.replay_filter_post(case, docs, rows.selected)
    assert gu.same_json(got, case["results"]), (got, case["results"])


# ------------------------------------------------------------------ the matchers

DEV_MAX_LEN = 128  # bytes of a string like_match_kernel takes (include/n1k.h, n1k_like_match_device)


def test_device_matcher_equals_host_matcher_and_mirror_on_the_cpu_tests_pairs():
    pairs = lu.random_pairs(20240607, 24000)
    for pattern, idx in lu.by_pattern(pairs):
        strings = [pairs[i][1].encode() for i in idx]
        dev, left = lu.device_match(pattern.encode(), strings)
        host = lu.host_match(pattern.encode(), strings)
        want = np.array([lu.like_mirror(pairs[i][1], pattern) for i in idx], dtype=np.uint8)
        assert left == 0 and np.array_equal(dev, host) and np.array_equal(dev, want), (pattern, strings[:4])


def test_device_matcher_on_a_million_strings_of_every_length():
    """Lengths from 0 to beyond the kernel's limit, two- and four-byte characters, line breaks; some strings that are not
    valid UTF-8.  out_left_to_host counts exactly the strings the documented limits exclude."""
    rng = np.random.default_rng(77)
    n = 1_050_000
    alphabet = np.array(list("aabbbc_%.\n") + ["é", "\U0001F600"], dtype=object)
    lens = rng.integers(0, 24, n)
    long_ix = rng.choice(n, 3000, replace=False)
    lens[long_ix] = rng.integers(DEV_MAX_LEN - 8, DEV_MAX_LEN + 40, 3000)
    chars = alphabet[rng.integers(0, len(alphabet), int(lens.sum()))]
    cuts = np.concatenate([[0], np.cumsum(lens)])
    texts = ["".join(chars[cuts[i]:cuts[i + 1]]) for i in range(n)]
    strings = [t.encode() for t in texts]
    bad_ix = set(int(i) for i in rng.choice(n, 500, replace=False))
    for i in bad_ix:
        strings[i] = strings[i][:5] + b"\xff" + strings[i][5:]
    excluded = sum(1 for i, s in enumerate(strings) if len(s) > DEV_MAX_LEN or i in bad_ix)
    assert excluded > 1000 and max(len(s) for s in strings) > DEV_MAX_LEN and min(len(s) for s in strings) == 0
    for pattern in ["%ab_b%", "a%b", "b__", "%\\%", "%é%\U0001F600%", ""]:
        dev, left = lu.device_match(pattern.encode(), strings)
        host = lu.host_match(pattern.encode(), strings)
        assert left == excluded, (pattern, left, excluded)
        assert np.array_equal(dev, host), pattern
        rx = lu.like_regex(pattern)
        want = np.fromiter((rx.search(t) is not None for t in texts), dtype=np.uint8, count=n)
        ok = np.ones(n, dtype=bool)
        ok[list(bad_ix)] = False  # (the mirror speaks of text; the undecodable strings are the host matcher's, checked on the CPU)
        assert np.array_equal(dev[ok], want[ok]), pattern
        assert 0 < int(want.sum()) < n or pattern == ""


def test_device_matcher_when_a_waves_strings_span_more_than_its_slab():
    """Runs of consecutive long strings with short ones in between: the 64 strings of such a wave span more than the 8 KiB
    LDS slab, and its lanes read the strings the kernel does take straight from global memory."""
    rng = np.random.default_rng(3)
    strings, texts = [], []
    for block in range(400):
        for i in range(64):
            if block % 2 == 0 and i % 8 != 7:  # 56 strings of 150-260 B, every eighth one short: 64 strings span > 8 KiB
                n = int(rng.integers(150, 260))
            else:
                n = int(rng.integers(0, 20))
            t = "".join(rng.choice(list("aabbc_%\né"), n))
            if block % 2 == 0 and i % 16 == 3:
                t = "ab" * 50  # within the limit (100 B) inside a long run
            texts.append(t)
            strings.append(t.encode())
    spans = [sum(len(s) for s in strings[w:w + 64]) for w in range(0, len(strings), 64)]
    assert max(spans) > 8192 and min(spans) < 8192
    excluded = sum(1 for s in strings if len(s) > DEV_MAX_LEN)
    taken_in_wide_waves = sum(1 for w in range(0, len(strings), 64) if spans[w // 64] > 8192 for s in strings[w:w + 64] if len(s) <= DEV_MAX_LEN)
    assert taken_in_wide_waves > 1000
    for pattern in ["%ab%", "ab%ab", "%b_", "a%", ""]:
        dev, left = lu.device_match(pattern.encode(), strings)
        host = lu.host_match(pattern.encode(), strings)
        rx = lu.like_regex(pattern)
        want = np.fromiter((rx.search(t) is not None for t in texts), dtype=np.uint8, count=len(texts))
        assert left == excluded and np.array_equal(dev, host) and np.array_equal(dev, want), pattern


BLOCK_EDGES = [1, 63, 64, 65, 255, 256, 257]  # the last lane's clamp, a full wave, a wave of one lane, a second workgroup of one string


def test_device_matcher_at_the_edges_of_a_block():
    """Blocks that end inside a wave, on a wave and one string into the next workgroup; strings of 0 to 40 bytes.  Once more
    with a last string of 10 KB: the final wave then spans more than its slab and reads what it takes from global memory."""
    rng = np.random.default_rng(11)
    pool = ["".join(rng.choice(list("aabbc_%\né"), int(rng.integers(0, 41)))).encode()[:40] for _ in range(max(BLOCK_EDGES))]
    pool[5] = pool[5][:3] + b"\xff"  # not valid UTF-8 (as is a string the cut at 40 bytes splits a character of): the host matcher's

    def valid(b):
        try:
            b.decode("utf-8")
            return True
        except UnicodeDecodeError:
            return False

    assert min(len(s) for s in pool) == 0 and max(len(s) for s in pool) == 40 and 0 < sum(not valid(s) for s in pool[:63]) < 10
    huge = b"ab" * 5000
    assert len(huge) > 64 * DEV_MAX_LEN
    for n in BLOCK_EDGES:
        for last in (None, huge):
            strings = pool[:n] if last is None else pool[:n - 1] + [last]
            excluded = sum(1 for s in strings if len(s) > DEV_MAX_LEN or not valid(s))
            for pattern in (b"%ab%", b"a%"):
                dev, left = lu.device_match(pattern, strings)
                host = lu.host_match(pattern, strings)
                assert np.array_equal(dev, host), (n, last is None, pattern, np.nonzero(dev != host))
                assert left == excluded, (n, last is None, left, excluded)
            assert n < 64 or 0 < int(host.sum()) < n


def test_like_term_on_both_sides_of_the_lds_switch():
    """The bounded and the run-time-built kernels stage a match table of at most 4096 entries in LDS and read a larger one
    from global memory: dictionaries of 3000 and of 6000 strings, DICT32 and TAGGED64 string column, against the oracle by
    substitution."""
    for nwords in (3000, 6000):
        rng = np.random.default_rng(nwords)
        words = ["w%da%sb" % (i, "x" * (i % 3)) for i in range(nwords)]
        n = 50_000
        sc = rng.integers(0, nwords, n).astype(np.uint32)
        sc[rng.random(n) < 0.03] = 0xFFFFFFFE
        mt = np.full(n, n1o.T_STRING, np.uint8)
        mp = rng.integers(0, nwords, n).astype(np.uint64)
        mt[rng.random(n) < 0.05] = n1o.T_NULL
        xt = np.full(n, n1o.T_INT, np.uint8)
        xp = rng.integers(0, 100, n).astype(np.int64).view(np.uint64).copy()
        gt = np.full(n, n1o.T_INT, np.uint8)
        gp = rng.integers(0, 5, n).astype(np.int64).view(np.uint64).copy()
        pattern = "w%7a_b"
        for col, scol in (("s", n1o.Column(D("s"), n1o.COL_DICT32, codes=sc)), ("m", n1o.Column(D("m"), n1o.COL_TAGGED64, tags=mt, payload=mp))):
            vals = [None if (c == 0xFFFFFFFE if col == "s" else tg == n1o.T_NULL) else words[int(c)]
                    for c, tg in zip((sc if col == "s" else mp).tolist(), mt.tolist())]
            ht = np.array([n1o.T_NULL if v is None else (n1o.T_TRUE if lu.like_mirror(v, pattern) else n1o.T_FALSE) for v in vals], np.uint8)
            cols = [scol, n1o.Column(D("x"), n1o.COL_TAGGED64, tags=xt, payload=xp), n1o.Column(D("g"), n1o.COL_TAGGED64, tags=gt, payload=gp)]
            t = n1o.Table(cols, [w.encode() for w in words])
            ot = n1o.Table(cols + [n1o.Column(D("h"), n1o.COL_TAGGED64, tags=ht, payload=np.zeros(n, np.uint64))], t.dictionary)
            dcond = '((%s like "%s") and (10 < %s))' % (D(col), pattern, D("x"))
            ocond = "(%s and (10 < %s))" % (D("h"), D("x"))
            aggs = sorted(["count(*)", "sum(%s)" % D("x")])
            # no key: the bounded kernel and the run-time-built one take the plan whatever the dictionary's size (a
            # dictionary KEY beyond the LDS table would send it to the interpreter); an integer key: the hashed run-time-built kernel
            for keys, families in (([], (({"jit": 2}, 2), ({"spec": 0}, 0), ({"fast": 0}, 0))), ([D("g")], (({"jit": 2}, 2),))):
                ora = n1o.run(ot, ocond, keys, aggs)
                assert 0 < ora.rows_passed < n // 2
                for opts, kernel in families:
                    gpu, st = pu.run_gpu(t, dcond, keys, aggs, batches=2, **opts)
                    pu.assert_same_groups(gpu, ora, aggs=aggs)
                    assert st["spec_kernel"] == kernel and st["rows_selected"] == ora.rows_passed, (nwords, col, keys, opts, st)


@pytest.mark.parametrize("nwords", [1400, 1480, 1530, 1580, 1700, 1850])
def test_like_with_two_count_distinct_where_the_lds_is_full(nwords):
    """`WHERE k LIKE "x%" GROUP BY k, COUNT(DISTINCT a), COUNT(DISTINCT b), SUM(b)` through the run-time-built scan: the
    DIRECT table (32 B per slot in the compact layout), two word scatters and their "already logged" caches are sized to
    fill a CU's 160 KiB of LDS, and the shape's 4 KiB for the staged match table has to be part of that budget — a key
    dictionary of about 1470 to 1580 strings is where a budget without it overflows the LDS and the launch fails."""
    rng = np.random.default_rng(nwords)
    words = [("x%d" if i % 3 else "y%d") % i for i in range(nwords)]
    n = 60_000
    kc = rng.integers(0, nwords, n).astype(np.uint32)
    kc[rng.random(n) < 0.02] = 0xFFFFFFFE
    kc[rng.random(n) < 0.02] = 0xFFFFFFFF
    it = np.full(n, n1o.T_INT, np.uint8)
    ap = rng.integers(0, 40, n).astype(np.int64).view(np.uint64).copy()
    bp = rng.integers(0, 6, n).astype(np.int64).view(np.uint64).copy()
    bt = it.copy()
    bt[rng.random(n) < 0.03] = n1o.T_NULL
    ht = np.array([n1o.T_MISSING if c == 0xFFFFFFFF else (n1o.T_NULL if c == 0xFFFFFFFE else (n1o.T_TRUE if lu.like_mirror(words[c], "x%") else n1o.T_FALSE))
                   for c in kc.tolist()], np.uint8)
    cols = [n1o.Column(D("k"), n1o.COL_DICT32, codes=kc), n1o.Column(D("a"), n1o.COL_TAGGED64, tags=it, payload=ap),
            n1o.Column(D("b"), n1o.COL_TAGGED64, tags=bt, payload=bp)]
    t = n1o.Table(cols, [w.encode() for w in words])
    ot = n1o.Table(cols + [n1o.Column(D("h"), n1o.COL_TAGGED64, tags=ht, payload=np.zeros(n, np.uint64))], t.dictionary)
    keys, aggs = [D("k")], sorted(["count(distinct %s)" % D("a"), "count(distinct %s)" % D("b"), "sum(%s)" % D("b")])
    ora = n1o.run(ot, D("h"), keys, aggs)
    gpu, st = pu.run_gpu(t, '(%s like "x%%")' % D("k"), keys, aggs, batches=2, jit=2)
    pu.assert_same_groups(gpu, ora, aggs=aggs)
    assert st["spec_kernel"] == 2 and st["rows_selected"] == ora.rows_passed, st


# ------------------------------------------------------------------ differential by substitution

# dictionary: strings the patterns below split in many ways, then two arrays (dictionary coded, but their tag is ARRAY)
WORDS = ["", "a", "ab", "abc", "abab", "b", "ba", "bab", "a%b", "a_b", "ab\nab", "x\nab", "ab\ny", "é", "aéb", "a\U0001F600b", "50%", "\\", "a\\b",
         "cat_1", "cat_10", "cat_11", "cat_2", "zz"]
DICT = [w.encode() for w in WORDS] + [b"[1,2]", b"[\"ab\"]"]
ARR0 = len(WORDS)
PATTERNS = ["ab%", "%b", "a_b", "%a%b%", "a\\_b", "50\\%", "ab", "", "%", "_", "cat\\_1%", "%\nab", "a%", "%é%", "__", "a\\b", "%\\%"]


def make_table(rng, n):
    """s: DICT32 strings with NULL / MISSING; m: TAGGED64 of every class (strings, numbers, booleans, NULL, MISSING, arrays);
    x: numbers; k: DICT32 key; g: small ints."""
    sc = rng.integers(0, len(WORDS), n).astype(np.uint32)
    sc[rng.random(n) < 0.05] = 0xFFFFFFFE
    sc[rng.random(n) < 0.05] = 0xFFFFFFFF
    mt = np.zeros(n, np.uint8)
    mp = np.zeros(n, np.uint64)
    r = rng.integers(0, 100, n)
    st = r < 55
    mt[st] = n1o.T_STRING
    mp[st] = rng.integers(0, len(WORDS), int(st.sum())).astype(np.uint64)
    it = (r >= 55) & (r < 65)
    mt[it] = n1o.T_INT
    mp[it] = rng.integers(-3, 4, int(it.sum())).astype(np.int64).view(np.uint64)
    mt[(r >= 65) & (r < 70)] = n1o.T_TRUE
    mt[(r >= 70) & (r < 75)] = n1o.T_FALSE
    mt[(r >= 75) & (r < 83)] = n1o.T_NULL
    mt[(r >= 83) & (r < 91)] = n1o.T_MISSING
    ar = r >= 91
    mt[ar] = n1o.T_ARRAY
    mp[ar] = (ARR0 + rng.integers(0, 2, int(ar.sum()))).astype(np.uint64)
    xt = np.full(n, n1o.T_FLOAT, np.uint8)
    xp = (rng.integers(0, 800, n) / 8.0 + 0.0625).view(np.uint64).copy()
    ints = rng.random(n) < 0.3
    xt[ints] = n1o.T_INT
    xp[ints] = rng.integers(0, 100, int(ints.sum())).astype(np.int64).view(np.uint64)
    xt[rng.random(n) < 0.03] = n1o.T_NULL
    kc = rng.integers(19, 24, n).astype(np.uint32)  # cat_1 .. zz
    kc[rng.random(n) < 0.04] = 0xFFFFFFFE
    kc[rng.random(n) < 0.03] = 0xFFFFFFFF
    gt = np.full(n, n1o.T_INT, np.uint8)
    gp = rng.integers(0, 7, n).astype(np.int64).view(np.uint64).copy()
    return n1o.Table([n1o.Column(D("s"), n1o.COL_DICT32, codes=sc), n1o.Column(D("m"), n1o.COL_TAGGED64, tags=mt, payload=mp),
                      n1o.Column(D("x"), n1o.COL_TAGGED64, tags=xt, payload=xp), n1o.Column(D("k"), n1o.COL_DICT32, codes=kc),
                      n1o.Column(D("g"), n1o.COL_TAGGED64, tags=gt, payload=gp)], list(DICT))


def column_values(t, name):
    """The python values of a string-capable column: str, lu.MISSING, None (NULL), or anything else for a non-string."""
    c = {c.name: c for c in t.columns}[D(name)]
    if c.kind == n1o.COL_DICT32:
        return [lu.MISSING if x == 0xFFFFFFFF else (None if x == 0xFFFFFFFE else WORDS[x]) for x in c.codes.tolist()]
    out = []
    for tg, p in zip(c.tags.tolist(), c.payload.tolist()):
        out.append(lu.MISSING if tg == n1o.T_MISSING else (None if tg == n1o.T_NULL else (WORDS[p] if tg == n1o.T_STRING else 0)))
    return out


class Substitution:
    """Collects the LIKE terms of one plan: the device sees the term, the oracle a helper column of its 4-valued results."""

    def __init__(self, table):
        self.table = table
        self.helpers = []

    def like(self, col, pattern):
        vals = column_values(self.table, col)
        n = len(vals)
        tags = np.zeros(n, np.uint8)
        for i, v in enumerate(vals):
            r = lu.MISSING if v is lu.MISSING else (None if not isinstance(v, str) else lu.like_mirror(v, pattern))
            tags[i] = n1o.T_MISSING if r is lu.MISSING else (n1o.T_NULL if r is None else (n1o.T_TRUE if r else n1o.T_FALSE))
        name = D("h%d" % len(self.helpers))
        self.helpers.append(n1o.Column(name, n1o.COL_TAGGED64, tags=tags, payload=np.zeros(n, np.uint64)))
        return "(%s like %s)" % (D(col), json.dumps(pattern, ensure_ascii=False)), name

    def oracle_table(self):
        return n1o.Table(list(self.table.columns) + self.helpers, self.table.dictionary)


def other_term(rng):
    r = rng.integers(0, 6)
    if r == 0: return "(%s < %s)" % (["10", "40.5", "70"][rng.integers(0, 3)], D("x"))
    if r == 1: return "(%s <= %s)" % (D("x"), ["30", "55.25"][rng.integers(0, 2)])
    if r == 2: return "(%s = %s)" % (D("s"), ["\"ab\"", "\"cat_1\""][rng.integers(0, 2)])
    if r == 3: return "(%s is %s)" % (D(["m", "s", "x"][rng.integers(0, 3)]), ["null", "not null", "missing", "valued"][rng.integers(0, 4)])
    if r == 4: return "(%s between 2 and 5)" % D("g")
    return "((%s + %s) < 60)" % (D("x"), D("g"))


def rand_tree(rng, sub, budget, depth=0):
    """A condition with LIKE terms among the existing kinds: (device text, oracle text)."""
    r = rng.integers(0, 10)
    if depth < 2 and r < 4:
        op = ["and", "or"][rng.integers(0, 2)]
        parts = [rand_tree(rng, sub, budget, depth + 1) for _ in range(int(rng.integers(2, 4)))]
        return "(%s)" % (" %s " % op).join(p[0] for p in parts), "(%s)" % (" %s " % op).join(p[1] for p in parts)
    if depth < 3 and r == 4:
        d, o = rand_tree(rng, sub, budget, depth + 1)
        return "(not %s)" % d, "(not %s)" % o
    if budget[0] > 0 and (r < 8 or budget[1] == 0):
        budget[0] -= 1
        budget[1] += 1
        return sub.like(["s", "m"][rng.integers(0, 2)], PATTERNS[rng.integers(0, len(PATTERNS))])
    t = other_term(rng)
    return t, t


def rand_like_plan(rng, t, bounded):
    sub = Substitution(t)
    if bounded:
        # the bounded family: a LIKE term over a column as one of <= 2 ANDed terms, <= 3 columns, dictionary key
        col = ["s", "m"][rng.integers(0, 2)]
        d, o = sub.like(col, PATTERNS[rng.integers(0, len(PATTERNS))])
        if rng.random() < 0.75:
            second = ["(%s < %s)" % (["10", "40.5"][rng.integers(0, 2)], D("x")), "(%s is not null)" % D("x"), "(%s <= 60)" % D("x")][rng.integers(0, 3)]
            if rng.random() < 0.5:
                d, o = "(%s and %s)" % (d, second), "(%s and %s)" % (o, second)
            else:
                d, o = "(%s and %s)" % (second, d), "(%s and %s)" % (second, o)
        keys = [D("k")]
        aggs = sorted(set(["sum(%s)" % D("x")] + [["count(*)", "avg(%s)" % D("x"), "max(%s)" % D("x"), "count(%s)" % D("x")][i]
                                                   for i in rng.choice(4, int(rng.integers(0, 3)), replace=False)]))
        return sub, d, o, keys, aggs
    budget = [int(rng.integers(1, 4)), 0]
    for _ in range(50):
        sub = Substitution(t)
        b = list(budget)
        d, o = rand_tree(rng, sub, b)
        if 1 <= b[1] <= 3 and d.count(" like ") == b[1]:
            break
    else:
        d, o = sub.like("s", "ab%")
    keys = [[D("k")], [D("g")], [D("k"), D("g")], []][rng.integers(0, 4)]
    aggs = sorted(set(["count(*)"] + [["sum(%s)" % D("x"), "avg(%s)" % D("x"), "min(%s)" % D("s"), "max(%s)" % D("x"), "count(%s)" % D("m")][i]
                                      for i in rng.choice(5, int(rng.integers(1, 3)), replace=False)]))
    return sub, d, o, keys, aggs


# NOTE: tests/test_like_cpu.py (test_the_bounded_family_takes_the_gpu_differentials_bounded_plans) re-derives the bounded
# plans of this test from FAMILIES, the seed base 515_000 and the order of the draws (table size, then rand_like_plan) to
# check without a GPU that the bounded family takes them: change those here and that test follows.
# (options, bounded shape, the kernel family stats["spec_kernel"] must report: 0 interpreter / bounded kernel, 2 run-time built)
FAMILIES = [({"fast": 0}, False, 0), ({}, False, 0), ({"fast": 0}, True, 0), ({"spec": 0}, True, 0), ({"jit": 2}, True, 2), ({"jit": 2}, True, 2)]


@pytest.mark.parametrize("seed", range(int(os.environ.get("N1K_LIKE_SEEDS", "240"))))
def test_like_plans_agree_with_the_oracle_by_substitution(seed):
    rng = np.random.default_rng(515_000 + seed)
    t = make_table(rng, int(rng.integers(1, 5000)))
    opts, bounded, kernel = FAMILIES[seed % len(FAMILIES)]
    sub, dcond, ocond, keys, aggs = rand_like_plan(rng, t, bounded)
    batches = int(rng.integers(1, 4))
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
    # (spec_kernel 0 is the bounded kernel with `fast` on and the interpreter with it off: that build_fast_args takes every
    #  bounded plan drawn here, LIKE term included, is checked without a GPU by tests/test_like_cpu.py over these very seeds)
    assert st["rows_selected"] == ora.rows_passed, what


def test_the_substitution_is_sound_on_the_cpu_side_of_this_test():
    """LIKE, NOT LIKE and (NOT LIKE) OR IS NULL through the oracle's helper column give the rows the mirror gives."""
    rng = np.random.default_rng(5)
    t = make_table(rng, 3000)
    sub = Substitution(t)
    _, h = sub.like("m", "a%b")
    vals = [lu.like4(v if (v is lu.MISSING or v is None or isinstance(v, str)) else 0, "a%b") for v in column_values(t, "m")]
    ot = sub.oracle_table()
    for cond, keep in [(h, lambda r: r is True), ("(not %s)" % h, lambda r: r is False),
                       ("((not %s) or (%s is null))" % (h, h), lambda r: r is False or r is None)]:
        got = n1o.run(ot, cond, [], [], has_group=False).selected
        assert sorted(got.tolist()) == [i for i, r in enumerate(vals) if keep(r)], cond


# ------------------------------------------------------------------ the match table's life

def _table(strings, dictionary, groups=None):
    n = len(strings)
    codes = np.array([dictionary.index(x) for x in strings], dtype=np.uint32)
    g = np.array(groups if groups is not None else [0] * n, dtype=np.uint64)
    return n1o.Table([n1o.Column(D("s"), n1o.COL_DICT32, codes=codes),
                      n1o.Column(D("g"), n1o.COL_TAGGED64, tags=np.full(n, n1o.T_INT, np.uint8), payload=g)], dictionary)


def test_like_when_the_dictionary_grows_between_batches():
    """Strings interned after the first push — some of which match — are seen by the later batches: the table is extended
    for the new codes.  n1k_reset keeps it."""
    cond, keys, aggs = '(%s like "new%%")' % D("s"), [D("g")], ["count(*)"]
    d1 = [b"old", b"newer"]
    d2 = [b"old", b"newer", b"new", b"news\n", b"renew", b"x\nnew"]
    b1 = _table([b"old", b"newer", b"old"], d1, [0, 0, 1])
    b2 = _table([b"new", b"news\n", b"renew", b"x\nnew", b"old", b"newer"], d2, [0, 1, 1, 2, 2, 2])
    want = {0: 2, 1: 1, 2: 2}
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs))
    for round_ in range(2):
        for b in (b1, b2):
            op.process_items([{c.name: c for c in b.columns}[p] for p in op.column_paths], b.dictionary)
        rows = op.after_items()
        assert {k[0][1]: a[0][1] for k, a in zip(rows.keys, rows.aggs)} == want
        stats = op.like_stats()
        # every dictionary string (the batches' and the three a TAGGED64 key column makes the handle intern: NaN, ±Infinity)
        # matched exactly once — also after the reset, which keeps the table
        ndict = int(_ffi.lib().n1k_dict_size(op._h))
        assert ndict >= len(d2) and stats["host_strings"] == ndict and stats["device_strings"] == 0, (stats, ndict)
        op.reopen()
    op.done()
    # the streaming path: every n1k_push_json interns the batch's new strings
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs))
    op.process_json([b'{"g": 0, "s": "old"}', b'{"g": 0, "s": "newer"}'])
    op.process_json([b'{"g": 0, "s": "new"}', b'{"g": 1, "s": "renew"}', b'{"g": 1, "s": "news"}', b'{"g": 1, "s": 5}'])
    rows = op.after_items()
    op.done()
    assert {k[0][1]: a[0][1] for k, a in zip(rows.keys, rows.aggs)} == {0: 2, 1: 1}


def test_a_large_dictionary_takes_the_device_route_and_a_small_one_the_host_route():
    probe = query_amd.GpuFilterGroup(plan.filter_group_plan('(%s like "a%%")' % D("s"), [], ["count(*)"]))
    threshold = probe.like_stats()["device_threshold"]
    probe.done()
    assert threshold * 4 <= 4_000_000, "a threshold that large means the kernel is not worth having"
    cond = '((%s like "%%7_") or (%s like "s1%%5"))' % (D("s"), D("s"))
    for n, route in ((4 * threshold, "device"), (100, "host")):
        texts = ["s%d" % i for i in range(n)]
        texts[3] = "x" * 300 + "75"  # beyond the kernel's limit: the host matcher's, on either route
        dictionary = [x.encode() for x in texts]
        rng = np.random.default_rng(n)
        codes = rng.integers(0, n, 200_000).astype(np.uint32)
        t = n1o.Table([n1o.Column(D("s"), n1o.COL_DICT32, codes=codes)], dictionary)
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], ["count(*)"]))
        op.process_items(t.columns, dictionary)
        rows = op.after_items()
        stats = op.like_stats()
        op.done()
        hit = np.array([lu.like_mirror(x, "%7_") or lu.like_mirror(x, "s1%5") for x in texts])
        assert rows.aggs[0][0][1] == int(hit[codes].sum())
        if route == "device":
            assert stats["device_strings"] == n - 1 and stats["host_strings"] == 1, stats
        else:
            assert stats["device_strings"] == 0 and stats["host_strings"] == n, stats


def test_having_like_over_a_string_group_key():
    rng = np.random.default_rng(9)
    t = make_table(rng, 4000)
    keys, aggs = [D("k")], ["count(*)"]
    ora = n1o.run(t, None, keys, aggs)
    for having, keep in [('(%s like "cat\\\\_1%%")' % D("k"), lambda v: v is True), ('(not (%s like "cat\\\\_1%%"))' % D("k"), lambda v: v is False)]:
        gpu, _ = pu.run_gpu(t, None, keys, aggs, having=having)

        def val(k):
            return lu.MISSING if k[0] == n1o.T_MISSING else (None if k[0] != n1o.T_STRING else k[1].decode())
        want = sorted((k[0], a[0][1]) for k, a in zip(ora.keys, ora.aggs) if keep(lu.like4(val(k[0]), "cat\\_1%")))
        got = sorted((k[0], a[0][1]) for k, a in zip(gpu.keys, gpu.aggs))
        assert got == want and len(want) >= 1 and len(want) < len(ora.keys), (having, got, want)
    # the key is NULL / MISSING in some groups: NOT LIKE keeps neither (NULL / MISSING are not TRUE)
    assert any(k[0][0] == n1o.T_NULL for k in ora.keys) and any(k[0][0] == n1o.T_MISSING for k in ora.keys)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("jit", [0, 2], ids=["interpreter", "runtime-built"])
def test_like_across_two_ranks_over_the_loopback_transport(jit):
    """World size 2, row exchange: the sender evaluates the Filter — LIKE through its own handle's table — and every rank ends
    with the substituted oracle's groups."""
    from query_amd import distributed as qd
    from query_amd.gpu_operator import GroupRows
    from test_gpu_distributed import _device_cols, _run_ranks
    world, n = 2, 60_011
    rng = np.random.default_rng(31 + jit)
    t = make_table(rng, n)
    sub = Substitution(t)
    d, o = sub.like("s", "%ab%")
    dcond, ocond = "(%s and (10 < %s))" % (d, D("x")), "(%s and (10 < %s))" % (o, D("x"))
    keys, aggs = [D("k")], sorted(["count(*)", "sum(%s)" % D("x")])
    ora = n1o.run(sub.oracle_table(), ocond, keys, aggs)
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
        assert (info["sender_kernel"] != 0) == (jit == 2), info  # scan_spec_partition_body saw the LIKE term, or partition_kernel did
    assert sum(info["recv_rows"] for _, info in outs) == ora.rows_passed
