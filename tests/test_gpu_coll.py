"""ANY / EVERY ... SATISFIES on the device: the reference's statements, the device evaluator against the host evaluator and
the mirror, and a differential against the oracle BY SUBSTITUTION, as tests/test_gpu_like.py does it for LIKE — the oracle
has no collection predicates, but it evaluates a bare path inside AND / OR / NOT with the full 4-valued logic, so every
`any ... end` term of the device's plan becomes, for the oracle, a helper column that holds the mirror's TRUE / FALSE / NULL
/ MISSING of that row (tests/coll_util.py)."""
import json
import os
import random

import numpy as np
import pytest

import coll_util as cu
import golden_util as gu
import like_util as lu
import parity_util as pu
import query_amd
from oracle import n1o
from query_amd import _ffi, plan

pytestmark = pytest.mark.gpu


def D(name):
    return plan.field_path("default", name)


with open(os.path.join(gu.GOLDEN, "cases_any.json")) as fh:
    ANY_CASES = json.load(fh)["cases"]


@pytest.mark.parametrize("case", ANY_CASES, ids=[c["id"] for c in ANY_CASES])
def test_the_references_any_statements(case):
    docs = gu.load_docs(case["keyspace"])
    table = gu.build_table(docs, case["columns"])
    p = case["plan"]
    if p.get("filter_only"):
        rows, _ = pu.run_gpu(table, p["condition"], [], [], filter_only=True)
        got = gu.replay_filter_post(case, docs, rows.selected)
    else:
        rows, _ = pu.run_gpu(table, p["condition"], p["group_keys"], p["aggregates"], having=case["having_text"])
        got = gu.replay_post(case, gu.groups_from_result(rows), having_done=True)
    assert gu.same_json(got, case["results"]), (got, case["results"])


# ------------------------------------------------------------------ the evaluators

DEV_MAX_LEN = 192  # bytes of canonical text coll_match_kernel takes (include/n1k.h, n1k_coll_eval_device)
SLAB = 64 * DEV_MAX_LEN

CPU_PAIRS = (20241017, 600, 40)  # the pairs of tests/test_coll_cpu.py: seed, terms, arrays per term


def mirror_bits(mode, cond, arrays):
    return np.array([cu.coll_mirror(mode, cond, a) is True for a in arrays], dtype=np.uint8)


def test_device_evaluator_equals_host_evaluator_and_mirror_on_the_cpu_tests_pairs():
    total = 0
    for mode, cond, arrays in cu.random_pairs(*CPU_PAIRS):
        term, texts = cu.term_text(mode, cond), cu.texts_of(arrays)
        dev, left = cu.device_eval(term, texts)
        host = cu.host_eval(term, texts)
        want = mirror_bits(mode, cond, arrays)
        assert np.array_equal(dev, host) and np.array_equal(dev, want), (term, texts[:4])
        assert left <= len(texts)
        total += len(texts)
    assert total >= 20000


MILLION_TERMS = [
    (cu.ANY, ("cmp", "=", [], "t_1", False)),
    (cu.EVERY, ("or", [("cmp", "<", [], "b", False), ("is", [], "null")])),
    (cu.ANY_EVERY, ("not", ("cmp", "=", [], 3, True))),
    (cu.ANY, ("and", [("like", [], "a%"), ("not", ("cmp", "=", [], "ab", False))])),
    (cu.ANY, ("cmp", "<=", ["f"], 2, True)),
    (cu.EVERY, ("is", ["f"], "missing")),
]


def test_device_evaluator_on_a_million_arrays_of_every_length():
    """Arrays of plain scalars and small objects, from empty to beyond the kernel's limit.  out_left_to_host counts exactly
    the arrays the documented limits exclude: the ones longer than 192 bytes and — for the terms that compare or match a
    string — the directed ones whose first element holds a backslash escape."""
    rng = np.random.default_rng(99)
    n = 1_050_000
    atoms = np.array(['"a"', '"b"', '"ab"', '"t_1"', '"é"', "1", "2", "3", "2.5", "null", "true", '{"f":1}', '{"f":3,"g":"a"}', "[1]"], dtype=object)
    lens = rng.integers(0, 6, n)
    long_ix = rng.choice(n, 3000, replace=False)
    lens[long_ix] = rng.integers(20, 250, 3000)  # 80 B to over 1 KiB of text: on both sides of the limit
    picks = atoms[rng.integers(0, len(atoms), int(lens.sum()))]
    cuts = np.concatenate([[0], np.cumsum(lens)])
    texts = ["[" + ",".join(picks[cuts[i]:cuts[i + 1]]) + "]" for i in range(n)]
    esc_ix = [int(i) for i in rng.choice(n, 400, replace=False) if lens[i] < 6]
    for i in esc_ix:  # an escaped string FIRST: no early exit can hide it from a term that compares strings
        texts[i] = '["x\\"y"' + ("," if lens[i] else "") + texts[i][1:]
    raw = [t.encode() for t in texts]
    too_long = sum(1 for b in raw if len(b) > DEV_MAX_LEN)
    assert too_long > 500 and max(len(b) for b in raw) > 4 * DEV_MAX_LEN and min(len(b) for b in raw) == 2
    assert sum(1 for b in raw if DEV_MAX_LEN - 40 < len(b) <= DEV_MAX_LEN) > 20
    uniq = {}
    for t in texts:
        uniq.setdefault(t, len(uniq))
    values = [json.loads(t) for t in uniq]
    index = np.fromiter((uniq[t] for t in texts), dtype=np.int64, count=n)
    for mode, cond in MILLION_TERMS:
        term = cu.term_text(mode, cond)
        dev, left = cu.device_eval(term, raw)
        host = cu.host_eval(term, raw)
        assert np.array_equal(dev, host), term
        want = mirror_bits(mode, cond, values)[index]
        assert np.array_equal(dev, want), term
        assert 0 < int(want.sum()) < n, term
        # a string meets a constant (or a pattern) only in the terms that compare the bare variable with a STRING; the
        # escaped first element is then the host's.  `= 3` and the field terms never decode a string.
        reads_strings = term.count('"') > 0 and "`v`.`f`" not in term
        assert left == too_long + (len(esc_ix) if reads_strings else 0), (term, left, too_long, len(esc_ix))


def test_device_evaluator_when_a_waves_entries_span_more_than_its_slab():
    """Runs of consecutive long arrays with short ones in between: the 64 entries of such a wave span more than the 12 KiB LDS
    slab, and its lanes read the arrays the kernel does take straight from global memory."""
    rng = random.Random(3)
    arrays = []
    for block in range(300):
        for i in range(64):
            if block % 2 == 0 and i % 8 != 7:
                a = [rng.choice(["a", "b", "t_1", "ab", 1, 2, None]) for _ in range(rng.randint(100, 140))]  # 200 B and up
            else:
                a = [rng.choice(["a", "b", "t_1", 1, None, {"f": 2}]) for _ in range(rng.randint(0, 4))]
            if block % 2 == 0 and i % 16 == 3:
                a = ["ab"] * 30 + ["t_1"]  # within the limit (157 B) inside a long run
            arrays.append(a)
    texts = cu.texts_of(arrays)
    spans = [sum(len(s) for s in texts[w:w + 64]) for w in range(0, len(texts), 64)]
    assert max(spans) > SLAB and min(spans) < SLAB
    excluded = sum(1 for s in texts if len(s) > DEV_MAX_LEN)
    taken_in_wide_waves = sum(1 for w in range(0, len(texts), 64) if spans[w // 64] > SLAB for s in texts[w:w + 64] if len(s) <= DEV_MAX_LEN)
    assert taken_in_wide_waves > 1000 and excluded > 1000
    for mode, cond in MILLION_TERMS[:4]:
        term = cu.term_text(mode, cond)
        dev, left = cu.device_eval(term, texts)
        host = cu.host_eval(term, texts)
        want = mirror_bits(mode, cond, arrays)
        assert left == excluded and np.array_equal(dev, host) and np.array_equal(dev, want), term


BLOCK_EDGES = [1, 63, 64, 65, 255, 256, 257]  # the last lane's clamp, a full wave, a wave of one lane, a second workgroup of one entry


def test_device_evaluator_at_the_edges_of_a_block():
    """Blocks that end inside a wave, on a wave and one entry into the next workgroup; entries of 0 to 40 bytes, some of them
    no array text.  Once more with a last array of 15 KB: the final wave then spans more than its slab and reads what it
    takes from global memory."""
    rng = random.Random(11)
    mode, cond = cu.ANY, ("cmp", "=", [], "t_1", False)
    term = cu.term_text(mode, cond)
    pool = []
    for i in range(max(BLOCK_EDGES)):
        if i % 7 == 3:
            pool.append(rng.choice([b"", b"[", b"plain", b"]["]))
            continue
        text = cu.texts_of([[rng.choice(["a", "t_1", "ab", 1, None, {"f": 2}]) for _ in range(rng.randint(0, 5))]])[0]
        pool.append(text if len(text) <= 40 else b"[]")
    assert min(len(e) for e in pool) == 0 and max(len(e) for e in pool) > 30
    huge = cu.texts_of([["ab"] * 3000 + ["t_1"]])[0]
    assert len(huge) > SLAB
    for n in BLOCK_EDGES:
        for last in (None, huge):
            entries = pool[:n] if last is None else pool[:n - 1] + [last]
            dev, left = cu.device_eval(term, entries)
            host = cu.host_eval(term, entries)
            assert np.array_equal(dev, host), (n, last is None, np.nonzero(dev != host))
            assert left == sum(1 for e in entries if len(e) >= 2 and e[:1] == b"[" and len(e) > DEV_MAX_LEN), (n, left)
            assert n < 64 or 0 < int(host.sum()) < n


# ------------------------------------------------------------------ differential by substitution

# dictionary: strings, then the canonical texts of arrays (and one object) that the terms below split in many ways
WORDS = ["", "a", "ab", "abc", "b", "t_1", "t_2", "é", "a\\b", "[not an array", "cat_1", "cat_10", "cat_11", "cat_2", "zz"]
KEY0 = WORDS.index("cat_1")
ARRAYS = [[], ["a"], ["t_1"], ["a", "t_1"], ["b", "ab", "abc"], [1], [1, 2, 3], [2.5, "a"], [None], [None, "t_1"], [True, False], [[1], ["a"]],
          [{"f": 1}], [{"f": "a", "g": {"h": 2}}], [{"g": {"h": "t_1"}}, {"f": 3}], [{"f": None}, 1], ["é", 'x"y'], ["a\\b", "a\nb"], [2 ** 53 + 1, 0.1],
          [{"f": 2}, {"f": 2}], ["ab", "ab"], [{"f": "t_1", "h": []}], [0], ["zz", {"f": True}]]
OBJECT = {"f": 1}
DICT = [w.encode() for w in WORDS] + [cu.canon(a).encode() for a in ARRAYS] + [cu.canon(OBJECT).encode()]
ARR0, OBJ0 = len(WORDS), len(WORDS) + len(ARRAYS)
PATTERNS = ["a%", "%b", "t\\_%", "", "%", "_", "ab"]


def make_table(rng, n):
    """a: TAGGED64 of every class — arrays most of all, strings, numbers, booleans, NULL, MISSING, an object; s: DICT32
    strings with NULL / MISSING; x: numbers; k: DICT32 key; g: small ints."""
    at = np.zeros(n, np.uint8)
    ap = np.zeros(n, np.uint64)
    r = rng.integers(0, 100, n)
    ar = r < 60
    at[ar] = n1o.T_ARRAY
    ap[ar] = (ARR0 + rng.integers(0, len(ARRAYS), int(ar.sum()))).astype(np.uint64)
    st = (r >= 60) & (r < 68)
    at[st] = n1o.T_STRING
    ap[st] = rng.integers(0, len(WORDS), int(st.sum())).astype(np.uint64)
    it = (r >= 68) & (r < 74)
    at[it] = n1o.T_INT
    ap[it] = rng.integers(-3, 4, int(it.sum())).astype(np.int64).view(np.uint64)
    ft = (r >= 74) & (r < 77)
    at[ft] = n1o.T_FLOAT
    ap[ft] = (rng.integers(0, 8, int(ft.sum())) + 0.5).view(np.uint64)
    at[(r >= 77) & (r < 80)] = n1o.T_TRUE
    at[(r >= 80) & (r < 83)] = n1o.T_FALSE
    at[(r >= 83) & (r < 89)] = n1o.T_NULL
    at[(r >= 89) & (r < 95)] = n1o.T_MISSING
    ob = r >= 95
    at[ob] = n1o.T_OBJECT
    ap[ob] = OBJ0
    sc = rng.integers(0, len(WORDS), n).astype(np.uint32)
    sc[rng.random(n) < 0.05] = 0xFFFFFFFE
    sc[rng.random(n) < 0.05] = 0xFFFFFFFF
    xt = np.full(n, n1o.T_FLOAT, np.uint8)
    xp = (rng.integers(0, 800, n) / 8.0 + 0.0625).view(np.uint64).copy()
    ints = rng.random(n) < 0.3
    xt[ints] = n1o.T_INT
    xp[ints] = rng.integers(0, 100, int(ints.sum())).astype(np.int64).view(np.uint64)
    xt[rng.random(n) < 0.03] = n1o.T_NULL
    kc = rng.integers(KEY0, len(WORDS), n).astype(np.uint32)  # cat_1 .. zz
    kc[rng.random(n) < 0.04] = 0xFFFFFFFE
    kc[rng.random(n) < 0.03] = 0xFFFFFFFF
    gt = np.full(n, n1o.T_INT, np.uint8)
    gp = rng.integers(0, 7, n).astype(np.int64).view(np.uint64).copy()
    return n1o.Table([n1o.Column(D("a"), n1o.COL_TAGGED64, tags=at, payload=ap), n1o.Column(D("s"), n1o.COL_DICT32, codes=sc),
                      n1o.Column(D("x"), n1o.COL_TAGGED64, tags=xt, payload=xp), n1o.Column(D("k"), n1o.COL_DICT32, codes=kc),
                      n1o.Column(D("g"), n1o.COL_TAGGED64, tags=gt, payload=gp)], list(DICT))


def column_values(t, name):
    """Python values of a column as the mirrors take them: a list for an array, a str for a string, cu.MISSING, None (NULL),
    a dict for the object, 0 for every other class."""
    c = {c.name: c for c in t.columns}[D(name)]
    if c.kind == n1o.COL_DICT32:
        return [cu.MISSING if x == 0xFFFFFFFF else (None if x == 0xFFFFFFFE else WORDS[x]) for x in c.codes.tolist()]
    out = []
    for tg, p in zip(c.tags.tolist(), c.payload.tolist()):
        if tg == n1o.T_MISSING:
            out.append(cu.MISSING)
        elif tg == n1o.T_NULL:
            out.append(None)
        elif tg == n1o.T_STRING:
            out.append(WORDS[p])
        elif tg == n1o.T_ARRAY:
            out.append(ARRAYS[p - ARR0])
        elif tg == n1o.T_OBJECT:
            out.append(OBJECT)
        else:
            out.append(0)
    return out


def logic_tags(results):
    return np.array([n1o.T_MISSING if r is cu.MISSING else (n1o.T_NULL if r is None else (n1o.T_TRUE if r else n1o.T_FALSE)) for r in results], np.uint8)


class Substitution:
    """Collects the collection and LIKE terms of one plan: the device sees the term, the oracle a helper column of its
    4-valued results."""

    def __init__(self, table):
        self.table = table
        self.helpers = []

    def _helper(self, results):
        name = D("h%d" % len(self.helpers))
        self.helpers.append(n1o.Column(name, n1o.COL_TAGGED64, tags=logic_tags(results), payload=np.zeros(len(results), np.uint64)))
        return name

    def coll(self, col, mode, cond):
        cache = {}
        res = []
        for v in column_values(self.table, col):
            key = id(v) if isinstance(v, (list, dict)) else v
            if key not in cache:
                cache[key] = cu.coll_mirror(mode, cond, v)
            res.append(cache[key])
        return cu.term_text(mode, cond, over=D(col), var=["v", "g", col][len(self.helpers) % 3]), self._helper(res)

    def like(self, col, pattern):
        res = [lu.like4(v if (v is cu.MISSING or v is None or isinstance(v, str)) else 0, pattern) for v in column_values(self.table, col)]
        return "(%s like %s)" % (D(col), json.dumps(pattern, ensure_ascii=False)), self._helper(res)

    def oracle_table(self):
        return n1o.Table(list(self.table.columns) + self.helpers, self.table.dictionary)


def py_rng(rng):
    return random.Random(int(rng.integers(0, 2 ** 31)))


def other_term(rng):
    r = rng.integers(0, 6)
    if r == 0: return "(%s < %s)" % (["10", "40.5", "70"][rng.integers(0, 3)], D("x"))
    if r == 1: return "(%s <= %s)" % (D("x"), ["30", "55.25"][rng.integers(0, 2)])
    if r == 2: return "(%s = %s)" % (D("s"), ["\"ab\"", "\"t_1\""][rng.integers(0, 2)])
    if r == 3: return "(%s is %s)" % (D(["a", "s", "x"][rng.integers(0, 3)]), ["null", "not null", "missing", "valued"][rng.integers(0, 4)])
    if r == 4: return "(%s between 2 and 5)" % D("g")
    return "((%s + %s) < 60)" % (D("x"), D("g"))


def draw_coll(rng, sub):
    """A seeded term that splits ARRAYS: some satisfy it, some do not (a term nothing satisfies tests little)."""
    r = py_rng(rng)
    for _ in range(40):
        mode, cond = cu.random_term(r)
        hits = sum(cu.coll_mirror(mode, cond, a) is True for a in ARRAYS)
        if 0 < hits < len(ARRAYS):
            break
    col = "a" if rng.random() < 0.8 else "s"  # (a DICT32 operand: NULL for every string)
    return sub.coll(col, mode, cond)


def rand_tree(rng, sub, budget, depth=0):
    """A condition with collection terms among the existing kinds and LIKE terms: (device text, oracle text)."""
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
        return draw_coll(rng, sub)
    if r == 9:
        return sub.like(["s", "a"][rng.integers(0, 2)], PATTERNS[rng.integers(0, len(PATTERNS))])
    t = other_term(rng)
    return t, t


def rand_coll_plan(rng, t, bounded):
    sub = Substitution(t)
    if bounded:
        # the bounded family: a collection term over a column as one of <= 2 ANDed terms, <= 3 columns, dictionary key
        d, o = draw_coll(rng, sub)
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
        if 1 <= b[1] <= 3 and d.count(" satisfies ") == b[1]:
            break
    else:
        sub = Substitution(t)
        d, o = sub.coll("a", cu.ANY, ("cmp", "=", [], "t_1", False))
    keys = [[D("k")], [D("g")], [D("k"), D("g")], []][rng.integers(0, 4)]
    aggs = sorted(set(["count(*)"] + [["sum(%s)" % D("x"), "avg(%s)" % D("x"), "min(%s)" % D("s"), "max(%s)" % D("x"), "count(%s)" % D("a")][i]
                                      for i in rng.choice(5, int(rng.integers(1, 3)), replace=False)]))
    return sub, d, o, keys, aggs


# NOTE: tests/test_coll_cpu.py re-derives the plans of this test from FAMILIES, the seed base 616_000 and the order of the
# draws (table size, then rand_coll_plan) to check without a GPU that n1k_create takes every one of them and that the bounded
# family takes the bounded ones: change those here and that test follows.
# (options, bounded shape, the kernel family stats["spec_kernel"] must report: 0 interpreter / bounded kernel, 2 run-time built)
FAMILIES = [({"fast": 0}, False, 0), ({}, False, 0), ({"fast": 0}, True, 0), ({"spec": 0}, True, 0), ({"jit": 2}, True, 2), ({"jit": 2}, True, 2)]
SEED_BASE = 616_000
NSEEDS = 240


def draw(seed):
    rng = np.random.default_rng(SEED_BASE + seed)
    t = make_table(rng, int(rng.integers(1, 5000)))
    opts, bounded, kernel = FAMILIES[seed % len(FAMILIES)]
    sub, dcond, ocond, keys, aggs = rand_coll_plan(rng, t, bounded)
    return rng, t, opts, bounded, kernel, sub, dcond, ocond, keys, aggs


@pytest.mark.parametrize("seed", range(NSEEDS))
def test_collection_plans_agree_with_the_oracle_by_substitution(seed):
    rng, t, opts, bounded, kernel, sub, dcond, ocond, keys, aggs = draw(seed)
    batches = int(rng.integers(1, 4))
    what = "device %r oracle %r keys %r aggs %r opts %r batches %d" % (dcond, ocond, keys, aggs, opts, batches)
    ot = sub.oracle_table()
    # Filter-only: the selected row ordinals (a skip or N1K_UNSUPPORTED is a failure: the generator draws the accepted subset)
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


def test_the_substitution_is_sound_on_the_cpu_side_of_this_test():
    """ANY, NOT ANY and (NOT ANY) OR IS NULL through the oracle's helper column give the rows the mirror gives — over a
    binding column of every tag class, and over the DICT32 one, where no row is TRUE or FALSE."""
    rng = np.random.default_rng(5)
    t = make_table(rng, 3000)
    cond = ("cmp", "=", [], "t_1", False)
    for col in ("a", "s"):
        sub = Substitution(t)
        _, h = sub.coll(col, cu.ANY, cond)
        vals = [cu.coll_mirror(cu.ANY, cond, v) for v in column_values(t, col)]
        assert (col == "s") == all(v is None or v is cu.MISSING for v in vals)
        ot = sub.oracle_table()
        for text, keep in [(h, lambda r: r is True), ("(not %s)" % h, lambda r: r is False),
                           ("((not %s) or (%s is null))" % (h, h), lambda r: r is False or r is None)]:
            got = n1o.run(ot, text, [], [], has_group=False).selected
            assert sorted(got.tolist()) == [i for i, r in enumerate(vals) if keep(r)], (col, text)
    assert {True, False, None, cu.MISSING} == set(cu.coll_mirror(cu.ANY, cond, v) for v in column_values(t, "a"))


# ------------------------------------------------------------------ the table's size, its life, its routes

def array_dictionary(nwords):
    """nwords distinct arrays (entry i holds "w<i>", a third of them "t_1" too), as values and as dictionary entries."""
    arrays = [["w%d" % i] + (["t_1"] if i % 3 == 0 else []) + ([i] if i % 2 else []) for i in range(nwords)]
    return arrays, cu.texts_of(arrays)


def test_collection_term_on_both_sides_of_the_lds_switch():
    """The bounded and the run-time-built kernels stage a table of at most 4096 entries in LDS and read a larger one from
    global memory: dictionaries of 3000 and of 6000 arrays, against the oracle by substitution."""
    mode, cond = cu.ANY, ("cmp", "=", [], "t_1", False)
    for nwords in (3000, 6000):
        rng = np.random.default_rng(nwords)
        arrays, texts = array_dictionary(nwords)
        n = 50_000
        at = np.full(n, n1o.T_ARRAY, np.uint8)
        ap = rng.integers(0, nwords, n).astype(np.uint64)
        at[rng.random(n) < 0.05] = n1o.T_NULL
        at[rng.random(n) < 0.03] = n1o.T_MISSING
        xt = np.full(n, n1o.T_INT, np.uint8)
        xp = rng.integers(0, 100, n).astype(np.int64).view(np.uint64).copy()
        gt = np.full(n, n1o.T_INT, np.uint8)
        gp = rng.integers(0, 5, n).astype(np.int64).view(np.uint64).copy()
        hit = mirror_bits(mode, cond, arrays)
        res = [cu.MISSING if tg == n1o.T_MISSING else (None if tg == n1o.T_NULL else bool(hit[int(p)])) for tg, p in zip(at.tolist(), ap.tolist())]
        cols = [n1o.Column(D("a"), n1o.COL_TAGGED64, tags=at, payload=ap), n1o.Column(D("x"), n1o.COL_TAGGED64, tags=xt, payload=xp),
                n1o.Column(D("g"), n1o.COL_TAGGED64, tags=gt, payload=gp)]
        t = n1o.Table(cols, list(texts))
        ot = n1o.Table(cols + [n1o.Column(D("h"), n1o.COL_TAGGED64, tags=logic_tags(res), payload=np.zeros(n, np.uint64))], t.dictionary)
        dcond = "(%s and (10 < %s))" % (cu.term_text(mode, cond, over=D("a")), D("x"))
        ocond = "(%s and (10 < %s))" % (D("h"), D("x"))
        aggs = sorted(["count(*)", "sum(%s)" % D("x")])
        for keys, families in (([], (({"jit": 2}, 2), ({"spec": 0}, 0), ({"fast": 0}, 0))), ([D("g")], (({"jit": 2}, 2),))):
            ora = n1o.run(ot, ocond, keys, aggs)
            assert 0 < ora.rows_passed < n // 2
            for opts, kernel in families:
                gpu, st = pu.run_gpu(t, dcond, keys, aggs, batches=2, **opts)
                pu.assert_same_groups(gpu, ora, aggs=aggs)
                assert st["spec_kernel"] == kernel and st["rows_selected"] == ora.rows_passed, (nwords, keys, opts, st)


def distinct_plan(nwords, n=60_000):
    """`WHERE ANY v IN r SATISFIES v = "t_1" END GROUP BY k, COUNT(DISTINCT b), COUNT(DISTINCT c), SUM(b)` cannot be a
    three-column shape, so the two DISTINCT operands are b and the key's own column: r (arrays, TAGGED64), k (DICT32 key),
    b (small ints)."""
    rng = np.random.default_rng(nwords)
    words = ["k%d" % i for i in range(nwords)]
    arrays = [["t_1", "a"], ["a"], [], ["b", {"f": "t_1"}], [1, "t_1"]]
    dictionary = [w.encode() for w in words] + cu.texts_of(arrays)
    kc = rng.integers(0, nwords, n).astype(np.uint32)
    kc[rng.random(n) < 0.02] = 0xFFFFFFFE
    kc[rng.random(n) < 0.02] = 0xFFFFFFFF
    rt = np.full(n, n1o.T_ARRAY, np.uint8)
    rp = (nwords + rng.integers(0, len(arrays), n)).astype(np.uint64)
    rt[rng.random(n) < 0.03] = n1o.T_NULL
    rt[rng.random(n) < 0.03] = n1o.T_MISSING
    bt = np.full(n, n1o.T_INT, np.uint8)
    bp = rng.integers(0, 6, n).astype(np.int64).view(np.uint64).copy()
    bt[rng.random(n) < 0.03] = n1o.T_NULL
    mode, cond = cu.ANY, ("cmp", "=", [], "t_1", False)
    hit = mirror_bits(mode, cond, arrays)
    res = [cu.MISSING if tg == n1o.T_MISSING else (None if tg == n1o.T_NULL else bool(hit[int(p) - nwords])) for tg, p in zip(rt.tolist(), rp.tolist())]
    cols = [n1o.Column(D("r"), n1o.COL_TAGGED64, tags=rt, payload=rp), n1o.Column(D("k"), n1o.COL_DICT32, codes=kc),
            n1o.Column(D("b"), n1o.COL_TAGGED64, tags=bt, payload=bp)]
    t = n1o.Table(cols, dictionary)
    ot = n1o.Table(cols + [n1o.Column(D("h"), n1o.COL_TAGGED64, tags=logic_tags(res), payload=np.zeros(n, np.uint64))], t.dictionary)
    keys, aggs = [D("k")], sorted(["count(distinct %s)" % D("b"), "count(distinct %s)" % D("r"), "sum(%s)" % D("b")])
    return t, ot, cu.term_text(mode, cond, over=D("r")), D("h"), keys, aggs


@pytest.mark.parametrize("nwords", [1400, 1480, 1530, 1580, 1700, 1850])
def test_collection_term_with_two_count_distinct_where_the_lds_is_full(nwords):
    """Through the run-time-built scan: the DIRECT table, two word scatters and their "already logged" caches are sized to fill
    a CU's 160 KiB of LDS, and the shape's 4 KiB for the staged table has to be part of that budget — the key dictionaries
    around which tests/test_gpu_like.py found a budget without it to overflow."""
    t, ot, dcond, ocond, keys, aggs = distinct_plan(nwords)
    ora = n1o.run(ot, ocond, keys, aggs)
    gpu, st = pu.run_gpu(t, dcond, keys, aggs, batches=2, jit=2)
    pu.assert_same_groups(gpu, ora, aggs=aggs)
    assert st["spec_kernel"] == 2 and st["rows_selected"] == ora.rows_passed, st


def _table(values, dictionary, groups):
    n = len(values)
    tags = np.full(n, n1o.T_ARRAY, np.uint8)
    codes = np.array([dictionary.index(cu.canon(v).encode()) for v in values], dtype=np.uint64)
    g = np.array(groups, dtype=np.uint64)
    return n1o.Table([n1o.Column(D("a"), n1o.COL_TAGGED64, tags=tags, payload=codes),
                      n1o.Column(D("g"), n1o.COL_TAGGED64, tags=np.full(n, n1o.T_INT, np.uint8), payload=g)], dictionary)


def test_collection_term_when_the_dictionary_grows_between_batches():
    """Arrays interned after the first push — some of which satisfy the term — are seen by the later batches: the table is
    extended for the new codes.  n1k_reset keeps it."""
    cond = cu.term_text(cu.ANY, ("like", [], "new%"), over=D("a"))
    keys, aggs = [D("g")], ["count(*)"]
    v1 = [["old"], ["newer", 1]]
    v2 = v1 + [["new"], [1, "news"], ["renew"], [{"f": "new"}]]
    d1, d2 = cu.texts_of(v1), cu.texts_of(v2)
    b1 = _table([["old"], ["newer", 1], ["old"]], d1, [0, 0, 1])
    b2 = _table([["new"], [1, "news"], ["renew"], [{"f": "new"}], ["old"], ["newer", 1]], d2, [0, 1, 1, 2, 2, 2])
    want = {0: 2, 1: 1, 2: 1}
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs))
    for round_ in range(2):
        for b in (b1, b2):
            op.process_items([{c.name: c for c in b.columns}[p] for p in op.column_paths], b.dictionary)
        rows = op.after_items()
        assert {k[0][1]: a[0][1] for k, a in zip(rows.keys, rows.aggs)} == want
        stats = op.coll_stats()
        # every array of the dictionary evaluated exactly once — also after the reset, which keeps the table
        assert stats["host_arrays"] == len(d2) and stats["device_arrays"] == 0 and stats["predicates"] == 1, stats
        op.reopen()
    op.done()


def test_a_large_dictionary_takes_the_device_route_and_a_small_one_the_host_route():
    probe = query_amd.GpuFilterGroup(plan.filter_group_plan(cu.term_text(cu.ANY, ("cmp", "=", [], "a", False), over=D("a")), [], ["count(*)"]))
    threshold = probe.coll_stats()["device_threshold"]
    probe.done()
    assert threshold * 4 <= 4_000_000, "a threshold that large means the kernel is not worth having"
    c1, c2 = ("cmp", "=", [], "t_1", False), ("like", [], "w%7")
    cond = "(%s or %s)" % (cu.term_text(cu.ANY, c1, over=D("a")), cu.term_text(cu.EVERY, c2, over=D("a")))
    for n, route in ((4 * threshold, "device"), (100, "host")):
        arrays, texts = array_dictionary(n)
        arrays[3] = ["w3"] * 60 + ["t_1"]  # beyond the kernel's limit: the host evaluator's, on either route
        arrays[5] = ['x"y', "t_1"]         # an escaped string under a comparison: idem
        texts = cu.texts_of(arrays)
        dictionary = list(texts) + [b"plain string", b"[looks like one"]  # (strings: no row with tag ARRAY reads their entries)
        rng = np.random.default_rng(n)
        codes = rng.integers(0, n, 200_000).astype(np.uint64)
        t = n1o.Table([n1o.Column(D("a"), n1o.COL_TAGGED64, tags=np.full(len(codes), n1o.T_ARRAY, np.uint8), payload=codes)], dictionary)
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], ["count(*)"]))
        op.process_items(t.columns, dictionary)
        rows = op.after_items()
        stats = op.coll_stats()
        op.done()
        hit = (mirror_bits(cu.ANY, c1, arrays) | mirror_bits(cu.EVERY, c2, arrays)).astype(bool)
        assert rows.aggs[0][0][1] == int(hit[codes.astype(np.int64)].sum())
        narr = n + 1  # (the string that begins with '[' is evaluated too: the dictionary does not record a tag)
        if route == "device":
            assert stats["device_arrays"] == narr - 2 and stats["host_arrays"] == 2, stats
        else:
            assert stats["device_arrays"] == 0 and stats["host_arrays"] == narr, stats
        assert stats["predicates"] == 2


LIKE_MAX_LEN = 128  # bytes of a string like_match_kernel takes (tests/test_gpu_like.py)
MIXED_PATTERNS = ["%7", "%b_c%"]
MIXED_PREDS = [(cu.ANY, ("cmp", "=", [], "t_1", False)), (cu.EVERY, ("like", [], "%w%4"))]


def mixed_dictionary(n, tag, with_bracket):
    """n distinct entries, strings then arrays, every one marked with `tag`; among them what each kernel leaves to the host
    and what only looks like an array.  Returns (entries, texts of the strings as Go reads them, array values)."""
    ns = n // 2
    strings = [("%s%d" % (tag, i)).encode() for i in range(ns)]
    strings[1] = (tag + "x" * 300 + "7").encode()     # over 128 B: the host matcher's (and matches "%7")
    strings[2] = b"ab\xffc" + tag.encode()            # not valid UTF-8: idem (the byte is one U+FFFD, which `_` takes)
    strings[3] = ("[looks like one " + tag).encode()  # a STRING that begins with '[': evaluated as array text, read by no ARRAY row
    if with_bracket:
        strings[4] = b"["                             # one byte: no array text
    arrays = [[tag + "w%d" % i] + (["t_1"] if i % 3 == 0 else []) + ([i] if i % 2 else []) for i in range(n - ns)]
    arrays[1] = [tag + "w1"] * 60 + ["t_1"]           # over 192 B: the host evaluator's
    arrays[2] = ['x"y', tag, "t_1"]                   # an escaped string FIRST, under both predicates: idem
    return strings + cu.texts_of(arrays), [s.decode("utf-8", errors="replace") for s in strings], arrays


def valid_utf8(b):
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def mixed_counts(entries, on_device):
    """(device strings, host strings, device arrays, host arrays) of one extension of the table by `entries`, by the rules
    DESIGN.md §4 states: LIKE is evaluated for every entry, and the kernel leaves a string over 128 B or not valid UTF-8;
    ANY / EVERY for an entry of at least 2 bytes that begins with '[', and the kernel leaves one over 192 B or one with an
    escaped string where these predicates compare (mixed_dictionary puts the escape first: no early exit hides it)."""
    like_left = sum(1 for e in entries if len(e) > LIKE_MAX_LEN or not valid_utf8(e))
    arr = [e for e in entries if len(e) >= 2 and e[:1] == b"["]
    coll_left = sum(1 for e in arr if len(e) > DEV_MAX_LEN or b"\\" in e)
    if not on_device:
        return 0, len(entries), 0, len(arr)
    return len(entries) - like_left, like_left, len(arr) - coll_left, coll_left


@pytest.mark.parametrize("below", [1, 0], ids=["host-route-then-device", "device-route-twice"])
def test_a_plan_with_like_and_collection_terms_builds_one_table_on_both_routes(below):
    """Two LIKE patterns over a string column and an ANY and an EVERY over an array column in one Filter: a dictionary of
    T - 1 entries goes through the host matchers for both kinds, one of T through both kernels (one upload, merged once).
    A second batch then interns T more: the table is extended — from an odd entry when the first held T - 1 — by both
    kernels, and the old entries keep their bits."""
    cond = "(%s or %s or %s or %s)" % tuple(["(%s like %s)" % (D("s"), json.dumps(p)) for p in MIXED_PATTERNS] +
                                            [cu.term_text(m, c, over=D("a")) for m, c in MIXED_PREDS])
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], ["count(*)"]))
    T = op.like_stats()["device_threshold"]
    assert T == op.coll_stats()["device_threshold"] and T % 2 == 0
    rng = np.random.default_rng(below)
    dictionary, str_hit, arr_hit, str_codes, arr_codes = [], [], [], [], []
    want_stats = np.zeros(4, np.int64)
    for tag, n in (("s", T - below), ("u", T)):
        entries, texts, arrays = mixed_dictionary(n, tag, with_bracket=tag == "s")
        base, ns = len(dictionary), len(texts)
        dictionary += entries
        str_codes += range(base, base + ns)
        arr_codes += range(base + ns, base + n)
        str_hit += [any(lu.like4(t, p) is True for p in MIXED_PATTERNS) for t in texts]
        arr_hit += [any(cu.coll_mirror(m, c, a) is True for m, c in MIXED_PREDS) for a in arrays]
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
        want_stats += mixed_counts(entries, on_device=n >= T)
        ls, cs = op.like_stats(), op.coll_stats()
        assert (ls["device_strings"], ls["host_strings"], cs["device_arrays"], cs["host_arrays"]) == tuple(want_stats), (tag, ls, cs, want_stats)
        assert ls["patterns"] == 2 and cs["predicates"] == 2
        op.reopen()  # (keeps the table)
    assert want_stats[0] > 0 and want_stats[2] > 0 and want_stats[1] >= 3 and want_stats[3] >= 2
    op.done()


def test_having_any_over_an_array_valued_group_key():
    rng = np.random.default_rng(9)
    t = make_table(rng, 4000)
    keys, aggs = [D("a")], ["count(*)"]
    ora = n1o.run(t, None, keys, aggs)
    mode, cond = cu.ANY, ("or", [("cmp", "=", [], "t_1", False), ("cmp", "<", ["f"], 3, False)])
    term = cu.term_text(mode, cond, over=D("a"))

    def val(k):
        if k[0] == n1o.T_MISSING:
            return cu.MISSING
        if k[0] == n1o.T_ARRAY:
            return json.loads(k[1].decode())
        return None if k[0] == n1o.T_NULL else 0

    for having, keep in [(term, lambda v: v is True), ("(not %s)" % term, lambda v: v is False)]:
        gpu, _ = pu.run_gpu(t, None, keys, aggs, having=having)
        want = sorted((k[0], a[0][1]) for k, a in zip(ora.keys, ora.aggs) if keep(cu.coll_mirror(mode, cond, val(k[0]))))
        got = sorted((k[0], a[0][1]) for k, a in zip(gpu.keys, gpu.aggs))
        assert got == want and len(want) >= 3 and len(want) < len(ora.keys), (having, got, want)
    classes = set(k[0][0] for k in ora.keys)
    assert {n1o.T_NULL, n1o.T_MISSING, n1o.T_STRING, n1o.T_OBJECT, n1o.T_ARRAY} <= classes


def test_eight_predicates_run_and_a_ninth_is_refused():
    """Five collection predicates and three LIKE patterns share the eight bits of a table entry."""
    rng = np.random.default_rng(8)
    t = make_table(rng, 3000)
    sub = Substitution(t)
    conds = [("cmp", "=", [], "t_1", False), ("cmp", "=", [], "a", False), ("is", ["f"], "valued"), ("like", [], "a%"), ("cmp", "=", ["g", "h"], 2, False)]
    parts = [sub.coll("a", [cu.ANY, cu.EVERY, cu.ANY_EVERY][i % 3], c) for i, c in enumerate(conds)]
    parts += [sub.like("s", p) for p in ("a%", "%b", "t\\_%")]
    dcond = "(%s)" % " or ".join(("(not %s)" % p[0]) if i % 4 == 3 else p[0] for i, p in enumerate(parts))
    ocond = "(%s)" % " or ".join(("(not %s)" % p[1]) if i % 4 == 3 else p[1] for i, p in enumerate(parts))
    keys, aggs = [D("k")], ["count(*)"]
    gpu, st = pu.run_gpu(t, dcond, keys, aggs)
    ora = n1o.run(sub.oracle_table(), ocond, keys, aggs)
    pu.assert_same_groups(gpu, ora, aggs=aggs)
    assert st["rows_selected"] == ora.rows_passed and 0 < ora.rows_passed < 3000
    ninth = "(%s or %s)" % (dcond, cu.term_text(cu.ANY, ("cmp", "=", [], "zz", False), over=D("a")))
    with pytest.raises(query_amd.N1kError) as ei:
        query_amd.GpuFilterGroup(plan.filter_group_plan(ninth, keys, aggs))
    assert ei.value.status == _ffi.UNSUPPORTED and "more than 8" in ei.value.message


@pytest.mark.timeout(600)
@pytest.mark.parametrize("jit", [0, 2], ids=["interpreter", "runtime-built"])
def test_collection_term_across_two_ranks_over_the_loopback_transport(jit):
    """World size 2, row exchange: the sender evaluates the Filter — the collection term through its own handle's table — and
    every rank ends with the substituted oracle's groups."""
    from query_amd import distributed as qd
    from query_amd.gpu_operator import GroupRows
    from test_gpu_distributed import _device_cols, _run_ranks
    world, n = 2, 60_011
    rng = np.random.default_rng(41 + jit)
    t = make_table(rng, n)
    sub = Substitution(t)
    d, o = sub.coll("a", cu.ANY, ("cmp", "=", [], "t_1", False))
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
        assert (info["sender_kernel"] != 0) == (jit == 2), info  # scan_spec_partition_body saw the term, or partition_kernel did
    assert sum(info["recv_rows"] for _, info in outs) == ora.rows_passed
