"""The yardstick of tests/test_gpu_topk.py without a GPU: collate_exact is a strict weak order with exactly the documented
ties, the image helpers invert each other, and every GPU case — on the reference alone — puts its keep-th row where the
case says it does, with 0 < keep < n, so that no GPU case can pass vacuously.  Every plan the GPU cases draw is accepted."""
import itertools

import numpy as np
import pytest

import parity_util as pu
import query_amd
import topk_util as tk
from oracle import n1o
from query_amd import plan

VALUES = list(tk.POOL.items())
CASES = tk.exact_cases() + [tk.digit_case(p, b, d) for p in range(8) for b in tk.DIGIT_BYTES for d in (False, True)] \
    + tk.sampled_cases() + tk.lean_cases()


def test_collate_exact_is_a_strict_weak_order_over_the_pool():
    vals = [v for _, v in VALUES] + [tk.MISSING, tk.F(float("nan"))]
    c = [[tk.collate_exact(a, b) for b in vals] for a in vals]
    n = len(vals)
    for i, j in itertools.product(range(n), repeat=2):
        assert c[i][j] == -c[j][i], (vals[i], vals[j])
    for i in range(n):
        assert c[i][i] == 0
    # transitivity of "<" and of "ties" (with antisymmetry: a strict weak order), over all triples
    for i, j, k in itertools.product(range(n), repeat=3):
        if c[i][j] <= 0 and c[j][k] <= 0:
            assert c[i][k] <= 0, (vals[i], vals[j], vals[k])
            if c[i][j] == 0 and c[j][k] == 0:
                assert c[i][k] == 0
            else:
                assert c[i][k] < 0, (vals[i], vals[j], vals[k])


def test_collate_exact_ties_the_documented_classes_and_nothing_else():
    cls = {n: i for i, s in enumerate(tk.TIE_CLASSES) for n in s}
    for (na, a), (nb, b) in itertools.combinations(VALUES, 2):
        tied = tk.collate_exact(a, b) == 0
        assert tied == (na in cls and nb in cls and cls[na] == cls[nb]), (na, nb)
    nan2 = tk.F(np.float64(np.uint64(0xFFF8000000000001).view(np.float64)))  # another NaN
    assert tk.collate_exact(tk.POOL["NaN"], nan2) == 0 and tk.collate_exact(nan2, tk.POOL["-inf"]) < 0
    assert tk.collate_exact(tk.I(2 ** 53 + 1), tk.F(2.0 ** 53)) > 0 and tk.collate_exact(tk.I(2 ** 63 - 1), tk.F(2.0 ** 63)) < 0
    assert tk.collate_exact(tk.S(b"a"), tk.S(b"a\x00")) < 0 and tk.collate_exact(tk.S(b"\x7f"), tk.S(b"\x80")) < 0
    assert tk.collate_exact(tk.MISSING, tk.NULL) < 0 and tk.collate_exact(tk.NULL, tk.FALSE) < 0 and tk.collate_exact(tk.TRUE, tk.POOL["NaN"]) < 0


def test_the_pool_is_in_the_order_the_issue_lists_it():
    """Type classes in order, and inside the numbers the list of the float line as written."""
    line = ["NaN", "-inf", "-max", "-2.5", "-5e-324", "-0.0", "0.0", "int0", "5e-324", "2.5", "max", "+inf"]
    for a, b in zip(line, line[1:]):
        assert tk.collate_exact(tk.POOL[a], tk.POOL[b]) <= 0, (a, b)
    ints = ["int-2^63", "int-2^53-1", "int-2^53", "flt-2^53", "int2^53", "flt2^53", "int2^53+1", "int2^53+2", "int2^63-1", "flt2^63"]
    for a, b in zip(ints, ints[1:]):
        assert tk.collate_exact(tk.POOL[a], tk.POOL[b]) <= 0, (a, b)
    strs = [tk.S(s) for s in tk.STRINGS]
    for a, b in zip(strs, strs[1:]):
        assert tk.collate_exact(a, b) < 0, (a, b)


def test_doubles_for_images_round_trips_and_keeps_the_order():
    rng = np.random.default_rng(11)
    # bodies of the non-NaN doubles: sortable forms from ~(-inf's bits) to +inf's, shifted
    lo, hi = (0x000FFFFFFFFFFFFF >> 3) + 1, 0xFFF0000000000000 >> 3
    bodies = np.unique(np.concatenate([rng.integers(lo, hi, 20000, dtype=np.uint64), np.array([lo, hi, 1 << 60, (1 << 60) - 1], dtype=np.uint64)]))
    d = tk.doubles_for_images(bodies)
    assert np.array_equal(tk.image_bodies(d), bodies)
    assert np.all(np.diff(d) > 0)  # ascending bodies are ascending doubles
    assert tk.image_bodies([float("nan")])[0] == 0
    ones = tk.image_bodies(tk.neighbours_of_one())
    assert len(set(ones.tolist())) == 1, "the eight neighbours of 1.0 share an image"
    # the raw sortable forms of the two zeros are neighbours, not one: why the image gives a zero one sign (image_key does)
    assert tk.image_bodies([-0.0])[0] + 1 == tk.image_bodies([0.0])[0]
    assert tk.image_key(tk.F(-0.0)) == tk.image_key(tk.F(0.0)) == tk.image_key(tk.I(0))
    assert tk.image_bodies([5e-324])[0] == tk.image_bodies([0.0])[0] and tk.image_bodies([float(2 ** 53 + 2)])[0] == tk.image_bodies([2.0 ** 53])[0]


def test_the_image_is_monotone_in_the_collation_and_equal_on_its_ties():
    vals = [v for _, v in VALUES]
    for a, b in itertools.permutations(vals, 2):
        if tk.collate_exact(a, b) < 0:
            assert tk.image_key(a) <= tk.image_key(b), (a, b)
        if tk.collate_exact(a, b) == 0:
            assert tk.image_key(a) == tk.image_key(b), (a, b)  # equal on ties: the later terms order those


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_gpu_case_puts_keep_where_it_says(case):
    e = case.expected()
    n = case.n
    terms = [tk.first_term(v, case.form) for v in case.pool]
    ranks = tk.dense_ranks(terms)
    assert sorted(set(case.idx.tolist())) == list(range(len(case.pool))), "every pool value is drawn"
    if case.injective:
        keys = {}
        for t, r in zip(terms, ranks):
            assert keys.setdefault(tk.image_key(t), r) == r, "two tie classes share an image"
    if case.claim is None:
        assert e.keep == 0 or e.keep >= n
        assert len(e.ks) == max(0, min(n, e.keep) - case.offset) and e.c_exact in (0, n)
        return
    assert 0 < e.keep < n and len(e.ks) == case.limit and 0 < e.c_exact <= n
    where, name = case.claim
    row = e.order[e.keep - 1]
    if where != "any":
        want = ranks[case.names.index(name)]
        assert e.ranks[row] == want, "the keep-th row is not in %s's tie class" % name
        before = e.keep >= 2 and e.ranks[e.order[e.keep - 2]] == want
        after = e.ranks[e.order[e.keep]] == want
        assert {"first": not before, "last": not after, "inside": before and after}[where], (where, before, after)
    # the expected rows are sorted under collate_exact itself, term by term, with no two rows equal
    rows = [(terms[case.idx[k]], k) for k in e.ks[:300]]
    for (ta, ka), (tb, kb) in zip(rows, rows[1:]):
        c = tk.collate_exact(ta, tb)
        c = -c if case.desc else c
        assert c < 0 or (c == 0 and (ka > kb if case.kdesc else ka < kb))
    # C_exact from its definition
    t = terms[case.idx[row]]
    cnt = np.array([(-1 if case.desc else 1) * tk.collate_exact(v, t) <= 0 for v in terms])[case.idx].sum()
    assert e.c_exact == int(cnt) and e.keep <= e.c_exact


@pytest.mark.parametrize("pas", range(8))
@pytest.mark.parametrize("byte", tk.DIGIT_BYTES, ids=["%02x" % b for b in tk.DIGIT_BYTES])
def test_digit_cases_put_the_threshold_on_the_chosen_bin(pas, byte):
    """The keep-th image's byte in pass `pas` is the chosen one (pass 0: its five free bits), and the images that share its
    higher bytes lie on both sides of that bin."""
    bodies, target = tk.digit_bodies(pas, byte)
    assert len(set(bodies.tolist())) == tk.N_DIGIT
    img = lambda b: (3 << 61) | int(b)  # noqa: E731  (a number's class in the top three bits)
    shift = 56 - 8 * pas
    want = 0x60 | (byte & 0x1F) if pas == 0 else byte
    assert (img(target) >> shift) & 255 == want
    peers = [(img(b) >> shift) & 255 for b in bodies if pas == 0 or img(b) >> (shift + 8) == img(target) >> (shift + 8)]
    lo_end, hi_end = (0x60, 0x7F) if pas == 0 else (0x00, 0xFF)
    assert (want == lo_end or min(peers) < want) and (want == hi_end or max(peers) > want) and len(set(peers)) == (32 if pas == 0 else 256)
    others = [b for b in bodies if pas and img(b) >> (shift + 8) != img(target) >> (shift + 8)]
    assert pas == 0 or (min(others) < target < max(others))
    for desc in (False, True):
        c = tk.digit_case(pas, byte, desc)
        e = c.expected()
        assert c.pool[int(c.idx[e.order[e.keep - 1]])] == tk.F(tk.doubles_for_images([target])[0])
        assert e.c_exact == e.keep  # distinct images: no ties


def test_the_sample_paths_size_bounds():
    assert not tk.can_sample(65535, 100) and tk.can_sample(65536, 100) and tk.can_sample(81919, 100)
    assert 81919 // tk.K_TOPK_SAMPLE == 4 and 81920 // tk.K_TOPK_SAMPLE == 5 and 81919 - 4 * tk.K_TOPK_SAMPLE == 16383
    lo, hi = tk.sample_bound_keeps(65536)
    assert (lo, hi) == (8161, 8162) and tk.can_sample(65536, lo) and not tk.can_sample(65536, hi)
    assert tk.can_sample(70000, 8001)
    flood = [c for c in tk.sampled_cases() if c.id.startswith("Sflood")]
    assert len(flood) == 2 and all(int((c.idx == 0).sum()) == 8000 and c.n == 70000 for c in flood)
    sizes = sorted({c.n for c in tk.sampled_cases()})
    assert sizes == [65535, 65536, 65537, 70000, 81919]


def test_every_plan_of_the_gpu_cases_is_accepted():
    """N1K_UNSUPPORTED on any of these plans would be a failure of the GPU test: found here, without a GPU."""
    seen = set()
    for c in CASES:
        keys, aggs, order, _, _ = tk.query(c.form, c.agg, c.desc, c.kdesc)
        opts = dict(c.options)
        for extra in ({"topk_sample": 0}, {"topk_sample": 1}, {"lean_topk": 0}, {"lean_topk": 1}):
            sig = (tuple(keys), tuple(aggs), tuple(order), c.offset, c.limit, tuple(sorted({**opts, **extra}.items())))
            if sig in seen:
                continue
            seen.add(sig)
            op = query_amd.GpuFilterGroup(plan.filter_group_plan(None, keys, aggs, order=order, limit=c.limit, offset=c.offset), **{**opts, **extra})
            assert len(op.column_paths) == 2
            op.done()
    assert len(seen) > 50


def test_the_builders_tables_mean_what_the_reference_says():
    """The oracle's MIN / MAX of every one-row group (its key, for the key form) is the first term the reference ranks."""
    seen = set()
    for c in tk.exact_cases() + [tk.digit_case(3, 0xFC, False)]:
        if c.table in seen:
            continue
        seen.add(c.table)
        t = tk.build_table(c.pool, c.idx, c.form)
        assert t.nrows == c.n and sorted(t.columns[0].payload.view(np.int64).tolist()) == list(range(c.n))
        keys, aggs, _, kpos, tpos = tk.query(c.form, "min", False, False)
        aggs = aggs if c.form == "key" else sorted(aggs + ["max(%s)" % tk.D("v")])
        ora = n1o.run(t, None, keys, aggs)
        assert len(ora.keys) == c.n
        for key, agg in zip(ora.keys, ora.aggs):
            term = tk.first_term(c.pool[int(c.idx[key[kpos][1]])], c.form)
            if c.form == "key":
                assert pu._canon_key(key[:1]) == pu._canon_key((term,)), (key, term)
            else:
                assert all(tk.vkey(a) == tk.vkey(term) for n_, a in zip(aggs, agg) if n_ != "count(*)"), (key, agg, term)
    assert len(seen) >= 8


def test_parity_utils_collation_agrees_with_the_reference_nan_rule_included():
    """pu.collate_values (what assert_ordered_groups sorts with) has the NaN rule: NaN first among numbers, NaN ties NaN."""
    vals = [v for _, v in VALUES] + [tk.MISSING, tk.F(float("nan"))]
    for a, b in itertools.product(vals, repeat=2):
        assert pu.collate_values(a, b) == tk.collate_exact(a, b), (a, b)
