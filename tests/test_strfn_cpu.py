"""String functions in Filter and HAVING without a GPU: what n1k_create accepts and refuses, the host evaluator against the
mirror (tests/strfn_util.py), the soundness of the substitution the GPU differential uses, and the run-time-built kernels of
a plan with a string-function term (compile only, gfx950)."""
import ctypes as C

import numpy as np
import pytest

import query_amd
import strfn_util as su
from query_amd import _ffi, plan

D = lambda name: "(`d`.`%s`)" % name  # noqa: E731


def accepted(cond, keys=(), aggs=("count(*)",)):
    return query_amd.GpuFilterGroup(plan.filter_group_plan(cond, list(keys), list(aggs)))


# ------------------------------------------------------------------ create

ACCEPTED = [
    'contains(%s, "amazon")' % D("s"),
    'contains(lower(%s), "amazon")' % D("s"),
    '(lower(%s) like "%%phone%%")' % D("s"),
    '(upper(%s) = "DE")' % D("s"),
    '(trim(%s) = "cat_1")' % D("s"),
    '(trim(%s, "xy") = "cat_1")' % D("s"),
    '(ltrim(%s) < "m")' % D("s"),
    '(rtrim(%s, " ") <= "m")' % D("s"),
    '("a" < lower(%s))' % D("s"),
    '("a" <= upper(%s))' % D("s"),
    '("ab" = lower(trim(%s)))' % D("s"),
    '(lower(%s) between "a" and "b")' % D("s"),
    '(trim(upper(ltrim(rtrim(%s, "x"), "y"))) like "A_")' % D("s"),
    '(trim(%s) like "ab%%")' % D("s"),
    '(trim(%s, "e") like "é%%")' % D("s"),              # an ASCII cutset, a pattern of any valid UTF-8 without a case step
    '(position(%s, "c") < 3)' % D("s"),
    '(pos(%s, "c") = 0)' % D("s"),
    '(position0(%s, "c") <= 2.5)' % D("s"),
    '(pos0(%s, "") = 0)' % D("s"),
    '(position1(%s, "c") between 1 and 4)' % D("s"),
    '(2 < pos1(%s, "c"))' % D("s"),
    '((-1) = position(%s, "zz"))' % D("s"),
    '(trim(%s) = "é")' % D("s"),                       # no case step: any constant
    'contains(%s, "é")' % D("s"),
    '(lower(cover (%s)) = "x")' % D("s"),
    '(lower(((`d`.`a`).`b`)) = "x")',
]


def _path_of(term):
    for p in ("cover (%s)" % D("s"), "((`d`.`a`).`b`)", D("s")):
        if p in term:
            return p
    raise AssertionError(term)


@pytest.mark.parametrize("term", ACCEPTED)
def test_create_accepts_the_subset_and_reports_its_paths_in_first_use_order(term):
    want = _path_of(term)
    for cond, paths in ((term, [want]), ("(not %s)" % term, [want]), ("((3 < %s) and %s)" % (D("n"), term), [D("n"), want]),
                        ("(%s and (3 < %s))" % (term, D("n")), [want, D("n")]),
                        ("((not %s) or (%s is null) or contains(%s, \"q\"))" % (term, D("n"), D("t")), [want, D("n"), D("t")])):
        op = accepted(cond)
        assert op.column_paths == paths, (cond, op.column_paths)
        assert op.strfn_stats()["predicates"] == 1 + (' contains(%s, "q")' % D("t") in cond) and op.like_stats()["patterns"] == 0
        op.done()
    assert su.host_status(term.encode()) == _ffi.OK


X300 = "x" * 300
REFUSED = [
    ("(length(%s) < 3)" % D("s"), "length"),
    ('(length(lower(%s)) < 3)' % D("s"), "length"),
    ('(lower(length(%s)) = "3")' % D("s"), "length"),
    ('(substr(%s, 1) = "a")' % D("s"), "substr"),
    ('(substr0(%s, 1, 2) = "a")' % D("s"), "substr0"),
    ('(substr1(lower(%s), 1) = "a")' % D("s"), "substr1"),
    ('(replace(%s, "a", "b") = "b")' % D("s"), "replace"),
    ('(repeat(%s, 2) = "aa")' % D("s"), "repeat"),
    ('(reverse(%s) = "a")' % D("s"), "reverse"),
    ('(title(%s) = "A")' % D("s"), "title"),
    ('(split(%s) = "A")' % D("s"), "split"),
    ('(suffixes(%s) = "A")' % D("s"), "suffixes"),
    ('regexp_contains(%s, "a")' % D("s"), "regexp_contains"),
    ('regexp_like(lower(%s), "a")' % D("s"), "regexp_like"),
    ('(trim(%s, %s) = "a")' % (D("s"), D("t")), "not a STRING constant"),
    ('(trim(%s, 5) = "a")' % D("s"), "not a STRING constant"),
    ('contains(%s, %s)' % (D("s"), D("t")), "not a STRING constant"),
    ('contains(%s, 5)' % D("s"), "not a STRING constant"),
    ('(position(%s, %s) = 1)' % (D("s"), D("t")), "not a STRING constant"),
    ('(lower(%s) = 5)' % D("s"), "not a STRING"),
    ('(lower(%s) = null)' % D("s"), "not a STRING"),
    ('(lower(%s) = missing)' % D("s"), "not a STRING"),
    ('(lower(%s) = true)' % D("s"), "not a STRING"),
    ('(lower(%s) between "a" and 5)' % D("s"), "not a STRING"),
    ('(position(%s, "a") < "a")' % D("s"), "not a NUMBER"),
    ('(position(%s, "a") = null)' % D("s"), "not a NUMBER"),
    ('(position1(%s, "a") between 1 and true)' % D("s"), "not a NUMBER"),
    ('(lower(%s) = %s)' % (D("s"), D("t")), "anything but a constant"),
    ('(lower(%s) = upper(%s))' % (D("s"), D("t")), "anything but a constant"),
    ('(lower(%s) like %s)' % (D("s"), D("t")), "not a STRING constant"),
    ('(lower((%s + 1)) = "a")' % D("n"), "leaf path"),
    ('(lower("ABC") = "abc")', "leaf path"),
    ('contains((%s + 1), "a")' % D("n"), "leaf path"),
    ('(position((%s + 1), "a") = 0)' % D("n"), "leaf path"),
    ('(lower(contains(%s, "a")) = "a")' % D("s"), "contains"),
    ('(lower(upper(lower(upper(lower(%s))))) = "a")' % D("s"), "more than 4"),
    ('(lower(%s) = "%s")' % (D("s"), X300), "256 bytes"),
    ('(trim(%s, "%s") = "%s")' % (D("s"), "y" * 200, "x" * 100), "256 bytes"),
    ('(lower(trim(%s, "%s")) like "%s")' % (D("s"), "y" * 100, "x" * 200), "256 bytes"),  # (the pattern's text counts)
    ('(trim(%s) like "%s")' % (D("s"), "a_" * 100), "longer than 240"),
    ('(lower(%s) = "é")' % D("s"), "non-ASCII compare constant"),
    ('contains(upper(%s), "É")' % D("s"), "non-ASCII needle"),
    ('(lower(%s) like "%%é%%")' % D("s"), "non-ASCII LIKE pattern"),
    ('(trim(lower(%s), "é") = "a")' % D("s"), "non-ASCII cutset"),
    ('(position(lower(%s), "a") = 0)' % D("s"), "position over lower / upper"),
    ('(pos1(trim(upper(%s)), "a") = 0)' % D("s"), "pos1 over lower / upper"),
    ('(position(trim(%s), "a") = 0)' % D("s"), "bare path"),
    ('(contains(%s, "a") = true)' % D("s"), "contains"),
    ('lower(%s)' % D("s"), "lower"),
    ('(3 < (position(%s, "a") + 1))' % D("s"), "position"),
]


@pytest.mark.parametrize("term,word", REFUSED, ids=[w.replace(" ", "_").replace("/", "") + str(i) for i, (_, w) in enumerate(REFUSED)])
def test_create_refuses_everything_else_and_names_the_construct(term, word):
    for cond in (term, "(%s and (3 < %s))" % (term, D("n")), "(not %s)" % term):
        with pytest.raises(query_amd.N1kError) as ei:
            accepted(cond)
        assert ei.value.status == _ffi.UNSUPPORTED and word in ei.value.message, (cond, ei.value.message)


def test_group_keys_aggregates_and_projections_over_a_string_function_are_refused():
    for keys, aggs in (["lower(%s)" % D("s")], ["count(*)"]), ([D("s")], ["min(lower(%s))" % D("s")]):
        with pytest.raises(query_amd.N1kError) as ei:
            accepted(None, keys, aggs)
        assert ei.value.status == _ffi.UNSUPPORTED and "lower" in ei.value.message, ei.value.message


def test_the_diagnostic_entry_point_tells_unsupported_from_invalid():
    assert su.host_status(('(lower(%s) = 5)' % D("s")).encode()) == _ffi.UNSUPPORTED
    assert su.host_status(('(length(%s) < 3)' % D("s")).encode()) == _ffi.UNSUPPORTED
    assert su.host_status(b"(3 < 4)") == _ffi.INVALID
    assert su.host_status(('(%s like "a%%")' % D("s")).encode()) == _ffi.INVALID  # the LIKE kind's own term
    assert su.host_status(b"(lower(") == _ffi.INVALID
    assert su.host_status(b'(lower(`s`, `t`) = "a")') == _ffi.INVALID


def test_what_was_refused_before_is_still_refused():
    with pytest.raises(query_amd.N1kError) as ei:
        query_amd.GpuFilterGroup('{"#operator":"Filter","condition":"(length((`a`.`b`)) < 3)"}')
    assert ei.value.status == _ffi.UNSUPPORTED and "length" in ei.value.message
    import coll_util as cu
    for pred, word in (("(5 < length(`v`))", "length"), ('(lower(to_string(`v`)) = "a")', "lower"), ('contains(`v`, "a")', "contains"),
                       ('(lower(`v`) = "a")', "lower"), ('(position(`v`, "a") = 0)', "position")):
        term = "any `v` in %s satisfies %s end" % (D("a"), pred)
        with pytest.raises(query_amd.N1kError) as ei:
            accepted(term)
        assert ei.value.status == _ffi.UNSUPPORTED and word in ei.value.message, ei.value.message
        assert cu.host_status(term.encode()) == _ffi.UNSUPPORTED


def test_the_four_kinds_share_eight_bits_and_equal_terms_share_one():
    strfns = ['(lower(%s) = "c%d")' % (D("s"), i) for i in range(3)]
    likes = ['(%s like "p%d%%")' % (D("s"), i) for i in range(2)]
    ins = ['(%s in ["q%d"])' % (D("s"), i) for i in range(2)]
    anys = ['any `v` in %s satisfies (`v` = "c0") end' % D("a")]
    # a repeated term shares its bit; so do two spellings of one program (the mirrored comparison)
    twice = strfns[:2] + ['("c2" = lower(%s))' % D("s"), '(lower(%s) = "c0")' % D("t")]
    op = accepted("(%s)" % " or ".join(strfns + likes + ins + anys + twice))
    assert op.strfn_stats()["predicates"] == 3 and op.like_stats()["patterns"] == 2 and op.coll_stats()["predicates"] == 1
    assert op.in_stats()["lists"] == 2
    op.done()
    for extra in ('(upper(%s) = "C0")' % D("s"), 'contains(%s, "c0")' % D("s"), '(%s like "q%%")' % D("s"), '(%s in ["zz"])' % D("s"),
                  'any `v` in %s satisfies (`v` = "c9") end' % D("a")):
        for cond in ("(%s)" % " or ".join(strfns + likes + ins + anys + [extra]), "(%s)" % " or ".join([extra] + anys + ins + likes + strfns)):
            with pytest.raises(query_amd.N1kError) as ei:
                accepted(cond)
            assert ei.value.status == _ffi.UNSUPPORTED and "more than 8" in ei.value.message and "string-function" in ei.value.message, ei.value.message
    op = accepted("(%s)" % " or ".join('(lower(%s) = "c%d")' % (D("s"), i) for i in range(8)))
    assert op.strfn_stats()["predicates"] == 8
    op.done()


def test_having_takes_the_term_over_a_group_key():
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(None, [D("k")], ["count(*)"], having='(lower(%s) like "cat\\\\_1%%")' % D("k")))
    assert op.column_paths == [D("k")]
    op.done()


# ------------------------------------------------------------------ the host evaluator against the mirror

def test_host_evaluator_equals_the_mirror_on_seeded_pairs():
    pairs = su.random_pairs(20261018)
    npairs = four = invalid = hits = 0
    chains = set()
    for term, strings in pairs:
        text = su.term_text(D("s"), term)
        got = su.host_eval(text, strings)
        chains.add(tuple(s[0] for s in term[0]))
        for g, s in zip(got, strings):
            want = su.strfn_mirror(s, term)
            assert bool(g) is want and g in (0, 1), (text, s, int(g), want)
            hits += want
            four += any(r.encode() in s for r in su.FOUR)
            invalid += not su.valid_utf8(s)
        npairs += len(strings)
    assert npairs >= 3000 and four >= 100 and invalid >= 100, (npairs, four, invalid)
    assert set(su.all_chains()) <= chains and len(set(su.all_chains())) == 155
    assert 0.15 < hits / npairs < 0.85, hits  # the alphabet makes both answers common


DIRECTED = [
    # (term text over `s`, string, TRUE?)
    ('(lower(%s) = "i")', "İ".encode(), 1), ('(upper(%s) = "I")', "İ".encode(), 0), ('(lower(%s) = "k")', "K".encode(), 1),
    ('(upper(%s) = "S")', "ſ".encode(), 1), ('(lower(%s) = "s")', "ſ".encode(), 0), ('(upper(%s) = "I")', "ı".encode(), 1),
    ('(upper(lower(%s)) = "K")', "K".encode(), 1), ('(lower(upper(%s)) = "s")', "ſ".encode(), 1),
    ('(lower(%s) like "_")', "İ".encode(), 1), ('(lower(%s) like "i_")', "İ".encode() + b"\xff", 1),
    ('(trim(lower(%s), "i") = "")', "İiI".encode(), 1), ('contains(lower(%s), "kk")', "KK".encode(), 1),
    ('(lower(%s) = "ab")', b"AB", 1), ('(lower(%s) = "ab")', b"aB ", 0), ('(lower(%s) < "b")', b"A\xff", 1), ('(lower(%s) < "a")', b"\xff", 0),
    ('(lower(%s) like "a_")', b"A\xff", 1), ('(lower(%s) like "a_")', b"A\xc3", 1), ('(lower(%s) like "a__")', b"A\xe2\x84", 1),
    ('(trim(%s) = "")', b" \t\n\f\r", 1), ('(trim(%s) = "")', b" \x0b ", 0), ('(trim(%s, "") = " a ")', b" a ", 1),
    ('(ltrim(%s, "ab") = "c ab")', b"abbac ab", 1), ('(rtrim(%s, "ab") = "ab c")', b"ab cabba", 1),
    ('(position0(%s, "b") = 1)', b"abab", 1), ('(position1(%s, "b") = 2)', b"abab", 1), ('(position0(%s, "z") = (-1))', b"abab", 1),
    ('(position1(%s, "z") = 0)', b"abab", 1), ('(position(%s, "") = 0)', b"abab", 1), ('(pos1(%s, "") = 1)', b"", 1),
    ('(position(%s, "b") = 2)', "éb".encode(), 1),      # a byte offset, as strings.Index gives it
    ('(1.5 < position(%s, "b"))', "éb".encode(), 1), ('(position(%s, "b") between 2 and 2)', "éb".encode(), 1),
    ('contains(%s, "")', b"", 1), ('contains(%s, "a")', b"", 0), ('(trim(%s) like "")', b"  ", 1), ('(trim(%s) like "a%%")', b" x\nab ", 1),
    ('(lower(%s) between "a" and "ab")', b"AB", 1), ('(lower(%s) between "a" and "ab")', b"ABA", 0),
]


@pytest.mark.parametrize("text,string,want", DIRECTED)
def test_host_evaluator_on_directed_cases(text, string, want):
    assert int(su.host_eval(text % D("s"), [string])[0]) == want


def test_host_evaluator_on_strings_of_every_length():
    rng = np.random.default_rng(4)
    strings = [bytes(rng.choice(np.frombuffer(b"abAB \n", np.uint8), n)) for n in range(0, 301)]
    for term in (([("lower", None), ("trim", None)], ("like", "%ab%a")), ([("upper", None)], ("contains", "ABBA")), ([], ("pos", "pos", "bb", "<", 100, False))):
        got = su.host_eval(su.term_text(D("s"), term), strings)
        want = [su.strfn_mirror(s, term) for s in strings]
        assert [bool(g) for g in got] == want and 0 < sum(want) < len(want)


# ------------------------------------------------------------------ the substitution

def test_the_substitution_is_sound_through_the_oracle():
    """A term, its NOT and (NOT term) OR IS NULL through the oracle's helper column give the rows the mirror gives."""
    from oracle import n1o
    rng = np.random.default_rng(5)
    t = su.make_table(rng, 3000)
    term = ([("lower", None), ("trim", None)], ("like", "%ab%"))
    sub = su.Substitution(t)
    _, h = sub.strfn("m", term)
    vals = [su.strfn4(v if (v is su.MISSING or isinstance(v, str)) else (None if v is None else 0), term) for v in su.column_values(t, "m")]
    assert {True, False, None, su.MISSING} == set(vals)
    ot = sub.oracle_table()
    for cond, keep in [(h, lambda r: r is True), ("(not %s)" % h, lambda r: r is False),
                       ("((not %s) or (%s is null))" % (h, h), lambda r: r is False or r is None)]:
        got = n1o.run(ot, cond, [], [], has_group=False).selected
        assert sorted(got.tolist()) == [i for i, r in enumerate(vals) if keep(r)], cond


# ------------------------------------------------------------------ plan building

def test_the_seeds_draw_every_accepted_form_and_every_kind():
    forms, kinds = set(), set()
    for seed in range(su.SEEDS):
        _, _, (_, dcond, _, _, _), _ = su.draw_plan(seed)
        for i, term in enumerate(su.PLAN_TERMS):
            if su.term_text(su.D("s"), term) in dcond or su.term_text(su.D("m"), term) in dcond:
                forms.add(i)
        kinds |= {k for k, mark in (("like", "`) like "), ("in", " in ["), ("any", "any `v`")) if mark in dcond}
    assert forms == set(range(len(su.PLAN_TERMS))) and kinds == {"like", "in", "any"}, (forms, kinds)


@pytest.mark.parametrize("kind", ["DICT32", "TAGGED64"])
def test_two_term_strfn_plan_compiles_for_gfx950_without_a_gpu(kind):
    """scan_spec_kernel / scan_spec_records_kernel / scan_spec_partition_body with a string-function term, through hiprtc."""
    pj = plan.filter_group_plan('((lower(%s) = "ab") and (5 < %s))' % (D("s"), D("x")), [D("k")], ["sum(%s)" % D("x")])
    op = query_amd.GpuFilterGroup(pj)
    assert op.column_paths == [D("s"), D("x"), D("k")]
    skind = _ffi.COL_DICT32 if kind == "DICT32" else _ffi.COL_TAGGED64
    kinds = np.array([skind, _ffi.COL_TAGGED64, _ffi.COL_DICT32], dtype=np.uint32)
    log = C.create_string_buffer(8192)
    st = _ffi.lib().n1k_jit_check(op._h, kinds.ctypes.data, 3, log, 8192)
    assert st == _ffi.OK, log.value.decode(errors="replace")
    op.done()


def test_the_bounded_family_takes_the_gpu_differentials_bounded_plans():
    """tests/test_gpu_strfn.py runs its bounded plans with `spec` off and reads stats["spec_kernel"] == 0, which the
    interpreter reports too.  What tells them apart is decided on the host: n1k_jit_check answers N1K_UNSUPPORTED unless
    build_fast_args takes the plan — here the first six distinct bounded shapes those seeds draw, string-function term
    included (column kinds, paths in order, aggregates, which side of the AND the term is on)."""
    seen = set()
    asked = 0
    for seed in range(su.SEEDS):
        opts, bounded, _ = su.FAMILIES[seed % len(su.FAMILIES)]
        if not bounded:
            continue
        t, _, (_, dcond, _, keys, aggs), _ = su.draw_plan(seed)
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(dcond, keys, aggs))
        assert op.strfn_stats()["predicates"] == 1
        by_name = {c.name: c for c in t.columns}
        kinds = np.array([by_name[p].kind for p in op.column_paths], dtype=np.uint32)
        shape = (tuple(kinds.tolist()), tuple(op.column_paths), tuple(aggs), " and " in dcond and dcond.index(" and ") < dcond.index("`s`" if "`s`" in dcond else "`m`"))
        if shape not in seen and len(seen) < 6:
            seen.add(shape)
            log = C.create_string_buffer(4096)
            st = _ffi.lib().n1k_jit_check(op._h, kinds.ctypes.data, len(kinds), log, 4096)
            assert st == _ffi.OK, (st, dcond, keys, aggs, log.value.decode(errors="replace"))
            asked += 1
        op.done()
    assert asked >= 6
