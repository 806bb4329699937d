"""LIKE / NOT LIKE without a GPU: the yardstick itself, the host matcher against it, what n1k_create accepts and refuses,
and the run-time-built kernels of a LIKE plan (compile only, gfx950).

The yardstick is tests/like_util.py's Python restatement of the reference's likeCompile (expression/comp_like.go:124-149);
its truth values below are the ones the reference's rewrite gives, accidents included."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import golden_util as gu
import like_util as lu
import query_amd
from query_amd import _ffi, plan

# (string, pattern, LIKE) — the rules of the rewrite, one by one
TRUTHS = [
    # 1. % any run, _ exactly one CHARACTER (a code point), both match '\n'
    ("Sherlock: Series 1", "Sherlock%", True), ("english", "english", True), ("imported", "english", False),
    ("abc", "a_c", True), ("ac", "a_c", False), ("a\nc", "a_c", True), ("a\n\nc", "a%c", True),
    ("aéc", "a_c", True), ("a\U0001F600c", "a_c", True), ("aéc", "a__c", False), ("é", "_", True), ("", "_", False), ("", "%", True),
    # 2. backslash before % or _ escapes it and is dropped; every other backslash is an ordinary character
    ("50%", "50\\%", True), ("50x", "50\\%", False), ("a_b", "a\\_b", True), ("axb", "a\\_b", False),
    ("a\\\\b", "a\\\\b", True), ("a\\b", "a\\\\b", False), ("\\%", "\\\\%", True), ("\\x", "\\\\%", False), ("%", "\\\\%", False),
    ("a\\b", "a\\b", True), ("a.b", "a.b", True), ("axb", "a.b", False), ("a*(b[^$", "a*(b[^$", True), ("aab", "a*b", False),
    # 3. the empty pattern matches every string
    ("", "", True), ("anything\nat all", "", True),
    # 4. anchored at the start of the string or right after any '\n'
    ("x\nabc\ny", "abc", True), ("x\nab", "a%", True), ("xabc", "abc", False), ("xab", "a%", False), ("x\n", "", True),
    # 5. anchored at the end of the string or right before any '\n' — unless the pattern ends in \% or \_
    ("abc\nxyz", "abc", True), ("abcx", "abc", False), ("abc%xyz", "abc\\%", True), ("abc", "abc\\%", False),
    ("a_z", "a\\_", True), ("xa_z", "a\\_", False), ("ab\nc", "%b", True), ("abc", "%b", False), ("abc", "%b%", True),
    ("a\n", "a", True), ("\na", "a", True), ("a\n", "a_", True),
]


@pytest.mark.parametrize("string,pattern,want", TRUTHS)
def test_the_mirror_gives_the_references_truth_values(string, pattern, want):
    assert lu.like_mirror(string, pattern) is want


def test_the_mirror_gives_the_references_filestore_rows():
    """case_where.json 4, 5, 10 over the catalog documents, evaluated by the mirror alone."""
    docs = [d["doc"] for d in gu.load_docs("catalog")]

    def tag1(d):
        t = d.get("tags")
        return t[1] if isinstance(t, list) and len(t) > 1 else lu.MISSING

    r4 = sorted(d["asin"] for d in docs if d.get("type") == "Movies&TV" and lu.like4(d.get("title", lu.MISSING), "Sherlock%") is True)
    r5 = sorted(d["asin"] for d in docs if d.get("type") == "Movies&TV" and lu.like4(tag1(d), "english") is True)
    r10 = sorted(d["asin"] for d in docs if lu.like4(tag1(d), "english") is False)
    assert (r4, r5, r10) == (["B0094QY3LI"], ["B0094QY3AB", "B0094QY3LI"], ["B0094QY7HE"])


@pytest.mark.parametrize("string,pattern,want", TRUTHS)
def test_host_matcher_on_the_directed_rules(string, pattern, want):
    assert bool(lu.host_match(pattern.encode(), [string.encode()])[0]) is want


def test_host_matcher_equals_the_mirror_on_seeded_pairs():
    pairs = lu.random_pairs(20240607, 24000)
    assert len(pairs) >= 20000
    matched = 0
    for pattern, idx in lu.by_pattern(pairs):
        got = lu.host_match(pattern.encode(), [pairs[i][1].encode() for i in idx])
        for g, i in zip(got, idx):
            want = lu.like_mirror(pairs[i][1], pattern)
            assert bool(g) is want and g in (0, 1), (pattern, pairs[i][1], int(g), want)
            matched += want
    assert 0.15 < matched / len(pairs) < 0.85, matched  # the alphabet makes both answers common


def test_host_matcher_on_strings_that_are_not_valid_utf8():
    """Go decodes every byte that begins no valid encoding as ONE character (U+FFFD); expectations derived by hand."""
    cases = [
        (b"a\xffb", "a_b", 1), (b"a\xffb", "a__b", 0), (b"a\xffb", "a%b", 1), (b"a\xe9b", "a_b", 1),
        (b"\xf0\x9f\x98", "___", 1), (b"\xf0\x9f\x98", "_", 0), (b"\xf0\x9f\x98", "____", 0),  # a 4-byte sequence cut short: 3 characters
        (b"\xc0\xaf", "__", 1), (b"\xc0\xaf", "_", 0),          # an overlong form: two characters
        (b"\xed\xa0\x80", "___", 1),                            # a surrogate: three characters
        (b"a\xff", "a\ufffd", 1),                               # the undecodable byte IS U+FFFD to Go's matcher
        (b"\xff\nabc", "abc", 1), (b"abc\n\xff", "abc", 1), (b"\xffabc", "abc", 0),
        (b"\xc3\xa9\xff", "é_", 1), (b"\xc3\xa9\xff", "é", 0),   # valid characters keep their width beside a bad byte
    ]
    for s, pattern, want in cases:
        assert int(lu.host_match(pattern.encode(), [s])[0]) == want, (s, pattern)


def test_host_matcher_refuses_a_pattern_that_is_not_valid_utf8():
    offs, blob = lu.pack([b"abc"])
    out = np.zeros(1, dtype=np.uint8)
    assert _ffi.lib().n1k_like_match(b"a\xff%", 3, 1, offs.ctypes.data, blob, out.ctypes.data) == _ffi.INVALID


def test_host_matcher_with_long_literals_and_many_strings():
    lit = "ab" * 300  # a literal longer than one program instruction takes
    strings = [lit.encode(), (lit + "x").encode(), ("x\n" + lit + "\ny").encode(), b""]
    assert list(lu.host_match(lit.encode(), strings)) == [1, 0, 1, 0]
    assert list(lu.host_match(("%" + lit + "_").encode(), strings)) == [0, 1, 0, 0]
    assert list(lu.host_match(b"", [])) == []
    # a long literal of two-byte characters (its 255-byte program chunks would cut one in half) against strings that are
    # not valid UTF-8: the matcher over code points sees the same characters, the stray byte as one more
    lit = "aé" * 200
    assert list(lu.host_match(lit.encode(), [lit.encode(), lit.encode() + b"\xff", b"\xff\n" + lit.encode()])) == [1, 0, 1]
    assert list(lu.host_match((lit + "_").encode(), [lit.encode() + b"\xff", lit.encode() + b"\xff\xff"])) == [1, 0]
    assert list(lu.host_match(("é" + lit).encode(), [b"\xc3\xa9" + lit.encode() + b"\n\xfe"])) == [1]


D = lambda name: "(`d`.`%s`)" % name  # noqa: E731


def test_create_accepts_like_inside_and_or_not_trees():
    cond = '((%s like "ab%%") and ((not (%s like "%%z")) or (%s is null) or ((%s + 1) like "x")) and (3 < %s))' % (
        D("s"), D("t"), D("t"), D("n"), D("n"))
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [D("k")], ["count(*)"]))
    assert op.column_paths == [D("s"), D("t"), D("n"), D("k")]
    assert op.like_stats()["patterns"] == 3 and op.like_stats()["device_strings"] == 0
    op.done()
    # the same pattern twice is one entry of the table; a constant on the left is an operand like any other
    cond = '((%s like "a_") or (%s like "a_") or ("ab" like "a_"))' % (D("s"), D("t"))
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], [], filter_only=True))
    assert op.column_paths == [D("s"), D("t")] and op.like_stats()["patterns"] == 1
    op.done()


@pytest.mark.parametrize("raw,word", [
    (('{"#operator":"Filter","condition":"(%s like %s)"}' % (D("s"), D("p"))).encode(), "constant"),
    (b'{"#operator":"Filter","condition":"((`d`.`s`) like \\"a\xff%\\")"}', "UTF-8"),
    (('{"#operator":"Filter","condition":"(%s)"}' % " or ".join('(%s like \\"p%d%%\\")' % (D("s"), i) for i in range(9))).encode(), "patterns"),
    (('{"#operator":"Filter","condition":"(%s like 5)"}' % D("s")).encode(), "constant"),
])
def test_create_refuses_what_the_table_cannot_hold(raw, word):
    with pytest.raises(query_amd.N1kError) as ei:
        query_amd.GpuFilterGroup(raw)
    assert ei.value.status == _ffi.UNSUPPORTED and word in ei.value.message, ei.value.message


def test_eight_patterns_fit():
    cond = "(%s)" % " or ".join('(%s like "p%d%%")' % (D("s"), i) for i in range(8))
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], [], filter_only=True))
    assert op.like_stats()["patterns"] == 8
    op.done()


def test_the_explain_subtrees_that_stopped_at_like():
    with open(os.path.join(gu.GOLDEN, "plans.json")) as fh:
        plans = json.load(fh)
    assert " like " in plans[63]["plan"]["condition"] and plans[63]["kind"] == "Filter"
    op = query_amd.GpuFilterGroup(json.dumps(plans[63]["plan"]))
    assert op.column_paths == ["cover ((`shellTest`.`email`))", "((cover ((`shellTest`.`VMs`))[0]).`RAM`)",
                               "cover ((10 < (`shellTest`.`join_day`)))"]
    op.done()
    with pytest.raises(query_amd.N1kError) as ei:  # the Parallel subtree: its un-grouped InitialProject stays outside
        query_amd.GpuFilterGroup(json.dumps(plans[62]["plan"]))
    assert ei.value.status == _ffi.UNSUPPORTED and ei.value.message
    assert "like" not in ei.value.message.lower() and "InitialProject" in ei.value.message


@pytest.mark.parametrize("kind", ["DICT32", "TAGGED64"])
def test_two_term_like_plan_compiles_for_gfx950_without_a_gpu(kind):
    """scan_spec_kernel / scan_spec_records_kernel / scan_spec_partition_body with a LIKE term, through hiprtc."""
    pj = plan.filter_group_plan('((%s like "ab%%") and (5 < %s))' % (D("s"), D("x")), [D("k")], ["sum(%s)" % D("x")])
    op = query_amd.GpuFilterGroup(pj)
    assert op.column_paths == [D("s"), D("x"), D("k")]
    skind = _ffi.COL_DICT32 if kind == "DICT32" else _ffi.COL_TAGGED64
    kinds = np.array([skind, _ffi.COL_TAGGED64, _ffi.COL_DICT32], dtype=np.uint32)
    log = C.create_string_buffer(8192)
    st = _ffi.lib().n1k_jit_check(op._h, kinds.ctypes.data, 3, log, 8192)
    assert st == _ffi.OK, log.value.decode(errors="replace")
    op.done()


def test_golden_like_fixture_holds_the_references_three_statements():
    with open(os.path.join(gu.GOLDEN, "cases_like.json")) as fh:
        fx = json.load(fh)
    assert [c["index"] for c in fx["cases"]] == [4, 5, 10] and all(c["keyspace"] == "catalog" for c in fx["cases"])
    for c in fx["cases"]:  # each condition is a plan the library takes, over the leaf paths the harness extracts
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(c["plan"]["condition"], [], [], filter_only=True))
        assert op.column_paths == gu.leaf_paths(c["plan"])
        op.done()


def test_the_bounded_family_takes_the_gpu_differentials_bounded_plans():
    """tests/test_gpu_like.py runs its bounded plans with `spec` off and reads stats["spec_kernel"] == 0, which the
    interpreter reports too.  What tells them apart is decided on the host: n1k_jit_check answers N1K_UNSUPPORTED unless
    build_fast_args takes the plan — here every distinct bounded shape those seeds draw, LIKE term included."""
    import test_gpu_like as tg
    seen = set()
    for seed in range(240):
        opts, bounded, _ = tg.FAMILIES[seed % len(tg.FAMILIES)]
        if not bounded or opts != {"spec": 0}:
            continue
        rng = np.random.default_rng(515_000 + seed)
        t = tg.make_table(rng, int(rng.integers(1, 5000)))
        _, dcond, _, keys, aggs = tg.rand_like_plan(rng, t, True)
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(dcond, keys, aggs))
        by_name = {c.name: c for c in t.columns}
        kinds = np.array([by_name[p].kind for p in op.column_paths], dtype=np.uint32)
        shape = (tuple(kinds.tolist()), tuple(op.column_paths), dcond.split(" like ")[0].count("("), " and " in dcond, tuple(aggs))
        if shape not in seen and len(seen) < 12:
            seen.add(shape)
            log = C.create_string_buffer(4096)
            st = _ffi.lib().n1k_jit_check(op._h, kinds.ctypes.data, len(kinds), log, 4096)
            assert st == _ffi.OK, (st, dcond, keys, aggs, log.value.decode(errors="replace"))
        op.done()
    assert len(seen) >= 6
