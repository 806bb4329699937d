"""An independent reference for ORDER BY <term> [DESC], k OFFSET o LIMIT l over one-row groups, and the cases the device
top-k filter (order_image, the radix selects, the sampled threshold, the lean route) is checked with.

Nothing here calls the device path or n1o's ordering.  `collate_exact` restates what host_collate documents (value.Collate
with an int and a float compared exactly); the expected row sequence comes from ranking the distinct first-term values with
it and sorting the groups by (rank, k).  `doubles_for_images` restates only the documented layout of a number's order image:
type class in the top 3 bits, the sortable form of the float64 shifted right by 3 below it.

Values are (tag, python value) pairs as everywhere in the tests: (T_INT, int), (T_FLOAT, float), (T_STRING, bytes), the
others with None.
"""
from __future__ import annotations

import functools
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import n1o
from query_amd import plan as qplan

T_MISSING, T_NULL, T_FALSE, T_TRUE, T_INT, T_FLOAT, T_STRING = (n1o.T_MISSING, n1o.T_NULL, n1o.T_FALSE, n1o.T_TRUE, n1o.T_INT,
                                                                n1o.T_FLOAT, n1o.T_STRING)
MISSING, NULL, FALSE, TRUE = (T_MISSING, None), (T_NULL, None), (T_FALSE, None), (T_TRUE, None)
NAN, INF, FMAX = float("nan"), float("inf"), 1.7976931348623157e308


def I(x):  # noqa: E743
    return (T_INT, int(x))


def F(x):
    return (T_FLOAT, float(x))


def S(b):
    return (T_STRING, bytes(b))


def D(name: str) -> str:
    return qplan.field_path("d", name)


# ------------------------------------------------------------------ the collation

_CLASS = {T_MISSING: 0, T_NULL: 1, T_FALSE: 2, T_TRUE: 2, T_INT: 3, T_FLOAT: 3, T_STRING: 4}


def collate_exact(a, b) -> int:
    """MISSING < NULL < BOOLEAN < NUMBER < STRING; false < true; NaN first among numbers and NaN ties NaN; an INT and a
    FLOAT compared exactly (python's own int / float comparison: 2^53 + 1 > 2.0 ** 53), so -0.0 = 0.0 = INT 0; strings
    bytewise, then by length (python's bytes comparison)."""
    ca, cb = _CLASS[a[0]], _CLASS[b[0]]
    if ca != cb:
        return -1 if ca < cb else 1
    if ca <= 1:
        return 0
    if ca == 2:
        return int(a[0] == T_TRUE) - int(b[0] == T_TRUE)
    x, y = a[1], b[1]
    if ca == 3:
        xn, yn = isinstance(x, float) and x != x, isinstance(y, float) and y != y
        if xn or yn:
            return 0 if (xn and yn) else (-1 if xn else 1)
    return int(x > y) - int(x < y)


def vkey(v):
    """Identity of a value (not its collation class): -0.0 and 0.0 differ, every NaN is one key."""
    if v[0] == T_FLOAT:
        return (T_FLOAT, b"nan" if v[1] != v[1] else struct.pack("<d", v[1]))
    return v


def same_value(g, o) -> bool:
    """Bit-exact equality of two result values, except that -0.0, 0.0 and INT 0 stand for each other (MIN / MAX keep
    the first of values that collate equal)."""
    if _CLASS.get(g[0]) == 3 and _CLASS.get(o[0]) == 3 and g[1] == 0 and o[1] == 0:
        return True
    return vkey(g) == vkey(o)


# ------------------------------------------------------------------ the value pool: the edges of the image

def neighbours_of_one() -> List[float]:
    """Eight consecutive doubles from 1.0 upward: their sortable forms differ only in the three bits the image drops."""
    out, x = [], 1.0
    for _ in range(8):
        out.append(x)
        x = float(np.nextafter(x, 2.0))
    return out


STRINGS = [b"", b"a", b"a\x00", b"ab", b"abcdefgh1", b"abcdefgh2", b"\x7f", b"\x80", b"\xc3\xa9", b"\xff"]

POOL: Dict[str, tuple] = {
    "NULL": NULL, "false": FALSE, "true": TRUE,
    "NaN": F(NAN), "-inf": F(-INF), "-max": F(-FMAX), "-2.5": F(-2.5), "-5e-324": F(-5e-324), "-0.0": F(-0.0), "0.0": F(0.0),
    "int0": I(0), "5e-324": F(5e-324), "2.5": F(2.5), "max": F(FMAX), "+inf": F(INF),
    "int-2^63": I(-2 ** 63), "int-2^53-1": I(-2 ** 53 - 1), "int-2^53": I(-2 ** 53), "flt-2^53": F(-2.0 ** 53),
    "int2^53": I(2 ** 53), "flt2^53": F(2.0 ** 53), "int2^53+1": I(2 ** 53 + 1), "int2^53+2": I(2 ** 53 + 2),
    "int2^63-1": I(2 ** 63 - 1), "flt2^63": F(2.0 ** 63),
}
POOL.update({"1+%dulp" % i: F(x) for i, x in enumerate(neighbours_of_one())})
POOL.update({"str%r" % s: S(s) for s in STRINGS})

# The classes of pool values that collate equal.  An exact comparison ties INT 2^53 with FLOAT 2.0 ** 53 (and their
# negatives) as well: they are the same number.
TIE_CLASSES = [{"-0.0", "0.0", "int0"}, {"int2^53", "flt2^53"}, {"int-2^53", "flt-2^53"}]


# ------------------------------------------------------------------ the number image, from its documented layout

_TOP = np.uint64(0x8000000000000000)


def doubles_for_images(bodies) -> np.ndarray:
    """The doubles whose order image has these 61-bit bodies: body -> sortable = body << 3 -> double (a sortable form with
    its top bit set is a non-negative double's bits with the sign bit set; one without is the complement of a negative's)."""
    s = np.asarray(bodies, dtype=np.uint64) << np.uint64(3)
    bits = np.where((s & _TOP) != 0, s & ~_TOP, ~s)
    d = bits.astype(np.uint64).view(np.float64)
    assert not np.isnan(d).any(), "a body outside the images of the non-NaN doubles"
    return d


def image_bodies(doubles) -> np.ndarray:
    """The inverse: sortable float64 >> 3, NaN -> 0.  This is the raw form, before the tie rule: it still tells -0.0 from
    0.0 (image_key applies the rule)."""
    d = np.asarray(doubles, dtype=np.float64)
    b = d.view(np.uint64)
    s = np.where((b & _TOP) != 0, ~b, b | _TOP)
    s = np.where(np.isnan(d), np.uint64(0), s)
    return s.astype(np.uint64) >> np.uint64(3)


def image_key(v):
    """(class, body) of a value under the documented image — equal on the collation's ties: a zero of either sign has the
    image of +0.0; strings by their bytes (a rank is injective and monotone)."""
    c = _CLASS[v[0]]
    if c == 2:
        return (c, int(v[0] == T_TRUE))
    if c == 3:
        return (c, int(image_bodies([0.0 if v[1] == 0 else float(v[1])])[0]))
    if c == 4:
        return (c, v[1])
    return (c, 0)


# ------------------------------------------------------------------ first terms, expected rows

def first_term(v, form: str):
    """What the first ORDER BY term of a one-row group holds.  'agg': MIN / MAX of the one operand — NULL when it is
    MISSING or NULL.  'key': the group key — an integral float below 2^53 is the INT it prints as (so -0.0 is INT 0)."""
    if form == "agg":
        return NULL if v[0] in (T_MISSING, T_NULL) else v
    if v[0] == T_FLOAT:
        x = v[1]
        assert x == x and abs(x) != INF, "NaN / Inf group keys become strings: not drawn here"
        if x == int(x):
            assert abs(x) < 2.0 ** 53
            return I(int(x))
    return v


def dense_ranks(values: Sequence[tuple]) -> List[int]:
    """Rank of every value among the distinct collation classes of `values` (ties share a rank)."""
    order = sorted(range(len(values)), key=functools.cmp_to_key(lambda i, j: collate_exact(values[i], values[j])))
    ranks, cur = [0] * len(values), -1
    for n, i in enumerate(order):
        if n == 0 or collate_exact(values[order[n - 1]], values[i]) != 0:
            cur += 1
        ranks[i] = cur
    return ranks


@dataclass
class Expected:
    ks: List[int]        # the k sequence of ORDER BY <term> [DESC], k [DESC] OFFSET o LIMIT l
    keep: int            # offset + limit
    c_exact: int         # groups whose first term collates <= (>= under DESC) the keep-th row's; 0 when keep is outside (0, n]
    ranks: np.ndarray    # per group: rank of its first term
    order: np.ndarray    # every group in the expected order


def expected(pool: Sequence[tuple], idx: np.ndarray, form: str, desc: bool, kdesc: bool, offset: int, limit: int) -> Expected:
    pr = np.array(dense_ranks([first_term(v, form) for v in pool]), dtype=np.int64)
    ranks = pr[idx]
    k = np.arange(len(idx), dtype=np.int64)
    order = np.lexsort((-k if kdesc else k, -ranks if desc else ranks))
    keep, n = offset + limit, len(idx)
    c_exact = 0
    if 0 < keep <= n:
        t = ranks[order[keep - 1]]
        c_exact = int(((ranks >= t) if desc else (ranks <= t)).sum())
    return Expected([int(x) for x in order[offset:min(n, keep)]], keep, c_exact, ranks, order)


def keep_at(pool, names, idx, form, desc, name, where) -> int:
    """The 1-based position, in the expected order, of the first / a middle / the last row of `name`'s tie class, or of
    the row one past it."""
    pr = dense_ranks([first_term(v, form) for v in pool])
    ranks = np.sort(np.asarray(pr, dtype=np.int64)[idx])
    if desc:
        ranks = ranks[::-1]
    pos = np.nonzero(ranks == pr[names.index(name)])[0]
    lo, hi = int(pos[0]) + 1, int(pos[-1]) + 1
    return {"first": lo, "inside": (lo + hi) // 2, "last": hi, "past": hi + 1}[where]


# ------------------------------------------------------------------ tables and queries

def build_table(pool: Sequence[tuple], idx: np.ndarray, form: str, seed: int = 0x70F) -> n1o.Table:
    """Column `k`: INT 0 .. n-1 in a seeded shuffled row order (every row its own group); column `v` (`a` for the key form):
    TAGGED64 with pool[idx[k]].  The dictionary holds the pool's strings in a shuffled order, so that a code is no rank."""
    n = len(idx)
    rng = np.random.default_rng(seed)
    rows = rng.permutation(n)
    strings = sorted({v[1] for v in pool if v[0] == T_STRING})
    dictionary = [strings[i] for i in rng.permutation(len(strings))] + [b"~never used"]
    code = {s: i for i, s in enumerate(dictionary)}
    ptag = np.array([v[0] for v in pool], dtype=np.uint8)
    ppay = np.zeros(len(pool), dtype=np.uint64)
    for i, v in enumerate(pool):
        if v[0] == T_INT:
            ppay[i] = np.array([v[1]], dtype=np.int64).view(np.uint64)[0]
        elif v[0] == T_FLOAT:
            ppay[i] = np.array([v[1]], dtype=np.float64).view(np.uint64)[0]
        elif v[0] == T_STRING:
            ppay[i] = code[v[1]]
    of_row = np.asarray(idx)[rows]
    return n1o.Table([n1o.Column(D("k"), n1o.COL_TAGGED64, tags=np.full(n, T_INT, np.uint8), payload=rows.astype(np.int64).view(np.uint64)),
                      n1o.Column(D("a" if form == "key" else "v"), n1o.COL_TAGGED64, tags=ptag[of_row], payload=ppay[of_row])],
                     dictionary)


def query(form: str, agg: str, desc: bool, kdesc: bool):
    """(keys, aggs, order, index of k among the keys, index of the first term among the aggregates or None)."""
    if form == "key":
        return [D("a"), D("k")], ["count(*)"], [(D("a"), desc), (D("k"), kdesc)], 1, None
    term = "%s(%s)" % (agg, D("v"))
    aggs = sorted(["count(*)", term])
    return [D("k")], aggs, [(term, desc), (D("k"), kdesc)], 0, aggs.index(term)


# ------------------------------------------------------------------ the cases

@dataclass
class Case:
    id: str
    names: List[str]
    pool: List[tuple]
    idx: np.ndarray              # per group k: index into pool
    claim: Optional[Tuple[str, str]]  # (where, pool name): where the keep-th row lies — "first" / "inside" / "last" row of that
                                 # value's tie class; None: the filter is not used (keep outside (0, n))
    form: str = "agg"
    agg: str = "min"
    desc: bool = False
    kdesc: bool = False
    offset: int = 0
    limit: int = 1
    injective: bool = False      # distinct tie classes have distinct images: the candidates are exactly C_exact
    options: Dict[str, int] = field(default_factory=dict)
    table: str = ""              # cases with the same string share one table (and one oracle run)

    @property
    def n(self) -> int:
        return len(self.idx)

    @property
    def keep(self) -> int:
        return self.offset + self.limit

    def expected(self) -> Expected:
        return expected(self.pool, self.idx, self.form, self.desc, self.kdesc, self.offset, self.limit)


N_EXACT, REPLICAS = 2560, 64  # 40 pool values x 64 replicas


def _numbers(count: int, sign: int = 1, start: int = 1) -> Tuple[List[str], List[tuple]]:
    """`count` distinct ordinary numbers of one sign, ints and floats in turn, away from every edge of the image."""
    names, vals = [], []
    for i in range(count):
        v = I(sign * (start + i)) if i % 2 == 0 else F(sign * (start + i + 0.5))
        names.append("%s%r" % ("int" if v[0] == T_INT else "flt", v[1]))
        vals.append(v)
    return names, vals


def _named(*names):
    return list(names), [POOL[n] for n in names]


def _join(*parts):
    names, vals = [], []
    for n, v in parts:
        names += n
        vals += v
    assert len(set(names)) == len(names)
    return names, vals


def _replicated(npool: int, n: int) -> np.ndarray:
    return (np.arange(n) % npool).astype(np.int64)  # value of group k = pool[k % npool]: the values interleave in k


def pool_zeros(sign: int):
    """Family A: the three zeros, 5e-324 (the image of 0.0 once its low bits are dropped) and ordinary numbers, all above
    the zeros (sign +1) or all below them (sign -1)."""
    tiny = _named("5e-324") if sign > 0 else _named("-5e-324")
    return _join(_named("-0.0", "0.0", "int0"), tiny, _numbers(36, sign))


def pool_float_line():
    """Family B: NaN, 19 negatives and 20 positives down to the subnormals; no zero, no two values closer than 8 ulp."""
    neg = (["-inf", "-max", "-1e300", "int-2^62", "-2.5e10", "int-2^40", "int-1000", "-123.456", "int-7", "int-3", "-2.5", "int-1",
            "-0.5", "-1e-10", "-1e-300", "-minnormal", "-1e-310", "-5e-324", "-125000.5"],
           [F(-INF), F(-FMAX), F(-1e300), I(-2 ** 62), F(-2.5e10), I(-2 ** 40), I(-1000), F(-123.456), I(-7), I(-3), F(-2.5), I(-1),
            F(-0.5), F(-1e-10), F(-1e-300), F(-2.2250738585072014e-308), F(-1e-310), F(-5e-324), F(-125000.5)])
    pos = (["5e-324", "1e-310", "minnormal", "1e-300", "1e-10", "0.5", "int1", "1.25", "2.5", "int3", "int7", "123.456", "int1000",
            "125000.5", "int2^40", "2.5e10", "int2^62", "1e300", "max", "+inf"],
           [F(5e-324), F(1e-310), F(2.2250738585072014e-308), F(1e-300), F(1e-10), F(0.5), I(1), F(1.25), F(2.5), I(3), I(7),
            F(123.456), I(1000), F(125000.5), I(2 ** 40), F(2.5e10), I(2 ** 62), F(1e300), F(FMAX), F(INF)])
    return _join(_named("NaN"), neg, pos)


def pool_clusters():
    """Family C: ints and floats around 2^53 and at the int64 ends whose images are equal and whose exact order is not."""
    ends = (["flt-2^63", "int-2^63+1"], [F(-2.0 ** 63), I(-2 ** 63 + 1)])
    return _join(_named("int-2^63"), ends, _named("int-2^53-1", "int-2^53", "flt-2^53"), _numbers(14, -1), _numbers(14, 1),
                 _named("int2^53", "flt2^53", "int2^53+1", "int2^53+2", "int2^63-1", "flt2^63"))


def pool_dropped_bits():
    """Family D: the eight neighbours of 1.0 between 16 smaller and 16 larger numbers."""
    return _join(_numbers(16, -1), _named(*["1+%dulp" % i for i in range(8)]), _numbers(16, 1, start=2))


def pool_classes(form: str):
    """Family E: every class in one query.  The key form adds MISSING as a class of its own and leaves out the values a
    group key turns into strings or folds."""
    strings = _named(*["str%r" % s for s in STRINGS])
    if form == "key":
        nums = _join(_named("-2.5", "-5e-324", "5e-324", "2.5"), (["int-7", "int7"], [I(-7), I(7)]), _numbers(20, 1, start=10))
    else:
        nums = _join(_named("NaN", "-inf", "-max", "-2.5", "-5e-324", "5e-324", "2.5", "max", "+inf"), (["int-7", "int7"], [I(-7), I(7)]),
                     _numbers(15, 1, start=10))
    return _join((["MISSING"], [MISSING]), _named("NULL", "false", "true"), nums, strings)


def _case(fam, pool, where, name, *, n=N_EXACT, idx=None, table=None, **kw) -> Case:
    names, vals = pool
    idx = _replicated(len(vals), n) if idx is None else idx
    form, desc = kw.get("form", "agg"), kw.get("desc", False)
    if "limit" not in kw:
        kw["limit"] = keep_at(vals, names, idx, form, desc, name, where) - kw.get("offset", 0)
    if where == "past":  # one past a tie class is the first row of the next: named by the row itself
        e = expected(vals, idx, form, desc, kw.get("kdesc", False), kw.get("offset", 0), kw["limit"])
        where, name = "first", names[int(idx[e.order[e.keep - 1]])]
    kw.setdefault("agg", "max" if desc and form == "agg" else "min")
    cid = "%s-%s-%s-%s%s%s-keep%d" % (fam, form if form == "key" else kw["agg"], where, name, "-desc" if desc else "", "-kdesc" if kw.get("kdesc") else "",
                                      kw.get("offset", 0) + kw["limit"])
    return Case(cid, names, vals, idx, (where, name), table="%s/%s/%d" % (table or fam, form, len(idx)), **kw)


def exact_cases() -> List[Case]:
    """Families A - F and H on the exact radix select: 2 560 groups, topk_min_groups=1."""
    opt = {"topk_min_groups": 1}
    out: List[Case] = []
    # A. zeros: keep inside the tie class of -0.0 / 0.0 / INT 0 (192 rows), on its last row, and one past it
    for desc in (False, True):
        pool = pool_zeros(-1 if desc else 1)
        for keep in (1, 10, 64, 65, 191, 192, 193):
            # (the other numbers lie below the zeros under DESC: the zeros are the first 192 rows either way)
            where = "first" if keep in (1, 193) else ("last" if keep == 192 else "inside")
            name = "-0.0" if keep <= 192 else ("-5e-324" if desc else "5e-324")
            for kdesc in (False, True):
                out.append(_case("A", pool, where, name, table="A%d" % desc, desc=desc, kdesc=kdesc, limit=keep, options=opt))
            out.append(_case("A", pool, where, name, table="A%d" % desc, desc=desc, form="key", limit=keep, options=opt))
    # B. the whole float line: keep on each class boundary
    pool = pool_float_line()
    for desc, marks in ((False, [("last", "NaN"), ("last", "-5e-324"), ("first", "5e-324"), ("inside", "-max")]),
                        (True, [("last", "5e-324"), ("first", "-5e-324"), ("first", "NaN"), ("last", "+inf")])):
        for i, (where, name) in enumerate(marks):
            for agg in ("min", "max"):
                out.append(_case("B", pool, where, name, desc=desc, kdesc=bool(i & 1), agg=agg, injective=True, options=opt))
    # C. around 2^53 and the int64 ends: keep inside a cluster of equal images
    pool = pool_clusters()
    for desc, marks in ((False, [("inside", "int2^53"), ("first", "int2^53+1"), ("inside", "int2^53+2"), ("inside", "int-2^63+1"),
                                 ("inside", "int-2^53-1"), ("last", "int-2^63")]),
                        (True, [("inside", "flt2^63"), ("inside", "int2^63-1"), ("inside", "int2^53+1"), ("last", "int2^53"),
                                ("inside", "int-2^53")])):
        for i, (where, name) in enumerate(marks):
            out.append(_case("C", pool, where, name, desc=desc, kdesc=bool(i & 1), options=opt))
    # D. dropped bits: keep inside the eight neighbours of 1.0, which share one image
    pool = pool_dropped_bits()
    for desc in (False, True):
        for where, name in (("first", "1+0ulp"), ("inside", "1+3ulp"), ("last", "1+7ulp")):
            out.append(_case("D", pool, where, name, desc=desc, kdesc=desc, options=opt))
    # E. every class in one query: keep on each class boundary, and between the strings that share eight bytes
    for form in ("agg", "key"):
        pool = pool_classes(form)
        first_num, last_num = ("NaN", "+inf") if form == "agg" else ("int-7", "flt29.5")
        asc = [("last", "NULL"), ("last", "false"), ("last", "true"), ("first", first_num), ("last", last_num), ("first", "str%r" % b""),
               ("last", "str%r" % b"abcdefgh1"), ("last", "str%r" % b"\x7f"), ("inside", "str%r" % b"\xc3\xa9")]
        dsc = [("last", "str%r" % b"\x80"), ("last", "str%r" % b""), ("first", last_num), ("last", "true"), ("last", "false"),
               ("first", "NULL"), ("first", "str%r" % b"abcdefgh1")]
        if form == "key":
            asc.append(("last", "MISSING"))
            dsc.append(("last", "NULL"))
        for desc, marks in ((False, asc), (True, dsc)):
            for i, (where, name) in enumerate(marks):
                out.append(_case("E", pool, where, name, desc=desc, kdesc=bool(i & 1), form=form, injective=True, options=opt))
    # F. floods: one value everywhere; two values with keep on the seam
    out.append(_case("F", _named("2.5"), "inside", "2.5", table="F1", limit=1000, injective=True, options=opt))
    two = (["int3", "flt3.5"], [I(3), F(3.5)])
    for desc in (False, True):
        lo, hi = ("flt3.5", "int3") if desc else ("int3", "flt3.5")
        out.append(_case("F", two, "last", lo, table="F2", desc=desc, injective=True, options=opt))
        out.append(_case("F", two, "first", hi, table="F2", desc=desc, injective=True, options=opt))
    # H. rank ends (the float line: every image its own class)
    pool, n = pool_float_line(), N_EXACT
    out.append(_case("H", pool, "first", "NaN", table="B", limit=1, injective=True, options=opt))
    out.append(_case("H", pool, "inside", "+inf", table="B", limit=n - 1, injective=True, options=opt))
    out.append(_case("H", pool, "inside", "+inf", table="B", offset=n - 2, limit=1, kdesc=True, injective=True, options=opt))
    out.append(_case("H", pool, "first", "+inf", table="B", desc=True, agg="max", limit=1, injective=True, options=opt))
    out.append(_case("H", pool, "inside", "NaN", table="B", desc=True, agg="max", offset=n - 2, limit=1, injective=True, options=opt))
    for off, lim, tag in ((n - 5, 5, "keep-is-n"), (n - 5, 10, "keep-over-n"), (0, 0, "limit-0")):
        names, vals = pool
        out.append(Case("H-%s" % tag, names, vals, _replicated(len(vals), n), None, offset=off, limit=lim, options=opt, table="B/agg/%d" % n))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


# G. digit boundaries -------------------------------------------------------------------------------------------------

DIGIT_BYTES = (0x00, 0x03, 0x04, 0xFB, 0xFC, 0xFF)  # the two ends of the bin walk and its lane seams (4 bins per lane)
N_DIGIT = 512


def digit_bodies(pas: int, byte: int, n: int = N_DIGIT) -> Tuple[np.ndarray, int]:
    """`n` distinct number-image bodies, and the target among them whose byte in radix pass `pas` (0 = the image's top byte)
    is `byte`, with the images that share the target's higher bytes spread over every value of that byte.

    Pass 0 holds the 3 class bits, which are 011 for every number: only the byte's low five bits can be chosen there, so the
    target's top byte is 0x60 | (byte & 0x1F) — 0x63 | 0x64 and 0x7B | 0x7C are lane seams all the same, 0x60 and 0x7F the ends
    of what a number can reach."""
    rng = np.random.default_rng([0x70D, pas, byte])
    shift = 56 - 8 * pas

    def low(bits):
        return int(rng.integers(0, 1 << bits, dtype=np.uint64)) if bits else 0

    def make(digit, prev=0):
        if pas == 0:
            t5, rest = digit & 31, low(56)
            if t5 == 0:
                rest |= 1 << 55    # (keeps the body below the images of the NaNs' bit patterns at either end)
            if t5 == 31:
                rest &= ~(1 << 55)
            return (t5 << 56) | rest
        img = 0x17 << 56           # top byte 0x77: a positive normal double whatever the lower bits are
        for j in range(1, pas):
            img |= 0x5A << (56 - 8 * j)
        img += prev << (shift + 8)  # a neighbouring prefix: the byte above this pass's, one less or one more
        return img | (digit << shift) | low(shift)

    same = sorted({make(byte) for _ in range(3 if pas < 7 else 1)})
    target = same[len(same) // 2]
    seen = set(same)
    for digit in range(32 if pas == 0 else 256):
        seen.add(make(digit))
    i = 0
    while len(seen) < n:
        seen.add(make(int(rng.integers(0, 256)), 0 if pas == 0 else (-1 if i & 1 else 1)))
        i += 1
    bodies = np.array(sorted(seen), dtype=np.uint64)
    return bodies[rng.permutation(len(bodies))], target


def digit_case(pas: int, byte: int, desc: bool) -> Case:
    bodies, target = digit_bodies(pas, byte)
    vals = [F(x) for x in doubles_for_images(bodies)]
    names = ["img%016x" % int(b) for b in bodies]
    keep = int((bodies >= np.uint64(target)).sum() if desc else (bodies <= np.uint64(target)).sum())
    return Case("G-pass%d-byte%02x%s" % (pas, byte, "-desc" if desc else ""), names, vals, np.arange(len(vals), dtype=np.int64),
                ("last", "img%016x" % target), desc=desc, agg="max" if desc else "min", limit=keep, injective=True,
                options={"topk_min_groups": 1}, table="G/%d/%d" % (pas, byte))


# the sampled route -----------------------------------------------------------------------------------------------------

K_TOPK_SAMPLE = 16384


def can_sample(n: int, keep: int) -> bool:
    """topk_can_sample's expression (integer arithmetic)."""
    return n >= 4 * K_TOPK_SAMPLE and n < (1 << 32) and keep * 2 * K_TOPK_SAMPLE // n + 16 <= K_TOPK_SAMPLE // 4


def sample_bound_keeps(n: int) -> Tuple[int, int]:
    """The largest keep that still samples at n groups, and the first that does not."""
    lo, hi = 1, n - 1
    assert can_sample(n, lo) and not can_sample(n, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if can_sample(n, mid):
            lo = mid
        else:
            hi = mid
    return lo, hi


def sampled_cases() -> List[Case]:
    """Families B and E at the sample path's size bounds; device-resident batches, the default topk_min_groups — except at
    65 535 groups, one below the default, where the option is lowered to that size so that the filter runs at all (the
    exact route: 65 535 < 4 * kTopkSample)."""
    out: List[Case] = []
    for fam, pool, marks in (("B", pool_float_line(), [(False, "NaN"), (True, "+inf")]),
                             ("E", pool_classes("agg"), [(False, "NULL"), (True, "str%r" % b"\xff")])):
        names, vals = pool
        for n in (65535, 65536, 65537, 81919):
            for desc, name in marks:
                opts = {"topk_min_groups": 65535} if n < 65536 else {}
                out.append(_case("S%s%d" % (fam, n), pool, "inside", name, n=n, table="S" + fam, desc=desc, kdesc=desc, limit=100,
                                 injective=True, options=opts))
        lo, hi = sample_bound_keeps(65536)
        for keep in (lo, hi):
            c = _case("S%sbound" % fam, pool, "inside", names[0], n=65536, table="S" + fam, limit=keep, injective=True)
            c.claim = None if c.claim is None else ("any", "")
            out.append(c)
        # 81 919 groups, stride 4: the last 16 383 slots of the device's group array are never sampled.  Which group gets
        # which slot is the engine's own (the key's hash), so these layouts do NOT control the tail; they are by k: the
        # first holds the smallest value only in k >= 65 536, the second holds the largest value only there.
        n = 81919
        k = np.arange(n)
        pr = dense_ranks([first_term(v, "agg") for v in vals])
        small = [i for i in range(len(vals)) if pr[i] == 0]  # (MISSING and NULL operands both give NULL)
        large = [i for i in range(len(vals)) if pr[i] == max(pr)]
        rest = [i for i in range(len(vals)) if 0 < pr[i] < max(pr)]
        highk_small = np.where(k >= 65536, np.array(small)[k % len(small)], np.array(rest + large)[k % len(rest + large)])
        highk_large = np.where(k >= 65536, np.array(large)[k % len(large)], np.array(small + rest)[k % len(small + rest)])
        out.append(_case("S%shighk-smallest" % fam, pool, "inside", names[small[0]], idx=highk_small.astype(np.int64), table="S%s-ts" % fam,
                         limit=100, injective=True))
        out.append(_case("S%shighk-largest" % fam, pool, "inside", names[small[0]], idx=highk_large.astype(np.int64), table="S%s-tl" % fam,
                         limit=100, injective=True))
    # a flood: 70 000 groups of two values, 8 000 of the low one; every group passes the sample's threshold, more than
    # kTopkSample of them: topk_refine_kernel's no-refine branch
    two = (["int3", "flt3.5"], [I(3), F(3.5)])
    idx = (np.arange(70000) % 35 >= 4).astype(np.int64)  # 4 of every 35 groups hold the low value: 8 000
    for where, name in (("last", "int3"), ("first", "flt3.5")):
        out.append(_case("Sflood", two, where, name, idx=idx, table="Sflood", injective=True))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


def lean_cases() -> List[Case]:
    """Families A, B and E over the partitioned path's kept region (agg_mode=4, one batch); the test runs each with
    lean_topk 1 and 0."""
    opt = {"topk_min_groups": 1, "agg_mode": 4}
    out: List[Case] = []
    for desc in (False, True):
        out.append(_case("LA", pool_zeros(-1 if desc else 1), "inside", "-0.0", table="A%d" % desc, desc=desc, limit=10, options=opt))
        out.append(_case("LA", pool_zeros(-1 if desc else 1), "first", "-5e-324" if desc else "5e-324", table="A%d" % desc, desc=desc,
                         kdesc=True, limit=193, options=opt))
        out.append(_case("LB", pool_float_line(), "last", "5e-324" if desc else "-5e-324", table="B", desc=desc, injective=True, options=opt))
        out.append(_case("LB", pool_float_line(), "last", "+inf" if desc else "NaN", table="B", desc=desc, kdesc=True, injective=True, options=opt))
        out.append(_case("LE", pool_classes("agg"), "last", "str%r" % b"\x80" if desc else "true", table="E", desc=desc, injective=True, options=opt))
        out.append(_case("LE", pool_classes("agg"), "first", "+inf" if desc else "str%r" % b"", table="E", desc=desc, kdesc=True, injective=True,
                         options=opt))
    return out
