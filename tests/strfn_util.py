"""String-function yardstick shared by tests/test_strfn_cpu.py and tests/test_gpu_strfn.py.

A TERM is (steps, terminal): `steps` the functions around the path, OUTERMOST first, each (name, cutset-or-None); `terminal`
one of ("cmp", op, const, const_on_the_left), ("between", lo, hi), ("contains", needle), ("like", pattern),
("pos", name, needle, op, number, const_on_the_left), ("posbetween", name, needle, lo, hi).  term_text writes it as
expression/stringer.go does; strfn4 is the mirror of the reference's semantics (expression/func_str.go).

The mirror works over BYTES.  lower maps A-Z, upper a-z, and the four non-ASCII runes whose simple case mapping is ASCII
(U+0130 -> i, U+212A -> k under lower; U+017F -> S, U+0131 -> I under upper).  Every other non-ASCII rune is left as it
is although Go would map some of them (É -> é): that is exact here because every constant the generators draw is ASCII, and
Go maps a non-ASCII rune outside those four to a non-ASCII rune — which, mapped or not, is not equal to an ASCII byte, is
not part of an ASCII needle, sorts above every ASCII byte, is in no ASCII cutset and is one character for `_` and `%`.
Under a case step Go's strings.Map turns each byte that begins no valid encoding into one U+FFFD; the mirror does so too.
Trimming by an ASCII cutset, comparing, contains and position are bytewise.  LIKE goes through like_util.like_mirror over
Go's decoding of the bytes (each invalid byte one U+FFFD).
"""
from __future__ import annotations

import ctypes as C
import itertools
import json
import random
from typing import List, Sequence

import numpy as np

import like_util as lu
from query_amd import _ffi

MISSING = lu.MISSING
DEV_MAX_LEN = 128  # bytes of a string strfn_match_kernel takes (include/n1k.h, n1k_strfn_eval_device)
WHITESPACE = " \t\n\f\r"  # func_str.go:301
STEP_NAMES = ["lower", "upper", "trim", "ltrim", "rtrim"]
POSITION_NAMES = {"position": 0, "pos": 0, "position0": 0, "pos0": 0, "position1": 1, "pos1": 1}  # func_registry.go:148-153

LOWER_RUNES = {0x130: ord("i"), 0x212A: ord("k")}
UPPER_RUNES = {0x17F: ord("S"), 0x131: ord("I")}


def go_runes(b: bytes) -> List[int]:
    """Go's decoding: code points, every byte that begins no valid encoding one U+FFFD."""
    out, i, n = [], 0, len(b)
    while i < n:
        c = b[i]
        ln = 1 if c < 0x80 else (2 if 0xC2 <= c < 0xE0 else (3 if 0xE0 <= c < 0xF0 else (4 if 0xF0 <= c <= 0xF4 else 0)))
        if ln:
            try:
                out.append(ord(b[i:i + ln].decode("utf-8")))
                i += ln
                continue
            except (UnicodeDecodeError, TypeError):
                pass
        out.append(0xFFFD)
        i += 1
    return out


def valid_utf8(b: bytes) -> bool:
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def _case(b: bytes, lower: bool) -> bytes:
    out = []
    for cp in go_runes(b):
        if lower:
            cp = cp + 32 if 0x41 <= cp <= 0x5A else LOWER_RUNES.get(cp, cp)
        else:
            cp = cp - 32 if 0x61 <= cp <= 0x7A else UPPER_RUNES.get(cp, cp)
        out.append(chr(cp))
    return "".join(out).encode("utf-8")


def apply_steps(b: bytes, steps) -> bytes:
    for name, cut in reversed(list(steps)):  # innermost first
        if name == "lower" or name == "upper":
            b = _case(b, name == "lower")
        else:
            cs = (WHITESPACE if cut is None else cut).encode()
            b = b.strip(cs) if name == "trim" else (b.lstrip(cs) if name == "ltrim" else b.rstrip(cs))
    return b


def _holds(op: str, c: int) -> bool:
    return {"=": c == 0, "<": c < 0, "<=": c <= 0}[op]


def _cmp(a, b) -> int:
    return -1 if a < b else (1 if a > b else 0)


def strfn_mirror(b: bytes, term) -> bool:
    steps, t = term
    v = apply_steps(b, steps)
    if t[0] == "cmp":
        _, op, const, left = t
        c = const.encode()
        return _holds(op, _cmp(c, v) if left else _cmp(v, c))
    if t[0] == "between":
        return t[1].encode() <= v <= t[2].encode()
    if t[0] == "contains":
        return t[1].encode() in v
    if t[0] == "like":
        return lu.like_mirror("".join(chr(cp) for cp in go_runes(v)), t[1])
    ix = v.find(t[2].encode()) + POSITION_NAMES[t[1]]  # strings.Index(...) + startPos, func_str.go:1168-1177
    if t[0] == "pos":
        _, _, _, op, num, left = t
        return _holds(op, _cmp(num, ix) if left else _cmp(ix, num))
    return t[3] <= ix <= t[4]


def strfn4(value, term):
    """MISSING for MISSING, None (NULL) for a non-STRING, else a bool.  A STRING is bytes or str."""
    if value is MISSING:
        return MISSING
    if isinstance(value, str):
        value = value.encode()
    if not isinstance(value, bytes):
        return None
    return strfn_mirror(value, term)


def left_to_host(b: bytes, term) -> bool:
    """What the documented rules send to the host evaluator."""
    steps, t = term
    runes = set(go_runes(b))
    names = {s[0] for s in steps}
    return (len(b) > DEV_MAX_LEN or ("lower" in names and bool(runes & set(LOWER_RUNES))) or ("upper" in names and bool(runes & set(UPPER_RUNES)))
            or (t[0] == "like" and not valid_utf8(b)))


def _q(s: str) -> str:
    return json.dumps(s, ensure_ascii=False)


def _num(x) -> str:
    return "(%s)" % x if x < 0 else str(x)


def chain_text(path: str, steps) -> str:
    text = path
    for name, cut in reversed(list(steps)):
        text = "%s(%s)" % (name, text) if cut is None else "%s(%s, %s)" % (name, text, _q(cut))
    return text


def term_text(path: str, term) -> str:
    steps, t = term
    v = chain_text(path, steps)
    if t[0] == "cmp":
        return "(%s %s %s)" % ((_q(t[2]), t[1], v) if t[3] else (v, t[1], _q(t[2])))
    if t[0] == "between":
        return "(%s between %s and %s)" % (v, _q(t[1]), _q(t[2]))
    if t[0] == "contains":
        return "contains(%s, %s)" % (v, _q(t[1]))
    if t[0] == "like":
        return "(%s like %s)" % (v, _q(t[1]))
    p = "%s(%s, %s)" % (t[1], v, _q(t[2]))
    if t[0] == "pos":
        return "(%s %s %s)" % ((_num(t[4]), t[3], p) if t[5] else (p, t[3], _num(t[4])))
    return "(%s between %s and %s)" % (p, _num(t[3]), _num(t[4]))


# a small alphabet that makes hits common and holds every character class the rules speak of
ASCII_CHARS = ["a", "b", "A", "B", " ", "\t", "\n", "%", "_"]
CHARS = ASCII_CHARS + ["é", "\U0001F600", "İ", "K", "ſ", "ı"]
FOUR = ["İ", "K", "ſ", "ı"]
BAD_BYTES = [b"\xff", b"\x80", b"\xc3", b"\xe2\x84", b"\xf0\x9f\x98", b"\xc0\xaf", b"\xed\xa0\x80"]
CUTSETS = [None, None, "", " ", "a", "ab", "aA", " \t", "b%", "_ "]
LIKE_PATTERNS = ["a%", "%b", "%a%b%", "a_", "_", "", "%", "ab", "%\\%", "a\\_b", "%\n%", "%ab%", "b__", "%A%", "AB%", "%B"]


def random_const(rng: random.Random, lo=0, hi=3) -> str:
    return "".join(rng.choice(ASCII_CHARS[:4] + ASCII_CHARS[:2]) for _ in range(rng.randint(lo, hi)))


def random_steps(rng: random.Random, depth: int):
    return [(n, rng.choice(CUTSETS) if n.endswith("trim") else None) for n in (rng.choice(STEP_NAMES) for _ in range(depth))]


def random_terminal(rng: random.Random, nsteps: int):
    # (LIKE over the bare path is the LIKE kind's own term, position over anything else is refused)
    kinds = ["contains"] + (["like", "cmp", "cmp", "between"] if nsteps else ["pos", "posbetween"])
    k = rng.choice(kinds)
    if k == "cmp":
        return ("cmp", rng.choice(["=", "<", "<="]), random_const(rng), rng.random() < 0.3)
    if k == "between":
        a, b = sorted([random_const(rng), random_const(rng, 1, 3)])
        return ("between", a, b)
    if k == "contains":
        return ("contains", random_const(rng, 0, 2))
    if k == "like":
        return ("like", rng.choice(LIKE_PATTERNS))
    name = rng.choice(sorted(POSITION_NAMES))
    if k == "pos":
        return ("pos", name, random_const(rng, 0, 2), rng.choice(["=", "<", "<="]), rng.choice([-1, 0, 1, 2, 1.5, 3]), rng.random() < 0.3)
    return ("posbetween", name, random_const(rng, 0, 2), rng.choice([-1, 0, 1]), rng.choice([1, 2, 4]))


def random_term(rng: random.Random, max_depth=3):
    steps = random_steps(rng, rng.randint(0, max_depth))
    return (steps, random_terminal(rng, len(steps)))


def random_string(rng: random.Random, kind: int = 0) -> bytes:
    """kind 0: anything of the alphabet; 1: holds one of the four runes; 2: not valid UTF-8."""
    chars = [rng.choice(CHARS if rng.random() < 0.5 else ASCII_CHARS) for _ in range(rng.randint(0, 9))]
    if kind == 1:
        chars.insert(rng.randint(0, len(chars)), rng.choice(FOUR))
    parts = [c.encode() for c in chars]
    if kind == 2:
        parts.insert(rng.randint(0, len(parts)), rng.choice(BAD_BYTES))
    b = b"".join(parts)
    assert kind != 2 or not valid_utf8(b)
    return b


def all_chains(max_depth=3):
    """Every order of the five functions up to the depth, each trim with a cutset drawn by the caller."""
    for d in range(1, max_depth + 1):
        for names in itertools.product(STEP_NAMES, repeat=d):
            yield names


def random_pairs(seed: int, per_term: int = 20):
    """[(term, [bytes...])]: every step order of depth <= 3 under a drawn terminal, the bare path under contains / like /
    position, position0 / position1 with hit, miss and empty needle; every term meets the empty string, strings with the four
    runes and strings that are not valid UTF-8."""
    rng = random.Random(seed)
    terms = []
    for names in all_chains():
        steps = [(n, rng.choice(CUTSETS) if n.endswith("trim") else None) for n in names]
        terms.append((steps, random_terminal(rng, len(steps))))
    for _ in range(30):
        terms.append(([], random_terminal(rng, 0)))
    for name in ("position0", "position1", "pos", "pos1"):
        for needle in ("a", "ab", "zz", ""):
            for op, num in (("=", 0), ("=", -1), ("=", 1), ("<", 2), ("<=", 0)):
                terms.append(([], ("pos", name, needle, op, num, False)))
    terms.append(([("trim", "")], ("cmp", "=", "", False)))
    terms.append(([("lower", None), ("trim", "")], ("cmp", "=", "a", False)))
    out = []
    for term in terms:
        strings = [b""] + [random_string(rng, 0) for _ in range(per_term - 5)] + [random_string(rng, 1) for _ in range(2)] + \
                  [random_string(rng, 2) for _ in range(2)]
        out.append((term, strings))
    return out


# ------------------------------------------------------------------ the library's evaluators

def host_eval(text: str, strings: Sequence[bytes]) -> np.ndarray:
    """n1k_strfn_eval over a block of strings; raises on a status other than N1K_OK."""
    t = text.encode()
    offs, blob = lu.pack(strings)
    out = np.full(max(len(strings), 1), 7, dtype=np.uint8)
    st = _ffi.lib().n1k_strfn_eval(t, len(t), len(strings), offs.ctypes.data, blob, out.ctypes.data)
    if st != _ffi.OK:
        raise RuntimeError("n1k_strfn_eval: status %d for %s" % (st, text))
    return out[:len(strings)]


def host_status(text: bytes) -> int:
    offs, blob = lu.pack([b"a"])
    out = np.zeros(1, dtype=np.uint8)
    return _ffi.lib().n1k_strfn_eval(text, len(text), 1, offs.ctypes.data, blob, out.ctypes.data)


def device_eval(text: str, strings: Sequence[bytes], device: int = 0):
    """n1k_strfn_eval_device: (bits, strings left to the host evaluator)."""
    t = text.encode()
    offs, blob = lu.pack(strings)
    out = np.full(max(len(strings), 1), 7, dtype=np.uint8)
    left = C.c_uint64(0)
    st = _ffi.lib().n1k_strfn_eval_device(device, t, len(t), len(strings), offs.ctypes.data, blob, out.ctypes.data, C.byref(left))
    if st != _ffi.OK:
        raise RuntimeError("n1k_strfn_eval_device: status %d for %s" % (st, text))
    return out[:len(strings)], int(left.value)


# ------------------------------------------------------------------ tables and plans of the differential by substitution

def D(name):
    return "(`default`.`%s`)" % name


# dictionary: strings the terms below split in many ways, then two arrays (dictionary coded, but their tag is ARRAY)
WORDS = ["", "a", "A", "ab", "AB", "aB", " ab ", "\tab\n", "abab", "b", "Ba", "bab", "a%b", "a_b", "ab\nab", "é", "aÉb", "a\U0001F600B", "İab",
         "aKB", "ſab", "ABı", "  ", "aa b aa", "cat_1", "Cat_10", "CAT_11", " cat_2", "zz"]
DICT = [w.encode() for w in WORDS] + [b"[1,2]", b"[\"ab\"]"]
ARR0 = len(WORDS)
KEY0 = WORDS.index("cat_1")
PLAN_TERMS = [
    ([("lower", None)], ("cmp", "=", "ab", False)), ([("upper", None)], ("cmp", "=", "AB", True)), ([("lower", None)], ("like", "%ab%")),
    ([("lower", None), ("trim", None)], ("cmp", "=", "ab", False)), ([("trim", "a")], ("cmp", "<", "c", False)), ([("ltrim", None)], ("cmp", "<=", "ab", True)),
    ([("rtrim", " \n")], ("between", "a", "b")), ([], ("contains", "ab")), ([("upper", None)], ("contains", "B")), ([("lower", None)], ("like", "cat\\_1%")),
    ([], ("pos", "position", "b", "=", 1, False)), ([], ("pos", "pos1", "ab", "<", 2, True)), ([], ("posbetween", "position1", "a", 1, 2)),
    ([("upper", None), ("rtrim", "b"), ("lower", None)], ("like", "A_")), ([("trim", None)], ("like", "ab%")), ([("lower", None)], ("between", "a", "b")),
    ([("ltrim", "aA"), ("upper", None)], ("cmp", "=", "B", False)), ([("lower", None)], ("contains", "")), ([("upper", None), ("trim", " ")], ("like", "CAT%")),
]
LIKE_TERMS = ["ab%", "%b", "a_b", "%a%b%", "cat\\_1%", ""]
IN_LISTS = [["ab", "zz"], ["a", "A", "cat_1"], ["b", "é", None]]  # (strings and null only: column_values keeps no other value)


def make_table(rng, n):
    """s: DICT32 strings with NULL / MISSING; m: TAGGED64 of every class (strings, numbers, booleans, NULL, MISSING, arrays);
    x: numbers; k: DICT32 key; g: small ints; a: DICT32 arrays."""
    from oracle import n1o
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
    kc = rng.integers(KEY0, len(WORDS), n).astype(np.uint32)  # cat_1 .. zz
    kc[rng.random(n) < 0.04] = 0xFFFFFFFE
    kc[rng.random(n) < 0.03] = 0xFFFFFFFF
    gt = np.full(n, n1o.T_INT, np.uint8)
    gp = rng.integers(0, 7, n).astype(np.int64).view(np.uint64).copy()
    at = np.full(n, n1o.T_ARRAY, np.uint8)
    ap = (ARR0 + rng.integers(0, 2, n)).astype(np.uint64)
    at[rng.random(n) < 0.1] = n1o.T_NULL
    return n1o.Table([n1o.Column(D("s"), n1o.COL_DICT32, codes=sc), n1o.Column(D("m"), n1o.COL_TAGGED64, tags=mt, payload=mp),
                      n1o.Column(D("x"), n1o.COL_TAGGED64, tags=xt, payload=xp), n1o.Column(D("k"), n1o.COL_DICT32, codes=kc),
                      n1o.Column(D("g"), n1o.COL_TAGGED64, tags=gt, payload=gp), n1o.Column(D("a"), n1o.COL_TAGGED64, tags=at, payload=ap)], list(DICT))


def column_values(t, name):
    """The python values of a column: str, MISSING, None (NULL), a parsed list for an array, 0 for any other non-string."""
    from oracle import n1o
    c = {c.name: c for c in t.columns}[D(name)]
    if c.kind == n1o.COL_DICT32:
        return [MISSING if x == 0xFFFFFFFF else (None if x == 0xFFFFFFFE else WORDS[x]) for x in c.codes.tolist()]
    out = []
    for tg, p in zip(c.tags.tolist(), c.payload.tolist()):
        out.append(MISSING if tg == n1o.T_MISSING else (None if tg == n1o.T_NULL else (WORDS[p] if tg == n1o.T_STRING else
                   (json.loads(DICT[p]) if tg == n1o.T_ARRAY else 0))))
    return out


class Substitution:
    """Collects the match-table terms of one plan: the device sees the term, the oracle a helper column of the mirror's
    4-valued results (the oracle evaluates a bare path inside AND / OR / NOT with the full 4-valued logic)."""

    def __init__(self, table):
        self.table = table
        self.helpers = []

    def _helper(self, results):
        from oracle import n1o
        tags = np.array([n1o.T_MISSING if r is MISSING else (n1o.T_NULL if r is None else (n1o.T_TRUE if r else n1o.T_FALSE)) for r in results], np.uint8)
        name = D("h%d" % len(self.helpers))
        self.helpers.append(n1o.Column(name, n1o.COL_TAGGED64, tags=tags, payload=np.zeros(len(results), np.uint64)))
        return name

    def strfn(self, col, term):
        vals = column_values(self.table, col)
        return term_text(D(col), term), self._helper([strfn4(v if (v is MISSING or isinstance(v, str)) else (None if v is None else 0), term) for v in vals])

    def like(self, col, pattern):
        vals = column_values(self.table, col)
        return "(%s like %s)" % (D(col), _q(pattern)), self._helper([lu.like4(v if (v is MISSING or v is None or isinstance(v, str)) else 0, pattern) for v in vals])

    def in_(self, col, consts):
        import in_util as iu
        vals = column_values(self.table, col)
        return iu.term(D(col), consts), self._helper([iu.in4(iu.MISSING if v is MISSING else v, consts) for v in vals])

    def any_(self, const):
        # any `v` in a satisfies (`v` = const) end over the array column: MISSING / NULL for a non-array, else a bool
        vals = column_values(self.table, "a")
        res = [MISSING if v is MISSING else (None if not isinstance(v, list) else any(type(e) is type(const) and e == const for e in v)) for v in vals]
        return "any `v` in %s satisfies (`v` = %s) end" % (D("a"), json.dumps(const)), self._helper(res)

    def oracle_table(self):
        from oracle import n1o
        return n1o.Table(list(self.table.columns) + self.helpers, self.table.dictionary)


def other_term(rng):
    r = rng.integers(0, 5)
    if r == 0: return "(%s < %s)" % (["10", "40.5", "70"][rng.integers(0, 3)], D("x"))
    if r == 1: return "(%s <= %s)" % (D("x"), ["30", "55.25"][rng.integers(0, 2)])
    if r == 2: return "(%s = %s)" % (D("s"), ["\"ab\"", "\"cat_1\""][rng.integers(0, 2)])
    if r == 3: return "(%s is %s)" % (D(["m", "s", "x"][rng.integers(0, 3)]), ["null", "not null", "missing", "valued"][rng.integers(0, 4)])
    return "(%s between 2 and 5)" % D("g")


def table_term(rng, sub, strfn_only=False):
    """A term of one of the four kinds of the match table (mostly a string-function term): (device text, oracle text)."""
    r = 0 if strfn_only else rng.integers(0, 10)
    col = ["s", "m"][rng.integers(0, 2)]
    if r < 6: return sub.strfn(col, PLAN_TERMS[rng.integers(0, len(PLAN_TERMS))])
    if r < 8: return sub.like(col, LIKE_TERMS[rng.integers(0, len(LIKE_TERMS))])
    if r == 8: return sub.in_(col, IN_LISTS[rng.integers(0, len(IN_LISTS))])
    return sub.any_([1, "ab"][rng.integers(0, 2)])


def rand_tree(rng, sub, budget, depth=0):
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
        return table_term(rng, sub, strfn_only=budget[1] == 1)  # (the first one is a string-function term)
    t = other_term(rng)
    return t, t


def rand_strfn_plan(rng, t, bounded):
    sub = Substitution(t)
    if bounded:
        # the bounded family: a string-function term over a column as one of <= 2 ANDed terms, <= 3 columns, dictionary key
        col = ["s", "m"][rng.integers(0, 2)]
        d, o = sub.strfn(col, PLAN_TERMS[rng.integers(0, len(PLAN_TERMS))])
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
    sub = Substitution(t)
    budget = [int(rng.integers(1, 5)), 0]
    d, o = rand_tree(rng, sub, budget)
    if budget[1] == 0:
        d2, o2 = table_term(rng, sub, strfn_only=True)
        d, o = "(%s and %s)" % (d, d2), "(%s and %s)" % (o, o2)
    # every plan outside the bounded family also holds a term of another kind of the table: the kinds share the byte
    col = ["s", "m"][rng.integers(0, 2)]
    k = int(rng.integers(0, 3))
    d2, o2 = (sub.like(col, LIKE_TERMS[rng.integers(0, len(LIKE_TERMS))]) if k == 0 else
              (sub.in_(col, IN_LISTS[rng.integers(0, len(IN_LISTS))]) if k == 1 else sub.any_([1, "ab"][rng.integers(0, 2)])))
    op = ["and", "or"][rng.integers(0, 2)]
    d, o = "(%s %s %s)" % (d, op, d2), "(%s %s %s)" % (o, op, o2)
    keys = [[D("k")], [D("g")], [D("k"), D("g")], []][rng.integers(0, 4)]
    aggs = sorted(set(["count(*)"] + [["sum(%s)" % D("x"), "avg(%s)" % D("x"), "min(%s)" % D("s"), "max(%s)" % D("x"), "count(%s)" % D("m")][i]
                                      for i in rng.choice(5, int(rng.integers(1, 3)), replace=False)]))
    return sub, d, o, keys, aggs


# (options, bounded shape, the kernel family stats["spec_kernel"] must report: 0 interpreter / bounded kernel, 2 run-time built)
FAMILIES = [({"fast": 0}, False, 0), ({}, False, 0), ({"fast": 0}, True, 0), ({"spec": 0}, True, 0), ({"jit": 2}, True, 2), ({"jit": 2}, True, 2)]
SEED_BASE = 717_000
SEEDS = 240


def draw_plan(seed):
    """Seed -> (table, family, plan): ONE order of draws for tests/test_gpu_strfn.py and the bounded-family check of
    tests/test_strfn_cpu.py."""
    rng = np.random.default_rng(SEED_BASE + seed)
    t = make_table(rng, int(rng.integers(1, 5000)))
    opts, bounded, kernel = FAMILIES[seed % len(FAMILIES)]
    sub, dcond, ocond, keys, aggs = rand_strfn_plan(rng, t, bounded)
    batches = int(rng.integers(1, 4))
    return t, (opts, bounded, kernel), (sub, dcond, ocond, keys, aggs), batches
