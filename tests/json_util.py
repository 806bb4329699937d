"""Per-document checks of the JSON extractors (n1k_json.cpp on the host, json_extract_kernel on the device).

Three things live here, none of which calls the code under test:

* a text-level reference: the wanted values of a document as (tag, payload) pairs, numbers typed from their LITERAL with
  int() / float() (float() is correctly rounded, as Go's ParseFloat) by value.NewValue's rules, strings / structure /
  canonical texts from json.loads with golden_util's rules, the first field of a name counting (go_json.FirstFind);
* stays_on_device(): the device extractor's hand-over rules restated from the header comment of n1k_jsondev.hip and
  DESIGN.md §8 item 7;
* seeded document generators that label every document device-kind or host-kind by construction.

The GPU tests read the device-extracted values through a grouping channel: every document carries a unique "id", the plan
groups by it, and so every group is one document (run_channel / channel_expected below).
"""
from __future__ import annotations

import json
import math
import re
import struct
from typing import List, Optional, Sequence, Tuple

import numpy as np

import golden_util as gu
import query_amd
from query_amd import _ffi, plan

T_MISSING, T_NULL, T_FALSE, T_TRUE, T_INT, T_FLOAT, T_STRING, T_ARRAY, T_OBJECT = range(9)
U64 = 0xFFFFFFFFFFFFFFFF

# the device extractor's limits (n1k_jsondev.hip, n1k_kernels.h, n1k_types.h)
WAVE_BYTES = 16 * 1024  # kJsonWaveBytes: LDS share of a wave
MAX_STEPS = 4           # kJsonMaxSteps
MAX_COLS = 16           # kMaxCols
SKIP_DEPTH = 64         # open non-empty brackets a skipped value may nest


def D(*steps):
    """Stringer text of a leaf path below the keyspace alias: field names, and ints for array elements"""
    s = "`default`"
    for st in steps:
        s = "(%s[%d])" % (s, st) if isinstance(st, int) else "(%s.`%s`)" % (s, st)
    return s


# ------------------------------------------------------------------------------------------------ the reference

class _Num:
    """A number as the document spells it."""
    __slots__ = ("text",)

    def __init__(self, text):
        self.text = text


class _Obj:
    """An object as the document spells it: every member, in order."""
    __slots__ = ("pairs",)

    def __init__(self, pairs):
        self.pairs = pairs


def type_number(text: str) -> Tuple[int, int]:
    """value.NewValue over go_json's number (value/value.go:375-382): an integer literal that fits int64 is INT, every other
    literal is the correctly rounded float64, and a float64 with no fraction inside int64 folds to INT."""
    if not any(c in text for c in ".eE"):
        v = int(text)
        if -2 ** 63 <= v < 2 ** 63:
            return T_INT, v & U64
    f = float(text)
    if math.isfinite(f) and f == math.floor(f) and -2.0 ** 63 <= f < 2.0 ** 63:
        return T_INT, int(f) & U64
    return T_FLOAT, struct.unpack("<Q", struct.pack("<d", f))[0]


def _plain(v):
    """_Num / _Obj tree -> what golden_util.canonical_json takes (a Go map keeps the LAST of equal names)."""
    if isinstance(v, _Num):
        t, p = type_number(v.text)
        return (p - (1 << 64) if p >> 63 else p) if t == T_INT else struct.unpack("<d", struct.pack("<Q", p))[0]
    if isinstance(v, _Obj):
        return {k: _plain(x) for k, x in v.pairs}
    if isinstance(v, list):
        return [_plain(x) for x in v]
    return v


def _value(v) -> Tuple[int, object]:
    if v is gu.MISSING:
        return T_MISSING, 0
    if v is None:
        return T_NULL, 0
    if v is True:
        return T_TRUE, 0
    if v is False:
        return T_FALSE, 0
    if isinstance(v, _Num):
        return type_number(v.text)
    if isinstance(v, str):
        return T_STRING, v.encode()
    if isinstance(v, list):
        return T_ARRAY, gu.canonical_json(_plain(v)).encode()
    return T_OBJECT, gu.canonical_json(_plain(v)).encode()


def reference_values(doc, paths: Sequence[Sequence[str]]) -> List[Tuple[int, object]]:
    """(tag, payload) of every path (a sequence of field names) in one document's text: payload is the 64 value bits of a
    number, the bytes of a string, the canonical text of an array / object, 0 otherwise."""
    text = doc.decode() if isinstance(doc, bytes) else doc
    root = json.loads(text, parse_int=_Num, parse_float=_Num, object_pairs_hook=_Obj, strict=False)
    out = []
    for steps in paths:
        cur = root
        for name in steps:
            nxt = gu.MISSING
            if isinstance(name, int):
                if isinstance(cur, list) and -len(cur) <= name < len(cur):
                    nxt = cur[name]
            elif isinstance(cur, _Obj):
                for k, x in cur.pairs:
                    if k == name:  # FirstFind: the first field of a name counts (value/parsed.go:189-193)
                        nxt = x
                        break
            cur = nxt
            if cur is gu.MISSING:
                break
        out.append(_value(cur))
    return out


# ------------------------------------------------------------------------------------- the hand-over rules

_NUMBER = re.compile(rb"-?[0-9]+(?:\.[0-9]+)?(?:[eE][+-]?[0-9]+)?")
_NUMBER_PARTS = re.compile(r"-?([0-9]+)(?:\.([0-9]+))?(?:[eE]([+-]?[0-9]+))?\Z")
_STRING = re.compile(rb'"((?:[^"\\]|\\(?:["\\/bfnrt]|u[0-9a-fA-F]{4}))*)"')
_WS = re.compile(rb"[ \t\r\n]*")


def number_on_device(literal: str) -> bool:
    """The device types a wanted number itself when the conversion is exact by construction.  With `digits` the digits
    from the first non-zero one to the last one written (integer and fraction part together, trailing zeros included) and
    e10 = the written exponent minus the number of fraction digits:
      * more than 18 digits: the host;
      * no fraction and no exponent: the device (the digits are an int64);
      * else more than 15 digits, or |e10| > 22: the host (outside Clinger's exact case);
      * else the device."""
    m = _NUMBER_PARTS.match(literal)
    if not m:
        return False
    ip, fp, ex = m.group(1), m.group(2), m.group(3)
    digits = len((ip + (fp or "")).lstrip("0"))
    if digits > 18:
        return False
    if fp is None and ex is None:
        return True
    e10 = (int(ex) if ex else 0) - len(fp or "")
    return digits <= 15 and -22 <= e10 <= 22


class _Host(Exception):
    pass


class _Walk:
    def __init__(self, doc: bytes, paths):
        self.s, self.p, self.paths = doc, 0, paths

    def ws(self):
        self.p = _WS.match(self.s, self.p).end()

    def peek(self):
        return self.s[self.p:self.p + 1]

    def string(self) -> bytes:
        m = _STRING.match(self.s, self.p)
        if not m:
            raise _Host("malformed")
        self.p = m.end()
        return m.group(1)

    def scalar(self) -> Optional[bytes]:
        """a literal or a number at p; returns the number's text"""
        for lit in (b"true", b"false", b"null"):
            if self.s.startswith(lit[:1], self.p):
                if not self.s.startswith(lit, self.p):
                    raise _Host("malformed")
                self.p += len(lit)
                return None
        m = _NUMBER.match(self.s, self.p)
        if not m:
            raise _Host("malformed")
        self.p = m.end()
        return m.group(0)

    def skip(self):
        """an unwanted value: validated whatever it holds, as long as no more than SKIP_DEPTH non-empty brackets are open"""
        stack = []
        while True:
            self.ws()
            c = self.peek()
            opened = False
            if c == b'"':
                self.string()
            elif c in (b"{", b"["):
                self.p += 1
                self.ws()
                if self.peek() == (b"}" if c == b"{" else b"]"):
                    self.p += 1
                else:
                    if len(stack) >= SKIP_DEPTH:
                        raise _Host("nested too deep")
                    stack.append(c)
                    if c == b"{":
                        self.name()
                    opened = True
            else:
                self.scalar()
            if opened:
                continue
            while True:
                if not stack:
                    return
                self.ws()
                c = self.peek()
                if c == b",":
                    self.p += 1
                    if stack[-1] == b"{":
                        self.ws()
                        self.name()
                    break
                if c == (b"}" if stack[-1] == b"{" else b"]"):
                    self.p += 1
                    stack.pop()
                    continue
                raise _Host("malformed")

    def name(self) -> bytes:
        n = self.string()
        self.ws()
        if self.peek() != b":":
            raise _Host("malformed")
        self.p += 1
        return n

    def wanted_object(self, level: int, active: set):
        """p behind the '{' of a non-empty object in which the paths `active` look up their step `level`"""
        found = set()
        while True:
            self.ws()
            raw = self.name()
            self.ws()
            cand = active - found
            if cand and b"\\" in raw:
                raise _Host("an escaped name while a path is still looked up at this level")
            hit = {i for i in cand if self.paths[i][level].encode() == raw}
            found |= hit
            leafs = {i for i in hit if len(self.paths[i]) == level + 1}
            deeper = hit - leafs
            c = self.peek()
            if leafs:
                if c == b'"':
                    if b"\\" in self.string():
                        raise _Host("an escape in a wanted string")
                elif c in (b"{", b"["):
                    raise _Host("an array / object value of a wanted path")
                else:
                    num = self.scalar()
                    if num is not None and not number_on_device(num.decode()):
                        raise _Host("a wanted number off the exact fast path")
            elif deeper and c == b"{":
                self.p += 1
                self.ws()
                if self.peek() == b"}":
                    self.p += 1
                else:
                    self.wanted_object(level + 1, deeper)
            else:
                self.skip()
            self.ws()
            c = self.peek()
            self.p += 1
            if c == b",":
                continue
            if c == b"}":
                return
            raise _Host("malformed")


def paths_on_device(paths) -> bool:
    """The plan's side of the rules: 1 to 16 leaf paths, each 1 to 4 field names, no array element."""
    return 1 <= len(paths) <= MAX_COLS and all(1 <= len(p) <= MAX_STEPS and all(isinstance(s, str) for s in p) for p in paths)


def stays_on_device(doc_text, paths, offset: int = 0) -> bool:
    """Does json_extract_kernel type this document itself (status 0)?  `offset` is where the document starts in its
    batch, counted from the batch's first byte.  The rules, from the header comment of n1k_jsondev.hip and DESIGN.md §8
    item 7 — a document goes to the host when
      * it does not fit the wave's LDS share staged from a 16-byte boundary: len + offset % 16 > kJsonWaveBytes - 16;
      * it is not an object, or does not parse (the host names the malformed one);
      * an object in which a path is still looked up has a member whose NAME is written with an escape (objects that are
        skipped, and levels where every path has found its field, may hold such names);
      * the value of a wanted path is a string written with an escape, an array or an object;
      * the value of a wanted path is a number for which number_on_device() does not hold;
      * a value that is skipped nests more than 64 non-empty arrays / objects.
    Duplicates of a name that was found, and everything inside skipped values, are validated and never handed over."""
    doc = doc_text.encode() if isinstance(doc_text, str) else bytes(doc_text)
    if not paths_on_device(paths):
        return False
    if len(doc) + offset % 16 > WAVE_BYTES - 16:
        return False
    w = _Walk(doc, [tuple(p) for p in paths])
    try:
        w.ws()
        if w.peek() != b"{":
            return False
        w.p += 1
        w.ws()
        if w.peek() == b"}":
            w.p += 1
        else:
            w.wanted_object(0, set(range(len(paths))))
        w.ws()
        return w.p == len(doc)
    except _Host:
        return False


# ----------------------------------------------------------------------------------------------- the channel

class Channel:
    """A plan that reads `paths` back per document: GROUP BY id and up to three `key_paths`, the `agg_paths` as operands
    of MIN (a lone value comes back unchanged; MISSING and NULL both come back as NULL).  Arrays and objects travel as
    keys only.  The keys share one 63-bit packed key (n1k_engine.cpp, fix_layout): two keys beside the id leave room for a
    few thousand documents, three for a few hundred."""

    def __init__(self, key_paths, agg_paths=(), condition=None):
        self.key_paths = [tuple(p) for p in key_paths]
        self.agg_paths = [tuple(p) for p in agg_paths]
        assert len(self.key_paths) <= 3 and len(self.agg_paths) <= 8
        self.keys = [D("id")] + [D(*p) for p in self.key_paths]
        self.aggs = sorted("min(%s)" % D(*p) for p in self.agg_paths) or ["count(*)"]
        self.condition = condition
        self.plan = plan.filter_group_plan(condition, self.keys, self.aggs)

    def expected(self, docs) -> dict:
        """id -> the reference's values in key order, then agg_paths order"""
        out = {}
        for doc in docs:
            vals = reference_values(doc, [("id",)] + self.key_paths + self.agg_paths)
            assert vals[0][0] == T_STRING and vals[0][1] not in out, doc
            nk = 1 + len(self.key_paths)
            aggs = [(T_NULL, 0) if t in (T_MISSING, T_NULL) else (t, p) for t, p in vals[nk:]]
            out[vals[0][1]] = tuple(vals[1:nk] + aggs)
        return out

    def run(self, batches, device: int, nonzero_base: int = 0, **options):
        """Push the batches (lists of documents) with one process_json each; returns ({id: values as expected()}, stats)."""
        op = query_amd.GpuFilterGroup(self.plan, json_device=device, json_device_min_docs=1, **options)
        try:
            names = op.aggregate_names
            for docs in batches:
                if nonzero_base:
                    push_with_base(op, docs, nonzero_base)
                else:
                    op.process_json(docs)
            raw = op.after_items_raw()
            st = op.stats()
            cache = {}

            def val(cell):
                t, v = int(cell["tag"]), int(cell["v"])
                if t >= T_STRING:
                    if v not in cache:
                        cache[v] = op.dict_get(v)
                    return t, cache[v]
                return (t, v) if t in (T_INT, T_FLOAT) else (t, 0)

            order = [names.index("min(%s)" % D(*p)) for p in self.agg_paths]
            out = {}
            for g in range(raw["ngroups"]):
                k = [val(c) for c in raw["keys"][g]]
                assert k[0][0] == T_STRING and k[0][1] not in out, k
                out[k[0][1]] = tuple(k[1:] + [val(raw["aggs"][g][a]) for a in order])
            return out, st
        finally:
            op.done()


def push_with_base(op, docs, junk: int):
    """n1k_push_json through the ctypes binding with offsets[0] == junk: the batch's bytes begin behind `junk` other bytes."""
    import ctypes as C
    offsets = np.zeros(len(docs) + 1, dtype=np.uint64)
    offsets[0] = junk
    np.cumsum([len(d) for d in docs], out=offsets[1:])
    offsets[1:] += np.uint64(junk)
    blob = b"#" * junk + b"".join(docs)
    op._check(op._lib.n1k_push_json(op._h, len(docs), offsets.ctypes.data_as(C.POINTER(C.c_uint64)), blob))


def batch_offsets(docs) -> List[int]:
    out, at = [], 0
    for d in docs:
        out.append(at)
        at += len(d)
    return out


def predicted_device_docs(batches, paths) -> int:
    return sum(stays_on_device(d, paths, o) for docs in batches for d, o in zip(docs, batch_offsets(docs)))


def first_difference(got: dict, want: dict):
    """None when equal, else a description of the first document that differs"""
    if got == want:
        return None
    for k in want:
        if k not in got:
            return "document %r is missing from the result" % k
        if got[k] != want[k]:
            return "document %r: got %r, want %r" % (k, got[k], want[k])
    return "documents not pushed: %r" % sorted(set(got) - set(want))[:5]


# --------------------------------------------------------------------------------------------- number literals

SIG_DIGITS = (1, 2, 3, 7, 14, 15, 16, 17, 18, 19, 20)
EXPONENTS = (0, 1, 2, 5, 15, 21, 22, 23, 24, 37, 300, 308, 323, 324)
PINNED = [str(2 ** 53), str(2 ** 53 + 1), str(2 ** 63 - 1), str(2 ** 63), str(-2 ** 63), "999999999999999999",
          str(10 ** 18), "1e18", "1.0e18", "-0", "-0.0", "0e5", "1e22", "1e23", "9e22", "0.1", "0.30000000000000004", "4.9e-324",
          "123456789012345e22", "123456789012345e-22", "123456789012345e23", "123456789012345e-23",  # 15 digits, e10 = ±22, ±23
          "1.23456789012345e36", "1234567890.12345e-17", "12345678901234.5e24", "0.123456789012345e-8",  # the same through a fraction
          "1234567890123456e0", "1234567890123456.0", "123456789012345.6", "1.234567890123456"]  # 16 digits, e10 = 0 and below


def random_literal(rng) -> str:
    nd = SIG_DIGITS[int(rng.integers(0, len(SIG_DIGITS)))]
    digits = str(int(rng.integers(1, 10))) + "".join(str(int(x)) for x in rng.integers(0, 10, nd - 1))
    s = "-" if rng.random() < 0.3 else ""
    if rng.random() < 0.6:  # a fraction, cut anywhere
        cut = int(rng.integers(0, nd + 1))
        lead = int(rng.integers(1, 25)) if rng.random() < 0.25 else 0
        trail = int(rng.integers(1, 5)) if rng.random() < 0.25 else 0
        frac = "0" * lead + digits[cut:] + "0" * trail
        s += (digits[:cut] or "0") + "." + (frac or "0")
    else:
        s += digits
    if rng.random() < 0.5:
        e = EXPONENTS[int(rng.integers(0, len(EXPONENTS)))]
        s += "eE"[int(rng.integers(0, 2))] + ["", "+", "-"][int(rng.integers(0, 3))] + "0" * int(rng.integers(0, 3)) + str(e)
    return s


def number_literals(seed: int, n: int, device_only: bool = False) -> List[str]:
    """n literals: the pinned ones, then random ones; none overflows to ±Inf (what the reference does there is open)."""
    rng = np.random.default_rng(9000 + seed)
    out = [x for x in PINNED if not device_only or number_on_device(x)]
    while len(out) < n:
        lit = random_literal(rng)
        if math.isinf(float(lit)) or (device_only and not number_on_device(lit)):
            continue
        out.append(lit)
    return out[:n]


NUMBER_PATHS = [("id",), ("a",), ("b",)]


def number_docs(seed: int, ndocs: int, device_only: bool = False) -> List[bytes]:
    """{"id": "d<i>", "a": <literal>, "b": <literal>}: two number paths per document (the channel reads a as a key, b
    through MIN)"""
    lits = number_literals(seed, 2 * ndocs, device_only)
    return [('{"id": "d%d", "a": %s, "b": %s}' % (i, lits[2 * i], lits[2 * i + 1])).encode() for i in range(ndocs)]


# --------------------------------------------------------------------------------------------------- structure

# id + two key paths (s and o may hold arrays / objects) + six MIN operands (scalars by construction)
STRUCT_KEYS = [("s",), ("o",)]
STRUCT_AGGS = [("price",), ("x", "y"), ("x", "z"), ("w", "y"), ("a", "b", "c", "d"), ("t",)]
STRUCT_PATHS = [("id",)] + STRUCT_KEYS + STRUCT_AGGS

_STRINGS = ["", "q", "f" * 15, "s" * 16, "v" * 17, "L" * 300, "été € \U0001F600", "price", "x", "alpha", "beta", "NaN"]
_DEV_NUMS = ["0", "7", "-12", "1.5", "-2.25", "1e3", "2.5E-3", "123456789012345678", "100e-2", "12.0", "-0.0", "0.001"]
_HOST_NUMS = ["0.30000000000000004", "1234567890123456789", "1e23", "1234567890123456.5", "4.9e-324", "9223372036854775808"]
_JUNK_NUMS = _DEV_NUMS + _HOST_NUMS


class _Gen:
    def __init__(self, rng):
        self.rng = rng
        self.host = False  # set by whatever makes the document the host's

    def pick(self, xs):
        return xs[int(self.rng.integers(0, len(xs)))]

    def chance(self, p):
        return self.rng.random() < p

    def sp(self):
        return self.pick(["", "", "", " ", "  ", "\n", "\t", "\r\n "])

    def plain_string(self):
        return json.dumps(self.pick(_STRINGS), ensure_ascii=False)

    def escaped_string(self):
        return self.pick(['"a\\"b"', '"tab\\there"', '"\\u00e9t\\u00e9"', '"back\\\\slash"', '"\\ud83d\\ude00"', '"sl\\/ash"'])

    def junk(self, depth=0):
        """a value nobody wants: anything goes inside it, wanted names and the host's kinds of value included"""
        r = int(self.rng.integers(0, 10))
        if r < 2:
            return self.pick(_JUNK_NUMS)
        if r < 4:
            return self.plain_string() if self.chance(0.6) else self.escaped_string()
        if r == 4:
            return self.pick(["true", "false", "null", "{}", "[]", "[ ]", "{ }"])
        if depth >= 3:
            return "1"
        if r < 7:
            return "[" + self.sp() + ("," + self.sp()).join(self.junk(depth + 1) for _ in range(int(self.rng.integers(1, 4)))) + self.sp() + "]"
        names = ["s", "price", "x", "y", "id", "k", "\\u0073", "o", "y"]
        return "{" + self.sp() + ("," + self.sp()).join('"%s"%s:%s%s' % (self.pick(names), self.sp(), self.sp(), self.junk(depth + 1))
                                                       for _ in range(int(self.rng.integers(1, 4)))) + self.sp() + "}"

    def scalar(self, host_ok=True):
        """a value of a wanted path; may make the document the host's"""
        r = int(self.rng.integers(0, 20))
        if r < 7:
            return self.pick(_DEV_NUMS)
        if r < 13:
            return self.plain_string()
        if r < 16:
            return self.pick(["true", "false", "null"])
        if not host_ok or r < 18:
            return self.pick(_DEV_NUMS)
        self.host = True
        return self.pick(_HOST_NUMS) if r == 18 else self.escaped_string()

    def obj(self, members):
        return "{" + self.sp() + ("," + self.sp()).join('"%s"%s:%s%s' % (n, self.sp(), self.sp(), v) for n, v in members) + self.sp() + "}"


def structure_doc(i: int, rng, host_share: float = 0.08) -> Tuple[bytes, bool]:
    """One valid document as text and whether the device keeps it.  Built from the features of the issue's list: whitespace,
    duplicate names at every level, wanted names inside skipped values, prefix / extension names, a name at several
    levels, escaped names before and after every path has found its field, strings of 0 / 1 / 15 / 16 / 17 / 300 bytes,
    multi-byte UTF-8, strings equal to a field name, few distinct strings over many documents."""
    g = _Gen(rng)
    host_ok = g.chance(host_share * 2)  # documents that MAY draw one of the host's kinds of value
    top = []    # (name as written, value text)
    full = g.chance(0.5)  # every top-level wanted name present: escaped names behind them are the device's business
    # x: paths x.y and x.z
    have_x = full or g.chance(0.9)
    xm = []
    xv = None
    if have_x and g.chance(0.1):
        xv = g.pick(["5", '"x"', "null", "[1, {\"y\": 2}]"])  # a field of a non-object is MISSING
    elif have_x:
        if g.chance(0.8):
            xm.append(("y", g.scalar(host_ok)))
        if g.chance(0.3):
            xm.insert(0, (g.pick(["yy", "Y", "x", "z2", ""]), g.junk()))
        if g.chance(0.7):
            xm.append(("z", g.scalar(host_ok)))
        if g.chance(0.3):
            nm = g.pick(["y", "z"])  # a duplicate (anything: it is skipped), or the first if the name was left out
            xm.append((nm, g.junk() if nm in [n for n, _ in xm] else g.scalar(host_ok)))
        if g.chance(0.15):  # an escaped name inside x: harmless only behind y AND z
            names = [n for n, _ in xm]
            at = int(rng.integers(0, len(xm) + 1))
            if not ("y" in names[:at] and "z" in names[:at]):
                g.host = True
            xm.insert(at, (g.pick(["\\u0079", "e\\\\sc", "\\u007a"]), g.pick(_JUNK_NUMS)))  # (may BE y or z: a MIN operand, so a scalar)
        if g.chance(0.1):
            xm.insert(int(rng.integers(0, len(xm) + 1)), ("x", g.obj([("y", g.junk())])))  # the same name a level down
        xv = g.obj(xm) if xm else g.pick(["{}", "{ }"])
    # a.b.c.d: four steps
    r = rng.random() if not full else rng.random() * 0.85
    if r < 0.5:
        av = g.obj([("b", g.obj([("c", g.obj([("d", g.scalar(host_ok))]))]))])
    elif r < 0.7:
        av = g.obj([("b", g.obj([("c", g.pick(["7", "[]", '"c"']))])), ("b", g.junk())])
    elif r < 0.85:
        av = g.obj([("a", "1"), ("b", g.obj([("b", "2"), ("c", g.obj([("c", "3"), ("d", g.scalar(host_ok)), ("d", g.junk())])), ("c", "4")]))])
    else:
        av = None
    wanted = [("id", '"d%d"' % i)]
    if full or g.chance(0.85):
        wanted.append(("s", g.scalar(host_ok)))
    if full or g.chance(0.85):
        wanted.append(("price", g.scalar(host_ok)))
    if full or g.chance(0.7):
        if host_ok and g.chance(0.3):
            g.host = True  # an array / object value of a wanted path
            wanted.append(("o", g.pick(['[1, 2.50, {"k": "v", "a": null}]', '{"b": 1.0, "a": [ ], "b": "last"}', "[]", "{}", '["\\u00e9"]'])))
        else:
            wanted.append(("o", g.scalar(host_ok)))
    if have_x:
        wanted.append(("x", xv))
    if full or g.chance(0.6):
        wanted.append(("w", g.obj([("k", g.junk()), ("y", g.scalar(host_ok)), ("y", g.junk())]) if g.chance(0.8)
                       else g.pick(["5", "[1, 2]", '"w"', "null", "{}", '[{"y": 1}]'])))
    if av is not None:
        wanted.append(("a", av))
    if full or g.chance(0.7):
        wanted.append(("t", g.pick(["true", "false", "null", "1", '"t"'])))
    order = list(rng.permutation(len(wanted)))
    top = [wanted[j] for j in order]
    # prefix / extension names, skipped subtrees that hold wanted names, duplicates of found names
    for _ in range(int(rng.integers(0, 4))):
        top.insert(int(rng.integers(0, len(top) + 1)), (g.pick(["pri", "prices", "pric", "ss", "xx", "i", "idd", "junk", "pad", ""]), g.junk()))
    for _ in range(int(rng.integers(0, 3))):
        j = int(rng.integers(0, len(top)))
        top.insert(int(rng.integers(j + 1, len(top) + 1)), (top[j][0], g.junk()))  # behind the first: never looked at
    if g.chance(0.12):  # an escaped name at the top level: harmless only behind every wanted name
        at = int(rng.integers(0, len(top) + 1)) if not full or g.chance(0.4) else len(top)
        seen = {n for n, _ in top[:at]}
        if not all(p[0] in seen for p in STRUCT_PATHS):
            g.host = True
        top.insert(at, (g.pick(["\\u0073", "na\\\"me", "\\u006f", "t\\tb"]), g.junk()))
    text = g.sp() + g.obj(top) + g.sp()
    return text.encode(), not g.host


def structure_docs(seed: int, n: int) -> Tuple[List[bytes], List[bool]]:
    rng = np.random.default_rng(7000 + seed)
    docs, labels = [], []
    for i in range(n):
        d, dev = structure_doc(i, rng)
        docs.append(d)
        labels.append(dev)
    return docs, labels


def padded_doc(i: int, size: int, tail: str = ', "s": "v", "x": {"y": 1.5}') -> bytes:
    """{"id": "d<i>", "pad": "ppp…"<tail>} of exactly `size` bytes"""
    head = '{"id": "d%d", "pad": "' % i
    rest = '"' + tail + "}"
    n = size - len(head) - len(rest)
    assert n >= 0, size
    return (head + "p" * n + rest).encode()
