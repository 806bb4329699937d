"""ANY / EVERY yardstick shared by tests/test_coll_cpu.py and tests/test_gpu_coll.py.

`coll_mirror` restates, over `json.loads` values, what the reference does for a collection predicate with one binding,
`in`, no name variable: collEval (expression/coll_util.go:17-120) types the binding value — MISSING gives MISSING, anything
but an ARRAY gives NULL (an OBJECT too: no name variable, no descend) — then Any / Every / AnyEvery.Evaluate
(coll_any.go:42-85, coll_every.go:42-85, coll_any_every.go:42-85) evaluate the SATISFIES condition once per element and
fold its Truth(): ANY is TRUE at the first hit, EVERY is FALSE at the first miss, an empty array makes ANY FALSE and EVERY
TRUE, ANY AND EVERY is EVERY but `n > 0` at the end.  The leaves follow value.Equals / Compare (value/integer.go:68-130,
float.go:74-184, string.go:82-142, boolean.go), Between.Apply (comp_between.go:58-78), Like.Apply (like_util.like4), the IS
predicates (comp_null.go, comp_missing.go, comp_valued.go) and And / Or / Not.Apply (logic_and.go:64-89, logic_or.go:98-123,
logic_not.go:57-69).  A field of an element that is no object, or lacks the name, is MISSING (nav_field.go).

A condition is a small tree of tuples; `term_text` writes it as expression/stringer.go does (GT / GE arrive as LT / LE with
the operands swapped, NE as NOT of EQ), which is the text n1k_create and n1k_coll_eval take.
"""
from __future__ import annotations

import ctypes as C
import json
import random
from decimal import Decimal
from typing import List, Sequence

import numpy as np

import like_util as lu
from query_amd import _ffi

MISSING = lu.MISSING
ANY, EVERY, ANY_EVERY = "any", "every", "any and every"


# ---------------------------------------------------------------- values

def norm(v):
    """json.loads value -> value.NewValue's typing: an integer literal beyond int64 is a float64, a float64 without a
    fraction that fits int64 is an int (value/value.go:375-382)."""
    if isinstance(v, bool) or v is None or isinstance(v, str):
        return v
    if isinstance(v, int):
        if -2 ** 63 <= v < 2 ** 63:
            return v
        v = float(v)
    if isinstance(v, float):
        if -9223372036854775808.0 <= v < 9223372036854775808.0 and v == int(v):
            return int(v)
        return v
    if isinstance(v, list):
        return [norm(x) for x in v]
    return {k: norm(x) for k, x in v.items()}


def _quote(s: str) -> str:
    out = ['"']
    for ch in s:
        if ch == '"':
            out.append('\\"')
        elif ch == "\\":
            out.append("\\\\")
        elif ch == "\n":
            out.append("\\n")
        elif ch == "\r":
            out.append("\\r")
        elif ch == "\t":
            out.append("\\t")
        elif ch == "\b":
            out.append("\\b")
        elif ch == "\f":
            out.append("\\f")
        elif ord(ch) < 0x20:
            out.append("\\u%04x" % ord(ch))
        else:
            out.append(ch)
    out.append('"')
    return "".join(out)


def canon(v) -> str:
    """Canonical JSON text as the library's dictionary holds it (value/object.go:30-78 MarshalJSON: compact, names sorted;
    value/float.go:31-48: a float in positional notation with the shortest digits that round-trip)."""
    v = norm(v)
    if v is None:
        return "null"
    if v is True:
        return "true"
    if v is False:
        return "false"
    if isinstance(v, int):
        return str(v)
    if isinstance(v, float):
        return format(Decimal(repr(v)), "f")
    if isinstance(v, str):
        return _quote(v)
    if isinstance(v, list):
        return "[" + ",".join(canon(x) for x in v) + "]"
    return "{" + ",".join(_quote(k) + ":" + canon(v[k]) for k in sorted(v, key=lambda k: k.encode())) + "}"


def _cls(v) -> int:
    if v is MISSING:
        return 0
    if v is None:
        return 1
    if isinstance(v, bool):
        return 2
    if isinstance(v, (int, float)):
        return 3
    if isinstance(v, str):
        return 4
    return 5 if isinstance(v, list) else 6


def _collate(a, b) -> int:
    """X.Collate(Y), X and Y above NULL; arrays / objects only ever meet a scalar constant here (type order decides)."""
    ca, cb = _cls(a), _cls(b)
    if ca != cb:
        return -1 if ca < cb else 1
    if ca == 3:
        if isinstance(a, int) and isinstance(b, int):
            return (a > b) - (a < b)
        a, b = float(a), float(b)
        return (a > b) - (a < b)
    if ca == 4:
        a, b = a.encode(), b.encode()
    assert ca in (2, 3, 4)
    return (a > b) - (a < b)


def _equals(a, b):
    if a is MISSING or b is MISSING:
        return MISSING
    if a is None or b is None:
        return None
    if _cls(a) != _cls(b):
        return False
    return _collate(a, b) == 0


def _compare(a, b):
    """X.Compare(Y): MISSING, None (NULL) or the collation."""
    if a is MISSING or b is MISSING:
        return MISSING
    if a is None or b is None:
        return None
    return _collate(a, b)


def _and(vals):
    if any(v is False for v in vals):
        return False
    if any(v is MISSING for v in vals):
        return MISSING
    if any(v is None for v in vals):
        return None
    return True


def _or(vals):
    if any(v is True for v in vals):
        return True
    if any(v is None for v in vals):
        return None
    if any(v is MISSING for v in vals):
        return MISSING
    return False


def _resolve(elem, fields):
    v = elem
    for f in fields:
        if not isinstance(v, dict) or f not in v:
            return MISSING
        v = v[f]
    return v


# ---------------------------------------------------------------- conditions
# ("and", [c...]) ("or", [c...]) ("not", c)
# ("cmp", op, fields, constant, const_first)   op in "=", "<", "<="
# ("between", fields, lo, hi) ("like", fields, pattern) ("is", fields, "null" | "not null" | "missing" | ...)

def eval_cond(c, elem):
    k = c[0]
    if k == "and":
        return _and([eval_cond(x, elem) for x in c[1]])
    if k == "or":
        return _or([eval_cond(x, elem) for x in c[1]])
    if k == "not":
        v = eval_cond(c[1], elem)
        return (not v) if isinstance(v, bool) else v
    if k == "cmp":
        _, op, fields, const, const_first = c
        v = _resolve(elem, fields)
        a, b = (const, v) if const_first else (v, const)
        if op == "=":
            return _equals(a, b)
        r = _compare(a, b)
        if r is MISSING or r is None:
            return r
        return r < 0 if op == "<" else r <= 0
    if k == "between":
        v = _resolve(elem, c[1])
        lo, hi = _compare(v, c[2]), _compare(v, c[3])
        if lo is MISSING or hi is MISSING:
            return MISSING
        if lo is None or hi is None:
            return None
        return lo >= 0 and hi <= 0
    if k == "like":
        return lu.like4(_resolve(elem, c[1]), c[2])
    assert k == "is"
    v = _resolve(elem, c[1])
    what = c[2]
    if what == "null":
        return MISSING if v is MISSING else v is None
    if what == "not null":
        return MISSING if v is MISSING else v is not None
    if what == "missing":
        return v is MISSING
    if what == "not missing":
        return v is not MISSING
    if what == "valued":
        return v is not MISSING and v is not None
    assert what == "not valued"
    return v is MISSING or v is None


def coll_mirror(mode: str, cond, value, early_exit: bool = True):
    """MISSING / None / bool for one binding value (a json.loads value, or MISSING)."""
    if value is MISSING:
        return MISSING
    if not isinstance(value, list):
        return None
    value = norm(value)
    truths = []
    for elem in value:
        t = eval_cond(cond, elem) is True
        truths.append(t)
        if early_exit and mode == ANY and t:
            return True
        if early_exit and mode != ANY and not t:
            return False
    if mode == ANY:
        return any(truths)
    if mode == EVERY:
        return all(truths)
    return all(truths) and len(value) > 0


def _const_text(v) -> str:
    return canon(v)


def _e_text(var: str, fields) -> str:
    t = "`%s`" % var
    for f in fields:
        t = "(%s.`%s`)" % (t, f)
    return t


def cond_text(c, var: str) -> str:
    k = c[0]
    if k in ("and", "or"):
        return "(" + (" %s " % k).join(cond_text(x, var) for x in c[1]) + ")"
    if k == "not":
        return "(not %s)" % cond_text(c[1], var)
    if k == "cmp":
        _, op, fields, const, const_first = c
        a, b = _e_text(var, fields), _const_text(const)
        if const_first:
            a, b = b, a
        return "(%s %s %s)" % (a, op, b)
    if k == "between":
        return "(%s between %s and %s)" % (_e_text(var, c[1]), _const_text(c[2]), _const_text(c[3]))
    if k == "like":
        return "(%s like %s)" % (_e_text(var, c[1]), _quote(c[2]))
    return "(%s is %s)" % (_e_text(var, c[1]), c[2])


def term_text(mode: str, cond, over: str = "(`d`.`a`)", var: str = "v") -> str:
    return "%s `%s` in %s satisfies %s end" % (mode, var, over, cond_text(cond, var))


def count_nodes(c) -> int:
    """Nodes of the compiled program: an n-ary AND / OR is n - 1 binary ones."""
    if c[0] in ("and", "or"):
        return sum(count_nodes(x) for x in c[1]) + len(c[1]) - 1
    if c[0] == "not":
        return 1 + count_nodes(c[1])
    return 1


# ---------------------------------------------------------------- seeded material
# a small alphabet, so that hits are common: the same few scalars as elements, as fields and as constants
STRINGS = ["a", "b", "ab", "t_1", "", "é", 'x"y', "a\\b", "a\nb"]
PLAIN_STRINGS = ["a", "b", "ab", "t_1", "", "é"]
NUMBERS = [0, 1, 2, -1, 1.5, 2.5, 0.1, 2 ** 53 + 1, 2 ** 53, 2 ** 63, 10 ** 20, 1e-7, 123456789012345.5]
PLAIN_NUMBERS = [0, 1, 2, -1, 1.5, 2.5, 0.1, 2 ** 53 + 1, 2 ** 53]
FIELDS = ["f", "g", "h"]
PATTERNS = ["a%", "%b", "_", "t\\_1", "%", "a_", "é", ""]
IS_KINDS = ["null", "not null", "missing", "not missing", "valued", "not valued"]


def random_scalar(rng: random.Random, plain: bool = False):
    r = rng.random()
    if r < 0.4:
        return rng.choice(PLAIN_STRINGS if plain else STRINGS)
    if r < 0.75:
        return rng.choice(PLAIN_NUMBERS if plain else NUMBERS)
    return rng.choice([None, True, False])


def random_element(rng: random.Random, plain: bool = False, depth: int = 0):
    r = rng.random()
    if r < 0.55 or depth >= 2:
        return random_scalar(rng, plain)
    if r < 0.7:
        return [random_element(rng, plain, depth + 1) for _ in range(rng.randint(0, 3))]
    obj = {}
    for f in FIELDS:
        if rng.random() < 0.6:
            obj[f] = random_element(rng, plain, depth + 1)
    if rng.random() < 0.1 and not plain:
        obj['q"'] = 1  # a member name with an escape
    return obj


def random_array(rng: random.Random, plain: bool = False):
    n = rng.choice([0, 1, 1, 2, 3, 4, 6])
    return [random_element(rng, plain) for _ in range(n)]


def random_const(rng: random.Random, plain: bool = False):
    r = rng.random()
    if r < 0.45:
        return rng.choice(PLAIN_STRINGS if plain else STRINGS)
    if r < 0.85:
        return norm(rng.choice(PLAIN_NUMBERS if plain else NUMBERS))
    return rng.choice([True, False])


def random_fields(rng: random.Random):
    r = rng.random()
    if r < 0.5:
        return []
    if r < 0.85:
        return [rng.choice(FIELDS)]
    return [rng.choice(FIELDS), rng.choice(FIELDS)]


def _is_number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def random_leaf(rng: random.Random, plain: bool = False):
    """A leaf of the accepted subset: the bare variable is not ORDERED against a NUMBER constant (refused)."""
    r = rng.random()
    f = random_fields(rng)
    if r < 0.5:
        op, const = rng.choice(["=", "=", "<", "<="]), random_const(rng, plain)
        while op != "=" and not f and _is_number(const):
            const = random_const(rng, plain)
        return ("cmp", op, f, const, rng.random() < 0.4)
    if r < 0.6:
        lo, hi = random_const(rng, plain), random_const(rng, plain)
        while not f and (_is_number(lo) or _is_number(hi)):
            lo, hi = random_const(rng, plain), random_const(rng, plain)
        return ("between", f, lo, hi)
    if r < 0.8:
        return ("like", f, rng.choice(PATTERNS))
    return ("is", f, rng.choice(IS_KINDS))


def random_cond(rng: random.Random, plain: bool = False, depth: int = 0):
    r = rng.random()
    if r < 0.45 or depth >= 2:
        return random_leaf(rng, plain)
    if r < 0.6:
        return ("not", random_cond(rng, plain, depth + 1))
    return (rng.choice(["and", "or"]), [random_cond(rng, plain, depth + 1) for _ in range(rng.randint(2, 3))])


def random_term(rng: random.Random, plain: bool = False):
    """(mode, condition) within the accepted subset: at most 16 nodes."""
    while True:
        c = random_cond(rng, plain)
        if count_nodes(c) <= 16:
            return rng.choice([ANY, ANY, EVERY, ANY_EVERY]), c


def random_pairs(seed: int, nterms: int, per_term: int):
    """[(mode, cond, [array...])]: nterms seeded terms with per_term arrays each."""
    rng = random.Random(seed)
    out = []
    for _ in range(nterms):
        mode, cond = random_term(rng)
        out.append((mode, cond, [random_array(rng) for _ in range(per_term)]))
    return out


# ---------------------------------------------------------------- the library's evaluators

def host_eval(term: str, texts: Sequence[bytes]) -> np.ndarray:
    """n1k_coll_eval over a block of canonical texts; raises on a status other than N1K_OK."""
    offs, blob = lu.pack(texts)
    out = np.full(max(len(texts), 1), 7, dtype=np.uint8)
    t = term.encode()
    st = _ffi.lib().n1k_coll_eval(t, len(t), len(texts), offs.ctypes.data, blob, out.ctypes.data)
    if st != _ffi.OK:
        raise RuntimeError("n1k_coll_eval: status %d for %s" % (st, term))
    return out[:len(texts)]


def host_status(term: bytes) -> int:
    offs, blob = lu.pack([b"[]"])
    out = np.zeros(1, dtype=np.uint8)
    return _ffi.lib().n1k_coll_eval(term, len(term), 1, offs.ctypes.data, blob, out.ctypes.data)


def device_eval(term: str, texts: Sequence[bytes], device: int = 0):
    """n1k_coll_eval_device: (bits, arrays left to the host evaluator)."""
    offs, blob = lu.pack(texts)
    out = np.full(max(len(texts), 1), 7, dtype=np.uint8)
    left = C.c_uint64(0)
    t = term.encode()
    st = _ffi.lib().n1k_coll_eval_device(device, t, len(t), len(texts), offs.ctypes.data, blob, out.ctypes.data, C.byref(left))
    if st != _ffi.OK:
        raise RuntimeError("n1k_coll_eval_device: status %d for %s" % (st, term))
    return out[:len(texts)], int(left.value)


def texts_of(arrays: Sequence) -> List[bytes]:
    return [canon(a).encode() for a in arrays]


def loads(text: bytes):
    return json.loads(text.decode())
