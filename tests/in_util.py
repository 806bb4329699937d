"""IN yardstick shared by tests/test_in_cpu.py and tests/test_gpu_in.py.

`in4` restates In.Apply (expression/coll_in.go:61-91) over python values.  The oracle has no IN, but for a non-empty list
the term equals the 4-valued `((x = c1) or (x = c2) or ...)`, which it evaluates: `expand` writes that form, and
tests/test_in_cpu.py checks the two against each other on a table with every tag before anything relies on it.
"""
from __future__ import annotations

import ctypes as C
import json
from typing import Sequence

import numpy as np

from like_util import MISSING, pack  # noqa: F401  (the same sentinel, the same packing)
from query_amd import _ffi, plan

IN_MAX_STRINGS = 4096  # distinct strings of one list (include/n1k.h)
IN_MAX_NUMBERS = 1024  # distinct numbers in the lists of one plan
DEV_MAX_LEN = 128      # bytes of a string in_match_kernel takes


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def equals(x, c) -> bool:
    """x.Equals(c) of two valued scalars: FALSE across type classes; two INTs exactly, any other pair of numbers through
    float64; strings bytewise; an ARRAY / OBJECT (a list / dict here) never equals a scalar."""
    if isinstance(x, bool) or isinstance(c, bool):
        return isinstance(x, bool) and isinstance(c, bool) and x == c
    if _number(x) and _number(c):
        if isinstance(x, int) and isinstance(c, int):
            return x == c
        return float(x) == float(c)
    if isinstance(x, str) and isinstance(c, str):
        return x.encode() == c.encode()
    return False


def fold(c):
    """A constant as the parser builds it: a float64 literal with an integral value inside int64 is an INT (NewValue,
    value/value.go:375-382) — `3.0` and `3e0` are the INT 3."""
    if isinstance(c, float) and c == c and abs(c) < 2.0 ** 63 and c == int(c):
        return int(c)
    return c


def in4(value, constants: Sequence):
    """In.Apply with a constant list: MISSING, None (NULL), True or False."""
    constants = [fold(c) for c in constants]
    if value is MISSING:
        return MISSING
    if len(constants) == 0:
        return False
    if value is None:
        return None
    if any(c is not None and equals(value, c) for c in constants):
        return True
    return None if any(c is None for c in constants) else False


def matcher(constants: Sequence):
    """in4 for one list as a function of the value, by sets: for lists too long to walk per row (test_in_cpu.py checks it
    against in4)."""
    constants = [fold(c) for c in constants]
    strs = {c for c in constants if isinstance(c, str)}
    bools = {c for c in constants if isinstance(c, bool)}
    ints = {c for c in constants if _number(c) and isinstance(c, int)}
    floats = {float(c) for c in constants if _number(c)}            # every number through float64
    fonly = {c for c in constants if isinstance(c, float)}
    has_null, empty = any(c is None for c in constants), len(constants) == 0

    def f(v):
        if v is MISSING:
            return MISSING
        if empty:
            return False
        if v is None:
            return None
        if isinstance(v, bool):
            hit = v in bools
        elif isinstance(v, str):
            hit = v in strs
        elif isinstance(v, int):
            hit = v in ints or float(v) in fonly
        elif isinstance(v, float):
            hit = v in floats
        else:
            hit = False
        return True if hit else (None if has_null else False)
    return f


def const_text(c, negative_in_parentheses=False) -> str:
    if isinstance(c, (str, bool)) or c is None:
        return json.dumps(c, ensure_ascii=False)
    t = repr(c) if isinstance(c, float) else str(c)
    return "(%s)" % t if negative_in_parentheses and t.startswith("-") else t


def term(path: str, constants: Sequence, folded=False) -> str:
    """The device's text: `(path in ["a", 3])` as the ArrayConstruct stringer writes it, or with the JSON of a folded
    constant `["a",3]`."""
    if folded:
        return "(%s in [%s])" % (path, ",".join(const_text(c) for c in constants))
    return plan.in_list(path, constants)


def expand(path: str, constants: Sequence) -> str:
    """The oracle's text: the OR of equalities (non-empty lists only)."""
    assert len(constants) > 0
    eqs = ["(%s = %s)" % (path, const_text(c)) for c in constants]
    return eqs[0] if len(eqs) == 1 else "(%s)" % " or ".join(eqs)


def list_text(strings: Sequence[bytes]) -> bytes:
    """A bracketed list of STRING constants holding exactly these bytes: control bytes, the quote and the backslash as
    \\u00XX; bytes from 0x80 on go in raw (an escape would turn them into two), which the parser takes as they are."""
    out = []
    for s in strings:
        b = bytearray()
        for ch in s:
            if ch in (0x22, 0x5C) or ch < 0x20:
                b += b"\\u%04x" % ch
            else:
                b.append(ch)
        out.append(b'"' + bytes(b) + b'"')
    return b"[" + b", ".join(out) + b"]"


def host_match(text: bytes, strings: Sequence[bytes]) -> np.ndarray:
    """n1k_in_match over a block of strings; raises on a status other than N1K_OK."""
    offs, blob = pack(strings)
    out = np.full(max(len(strings), 1), 7, dtype=np.uint8)
    st = _ffi.lib().n1k_in_match(text, len(text), len(strings), offs.ctypes.data, blob, out.ctypes.data)
    if st != _ffi.OK:
        raise RuntimeError("n1k_in_match: status %d" % st)
    return out[:len(strings)]


def device_match(text: bytes, strings: Sequence[bytes], device: int = 0):
    """n1k_in_match_device: (bits, strings left to the host matcher)."""
    offs, blob = pack(strings)
    out = np.full(max(len(strings), 1), 7, dtype=np.uint8)
    left = C.c_uint64(0)
    st = _ffi.lib().n1k_in_match_device(device, text, len(text), len(strings), offs.ctypes.data, blob, out.ctypes.data, C.byref(left))
    if st != _ffi.OK:
        raise RuntimeError("n1k_in_match_device: status %d" % st)
    return out[:len(strings)], int(left.value)


def tag_of(r, n1o):
    """A 4-valued result as the tag of an oracle helper column."""
    return n1o.T_MISSING if r is MISSING else (n1o.T_NULL if r is None else (n1o.T_TRUE if r else n1o.T_FALSE))
