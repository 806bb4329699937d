"""LIKE yardstick shared by tests/test_like_cpu.py and tests/test_gpu_like.py.

`like_mirror` restates the reference's likeCompile (expression/comp_like.go:124-149) step by step in Python's `re`:
QuoteMeta over the pattern, the `\\_|\\%|_|%` replacement over the QUOTED text, `^` / `$` by the first / last character
of the REPLACED text, flags m and s, and a search.  What the matchers of the library are compared with.
"""
from __future__ import annotations

import ctypes as C
import functools
import random
import re
from typing import List, Sequence, Tuple

import numpy as np

from query_amd import _ffi

_GO_META = set("\\.+*?()|[]{}^$")  # regexp.QuoteMeta's special characters
_REPL = re.compile(r"\\_|\\%|_|%")
_REPLACER = {"\\_": "_", "\\%": "%", "_": "(.)", "%": "(.*)"}  # comp_like.go:162-175


@functools.lru_cache(maxsize=None)
def like_regex(pattern: str):
    s = "".join("\\" + c if c in _GO_META else c for c in pattern)
    s = _REPL.sub(lambda m: _REPLACER[m.group(0)], s)
    if s != "" and s[0] != "%" and s[0] != "_":
        s = "^" + s
    if len(s) > 0 and s[-1] != "%" and s[-1] != "_":
        s = s + "$"
    return re.compile(s, re.M | re.S)


def like_mirror(string: str, pattern: str) -> bool:
    return like_regex(pattern).search(string) is not None


MISSING = object()


def like4(value, pattern: str):
    """Like.Apply (comp_like.go:68-88) with a STRING constant pattern: MISSING, None (NULL) for a non-string, else a bool."""
    if value is MISSING:
        return MISSING
    if not isinstance(value, str):
        return None
    return like_mirror(value, pattern)


# a small alphabet that makes matches common and holds every character class the rules speak of
LETTERS = ["a", "b"]
OTHERS = ["\\", "\n", ".", "*", "(", "[", "^", "$", "é", "\U0001F600", "%", "_"]
PATTERN_TOKENS = LETTERS * 3 + ["%", "%", "_", "_", "\\%", "\\_", "\\", "\\\\", "\n", ".", "*", "(", "[", "^", "$", "é", "\U0001F600"]
STRING_CHARS = LETTERS * 6 + OTHERS


def random_pattern(rng: random.Random) -> str:
    toks = [rng.choice(PATTERN_TOKENS) for _ in range(rng.randint(0, 8))]
    if toks and rng.random() < 0.15:
        toks[-1] = rng.choice(["\\%", "\\_"])  # escaped wildcards at the end: no end anchor
    return "".join(toks)


def _instance(rng: random.Random, pattern: str) -> str:
    """A string the pattern is likely to match: wildcards filled in, escapes dropped, sometimes on a line of its own."""
    out = []
    i = 0
    while i < len(pattern):
        c = pattern[i]
        if c == "\\" and i + 1 < len(pattern) and pattern[i + 1] in "%_":
            out.append(pattern[i + 1])
            i += 2
            continue
        if c == "%":
            out.append("".join(rng.choice(STRING_CHARS) for _ in range(rng.randint(0, 3))))
        elif c == "_":
            out.append(rng.choice(STRING_CHARS))
        else:
            out.append(c)
        i += 1
    s = "".join(out)
    r = rng.random()
    if r < 0.15:
        s = rng.choice(["x", "", "ab"]) + "\n" + s
    elif r < 0.3:
        s = s + "\n" + rng.choice(["y", "", "ab"])
    elif r < 0.4:
        s = s + rng.choice(STRING_CHARS)
    elif r < 0.5:
        s = rng.choice(STRING_CHARS) + s
    return s


def random_pairs(seed: int, n: int) -> List[Tuple[str, str]]:
    rng = random.Random(seed)
    pairs = []
    for _ in range(n):
        p = random_pattern(rng)
        if rng.random() < 0.6:
            s = _instance(rng, p)
        else:
            s = "".join(rng.choice(STRING_CHARS) for _ in range(rng.randint(0, 10)))
        pairs.append((p, s))
    return pairs


def pack(strings: Sequence[bytes]):
    offs = np.zeros(len(strings) + 1, dtype=np.uint64)
    if strings:
        offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    return offs, b"".join(strings) + b"\0"


def host_match(pattern: bytes, strings: Sequence[bytes]) -> np.ndarray:
    """n1k_like_match over a block of strings; raises on a status other than N1K_OK."""
    offs, blob = pack(strings)
    out = np.full(max(len(strings), 1), 7, dtype=np.uint8)
    st = _ffi.lib().n1k_like_match(pattern, len(pattern), len(strings), offs.ctypes.data, blob, out.ctypes.data)
    if st != _ffi.OK:
        raise RuntimeError("n1k_like_match: status %d" % st)
    return out[:len(strings)]


def device_match(pattern: bytes, strings: Sequence[bytes], device: int = 0):
    """n1k_like_match_device: (bits, strings left to the host matcher)."""
    offs, blob = pack(strings)
    out = np.full(max(len(strings), 1), 7, dtype=np.uint8)
    left = C.c_uint64(0)
    st = _ffi.lib().n1k_like_match_device(device, pattern, len(pattern), len(strings), offs.ctypes.data, blob, out.ctypes.data,
                                          C.byref(left))
    if st != _ffi.OK:
        raise RuntimeError("n1k_like_match_device: status %d" % st)
    return out[:len(strings)], int(left.value)


def by_pattern(pairs):
    """(pattern, string) pairs grouped by pattern, order kept: [(pattern, [index...])]."""
    groups = {}
    for i, (p, _) in enumerate(pairs):
        groups.setdefault(p, []).append(i)
    return list(groups.items())
