// n1k_like.h — LIKE (expression/comp_like.go): the pattern program and the matcher both the host and the device run.
//
// The reference rewrites a pattern into a Go regexp (likeCompile, comp_like.go:124-149) and asks MatchString.  The
// same language without regexps, including what the rewrite does by accident:
//   %  any run of characters, _ exactly one; a character is a UTF-8 code point, both match '\n' (flag s);
//   a backslash right before % or _ makes it an ordinary character and is dropped; every other backslash — also one
//   before another backslash — is an ordinary character; regexp metacharacters are ordinary (QuoteMeta);
//   the empty pattern matches everything; a non-empty one is anchored at its start, which with flag m is offset 0 or
//   right after any '\n', and at its end (end of string or right before any '\n') UNLESS it ends in \% or \_ (the
//   rewrite looks at the last byte of the REPLACED text, and only an escaped wildcard leaves % or _ there).
//
// A pattern compiles once into a byte program:  OP_MANY | OP_ONE | OP_LIT len byte*len  (len <= 255), plus the end anchor
// flag.  Between two MANYs only literals and fixed-width ONEs occur, so placing every such segment at its leftmost
// position is exact: a segment covers a fixed number of characters, hence "starts earlier" is "ends earlier".  The first
// segment is tried at every start of a line, the last one has to end at an end of a line.
//
// like_match<Text> is the one algorithm; Text says what a position is: bytes of valid UTF-8 (device and host) or
// decoded code points (host only: Go decodes every byte that does not begin a valid encoding as ONE character, U+FFFD).
#pragma once
#include "n1k_types.h"

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define N1K_HD __host__ __device__ inline
#else
#define N1K_HD inline
#endif

namespace n1k {

enum : uint8_t { LIKE_OP_MANY = 0, LIKE_OP_ONE = 1, LIKE_OP_LIT = 2 };

constexpr uint32_t kMatchBits = 8;          // bits of a match-table entry: one byte per dictionary code carries every LIKE pattern,
                                            // ANY / EVERY predicate, IN list of strings and string-function predicate of a plan ("The match table")
constexpr uint32_t kLikeDevProgBytes = 240;  // a longer program stays with the host matcher
constexpr uint32_t kLikeDevMaxLen = 128;     // bytes of a dictionary string the device kernel takes
// New dictionary entries below this count are matched on the host and copied; from it on they go through
// like_match_kernel.  Measured through the handle itself ("LIKE: measured", tools/exp_like.py route; strings
// of 29 B, three patterns): the host route costs 0.127 ms for 1 Ki new strings, 0.218 for 2 Ki, 0.41 for 4 Ki; the device
// route 0.134 ms for 4 Ki and 0.15 for 8 Ki — a fixed 0.13 ms, which the host route reaches at about 1 Ki strings.
constexpr uint32_t kLikeDeviceThreshold = 1024;

// bytes of the UTF-8 sequence a lead byte announces (valid text only)
N1K_HD uint32_t like_utf8_len(uint8_t c) { return c < 0x80 ? 1u : (c < 0xE0 ? 2u : (c < 0xF0 ? 3u : 4u)); }

// length of the valid encoding that begins at s[i], 0 if none does (unicode/utf8: no overlong forms, no surrogates,
// nothing above U+10FFFF)
N1K_HD uint32_t like_utf8_valid_at(const uint8_t* s, uint32_t n, uint32_t i) {
    const uint8_t c = s[i];
    if (c < 0x80) return 1;
    if (c < 0xC2 || c > 0xF4) return 0;
    const uint32_t len = like_utf8_len(c);
    if (i + len > n) return 0;
    const uint8_t c1 = s[i + 1];
    const uint8_t lo = c == 0xE0 ? 0xA0 : (c == 0xF0 ? 0x90 : 0x80), hi = c == 0xED ? 0x9F : (c == 0xF4 ? 0x8F : 0xBF);
    if (c1 < lo || c1 > hi) return 0;
    for (uint32_t k = 2; k < len; k++)
        if ((s[i + k] & 0xC0) != 0x80) return 0;
    return len;
}
N1K_HD bool like_utf8_valid(const uint8_t* s, uint32_t n) {
    for (uint32_t i = 0; i < n;) {
        const uint32_t l = like_utf8_valid_at(s, n, i);
        if (!l) return false;
        i += l;
    }
    return true;
}

// valid UTF-8 as it lies in memory: a position is a byte offset on a character boundary
struct LikeBytes {
    const uint8_t* s;
    uint32_t n;
    N1K_HD uint32_t next(uint32_t p) const { return p + like_utf8_len(s[p]); }
    N1K_HD bool newline(uint32_t p) const { return s[p] == '\n'; }
    // the literal at position p: the position behind it, or 0xFFFFFFFF
    N1K_HD uint32_t lit(uint32_t p, const uint8_t* b, uint32_t len) const {
        if (len > n - p) return 0xFFFFFFFFu;
        for (uint32_t k = 0; k < len; k++)
            if (s[p + k] != b[k]) return 0xFFFFFFFFu;
        return p + len;
    }
};

// end of the segment that begins at program offset pi (the next MANY, or the end of the program)
N1K_HD uint32_t like_seg_end(const uint8_t* prog, uint32_t plen, uint32_t pi) {
    while (pi < plen && prog[pi] != LIKE_OP_MANY) pi += prog[pi] == LIKE_OP_ONE ? 1u : 2u + prog[pi + 1];
    return pi;
}

// the segment prog[pi, se) at position p: the position behind it, or 0xFFFFFFFF
template <class Text>
N1K_HD uint32_t like_seg_at(const uint8_t* prog, uint32_t pi, uint32_t se, const Text& t, uint32_t p) {
    while (pi < se) {
        if (prog[pi] == LIKE_OP_ONE) {
            if (p >= t.n) return 0xFFFFFFFFu;
            p = t.next(p);
            pi++;
        } else {
            p = t.lit(p, prog + pi + 2, prog[pi + 1]);
            if (p == 0xFFFFFFFFu) return p;
            pi += 2u + prog[pi + 1];
        }
    }
    return p;
}

template <class Text>
N1K_HD bool like_match(const uint8_t* prog, uint32_t plen, bool anchor_end, const Text& t) {
    if (plen == 0) return true;
    const uint32_t n = t.n;
    uint32_t pi = 0, se = like_seg_end(prog, plen, 0), cur = 0;
    // first segment: at offset 0 or right after a '\n'
    for (uint32_t s0 = 0;;) {
        const uint32_t e = like_seg_at(prog, pi, se, t, s0);
        if (e != 0xFFFFFFFFu) {
            if (se < plen) {
                cur = e;
                break;
            }
            if (!anchor_end || e == n || t.newline(e)) return true;
        }
        while (s0 < n && !t.newline(s0)) s0 = t.next(s0);
        if (s0 >= n) return false;
        s0 = t.next(s0);
    }
    for (;;) {
        pi = se + 1;  // behind the MANY
        se = like_seg_end(prog, plen, pi);
        const bool last = se == plen;
        if (pi == se) {
            if (last) return true;  // a trailing MANY runs to the end of the string
            continue;
        }
        bool found = false;
        for (uint32_t p = cur;; p = t.next(p)) {
            const uint32_t e = like_seg_at(prog, pi, se, t, p);
            if (e != 0xFFFFFFFFu) {
                if (!last) {
                    cur = e;
                    found = true;
                    break;
                }
                if (!anchor_end || e == n || t.newline(e)) return true;
            }
            if (p >= n) break;
        }
        if (!found) return false;
    }
}

// the patterns of one plan as the device kernel takes them (a kernel argument)
struct LikeDevPatterns {
    uint32_t npat;
    uint8_t plen[kMatchBits];
    uint8_t anchor_end[kMatchBits];
    uint8_t prog[kMatchBits][kLikeDevProgBytes];
};

// a block of dictionary entries as the match table's kernels take it (n1k_matchtable.hip), whatever they evaluate
struct EntryBlockArgs {
    const uint8_t* bytes;     // the entries' bytes back to back (+ 16 spare bytes)
    const uint64_t* offsets;  // n + 1; entry i = bytes[offsets[i] - offsets[0], offsets[i + 1] - offsets[0])
    uint32_t n, pad;
    uint8_t* out_bits;        // n bytes: the matcher's bits of entry i (0 for an entry that is not its business or left to the host)
    uint8_t* out_left;        // n bytes: 1 = left to the host (longer than the matcher's limit, or what only the host does)
};

struct LikeKernelArgs {
    EntryBlockArgs blk;   // out_bits: bit p = pattern p matches; left: longer than kLikeDevMaxLen, or not valid UTF-8
    LikeDevPatterns pat;
};
static_assert(sizeof(EntryBlockArgs) == 40 && sizeof(LikeDevPatterns) == 1940 && sizeof(LikeKernelArgs) == 1984, "kernel argument layout");

}  // namespace n1k

#if !defined(__HIPCC_RTC__)
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

namespace n1k {

struct LikePattern {
    std::string text;           // the pattern as the plan wrote it
    std::vector<uint8_t> prog;  // the program (any length; the device takes it up to kLikeDevProgBytes)
    bool anchor_end = true;
};

// false: the pattern is not valid UTF-8 (the reference's regexp.Compile fails on it)
bool like_compile(const char* pattern, size_t len, LikePattern& out);
// one string against one pattern, any bytes (the host matcher: invalid UTF-8 decodes byte by byte, as Go does)
bool like_match_host(const LikePattern& p, const uint8_t* s, size_t n);
// Go's view of any bytes: code points, every byte that begins no valid encoding one U+FFFD; and a program over them
void like_decode_runes(const uint8_t* s, uint32_t n, std::vector<uint32_t>& out);
bool like_match_runes(const uint8_t* prog, uint32_t plen, bool anchor_end, const uint32_t* r, uint32_t n);
// bits[i] |= OR over patterns p of (match << p), for the n strings bytes[offsets[i] - offsets[0] ..)
void like_match_block_host(const std::vector<LikePattern>& pats, uint64_t n, const uint64_t* offsets, const uint8_t* bytes, uint8_t* bits);
// false: some pattern's program is longer than the device kernel takes
bool like_dev_patterns(const std::vector<LikePattern>& pats, LikeDevPatterns& out);
hipError_t launch_like_match(const LikeKernelArgs& A, hipStream_t st);

}  // namespace n1k
#endif
