// n1k_matchtable.hip — the match table's kernels (gfx950): a predicate over a block of dictionary entries, evaluated once
// per distinct entry into one byte per entry.  The scan kernels then test one bit per row.
//
// One skeleton, the shape json_extract_kernel established: a wave owns 64 consecutive entries, copies the bytes they span
// into its LDS slab with coalesced word loads, then one lane per entry walks its own text there.  An entry longer than the
// matcher's kMaxLen bytes is flagged for the host.  A wave whose 64 entries span more than its slab (some entry beyond the
// limit sits among them) reads the entries it does take straight from global memory.
//
// A matcher says what is evaluated — with the very code the host runs, so the two agree by construction:
//   LikeMatcher (like_match_kernel): like_match (n1k_like.h) per pattern, bit p = pattern p.  Every entry is its business.
//     A string that is not valid UTF-8 is flagged for the host (Go then decodes byte by byte, which only the host does).
//   CollMatcher (coll_match_kernel): coll_eval<false> (n1k_coll.h) per predicate, bit first_bit - q = predicate q.  An entry
//     that is no array text (coll_array_text) gets no bit and is not the host's either: no row with tag ARRAY reads it.  An
//     array on which the evaluator met what only the host does (an escaped string under a comparison, a number beyond the
//     exact conversions, a string under LIKE that is not valid UTF-8) is flagged for the host.
//   InMatcher (in_match_kernel): in_lookup (n1k_in.h) — hash the entry's bytes, probe the plan's table of IN-list string
//     constants, compare the candidate's bytes — gives the mask of the lists that hold the entry.  Every entry is its
//     business; bytes are bytes, so only an entry beyond the limit is the host's.
//   StrFnMatcher (strfn_match_kernel): strfn_eval (n1k_strfn.h) per predicate — the view {begin, end, case mode} over the
//     entry's bytes where they lie, no copy — bit first_bit + q = predicate q.  Every entry is its business.  An entry
//     that holds one of the four runes with an ASCII case mapping under the matching case step, or that is not valid UTF-8
//     under LIKE (strfn_needs_host), is flagged for the host.
#include <hip/hip_runtime.h>
#include "n1k_coll.h"
#include "n1k_in.h"
#include "n1k_strfn.h"

namespace n1k {

constexpr uint32_t kMatchBlock = 256, kMatchWaves = kMatchBlock / 64;

struct LikeMatcher {
    using Args = LikeKernelArgs;
    using Params = LikeDevPatterns;
    static constexpr uint32_t kMaxLen = kLikeDevMaxLen;
    static __device__ void stage(Params& pat, const Args& A, uint32_t tid) {
        const uint32_t* src = (const uint32_t*)&A.pat;
        uint32_t* dst = (uint32_t*)&pat;
        for (uint32_t k = tid; k < sizeof(LikeDevPatterns) / 4; k += kMatchBlock) dst[k] = src[k];
    }
    static __device__ bool wants(const uint8_t*, uint64_t) { return true; }
    static __device__ uint8_t match(const Params& pat, const Args&, const uint8_t* s, uint32_t len, bool& left) {
        uint8_t bits = 0;
        if (!like_utf8_valid(s, len)) left = true;
        else {
            const LikeBytes t{s, len};
            for (uint32_t p = 0; p < pat.npat; p++)
                bits |= (uint8_t)(like_match(pat.prog[p], pat.plen[p], pat.anchor_end[p] != 0, t) ? 1u << p : 0u);
        }
        return bits;
    }
};

struct CollMatcher {
    using Args = CollKernelArgs;
    struct Params { CollProg progs[kMatchBits]; };
    static constexpr uint32_t kMaxLen = kCollDevMaxLen;
    static __device__ void stage(Params& par, const Args& A, uint32_t tid) {
        const uint32_t* src = (const uint32_t*)A.progs;
        uint32_t* dst = (uint32_t*)&par.progs[0];
        for (uint32_t k = tid; k < A.nprog * (uint32_t)(sizeof(CollProg) / 4); k += kMatchBlock) dst[k] = src[k];
    }
    static __device__ bool wants(const uint8_t* s, uint64_t len) { return coll_array_text(s, len); }
    static __device__ uint8_t match(const Params& par, const Args& A, const uint8_t* s, uint32_t len, bool& left) {
        uint8_t bits = 0;
        for (uint32_t q = 0; q < A.nprog; q++)
            bits |= (uint8_t)(coll_eval<false>(par.progs[q], s, len, left) ? 1u << (A.first_bit - q) : 0u);
        return bits;
    }
};

struct InMatcher {
    using Args = InKernelArgs;
    struct Params { uint32_t none; };  // (the table is probed where it lies: a few dependent reads per entry, L2-resident)
    static constexpr uint32_t kMaxLen = kInDevMaxLen;
    static __device__ void stage(Params&, const Args&, uint32_t) {}
    static __device__ bool wants(const uint8_t*, uint64_t) { return true; }
    static __device__ uint8_t match(const Params&, const Args& A, const uint8_t* s, uint32_t len, bool&) { return in_lookup(A.tab, s, len); }
};

struct StrFnMatcher {
    using Args = StrFnKernelArgs;
    struct Params { StrFnProg progs[kMatchBits]; };
    static constexpr uint32_t kMaxLen = kStrFnDevMaxLen;
    static __device__ void stage(Params& par, const Args& A, uint32_t tid) {
        const uint32_t* src = (const uint32_t*)A.progs;
        uint32_t* dst = (uint32_t*)&par.progs[0];
        for (uint32_t k = tid; k < A.nprog * (uint32_t)(sizeof(StrFnProg) / 4); k += kMatchBlock) dst[k] = src[k];
    }
    static __device__ bool wants(const uint8_t*, uint64_t) { return true; }
    static __device__ uint8_t match(const Params& par, const Args& A, const uint8_t* s, uint32_t len, bool& left) {
        uint8_t bits = 0;
        for (uint32_t q = 0; q < A.nprog; q++) {
            if (strfn_needs_host(par.progs[q], s, len)) left = true;
            else bits |= (uint8_t)(strfn_eval(par.progs[q], s, len) ? 1u << (A.first_bit + q) : 0u);
        }
        return bits;
    }
};

template <class Matcher>
__global__ __launch_bounds__(256) void match_table_kernel(const typename Matcher::Args A) {
    constexpr uint32_t kSlab = 64 * Matcher::kMaxLen;  // bytes 64 entries within the limit span at most
    __shared__ uint32_t slab[kMatchWaves][kSlab / 4 + 4];
    __shared__ typename Matcher::Params par;
    const EntryBlockArgs& B = A.blk;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    Matcher::stage(par, A, tid);
    const uint64_t w0 = ((uint64_t)blockIdx.x * kMatchWaves + wave) * 64ull;
    const uint64_t i = w0 + lane;
    const bool valid = i < B.n;
    // unconditional loads with the mask beside them: a lane beyond the block re-reads the last entry's offsets
    const uint64_t ii = valid ? i : (uint64_t)B.n - 1;
    const uint64_t base0 = B.offsets[0];
    const uint64_t o0 = B.offsets[ii] - base0, o1 = B.offsets[ii + 1] - base0;
    const uint64_t wb = B.offsets[w0 < B.n ? w0 : B.n] - base0;
    const uint64_t we = B.offsets[w0 + 64 < B.n ? w0 + 64 : B.n] - base0;
    const uint64_t wb_al = wb & ~3ull;  // (the bytes' base is allocation aligned: whole words from here)
    const bool in_lds = we - wb <= kSlab;
    if (in_lds) {
        const uint32_t nwords = (uint32_t)((we - wb_al + 3) / 4);  // <= kSlab / 4 + 1; reads at most 3 of the spare bytes
        const uint32_t* src = (const uint32_t*)(B.bytes + wb_al);
        for (uint32_t k = lane; k < nwords; k += 64) slab[wave][k] = src[k];
    }
    __syncthreads();
    const uint64_t len64 = o1 - o0;
    const bool mine = valid && Matcher::wants(B.bytes + o0, len64);
    const bool take = mine && len64 <= Matcher::kMaxLen;
    uint8_t bits = 0;
    bool left = mine && !take;
    if (take) {
        const uint8_t* s = in_lds ? (const uint8_t*)&slab[wave][0] + (o0 - wb_al) : B.bytes + o0;
        bits = Matcher::match(par, A, s, (uint32_t)len64, left);
    }
    if (valid) {
        B.out_bits[i] = left ? (uint8_t)0 : bits;
        B.out_left[i] = left ? 1 : 0;
    }
}

constexpr auto like_match_kernel = match_table_kernel<LikeMatcher>;
constexpr auto coll_match_kernel = match_table_kernel<CollMatcher>;
constexpr auto in_match_kernel = match_table_kernel<InMatcher>;
constexpr auto strfn_match_kernel = match_table_kernel<StrFnMatcher>;

hipError_t launch_like_match(const LikeKernelArgs& A, hipStream_t st) {
    if (A.blk.n == 0) return hipSuccess;
    const uint32_t grid = (A.blk.n + kMatchBlock - 1) / kMatchBlock;
    hipLaunchKernelGGL(like_match_kernel, dim3(grid), dim3(kMatchBlock), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_coll_match(const CollKernelArgs& A, hipStream_t st) {
    if (A.blk.n == 0 || A.nprog == 0) return hipSuccess;
    if (A.nprog > kMatchBits) return hipErrorInvalidValue;
    const uint32_t grid = (A.blk.n + kMatchBlock - 1) / kMatchBlock;
    hipLaunchKernelGGL(coll_match_kernel, dim3(grid), dim3(kMatchBlock), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_in_match(const InKernelArgs& A, hipStream_t st) {
    if (A.blk.n == 0) return hipSuccess;
    if (A.tab.nconst == 0 || !A.tab.slots) return hipErrorInvalidValue;
    const uint32_t grid = (A.blk.n + kMatchBlock - 1) / kMatchBlock;
    hipLaunchKernelGGL(in_match_kernel, dim3(grid), dim3(kMatchBlock), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_strfn_match(const StrFnKernelArgs& A, hipStream_t st) {
    if (A.blk.n == 0 || A.nprog == 0) return hipSuccess;
    if (A.nprog > kMatchBits || A.first_bit + A.nprog > kMatchBits || !A.progs) return hipErrorInvalidValue;
    const uint32_t grid = (A.blk.n + kMatchBlock - 1) / kMatchBlock;
    hipLaunchKernelGGL(strfn_match_kernel, dim3(grid), dim3(kMatchBlock), 0, st, A);
    return hipGetLastError();
}

}  // namespace n1k
