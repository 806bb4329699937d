// n1k_like.hip — LIKE over a block of dictionary entries on the device (gfx950): one match per distinct string and
// pattern, written as one byte per string (bit p = pattern p).  The scan kernels then test one bit per row.
//
// The shape json_extract_kernel established: a wave owns 64 consecutive strings, copies the bytes they span into its LDS
// slab with coalesced word loads, then one lane per string walks its own text there with like_match (n1k_like.h — the
// very code the host matcher runs, so the two agree by construction).  A string longer than kLikeDevMaxLen bytes, or one
// that is not valid UTF-8 (Go then decodes byte by byte, which only the host matcher does), is flagged for the host.
// A wave whose 64 strings span more than its slab (some string beyond the limit sits among them) reads the strings it
// does take straight from global memory.
#include <hip/hip_runtime.h>
#include "n1k_like.h"

namespace n1k {

constexpr uint32_t kLikeBlock = 256, kLikeWaves = kLikeBlock / 64;
constexpr uint32_t kLikeSlab = 64 * kLikeDevMaxLen;  // bytes 64 strings within the limit span at most

__global__ __launch_bounds__(256) void like_match_kernel(const LikeKernelArgs A) {
    __shared__ uint32_t slab[kLikeWaves][kLikeSlab / 4 + 4];
    __shared__ LikeDevPatterns pat;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    {
        const uint32_t* src = (const uint32_t*)&A.pat;
        uint32_t* dst = (uint32_t*)&pat;
        for (uint32_t k = tid; k < sizeof(LikeDevPatterns) / 4; k += kLikeBlock) dst[k] = src[k];
    }
    const uint64_t w0 = ((uint64_t)blockIdx.x * kLikeWaves + wave) * 64ull;
    const uint64_t i = w0 + lane;
    const bool valid = i < A.n;
    // unconditional loads with the mask beside them: a lane beyond the block re-reads the last string's offsets
    const uint64_t ii = valid ? i : (uint64_t)A.n - 1;
    const uint64_t base0 = A.offsets[0];
    const uint64_t o0 = A.offsets[ii] - base0, o1 = A.offsets[ii + 1] - base0;
    const uint64_t wb = A.offsets[w0 < A.n ? w0 : A.n] - base0;
    const uint64_t we = A.offsets[w0 + 64 < A.n ? w0 + 64 : A.n] - base0;
    const uint64_t wb_al = wb & ~3ull;  // (the bytes' base is allocation aligned: whole words from here)
    const bool in_lds = we - wb <= kLikeSlab;
    if (in_lds) {
        const uint32_t nwords = (uint32_t)((we - wb_al + 3) / 4);  // <= kLikeSlab / 4 + 1; reads at most 3 of the spare bytes
        const uint32_t* src = (const uint32_t*)(A.bytes + wb_al);
        for (uint32_t k = lane; k < nwords; k += 64) slab[wave][k] = src[k];
    }
    __syncthreads();
    const uint64_t len64 = o1 - o0;
    const bool take = valid && len64 <= kLikeDevMaxLen;
    uint8_t bits = 0, left = valid && !take ? 1 : 0;
    if (take) {
        const uint32_t len = (uint32_t)len64;
        const uint8_t* s = in_lds ? (const uint8_t*)&slab[wave][0] + (o0 - wb_al) : A.bytes + o0;
        if (!like_utf8_valid(s, len)) left = 1;
        else {
            const LikeBytes t{s, len};
            for (uint32_t p = 0; p < pat.npat; p++)
                bits |= (uint8_t)(like_match(pat.prog[p], pat.plen[p], pat.anchor_end[p] != 0, t) ? 1u << p : 0u);
        }
    }
    if (valid) {
        A.out_bits[i] = bits;
        A.out_left[i] = left;
    }
}

hipError_t launch_like_match(const LikeKernelArgs& A, hipStream_t st) {
    if (A.n == 0) return hipSuccess;
    const uint32_t grid = (A.n + kLikeBlock - 1) / kLikeBlock;
    hipLaunchKernelGGL(like_match_kernel, dim3(grid), dim3(kLikeBlock), 0, st, A);
    return hipGetLastError();
}

}  // namespace n1k
