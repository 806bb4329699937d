// n1k_coll.hip — ANY / EVERY over a block of dictionary entries on the device (gfx950): one evaluation per distinct array
// and predicate, written as one byte per entry (bit first_bit - q = predicate q).  The scan kernels then test one bit per row.
//
// like_match_kernel's shape: a wave owns 64 consecutive entries, copies the bytes they span into its LDS slab with
// coalesced word loads, then one lane per entry walks its own text there with coll_eval<false> (n1k_coll.h — the code the
// host evaluator runs, so the two agree by construction).  An entry that is no array text ('[' first) gets no bit and is
// not the host's either: no row with tag ARRAY reads it.  An array longer than kCollDevMaxLen bytes is flagged for the host,
// and so is one on which the evaluator met what only the host does (an escaped string under a comparison, a number beyond
// the exact conversions, a string under LIKE that is not valid UTF-8).  A wave whose 64 entries span more than its slab
// reads the entries it does take straight from global memory.
#include <hip/hip_runtime.h>
#include "n1k_coll.h"

namespace n1k {

constexpr uint32_t kCollBlock = 256, kCollWaves = kCollBlock / 64;
constexpr uint32_t kCollSlab = 64 * kCollDevMaxLen;  // bytes 64 entries within the limit span at most

__global__ __launch_bounds__(256) void coll_match_kernel(const CollKernelArgs A) {
    __shared__ uint32_t slab[kCollWaves][kCollSlab / 4 + 4];
    __shared__ CollProg progs[kLikeMaxPatterns];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    {
        const uint32_t* src = (const uint32_t*)A.progs;
        uint32_t* dst = (uint32_t*)&progs[0];
        for (uint32_t k = tid; k < A.nprog * (uint32_t)(sizeof(CollProg) / 4); k += kCollBlock) dst[k] = src[k];
    }
    const uint64_t w0 = ((uint64_t)blockIdx.x * kCollWaves + wave) * 64ull;
    const uint64_t i = w0 + lane;
    const bool valid = i < A.n;
    // unconditional loads with the mask beside them: a lane beyond the block re-reads the last entry's offsets
    const uint64_t ii = valid ? i : (uint64_t)A.n - 1;
    const uint64_t base0 = A.offsets[0];
    const uint64_t o0 = A.offsets[ii] - base0, o1 = A.offsets[ii + 1] - base0;
    const uint64_t wb = A.offsets[w0 < A.n ? w0 : A.n] - base0;
    const uint64_t we = A.offsets[w0 + 64 < A.n ? w0 + 64 : A.n] - base0;
    const uint64_t wb_al = wb & ~3ull;  // (the bytes' base is allocation aligned: whole words from here)
    const bool in_lds = we - wb <= kCollSlab;
    if (in_lds) {
        const uint32_t nwords = (uint32_t)((we - wb_al + 3) / 4);  // <= kCollSlab / 4 + 1; reads at most 3 of the spare bytes
        const uint32_t* src = (const uint32_t*)(A.bytes + wb_al);
        for (uint32_t k = lane; k < nwords; k += 64) slab[wave][k] = src[k];
    }
    __syncthreads();
    const uint64_t len64 = o1 - o0;
    const bool array = valid && len64 >= 2 && A.bytes[o0] == '[';
    const bool take = array && len64 <= kCollDevMaxLen;
    uint8_t bits = 0;
    bool left = array && !take;
    if (take) {
        const uint32_t len = (uint32_t)len64;
        const uint8_t* s = in_lds ? (const uint8_t*)&slab[wave][0] + (o0 - wb_al) : A.bytes + o0;
        for (uint32_t q = 0; q < A.nprog; q++)
            bits |= (uint8_t)(coll_eval<false>(progs[q], s, len, left) ? 1u << (A.first_bit - q) : 0u);
    }
    if (valid) {
        A.out_bits[i] = left ? (uint8_t)0 : bits;
        A.out_left[i] = left ? 1 : 0;
    }
}

hipError_t launch_coll_match(const CollKernelArgs& A, hipStream_t st) {
    if (A.n == 0 || A.nprog == 0) return hipSuccess;
    if (A.nprog > kLikeMaxPatterns) return hipErrorInvalidValue;
    const uint32_t grid = (A.n + kCollBlock - 1) / kCollBlock;
    hipLaunchKernelGGL(coll_match_kernel, dim3(grid), dim3(kCollBlock), 0, st, A);
    return hipGetLastError();
}

}  // namespace n1k
