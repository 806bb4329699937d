// n1k_arrfn.hip — the array functions' kernels (gfx950) and, beside them, the host flavour of the same evaluator.
//
// arrfn_table_kernel builds value-table entries: the match table skeleton's geometry (n1k_matchtable.hip), because it
// has the same access pattern.  A wave owns 64 consecutive dictionary entries, copies the bytes they span into its LDS
// slab (64 x kCollDevMaxLen bytes) with coalesced word loads, then one lane per entry walks its own text there with
// arrfn_eval<false> (n1k_arrfn.h), once per term of the plan.  A wave whose entries span more than the slab (some entry
// beyond the limit sits among them) reads the entries it does take from global memory.  Per entry it writes one (tag,
// payload) per term and one `left` byte: the entry is array text longer than the limit, or some term met what only the
// host decides (n1k_arrfn.h lists it).  An entry that is no array text gets NULL and is nobody's business.
//
// arrfn_lookup_kernel is the per-row half, arith_kernel's geometry: one row per lane, 256 lanes.  MISSING for MISSING, the
// table's entry at the code for an ARRAY, NULL for everything else (func_array.go: "not an ARRAY -> NULL").
//
// arrfn_eval_block_host is arrfn_eval<true> over a block: this unit holds both flavours because both add with num_add
// (n1k_device.h), which only a kernel unit includes.
#include <hip/hip_runtime.h>
#include "n1k_device.h"
#define N1K_ARRFN_EVAL 1
#include "n1k_arrfn.h"

namespace n1k {

constexpr uint32_t kArrFnBlock = 256, kArrFnWaves = kArrFnBlock / 64;

__global__ __launch_bounds__(256) void arrfn_table_kernel(const ArrFnKernelArgs A) {
    constexpr uint32_t kSlab = 64 * kCollDevMaxLen;  // bytes 64 entries within the limit span at most
    __shared__ uint32_t slab[kArrFnWaves][kSlab / 4 + 4];
    __shared__ ArrFnProg progs[kArrFnMaxTerms];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    {
        const uint32_t* src = (const uint32_t*)A.progs;
        uint32_t* dst = (uint32_t*)&progs[0];
        for (uint32_t k = tid; k < A.nprog * (uint32_t)(sizeof(ArrFnProg) / 4); k += kArrFnBlock) dst[k] = src[k];
    }
    const uint64_t w0 = ((uint64_t)blockIdx.x * kArrFnWaves + wave) * 64ull;
    const uint64_t i = w0 + lane;
    const bool valid = i < A.n;
    // unconditional loads with the mask beside them: a lane beyond the block re-reads the last entry's offsets
    const uint64_t ii = valid ? i : (uint64_t)A.n - 1;
    const uint64_t base0 = A.offsets[0];
    const uint64_t o0 = A.offsets[ii] - base0, o1 = A.offsets[ii + 1] - base0;
    const uint64_t wb = A.offsets[w0 < A.n ? w0 : A.n] - base0;
    const uint64_t we = A.offsets[w0 + 64 < A.n ? w0 + 64 : A.n] - base0;
    const uint64_t wb_al = wb & ~3ull;  // (the bytes' base is allocation aligned: whole words from here)
    const bool in_lds = we - wb <= kSlab;
    if (in_lds) {
        const uint32_t nwords = (uint32_t)((we - wb_al + 3) / 4);  // <= kSlab / 4 + 1; reads at most 3 of the spare bytes
        const uint32_t* src = (const uint32_t*)(A.bytes + wb_al);
        for (uint32_t k = lane; k < nwords; k += 64) slab[wave][k] = src[k];
    }
    __syncthreads();
    const uint64_t len64 = o1 - o0;
    const bool mine = valid && coll_array_text(A.bytes + o0, len64);
    const bool take = mine && len64 <= kCollDevMaxLen;
    bool left = mine && !take;
    uint32_t tg[kArrFnMaxTerms];
    uint64_t pv[kArrFnMaxTerms];
#pragma unroll
    for (uint32_t q = 0; q < kArrFnMaxTerms; q++) {
        tg[q] = T_NULL;
        pv[q] = 0;
    }
    if (take) {
        const uint8_t* s = in_lds ? (const uint8_t*)&slab[wave][0] + (o0 - wb_al) : A.bytes + o0;
#pragma unroll
        for (uint32_t q = 0; q < kArrFnMaxTerms; q++)
            if (q < A.nprog) arrfn_eval<false>(progs[q], s, (uint32_t)len64, tg[q], pv[q], left);
    }
    if (valid) {
#pragma unroll
        for (uint32_t q = 0; q < kArrFnMaxTerms; q++)
            if (q < A.nprog) {
                A.out_tags[q * A.stride + i] = left ? (uint8_t)T_NULL : (uint8_t)tg[q];
                A.out_payload[q * A.stride + i] = left ? 0ull : pv[q];
            }
        A.out_left[i] = left ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void arrfn_lookup_kernel(const ArrFnLookupArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows) return;
    bool in = true;
    if (A.nseg > 1) {
        const uint64_t s = i / A.seg_rows;
        in = s < A.nseg && i - s * A.seg_rows < A.seg_counts[s * kCursorStride];
    } else if (A.nrows_dev)
        in = i < *A.nrows_dev;
    uint32_t rt = T_NULL;  // (a row the batch does not hold: NULL, which nothing reads)
    uint64_t rp = 0;
    if (in) {
        if (A.col.kind == COLK_DICT32) {  // a code is a STRING, NULL or MISSING, never an ARRAY
            rt = A.col.codes[i] == 0xFFFFFFFFu ? (uint32_t)T_MISSING : (uint32_t)T_NULL;
        } else {
            const uint32_t tg = A.col.tags[i];
            if (tg == T_MISSING) rt = T_MISSING;
            else if (tg == T_ARRAY) {
                const uint64_t code = A.col.payload[i];
                if (code < A.tab_n) {  // (every code of the batch is below the table's extent: ensure_value_table came first)
                    rt = A.tab_tags[code];
                    rp = A.tab_payload[code];
                }
            }
        }
    }
    A.out_tags[i] = (uint8_t)rt;
    A.out_payload[i] = rp;
}

hipError_t launch_arrfn_table(const ArrFnKernelArgs& A, hipStream_t st) {
    if (A.n == 0 || A.nprog == 0) return hipSuccess;
    if (A.nprog > kArrFnMaxTerms || !A.progs) return hipErrorInvalidValue;
    const uint32_t grid = (A.n + kArrFnBlock - 1) / kArrFnBlock;
    hipLaunchKernelGGL(arrfn_table_kernel, dim3(grid), dim3(kArrFnBlock), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_arrfn_lookup(const ArrFnLookupArgs& A, hipStream_t st) {
    if (A.nrows == 0) return hipSuccess;
    const uint64_t blocks = (A.nrows + 255) / 256;
    hipLaunchKernelGGL(arrfn_lookup_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, A);
    return hipGetLastError();
}

void arrfn_eval_block_host(const ArrFnProg* progs, uint32_t nprog, uint64_t n, const uint64_t* offsets, const uint8_t* bytes, uint8_t* tags,
                           uint64_t* payload, uint64_t stride) {
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t* s = bytes + (offsets[i] - offsets[0]);
        const uint64_t len = offsets[i + 1] - offsets[i];
        const bool arr = coll_array_text(s, len);
        for (uint32_t q = 0; q < nprog; q++) {
            uint32_t tg = T_NULL;
            uint64_t pv = 0;
            bool left = false;
            if (arr) arrfn_eval<true>(progs[q], s, (uint32_t)len, tg, pv, left);
            tags[q * stride + i] = (uint8_t)tg;
            payload[q * stride + i] = pv;
        }
    }
}

}  // namespace n1k
