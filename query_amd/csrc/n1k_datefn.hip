// n1k_datefn.hip — the date functions over a millis NUMBER as materialised derived columns ("Date functions"):
// DATE_PART_MILLIS, DATE_TRUNC_MILLIS, DATE_ADD_MILLIS.
//
// datefn_kernel<OP> is mathfn_kernel (n1k_mathfn.hip) with date_apply<OP> (n1k_device.h) in place of math_apply<OP>: the same
// ArithArgs, the same operand loading, the same output — the node's tag and payload as a TAGGED64 column (9 B read per
// TAGGED64 operand, 9 B written per row).  One instantiation per function; arith_kernel, which takes its op at run time and
// serves every arithmetic node of every plan, carries none of the calendar arithmetic.
//
// Unlike the library functions these can raise: a row whose millis or result lies outside years 1 .. 9999, is NaN or an
// infinity, or whose n overflows sets ERR_UNSUPPORTED_VALUE.  So a row the batch does not hold (a region received from
// another GPU is launched at its capacity) is not evaluated: it gets NULL, which nothing reads.
//
// Geometry: one row per lane, 256 lanes per workgroup, ceil(nrows / 256) workgroups; a lane past nrows leaves at once and
// nothing else depends on the row's position, so the edges are nrows % 64 and nrows % 256.
//
// The string half, str_to_millis and date_part_str over a dictionary string (n1k_datefn.h):
//   datestr_table_kernel   builds value-table entries with the match-table skeleton's geometry (n1k_matchtable.hip,
//     arrfn_table_kernel): a wave owns 64 consecutive dictionary entries, copies the bytes they span into its LDS slab (64 x
//     kDateStrDevMaxLen bytes) with coalesced word loads, then one lane per entry classes its own text there and does the
//     field arithmetic (datestr_eval), once per term of the plan.  A wave whose entries span more than the slab (some entry
//     beyond the limit sits among them) reads the entries it does take from global memory.  An entry beyond the limit is
//     flagged `left`: the host evaluator's, which runs the same template (such a string can only be NULL or UNSURE).
//   datestr_lookup_kernel  the per-row half, arith_kernel's geometry: MISSING for MISSING, the table's entry at the code for
//     a STRING, NULL for everything else; an UNSURE entry gives NULL and raises ERR_UNSUPPORTED_VALUE.
// datefn_eval_host and datestr_eval_block_host are the host flavours of date_apply<OP> and datestr_eval: this unit holds both
// because both need n1k_device.h, which only a kernel unit includes.
#include <hip/hip_runtime.h>
#include "n1k_device.h"
#include "n1k_kernels.h"
#define N1K_DATEFN_EVAL 1
#include "n1k_datefn.h"

namespace n1k {

template <uint32_t OP>
__global__ __launch_bounds__(256) void datefn_kernel(const ArithArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows) return;
    bool in = true;
    if (A.nseg > 1) {
        const uint64_t s = i / A.seg_rows;
        in = s < A.nseg && i - s * A.seg_rows < A.seg_counts[s * kCursorStride];
    } else if (A.nrows_dev)
        in = i < *A.nrows_dev;
    uint32_t tg[4] = {T_MISSING, T_MISSING, T_MISSING, T_MISSING};
    uint64_t pv[4] = {0, 0, 0, 0};
    constexpr uint32_t kOps = OP == AR_DATE_ADD ? 3u : 2u;
#pragma unroll
    for (uint32_t k = 0; k < kOps; k++) {
        if (k >= A.nops || !in) continue;
        const Operand& o = A.ops[k];
        if (o.is_const) {
            tg[k] = o.ctag;
            pv[k] = o.cpayload;
        } else {
            const DevCol& c = A.cols[o.col];
            if (c.kind == COLK_DICT32) {
                const uint32_t code = c.codes[i];
                tg[k] = code == 0xFFFFFFFFu ? (uint32_t)T_MISSING : (code == 0xFFFFFFFEu ? (uint32_t)T_NULL : (uint32_t)T_STRING);
                pv[k] = code;
            } else {
                tg[k] = c.tags[i];
                pv[k] = c.payload[i];
            }
        }
    }
    uint32_t rt = T_NULL;
    uint64_t rp = 0;
    if (in && date_apply<OP>(tg, pv, rt, rp)) atomicOr(A.err_flags, (uint32_t)ERR_UNSUPPORTED_VALUE);
    A.out_tags[i] = (uint8_t)rt;
    A.out_payload[i] = rp;
}

template <uint32_t OP>
static hipError_t launch_one(const ArithArgs& A, uint32_t blocks, hipStream_t st) {
    hipLaunchKernelGGL(datefn_kernel<OP>, dim3(blocks), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_datefn(const ArithArgs& A, hipStream_t st) {
    if (A.nrows == 0) return hipSuccess;
    if (!A.err_flags || A.nops != (A.op == AR_DATE_ADD ? 3u : 2u)) return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)((A.nrows + 255) / 256);
    switch (A.op) {
        case AR_DATE_PART: return launch_one<AR_DATE_PART>(A, blocks, st);
        case AR_DATE_TRUNC: return launch_one<AR_DATE_TRUNC>(A, blocks, st);
        case AR_DATE_ADD: return launch_one<AR_DATE_ADD>(A, blocks, st);
        default: return hipErrorInvalidValue;  // (not a date function: a missing kernel is an error, never another route)
    }
}

bool datefn_eval_host(uint32_t op, const uint32_t (&tg)[4], const uint64_t (&pv)[4], uint32_t& rt, uint64_t& rp) {
    return op == AR_DATE_PART ? date_apply<AR_DATE_PART>(tg, pv, rt, rp)
           : op == AR_DATE_TRUNC ? date_apply<AR_DATE_TRUNC>(tg, pv, rt, rp) : date_apply<AR_DATE_ADD>(tg, pv, rt, rp);
}

// ---- the string half

constexpr uint32_t kDateStrBlock = 256, kDateStrWaves = kDateStrBlock / 64;

__global__ __launch_bounds__(256) void datestr_table_kernel(const DateStrKernelArgs A) {
    constexpr uint32_t kSlab = 64 * kDateStrDevMaxLen;  // bytes 64 entries within the limit span at most
    __shared__ uint32_t slab[kDateStrWaves][kSlab / 4 + 4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t w0 = ((uint64_t)blockIdx.x * kDateStrWaves + wave) * 64ull;
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
    // (a wave reads only the slab it staged itself: wave-level visibility would do; the workgroup barrier is the skeleton's, and
    //  every lane reaches it — the lanes beyond the block leave behind it)
    __syncthreads();
    if (!valid) return;
    const uint64_t len64 = o1 - o0;
    const bool take = len64 <= kDateStrDevMaxLen;
    const uint8_t* s = in_lds ? (const uint8_t*)&slab[wave][0] + (o0 - wb_al) : A.bytes + o0;
#pragma unroll
    for (uint32_t q = 0; q < kDateStrMaxTerms; q++)
        if (q < A.nprog) {
            uint32_t tg = T_NULL;
            uint64_t pv = 0;
            if (take) datestr_eval(A.progs[q], s, (uint32_t)len64, tg, pv);
            A.out_tags[q * A.stride + i] = (uint8_t)tg;
            A.out_payload[q * A.stride + i] = pv;
        }
    A.out_left[i] = take ? 0 : 1;
}

__global__ __launch_bounds__(256) void datestr_lookup_kernel(const DateStrLookupArgs A) {
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
        uint32_t tg;
        uint64_t code;
        if (A.col.kind == COLK_DICT32) {
            const uint32_t c = A.col.codes[i];
            tg = c == 0xFFFFFFFFu ? (uint32_t)T_MISSING : (c == 0xFFFFFFFEu ? (uint32_t)T_NULL : (uint32_t)T_STRING);
            code = c;
        } else {
            tg = A.col.tags[i];
            code = A.col.payload[i];
        }
        if (tg == T_MISSING) rt = T_MISSING;
        else if (tg == T_STRING && code < A.tab_n) {  // (every code of the batch is below the table's extent: ensure_datestr_table came first)
            rt = A.tab_tags[code];
            rp = A.tab_payload[code];
            if (rt == DS_UNSURE) {
                rt = T_NULL;
                atomicOr(A.err_flags, (uint32_t)ERR_UNSUPPORTED_VALUE);
            }
        }
    }
    A.out_tags[i] = (uint8_t)rt;
    A.out_payload[i] = rp;
}

hipError_t launch_datestr_table(const DateStrKernelArgs& A, hipStream_t st) {
    if (A.n == 0 || A.nprog == 0) return hipSuccess;
    if (A.nprog > kDateStrMaxTerms) return hipErrorInvalidValue;
    const uint32_t grid = (A.n + kDateStrBlock - 1) / kDateStrBlock;
    hipLaunchKernelGGL(datestr_table_kernel, dim3(grid), dim3(kDateStrBlock), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_datestr_lookup(const DateStrLookupArgs& A, hipStream_t st) {
    if (A.nrows == 0) return hipSuccess;
    if (!A.err_flags) return hipErrorInvalidValue;
    const uint64_t blocks = (A.nrows + 255) / 256;
    hipLaunchKernelGGL(datestr_lookup_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, A);
    return hipGetLastError();
}

void datestr_eval_block_host(const DateStrProg* progs, uint32_t nprog, uint64_t n, const uint64_t* offsets, const uint8_t* bytes, uint8_t* tags,
                             uint64_t* payload, uint64_t stride) {
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t* s = bytes + (offsets[i] - offsets[0]);
        const uint64_t len = offsets[i + 1] - offsets[i];
        for (uint32_t q = 0; q < nprog; q++) {
            uint32_t tg = T_NULL;
            uint64_t pv = 0;
            if (len <= 0x7FFFFFFFull) datestr_eval(progs[q], s, (uint32_t)len, tg, pv);
            tags[q * stride + i] = (uint8_t)tg;
            payload[q * stride + i] = pv;
        }
    }
}

}  // namespace n1k
