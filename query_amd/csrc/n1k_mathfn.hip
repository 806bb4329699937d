// n1k_mathfn.hip — the library functions as materialised derived columns ("Numeric functions"): ACOS ASIN ATAN
// COS SIN TAN EXP LN LOG DEGREES RADIANS, ATAN2, POWER and IFINF / IFNAN / IFNANORINF.
//
// mathfn_kernel<OP> is arith_kernel (n1k_kernels.hip) with the function chosen at compile time: the same ArithArgs, the same
// operand loading — a DICT32 operand is MISSING / NULL by its code and a STRING otherwise, which every function here answers
// with NULL — and the same output, the node's tag and payload as a TAGGED64 column (9 B read per TAGGED64 operand, 9 B
// written per row).  One instantiation per function, so that each carries its own double-precision routine and arith_kernel,
// which takes its op at run time and serves every arithmetic node of every plan, carries none of them.
//
// Geometry: one row per lane, 256 lanes per workgroup, ceil(nrows / 256) workgroups; a lane past nrows leaves at once and
// nothing else depends on the row's position, so the edges are nrows % 64 and nrows % 256.
#include <hip/hip_runtime.h>
#include "n1k_device.h"
#include "n1k_kernels.h"

namespace n1k {

template <uint32_t OP>
__global__ __launch_bounds__(256) void mathfn_kernel(const ArithArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.nrows) return;
    uint32_t tg[4] = {T_MISSING, T_MISSING, T_MISSING, T_MISSING};
    uint64_t pv[4] = {0, 0, 0, 0};
    constexpr uint32_t kOps = ar_is_ifnum(OP) ? 4u : (ar_is_mathfn2(OP) ? 2u : 1u);
#pragma unroll
    for (uint32_t k = 0; k < kOps; k++) {
        if (k >= A.nops) continue;
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
    uint32_t rt;
    uint64_t rp;
    math_apply<OP>(A.nops, tg, pv, rt, rp);
    A.out_tags[i] = (uint8_t)rt;
    A.out_payload[i] = rp;
}

template <uint32_t OP>
static hipError_t launch_one(const ArithArgs& A, uint32_t blocks, hipStream_t st) {
    hipLaunchKernelGGL(mathfn_kernel<OP>, dim3(blocks), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_mathfn(const ArithArgs& A, hipStream_t st) {
    if (A.nrows == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)((A.nrows + 255) / 256);
    switch (A.op) {
        case AR_ACOS: return launch_one<AR_ACOS>(A, blocks, st);
        case AR_ASIN: return launch_one<AR_ASIN>(A, blocks, st);
        case AR_ATAN: return launch_one<AR_ATAN>(A, blocks, st);
        case AR_COS: return launch_one<AR_COS>(A, blocks, st);
        case AR_SIN: return launch_one<AR_SIN>(A, blocks, st);
        case AR_TAN: return launch_one<AR_TAN>(A, blocks, st);
        case AR_EXP: return launch_one<AR_EXP>(A, blocks, st);
        case AR_LN: return launch_one<AR_LN>(A, blocks, st);
        case AR_LOG: return launch_one<AR_LOG>(A, blocks, st);
        case AR_DEGREES: return launch_one<AR_DEGREES>(A, blocks, st);
        case AR_RADIANS: return launch_one<AR_RADIANS>(A, blocks, st);
        case AR_ATAN2: return launch_one<AR_ATAN2>(A, blocks, st);
        case AR_POWER: return launch_one<AR_POWER>(A, blocks, st);
        case AR_IFINF: return launch_one<AR_IFINF>(A, blocks, st);
        case AR_IFNAN: return launch_one<AR_IFNAN>(A, blocks, st);
        case AR_IFNANORINF: return launch_one<AR_IFNANORINF>(A, blocks, st);
        default: return hipErrorInvalidValue;  // (not a library function: a missing kernel is an error, never another route)
    }
}

}  // namespace n1k
