// n1k_order.hip — ORDER BY over the rows a Filter-only plan selects (execution/order.go:121-169), sorted on the device.
//
// order_keys_kernel turns the survivors' sort values into (key, residual) pairs (n1k_order.h) and counts the 256-bin
// histograms of every digit, so that the host launches only the digit passes that can move anything.  A pass is one stable
// LSD step over pairs (64-bit key, 32-bit position): order_tile_hist_kernel counts the digit per tile of kOrdTile elements,
// order_scan_kernel turns the digit-major counts into every tile's output offset per digit, order_scatter_kernel ranks the
// tile's elements stably and writes them out in runs through LDS.  All of it is integer work bound by HBM.
#include <hip/hip_runtime.h>

#include "n1k_device.h"
#include "n1k_order.h"

namespace n1k {

// Lanes of a wave that count the same bin as its first counting lane add once: the high digits of keys of one type class are
// all alike, and 64 atomics on one LDS word serialise.  What is left goes in lane by lane.  Called by whole waves.
N1K_DEV void wave_hist_add(uint32_t* h, uint32_t bin, bool in) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long todo = __ballot(in);
    if (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lb = (uint32_t)__shfl((int)bin, leader, 64);
        const unsigned long long same = __ballot(in && bin == lb);
        if ((int)lane == leader) atomicAdd(&h[lb], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&h[bin], 1u);
}

__global__ __launch_bounds__(kOrdBlock) void order_keys_kernel(const OrderKeyArgs A) {
    extern __shared__ uint32_t lh[];  // [nh][kOrdDigits][256]
    const uint32_t tid = threadIdx.x;
    const uint32_t nh = A.hist ? A.nterms + A.pos_term : 0u;
    for (uint32_t i = tid; i < nh * kOrdDigits * 256u; i += kOrdBlock) lh[i] = 0;
    __syncthreads();
    uint32_t bad = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * kOrdBlock; base < A.n; base += (uint64_t)gridDim.x * kOrdBlock) {
        const uint64_t i = base + tid;
        const bool valid = i < A.n;
        const uint32_t pos = valid ? (A.cand ? A.cand[i] : (uint32_t)i) : 0u;
        const uint32_t row = valid ? A.rows[pos] : 0u;
        for (uint32_t t = 0; t < A.nterms; t++) {
            const DevCol& c = A.cols[t];
            uint32_t tag = T_MISSING;
            uint64_t p = 0;
            if (valid) {
                if (c.kind == COLK_DICT32) {
                    const uint32_t code = c.codes[row];
                    tag = code == 0xFFFFFFFFu ? (uint32_t)T_MISSING : (code == 0xFFFFFFFEu ? (uint32_t)T_NULL : (uint32_t)T_STRING);
                    p = code;
                } else {
                    tag = c.tags[row];
                    p = c.payload[row];
                }
            }
            const uint32_t rank = tag == T_STRING && A.str_rank ? A.str_rank[(uint32_t)p] : 0u;
            const OrderKey k = order_key(tag, p, rank, A.desc[t] != 0);
            if (valid) {
                bad |= k.unsupported;
                if ((A.store >> t) & 1u) {
                    A.key[t][i] = k.key;
                    A.res[t][i] = (uint16_t)k.res;
                }
            }
            if (nh) {
                uint32_t* h = lh + t * kOrdDigits * 256u;
#pragma unroll
                for (uint32_t d = 0; d < kOrdKeyDigits; d++) wave_hist_add(h + d * 256u, (uint32_t)(k.key >> (8u * d)) & 255u, valid);
                wave_hist_add(h + 8u * 256u, k.res & 255u, valid);
                wave_hist_add(h + 9u * 256u, (k.res >> 8) & 255u, valid);
            }
        }
        if (A.pos_term) {
            if (valid) A.key[A.nterms][i] = pos;
            if (nh) {
                uint32_t* h = lh + A.nterms * kOrdDigits * 256u;
#pragma unroll
                for (uint32_t d = 0; d < 4; d++) wave_hist_add(h + d * 256u, (pos >> (8u * d)) & 255u, valid);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < nh * kOrdDigits * 256u; i += kOrdBlock)
        if (lh[i]) atomicAdd(&A.hist[i], lh[i]);
    if (bad) atomicOr(A.err_flags, (uint32_t)ERR_UNSUPPORTED_VALUE);
}

__global__ __launch_bounds__(256) void order_gather_kernel(const uint64_t* key, const uint16_t* res, const uint32_t* perm, uint64_t n, uint64_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t j = perm ? perm[i] : i;
    out[i] = res ? (uint64_t)res[j] : key[j];
}

__global__ __launch_bounds__(256) void order_finish_kernel(const uint32_t* rows, const uint32_t* cand, const uint32_t* perm, uint64_t first, uint64_t last,
                                                           uint32_t* out) {
    const uint64_t i = first + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= last) return;
    const uint32_t j = perm ? perm[i] : (uint32_t)i;
    out[i - first] = rows[cand ? cand[j] : j];
}

// tile_hist[d * ntiles + tile]: elements of the tile whose digit is d
__global__ __launch_bounds__(kOrdBlock) void order_tile_hist_kernel(const uint64_t* keys, uint64_t n, uint32_t shift, uint32_t ntiles, uint32_t* tile_hist) {
    __shared__ uint32_t h[256];
    const uint32_t tid = threadIdx.x;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        h[tid] = 0;
        __syncthreads();
        const uint64_t base = (uint64_t)tile * kOrdTile;
        const uint32_t cnt = (uint32_t)(n - base < kOrdTile ? n - base : kOrdTile);
        for (uint32_t j0 = 0; j0 < cnt; j0 += kOrdBlock) {
            const uint32_t j = j0 + tid;
            const bool valid = j < cnt;
            const uint64_t x = valid ? keys[base + j] : 0ull;
            wave_hist_add(h, (uint32_t)(x >> shift) & 255u, valid);
        }
        __syncthreads();
        tile_hist[(size_t)tid * ntiles + tile] = h[tid];
        __syncthreads();
    }
}

// exclusive scan of `v` over the 256 threads of the workgroup (s: 256 words of LDS); *total: the sum
N1K_DEV uint32_t block_excl_scan(uint32_t v, uint32_t* s, uint32_t* total) {
    const uint32_t tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        const uint32_t t = tid >= off ? s[tid - off] : 0u;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    const uint32_t incl = s[tid];
    *total = s[255];
    __syncthreads();
    return incl - v;
}

// Workgroup d: row d of tile_hist (the tiles' counts of digit d) becomes the tiles' output offsets for that digit: the elements
// of the smaller digits (ghist: the digit's totals over all keys) come first, then the earlier tiles' elements of digit d.
__global__ __launch_bounds__(256) void order_scan_kernel(uint32_t* tile_hist, uint32_t ntiles, const uint32_t* ghist) {
    __shared__ uint32_t s[256];
    const uint32_t tid = threadIdx.x, d = blockIdx.x;
    uint32_t total;
    (void)block_excl_scan(tid < d ? ghist[tid] : 0u, s, &total);
    uint32_t running = total;  // keys whose digit is below d
    uint32_t* row = tile_hist + (size_t)d * ntiles;
    for (uint32_t c0 = 0; c0 < ntiles; c0 += 256) {
        const uint32_t i = c0 + tid;
        const uint32_t v = i < ntiles ? row[i] : 0u;
        const uint32_t excl = block_excl_scan(v, s, &total);
        if (i < ntiles) row[i] = running + excl;
        running += total;
    }
}

// The stable scatter of one tile.  Wave w owns elements [w * 1024, (w + 1) * 1024) of the tile, 64 at a time (a round): the
// rank of an element among the wave's earlier elements of the same digit is the wave's running count of the digit (LDS, one
// row per wave) plus the number of lower lanes of the round with that digit — the peer mask of the lanes that share the digit
// comes from eight ballots over its bits.  Waves, then digits, are summed up once all rounds are counted; the elements go to
// their place of the tile's sorted order in LDS and leave from there, so that each digit's elements are written in one run.
template <bool kKeysOut>
__global__ __launch_bounds__(kOrdBlock) void order_scatter_kernel(const uint64_t* kin, const uint32_t* vin, uint64_t* kout, uint32_t* vout, uint64_t n,
                                                                  uint32_t shift, uint32_t ntiles, const uint32_t* tile_off) {
    __shared__ uint64_t sk[kOrdTile];
    __shared__ uint32_t sv[kOrdTile];
    __shared__ uint32_t wcnt[4][256];
    __shared__ uint32_t lstart[256], goff[256], tmp[256];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const unsigned long long below_mask = (1ull << lane) - 1ull;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * kOrdTile;
        const uint32_t cnt = (uint32_t)(n - base < kOrdTile ? n - base : kOrdTile);
#pragma unroll
        for (uint32_t w = 0; w < 4; w++) wcnt[w][tid] = 0;
        goff[tid] = tile_off[(size_t)tid * ntiles + tile];
        __syncthreads();
        uint64_t k[kOrdRounds];
        uint32_t v[kOrdRounds], rk[kOrdRounds];
#pragma unroll
        for (uint32_t r = 0; r < kOrdRounds; r++) {
            const uint32_t j = wave * (kOrdTile / 4) + r * 64u + lane;
            const bool valid = j < cnt;
            k[r] = valid ? kin[base + j] : 0ull;
            v[r] = valid ? (vin ? vin[base + j] : (uint32_t)(base + j)) : 0u;
        }
#pragma unroll
        for (uint32_t r = 0; r < kOrdRounds; r++) {
            const uint32_t j = wave * (kOrdTile / 4) + r * 64u + lane;
            const bool valid = j < cnt;
            const uint32_t digit = (uint32_t)(k[r] >> shift) & 255u;
            unsigned long long peers = __ballot(valid);
#pragma unroll
            for (uint32_t b = 0; b < 8; b++) {
                const bool bit = (digit >> b) & 1u;
                const unsigned long long bal = __ballot(bit);
                peers &= bit ? bal : ~bal;
            }
            const uint32_t below = (uint32_t)__popcll(peers & below_mask);
            const uint32_t old = wcnt[wave][digit];
            __builtin_amdgcn_wave_barrier();
            if (valid && below == 0) wcnt[wave][digit] = old + (uint32_t)__popcll(peers);  // the digit's first lane of the round
            __builtin_amdgcn_wave_barrier();
            rk[r] = old + below;
        }
        __syncthreads();
        // digit `tid`: the waves' counts -> their exclusive prefix over the waves; the digits' totals -> the tile's sorted order
        const uint32_t c0 = wcnt[0][tid], c1 = wcnt[1][tid], c2 = wcnt[2][tid], c3 = wcnt[3][tid];
        wcnt[0][tid] = 0;
        wcnt[1][tid] = c0;
        wcnt[2][tid] = c0 + c1;
        wcnt[3][tid] = c0 + c1 + c2;
        uint32_t total;
        lstart[tid] = block_excl_scan(c0 + c1 + c2 + c3, tmp, &total);
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < kOrdRounds; r++) {
            const uint32_t j = wave * (kOrdTile / 4) + r * 64u + lane;
            const uint32_t digit = (uint32_t)(k[r] >> shift) & 255u;
            const uint32_t at = lstart[digit] + wcnt[wave][digit] + rk[r];
            if (j < cnt && at < kOrdTile) {
                sk[at] = k[r];
                sv[at] = v[r];
            }
        }
        __syncthreads();
        for (uint32_t j = tid; j < cnt; j += kOrdBlock) {
            const uint64_t key = sk[j];
            const uint32_t digit = (uint32_t)(key >> shift) & 255u;
            const uint64_t dst = (uint64_t)goff[digit] + (j - lstart[digit]);
            if (dst < n) {  // (always, when the offsets are those of these keys)
                if (kKeysOut) kout[dst] = key;
                vout[dst] = sv[j];
            }
        }
        __syncthreads();
    }
}

hipError_t launch_order_keys(const OrderKeyArgs& A, uint32_t grid, hipStream_t st) {
    if (!A.n) return hipSuccess;
    const size_t shmem = A.hist ? (size_t)(A.nterms + A.pos_term) * kOrdDigits * 256 * sizeof(uint32_t) : 0;
    auto k = order_keys_kernel;
    if (shmem > 48 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    const uint64_t blocks = (A.n + kOrdBlock - 1) / kOrdBlock;
    hipLaunchKernelGGL(k, dim3((uint32_t)(blocks < grid ? blocks : grid)), dim3(kOrdBlock), shmem, st, A);
    return hipGetLastError();
}

hipError_t launch_order_gather(const uint64_t* key, const uint16_t* res, const uint32_t* perm, uint64_t n, uint64_t* out, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(order_gather_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, key, res, perm, n, out);
    return hipGetLastError();
}

hipError_t launch_order_pass(const uint64_t* kin, const uint32_t* vin, uint64_t* kout, uint32_t* vout, uint64_t n, uint32_t shift,
                             const uint32_t* ghist, uint32_t* tile_hist, uint32_t grid, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint32_t ntiles = (uint32_t)((n + kOrdTile - 1) / kOrdTile);
    const uint32_t g = ntiles < grid ? ntiles : grid;
    hipLaunchKernelGGL(order_tile_hist_kernel, dim3(g), dim3(kOrdBlock), 0, st, kin, n, shift, ntiles, tile_hist);
    hipLaunchKernelGGL(order_scan_kernel, dim3(256), dim3(256), 0, st, tile_hist, ntiles, ghist);
    if (kout) hipLaunchKernelGGL(order_scatter_kernel<true>, dim3(g), dim3(kOrdBlock), 0, st, kin, vin, kout, vout, n, shift, ntiles, tile_hist);
    else hipLaunchKernelGGL(order_scatter_kernel<false>, dim3(g), dim3(kOrdBlock), 0, st, kin, vin, kout, vout, n, shift, ntiles, tile_hist);
    return hipGetLastError();
}

hipError_t launch_order_finish(const uint32_t* rows, const uint32_t* cand, const uint32_t* perm, uint64_t first, uint64_t last,
                               uint32_t* out, hipStream_t st) {
    if (last <= first) return hipSuccess;
    hipLaunchKernelGGL(order_finish_kernel, dim3((uint32_t)((last - first + 255) / 256)), dim3(256), 0, st, rows, cand, perm, first, last, out);
    return hipGetLastError();
}

}  // namespace n1k
