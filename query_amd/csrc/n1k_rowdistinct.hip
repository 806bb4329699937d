// n1k_rowdistinct.hip — SELECT DISTINCT over the rows a Filter-only plan selects: the representatives of the distinct row
// keys, de-duplicated on the device (n1k_rowdistinct.h has the key, the steps and their invariants).
//
// rd_insert_kernel   the global table of ordinals; optionally an LDS set per workgroup ahead of it (only each key's smallest
//                    ordinal the workgroup has met goes on)
// rd_mark_kernel     representative iff the key's slot holds the survivor's own ordinal; the tiles' counts
// rd_scan_kernel     one workgroup: exclusive scan of the tiles' counts, the total
// rd_compact_kernel  the stable scatter of the representatives
//
// Integer work bound by scattered reads and — for the rows that reach the table — vector atomics on 32-bit words.
#include <hip/hip_runtime.h>

#include "n1k_device.h"
#include "n1k_rowdistinct.h"

namespace n1k {

struct RdKey {
    uint64_t w[kRdMaxTerms];
    uint32_t cls;  // one byte per term
};

// one value -> (class, word): equal values, and only they, give equal pairs
N1K_DEV void rd_normalise(uint32_t tag, uint64_t p, uint32_t& cls, uint64_t& word) {
    cls = tag;
    word = 0;
    if (tag == T_INT || tag >= T_STRING) word = p;
    else if (tag == T_FLOAT) {
        const double d = as_f64(p);
        if (d != d) word = 0x7FF8000000000000ull;
        else if (d >= -9223372036854775808.0 && d < 9223372036854775808.0 && d == (double)(int64_t)d) {
            cls = T_INT;  // value/float.go:41-45: an integral float marshals as its integer (-0.0 as 0)
            word = (uint64_t)(int64_t)d;
        } else
            word = p;
    }
}

N1K_DEV RdKey rd_load_key(const RowDistinctArgs& A, uint32_t row) {
    RdKey k;
    k.cls = 0;
#pragma unroll
    for (uint32_t t = 0; t < kRdMaxTerms; t++) {
        k.w[t] = 0;
        if (t < A.nterms) {
            const DevCol& c = A.cols[t];
            uint32_t tag;
            uint64_t p;
            if (c.kind == COLK_DICT32) {
                const uint32_t code = c.codes[row];
                tag = code == 0xFFFFFFFFu ? (uint32_t)T_MISSING : (code == 0xFFFFFFFEu ? (uint32_t)T_NULL : (uint32_t)T_STRING);
                p = code;
            } else {
                tag = c.tags[row];
                p = c.payload[row];
            }
            uint32_t cls;
            rd_normalise(tag, p, cls, k.w[t]);
            k.cls |= cls << (8u * t);
        }
    }
    return k;
}

N1K_DEV bool rd_equal(const RdKey& a, const RdKey& b) {
    return a.cls == b.cls && a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3];
}

// (the terms in their order: (a, b) and (b, a) hash apart)
N1K_DEV uint64_t rd_hash(const RdKey& k) {
    uint64_t h = mix64((uint64_t)k.cls + 0x9E3779B97F4A7C15ull);
#pragma unroll
    for (uint32_t t = 0; t < kRdMaxTerms; t++) h = mix64(h ^ k.w[t]) + t;
    return mix64(h);
}

N1K_DEV uint32_t rd_peek(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Find the key's slot in an open-addressed set of `slots` ordinals or take a free one, and leave min(slot, ord) there.
// At most `probes` slots are examined.  Returns the slot, or kRdEmpty when none of them is free or the key's.
N1K_DEV uint32_t rd_find_or_insert(const RowDistinctArgs& A, uint32_t* set, uint64_t slots, uint64_t probes, uint32_t at, const RdKey& key, uint32_t ord) {
    for (uint64_t i = 0; i < probes; i++) {
        uint32_t cur = rd_peek(&set[at]);
        if (cur == kRdEmpty) {
            cur = atomicCAS(&set[at], kRdEmpty, ord);
            if (cur == kRdEmpty) return at;
        }
        // occupied, by a key that never changes: every ordinal the slot ever holds has it
        if (cur == ord || rd_equal(rd_load_key(A, cur), key)) {
            if (cur > ord) atomicMin(&set[at], ord);  // (a stale `cur` is larger than the slot's: the atomic is then only superfluous)
            return at;
        }
        at = (uint64_t)at + 1 == slots ? 0u : at + 1;
    }
    return kRdEmpty;
}

// The same over the workgroup's set in LDS, whose words are fingerprint << 32 | ordinal (the low half of the key's hash: a
// slot of another key is passed by without reading that key's columns; equal keys have equal fingerprints, so the 64-bit
// minimum is the smaller ordinal).  kRdLdsEmpty is no such word: an ordinal is below 2^32 - 1.
constexpr unsigned long long kRdLdsEmpty = ~0ull;
N1K_DEV uint32_t rd_lds_find_or_insert(const RowDistinctArgs& A, unsigned long long* set, uint32_t slots, uint32_t probes, uint32_t at, const RdKey& key,
                                       uint32_t fp, uint32_t ord) {
    const unsigned long long mine = (unsigned long long)fp << 32 | ord;
    for (uint32_t i = 0; i < probes; i++) {
        unsigned long long cur = *(volatile unsigned long long*)&set[at];
        if (cur == kRdLdsEmpty) {
            cur = atomicCAS(&set[at], kRdLdsEmpty, mine);
            if (cur == kRdLdsEmpty) return at;
        }
        if ((uint32_t)(cur >> 32) == fp && ((uint32_t)cur == ord || rd_equal(rd_load_key(A, (uint32_t)cur), key))) {
            if (cur > mine) atomicMin(&set[at], mine);
            return at;
        }
        at = at + 1 == slots ? 0u : at + 1;
    }
    return kRdEmpty;
}

N1K_DEV uint32_t rd_ordinal(const RowDistinctArgs& A, uint64_t i) { return A.sel ? A.sel[i] : (uint32_t)i; }

__global__ __launch_bounds__(kRdBlock) void rd_insert_kernel(const RowDistinctArgs A) {
    extern __shared__ unsigned long long lset[];
    const uint32_t tid = threadIdx.x, L = A.lds_slots;
    const uint32_t ntiles = (uint32_t)((A.n + kRdTile - 1) / kRdTile);
    const uint32_t lprobes = L < kRdLdsProbes ? L : kRdLdsProbes;
    uint32_t reached = 0;
    bool full = false;
    // The set is the workgroup's, not the tile's: it is cleared once.  A workgroup takes its tiles in ascending order, so a key
    // it has met before holds a smaller ordinal than any row of a later tile, and those rows fall without leaving the LDS.
    for (uint32_t i = tid; i < L; i += kRdBlock) lset[i] = kRdLdsEmpty;
    if (L) __syncthreads();
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * kRdTile;
        const uint32_t cnt = (uint32_t)(A.n - base < kRdTile ? A.n - base : kRdTile);
        uint32_t ord[kRdPer], lslot[kRdPer];
        if (L) {
#pragma unroll
            for (uint32_t r = 0; r < kRdPer; r++) {
                const uint32_t j = r * kRdBlock + tid;
                lslot[r] = kRdEmpty;
                if (j < cnt) {
                    ord[r] = rd_ordinal(A, base + j);
                    const RdKey key = rd_load_key(A, ord[r]);
                    const uint64_t h = rd_hash(key);
                    lslot[r] = rd_lds_find_or_insert(A, lset, L, lprobes, (uint32_t)(((h >> 32) * (uint64_t)L) >> 32), key, (uint32_t)h, ord[r]);
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (uint32_t r = 0; r < kRdPer; r++) {
            const uint32_t j = r * kRdBlock + tid;
            if (j >= cnt) continue;
            if (!L) ord[r] = rd_ordinal(A, base + j);
            // the set holds the key: only the smallest ordinal the workgroup has met of it goes on; it had no room: the row goes on
            uint32_t slot = kRdEmpty;
            if (!L || lslot[r] == kRdEmpty || (uint32_t)lset[lslot[r]] == ord[r]) {
                const RdKey key = rd_load_key(A, ord[r]);
                const uint32_t at = (uint32_t)__umul64hi(rd_hash(key), A.slots);
                slot = rd_find_or_insert(A, A.table, A.slots, A.slots, at, key, ord[r]);
                full = full || slot == kRdEmpty;
                reached++;
            }
            A.slot_of[base + j] = slot;
        }
        if (L) __syncthreads();  // (the next tile's rows enter the set only when this tile's have been looked up)
    }
    if (full) atomicOr(A.err_flags, (uint32_t)ERR_TABLE_FULL);
    for (uint32_t off = 32; off; off >>= 1) reached += (uint32_t)__shfl_down((int)reached, off, 64);
    if ((tid & 63u) == 0 && reached) atomicAdd(A.reached, (unsigned long long)reached);
}

// exclusive scan of `v` over the kRdBlock threads (s: kRdBlock words of LDS); *total: the sum
N1K_DEV uint32_t rd_block_excl_scan(uint32_t v, uint32_t* s, uint32_t* total) {
    const uint32_t tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < kRdBlock; off <<= 1) {
        const uint32_t t = tid >= off ? s[tid - off] : 0u;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    const uint32_t incl = s[tid];
    *total = s[kRdBlock - 1];
    __syncthreads();
    return incl - v;
}

// Thread tid owns survivors [tid * kRdPer, (tid + 1) * kRdPer) of the tile in both kernels below: ranks in survivor order.
__global__ __launch_bounds__(kRdBlock) void rd_mark_kernel(const RowDistinctArgs A) {
    __shared__ uint32_t s[kRdBlock];
    const uint32_t tid = threadIdx.x;
    const uint32_t ntiles = (uint32_t)((A.n + kRdTile - 1) / kRdTile);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * kRdTile;
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t r = 0; r < kRdPer; r++) {
            const uint64_t i = base + tid * kRdPer + r;
            if (i < A.n) {
                const uint32_t slot = A.slot_of[i];
                const uint32_t rep = slot != kRdEmpty && (uint64_t)slot < A.slots && A.table[slot] == rd_ordinal(A, i) ? 1u : 0u;
                A.slot_of[i] = rep;
                mine += rep;
            }
        }
        uint32_t total;
        (void)rd_block_excl_scan(mine, s, &total);
        if (tid == 0) A.tile_count[tile] = total;
    }
}

__global__ __launch_bounds__(kRdBlock) void rd_scan_kernel(const RowDistinctArgs A) {
    __shared__ uint32_t s[kRdBlock];
    const uint32_t tid = threadIdx.x;
    const uint32_t ntiles = (uint32_t)((A.n + kRdTile - 1) / kRdTile);
    uint32_t running = 0;
    for (uint32_t c0 = 0; c0 < ntiles; c0 += kRdBlock) {
        const uint32_t i = c0 + tid;
        const uint32_t v = i < ntiles ? A.tile_count[i] : 0u;
        uint32_t total;
        const uint32_t excl = rd_block_excl_scan(v, s, &total);
        if (i < ntiles) A.tile_count[i] = running + excl;
        running += total;
    }
    if (tid == 0) {
        A.tile_count[ntiles] = running;
        *A.count = running;
    }
}

__global__ __launch_bounds__(kRdBlock) void rd_compact_kernel(const RowDistinctArgs A) {
    __shared__ uint32_t s[kRdBlock];
    const uint32_t tid = threadIdx.x;
    const uint32_t ntiles = (uint32_t)((A.n + kRdTile - 1) / kRdTile);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * kRdTile;
        uint32_t rep[kRdPer], mine = 0;
#pragma unroll
        for (uint32_t r = 0; r < kRdPer; r++) {
            const uint64_t i = base + tid * kRdPer + r;
            rep[r] = i < A.n ? A.slot_of[i] : 0u;
            mine += rep[r];
        }
        uint32_t total;
        uint64_t at = (uint64_t)A.tile_count[tile] + rd_block_excl_scan(mine, s, &total);
#pragma unroll
        for (uint32_t r = 0; r < kRdPer; r++) {
            const uint64_t i = base + tid * kRdPer + r;
            if (rep[r] == 1u && at < A.n) A.out[at++] = rd_ordinal(A, i);  // (at < n always: there are no more representatives than survivors)
        }
    }
}

hipError_t launch_row_distinct(const RowDistinctArgs& A, uint32_t grid, hipStream_t st) {
    if (!A.n) return hipSuccess;
    if ((A.n >> 32) || A.nterms < 1 || A.nterms > kRdMaxTerms || A.slots < 1 || A.slots > kRdMaxSlots || A.lds_slots > kRdLdsMaxSlots) return hipErrorInvalidValue;
    const uint64_t ntiles = (A.n + kRdTile - 1) / kRdTile;
    const uint32_t g = (uint32_t)(ntiles < grid ? ntiles : (grid ? grid : 1u));
    hipLaunchKernelGGL(rd_insert_kernel, dim3(g), dim3(kRdBlock), A.lds_slots * sizeof(unsigned long long), st, A);
    hipLaunchKernelGGL(rd_mark_kernel, dim3(g), dim3(kRdBlock), 0, st, A);
    hipLaunchKernelGGL(rd_scan_kernel, dim3(1), dim3(kRdBlock), 0, st, A);
    hipLaunchKernelGGL(rd_compact_kernel, dim3(g), dim3(kRdBlock), 0, st, A);
    return hipGetLastError();
}

}  // namespace n1k
