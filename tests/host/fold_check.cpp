// fold_check.cpp — the fold of workgroup slabs into table rows (query_amd/csrc/n1k_fold.h) on the CPU.
//
// A stand-alone host program: no HIP, no GPU.  It builds synthetic slabs (word-major, as the DIRECT scans store them: word w of
// slot s of workgroup b at slabs[b * W * S + w * S + s]) for one slot layout that holds every aggregate kind, folds them
//   * slab by slab in order (what a single thread would do), and
//   * in fold_rows_kernel's geometry: LANES slab-lanes per slot taking slabs bl, bl + LANES, ... in chunks with slabs beyond
//     the end replaced by fold_slab_identity, the lanes of a wave joined in a xor tree, the 16 waves joined in order,
// and holds both against a straightforward per-slot loop over the values the slabs were made from.  Float operands are small
// multiples of 1/4, so every order of additions gives the same sum.  Built with -fsanitize=address,undefined by
// tests/test_fold_cpu.py.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../query_amd/csrc/n1k_fold.h"

using namespace n1k;

static int g_failures = 0;
static std::string g_case;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            if (g_failures < 20) fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, g_case.c_str()); \
            g_failures++;                                                                            \
        }                                                                                            \
    } while (0)

static const uint32_t kKinds[] = {AGG_COUNT, AGG_COUNTN, AGG_SUM, AGG_AVG, AGG_MIN, AGG_MAX};
constexpr uint32_t kNA = 6;

static uint64_t bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }
static double dbl(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
// the sortable image of a double that MIN / MAX keep (n1k_device.h f64_sortable)
static uint64_t sortable(double d) { const uint64_t b = bits(d); return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull); }

// what one slot should end up with, kept by the straightforward loop
struct Expect {
    uint64_t count = 0, countn = 0;
    __int128 isum = 0;
    double fsum = 0.0;
    uint64_t sflags = 0, n = 0;
    uint64_t mflags = 0;
    int64_t imin = INT64_MAX, imax = INT64_MIN;
    uint64_t fmin = ~0ull, fmax = 0, smin = ~0ull, smax = 0;
    bool touched = false;
};

struct Layout {
    uint32_t off[kNA], W;
    Layout() {
        uint32_t w = 1;  // word 0: the key / touched word
        for (uint32_t a = 0; a < kNA; a++) { off[a] = w; w += fold_slab_words(kKinds[a]); }
        W = w;
    }
};

static void run_case(uint32_t nslabs, uint32_t S, uint32_t mode, uint32_t seed) {
    g_case = "slabs " + std::to_string(nslabs) + " S " + std::to_string(S) + " mode " + std::to_string(mode);
    const Layout L;
    std::mt19937_64 rng(seed);
    std::vector<uint64_t> slabs((size_t)nslabs * L.W * S);
    std::vector<Expect> exp(S);
    auto word = [&](uint32_t b, uint32_t w, uint32_t s) -> uint64_t& { return slabs[(size_t)b * L.W * S + (size_t)w * S + s]; };
    // every slab starts as lds_table_init leaves it
    for (uint32_t b = 0; b < nslabs; b++)
        for (uint32_t s = 0; s < S; s++) {
            word(b, 0, s) = kEmptyKey;
            for (uint32_t a = 0; a < kNA; a++)
                for (uint32_t i = 0; i < fold_slab_words(kKinds[a]); i++) {
                    uint64_t ident = 0;
                    if (kKinds[a] == AGG_MIN) ident = i == 1 ? (uint64_t)INT64_MAX : (i >= 2 ? ~0ull : 0ull);
                    if (kKinds[a] == AGG_MAX) ident = i == 1 ? (uint64_t)INT64_MIN : 0ull;
                    word(b, L.off[a] + i, s) = ident;
                    CHECK(ident == fold_slab_identity(kKinds[a], i));
                }
        }
    for (uint32_t s = 0; s < S; s++) {
        // mode 0: random slabs touch the slot; 1: exactly one slab does; 2: none; 3: all, with int sums near +-2^62
        const uint32_t only = (uint32_t)(rng() % nslabs);
        for (uint32_t b = 0; b < nslabs; b++) {
            const bool touch = mode == 0 ? (rng() % 3 == 0) : (mode == 1 ? b == only : mode == 3);
            if (!touch) continue;
            Expect& e = exp[s];
            e.touched = true;
            word(b, 0, s) = s;  // the key word: anything but kEmptyKey
            const uint32_t what = (uint32_t)(rng() % 8);  // which kinds of operands the workgroup met for this slot
            const bool has_int = what & 1, has_flt = what & 2, has_str = what & 4;
            int64_t iv = (int64_t)(rng() % 2000001) - 1000000;
            if (mode == 3) iv = (s & 1 ? -1 : 1) * ((int64_t)1 << 62) + (int64_t)(rng() % 1000);
            const double fv = ((double)(int64_t)(rng() % 4001) - 2000.0) / 4.0;
            const uint64_t sv = ((rng() % 1000) << 32) | (rng() % 1000);
            const uint64_t cnt = rng() % 100000 + 1;
            for (uint32_t a = 0; a < kNA; a++) {
                const uint32_t o = L.off[a];
                switch (kKinds[a]) {
                    case AGG_COUNT: word(b, o, s) = cnt; e.count += cnt; break;
                    case AGG_COUNTN: { const uint64_t c = has_int || has_flt ? cnt / 2 : 0; word(b, o, s) = c; e.countn += c; break; }
                    case AGG_SUM:
                    case AGG_AVG: {
                        uint64_t fl = 0;
                        if (has_int) { word(b, o, s) = (uint64_t)iv; fl |= iv < 0 ? SF_NEG_INT : SF_NONNEG_INT; }
                        if (has_flt) { word(b, o + 1, s) = bits(fv); fl |= SF_FLOAT; }
                        word(b, o + 2, s) = fl;
                        if (kKinds[a] == AGG_AVG) { word(b, o + 3, s) = fl ? cnt : 0; if (fl) e.n += cnt; }
                        if (kKinds[a] == AGG_SUM) {  // (AVG holds the same sums: kept once)
                            if (has_int) e.isum += iv;
                            if (has_flt) e.fsum += fv;
                            e.sflags |= fl;
                        }
                        break;
                    }
                    default: {
                        uint64_t fl = (what == 0 ? MM_TRUE : 0) | (has_int ? MM_INT : 0) | (has_flt ? MM_FLOAT : 0) | (has_str ? MM_STRING : 0);
                        word(b, o, s) = fl;
                        if (has_int) word(b, o + 1, s) = (uint64_t)iv;
                        if (has_flt) word(b, o + 2, s) = sortable(fv);
                        if (has_str) word(b, o + 3, s) = sv;
                        if (kKinds[a] == AGG_MIN) {
                            e.mflags |= fl;
                            if (has_int) { e.imin = std::min(e.imin, iv); e.imax = std::max(e.imax, iv); }
                            if (has_flt) { e.fmin = std::min(e.fmin, sortable(fv)); e.fmax = std::max(e.fmax, sortable(fv)); }
                            if (has_str) { e.smin = std::min(e.smin, sv); e.smax = std::max(e.smax, sv); }
                        }
                        break;
                    }
                }
            }
        }
    }

    auto load = [&](uint32_t b, uint32_t a, uint32_t s, uint64_t* x) {
        for (uint32_t i = 0; i < fold_slab_words(kKinds[a]); i++) x[i] = word(b, L.off[a] + i, s);
    };
    auto check_row = [&](uint32_t a, uint32_t s, const uint64_t* acc, bool touched) {
        const Expect& e = exp[s];
        const uint32_t kind = kKinds[a];
        uint64_t row[kFoldMaxWords + 1];
        row[fold_acc_words(kind)] = 0xABCDull;  // (fold_row writes the aggregate's words and no more)
        fold_row(kind, acc, row);
        CHECK(row[fold_acc_words(kind)] == 0xABCDull);
        CHECK(touched == e.touched);
        // a word that is not live holds its identity: what glob_row_init writes
        const uint64_t fl = row[fold_flags_word(kind)];
        for (uint32_t i = 0; i < fold_acc_words(kind); i++)
            if (!fold_word_live(kind, i, fl)) CHECK(row[i] == fold_identity(kind, i) || (fold_word_op(kind, i) == FOLD_ADD_F64 && dbl(row[i]) == 0.0));
        switch (kind) {
            case AGG_COUNT: CHECK(row[0] == e.count); break;
            case AGG_COUNTN: CHECK(row[0] == e.countn); break;
            case AGG_SUM:
            case AGG_AVG: {
                const __int128 tot = (__int128)(int64_t)row[1] * 4294967296 + (__int128)(unsigned __int128)row[0];  // hi * 2^32 + lo, as finalize_agg reads it
                CHECK(tot == e.isum);
                CHECK(dbl(row[2]) == e.fsum);
                CHECK(row[3] == e.sflags);
                if (kind == AGG_AVG) CHECK(row[4] == e.n);
                break;
            }
            case AGG_MIN:
                CHECK(row[0] == e.mflags && (int64_t)row[1] == e.imin && row[2] == e.fmin && row[3] == e.smin);
                break;
            default:
                CHECK(row[0] == e.mflags && (int64_t)row[1] == e.imax && row[2] == e.fmax && row[3] == e.smax);
                break;
        }
    };

    for (uint32_t s = 0; s < S; s++)
        for (uint32_t a = 0; a < kNA; a++) {
            const uint32_t kind = kKinds[a];
            // in order
            uint64_t acc[kFoldMaxWords], x[kFoldMaxWords], touched = 0;
            fold_init(kind, acc);
            for (uint32_t b = 0; b < nslabs; b++) {
                load(b, a, s, x);
                fold_slab(kind, acc, x);
                touched |= word(b, 0, s) ^ kEmptyKey;
            }
            check_row(a, s, acc, touched != 0);
            // the kernel's geometry, for 16 and for 8 slots per workgroup (64 and 128 slab-lanes, 4 and 8 of them per wave)
            for (uint32_t lanes : {64u, 128u}) {
                const uint32_t per_wave = lanes / 16, chunk = 4;
                std::vector<uint64_t> part((size_t)lanes * kFoldMaxWords), tch(lanes, 0);
                for (uint32_t bl = 0; bl < lanes; bl++) {
                    uint64_t* p = &part[(size_t)bl * kFoldMaxWords];
                    fold_init(kind, p);
                    for (uint32_t b0 = 0; b0 < nslabs; b0 += lanes * chunk)
                        for (uint32_t c = 0; c < chunk; c++) {
                            const uint32_t b = b0 + c * lanes + bl;
                            load(b < nslabs ? b : 0, a, s, x);
                            if (b >= nslabs)
                                for (uint32_t i = 0; i < fold_slab_words(kind); i++) x[i] = fold_slab_identity(kind, i);
                            fold_slab(kind, p, x);
                            if (b < nslabs) tch[bl] |= word(b, 0, s) ^ kEmptyKey;
                        }
                }
                uint64_t total[kFoldMaxWords], tt = 0;
                for (uint32_t w = 0; w < 16; w++) {
                    for (uint32_t off = 1; off < per_wave; off <<= 1)  // the xor tree: lane 0 of the wave ends up with all
                        for (uint32_t k = 0; k < per_wave; k++) {
                            if (k & off) continue;
                            fold_join(kind, &part[(size_t)(w * per_wave + k) * kFoldMaxWords], &part[(size_t)(w * per_wave + (k ^ off)) * kFoldMaxWords]);
                            tch[w * per_wave + k] |= tch[w * per_wave + (k ^ off)];
                        }
                    const uint64_t* wv = &part[(size_t)w * per_wave * kFoldMaxWords];
                    if (w == 0) memcpy(total, wv, sizeof total);
                    else
                        for (uint32_t i = 0; i < fold_acc_words(kind); i++) total[i] = fold_word(fold_word_op(kind, i), total[i], wv[i]);
                    tt |= tch[w * per_wave];
                }
                check_row(a, s, total, tt != 0);
            }
        }
}

int main() {
    uint32_t seed = 1;
    for (uint32_t nslabs : {1u, 2u, 63u, 64u, 65u, 768u})
        for (uint32_t S : {2u, 39u, 1002u})
            for (uint32_t mode = 0; mode < 4; mode++) {
                if (nslabs == 768 && S == 1002 && mode != 0 && mode != 3) continue;  // (seconds: the large case twice)
                run_case(nslabs, S, mode, seed++);
            }
    if (g_failures) {
        fprintf(stderr, "fold_check: %d failures\n", g_failures);
        return 1;
    }
    printf("fold_check: ok\n");
    return 0;
}
