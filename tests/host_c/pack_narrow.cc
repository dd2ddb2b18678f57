// pack_narrow.cc -- stand-alone check of sda_amd/csrc/host_pack.h (tests/test_host_pack.py builds it with
// -fsanitize=address,undefined and runs it): pack_rows32 against a scalar loop, pack_rows as a byte copy.
// Exit status 0 and a last line "pack_narrow OK" when every case passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../sda_amd/csrc/host_pack.h"

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++g_failed;                  \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);         \
            printf("\n");                \
        }                                \
    } while (0)

const int64_t kMin32 = -((int64_t)1 << 31), kMax32 = ((int64_t)1 << 31) - 1;

uint64_t g_rng = 0x5DA5DA5DAull;
uint64_t next() {                        // xorshift64
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

// N rows of `len` values in int32 range, each row in its own allocation at byte offset `skew` (rows of the
// caller's i64 vectors may sit at any address; the row pointers are only ever read through memcpy)
struct Rows {
    std::vector<std::vector<unsigned char>> store;
    std::vector<const int64_t*> ptr;
    uint64_t len;
    size_t skew;
    Rows(uint64_t n, uint64_t len_, size_t skew_) : store(n), ptr(n), len(len_), skew(skew_) {
        for (uint64_t r = 0; r < n; ++r) {
            store[r].resize(len * 8 + skew);
            ptr[r] = reinterpret_cast<const int64_t*>(store[r].data() + skew);
            for (uint64_t c = 0; c < len; ++c) set(r, c, (int64_t)(next() % ((uint64_t)1 << 32)) + kMin32);
        }
    }
    void set(uint64_t r, uint64_t c, int64_t v) { memcpy(store[r].data() + skew + c * 8, &v, 8); }
    int64_t get(uint64_t r, uint64_t c) const {
        int64_t v;
        memcpy(&v, store[r].data() + skew + c * 8, 8);
        return v;
    }
};

// one case: the slice rows [r0, r0 + R) x columns [lo, lo + w) on `threads` threads
void check_slice(const Rows& x, uint64_t r0, uint64_t R, uint64_t lo, uint64_t w, int threads, bool expect_fit,
                 const char* what) {
    // exact-size heap buffers: a write past the tile is an ASan report
    std::vector<int32_t> d32(R * w);
    std::vector<int64_t> d64(R * w);
    const bool fit = sda::pack_rows32(d32.data(), x.ptr.data(), r0, R, lo, w, threads);
    bool ref_fit = true;
    for (uint64_t r = 0; r < R; ++r)
        for (uint64_t c = 0; c < w; ++c) {
            const int64_t v = x.get(r0 + r, lo + c);
            if (v < kMin32 || v > kMax32) ref_fit = false;
        }
    CHECK(ref_fit == expect_fit, "%s: the case itself is wrong", what);
    CHECK(fit == ref_fit, "%s: pack_rows32 returned %d, scalar loop says %d (T=%d)", what, (int)fit, (int)ref_fit,
          threads);
    if (fit && ref_fit) {
        uint64_t bad = 0;
        for (uint64_t r = 0; r < R; ++r)
            for (uint64_t c = 0; c < w; ++c) bad += (int64_t)d32[r * w + c] != x.get(r0 + r, lo + c);
        CHECK(bad == 0, "%s: %llu int32 values differ (T=%d)", what, (unsigned long long)bad, threads);
    }
    sda::pack_rows(d64.data(), x.ptr.data(), r0, R, lo, w, threads);
    uint64_t bad = 0;
    for (uint64_t r = 0; r < R; ++r)
        bad += memcmp(&d64[r * w], reinterpret_cast<const unsigned char*>(x.ptr[r0 + r]) + (lo * 8), w * 8) != 0;
    CHECK(bad == 0, "%s: pack_rows is not a byte copy in %llu rows (T=%d)", what, (unsigned long long)bad, threads);
}

}  // namespace

int main() {
    const int thread_counts[] = {1, 3, 16};
    // large: the slice 7 x 1,200,001 of a 9 x 1,200,011 job = 8.4M elements, 16 x the 512K-element piece a
    // thread is worth, so 16 threads really run, on pieces that start and end mid-row.  tiny: a few elements.
    const uint64_t W = 1200011, w = 1200001;
    for (size_t skew : {(size_t)0, (size_t)4, (size_t)1}) {          // rows at 8-, 4- and 1-byte alignment
        Rows big(9, W, skew), tiny(3, 5, skew);
        for (int T : thread_counts) {
            if (skew == 0 || T == 16) check_slice(big, 1, 7, 3, w, T, true, "large slice, mid-row start and end");
            if (skew == 0) check_slice(big, 0, 9, 0, W, T, true, "large, whole rows");
            check_slice(tiny, 1, 2, 1, 3, T, true, "tiny slice");
            check_slice(tiny, 0, 3, 0, 5, T, true, "tiny, whole rows");
            check_slice(tiny, 2, 1, 4, 1, T, true, "one element");
        }
        // the int32 limits fit
        big.set(1, 3, kMin32);
        big.set(7, w + 2, kMax32);
        big.set(4, 450000, kMin32);
        big.set(4, 450001, kMax32);
        tiny.set(1, 1, kMax32);
        tiny.set(2, 3, kMin32);
        check_slice(big, 1, 7, 3, w, skew == 0 ? 3 : 16, true, "large, int32 limits");
        check_slice(tiny, 1, 2, 1, 3, 1, true, "tiny, int32 limits");
        // one value past the limits: at the first element, at the last element, and on both sides of a thread
        // boundary of the slice (16 threads: pieces of ceil(7 w / 16) = 525,001 elements; 3 threads: 2,800,003)
        struct Spot { uint64_t e; int threads; };
        const Spot spots[] = {{0, 1}, {0, 3}, {0, 16}, {7 * w - 1, 1}, {7 * w - 1, 3}, {7 * w - 1, 16},
                              {525001 - 1, 16}, {525001, 16}, {5 * 525001, 16}, {2800003 - 1, 3}, {2800003, 3}};
        const int64_t wide_vals[] = {kMax32 + 1, kMin32 - 1};
        int k = 0;
        for (const Spot& sp : spots) {
            if (skew != 0 && sp.threads != 16) continue;
            const int64_t v = wide_vals[k++ & 1];
            const uint64_t r = 1 + sp.e / w, c = 3 + sp.e % w;
            const int64_t keep = big.get(r, c);
            big.set(r, c, v);
            check_slice(big, 1, 7, 3, w, sp.threads, false, "large, one wide value");
            big.set(r, c, keep);
        }
        // outside the slice a wide value does not matter
        big.set(0, 5, kMax32 + 1);
        big.set(8, 2, kMin32 - 1);
        big.set(3, 2, INT64_MAX);
        big.set(3, w + 3, INT64_MIN);
        check_slice(big, 1, 7, 3, w, 16, true, "large, wide values outside the slice");
        for (int64_t v : wide_vals) {
            tiny.set(1, 1, v);
            check_slice(tiny, 1, 2, 1, 3, 16, false, "tiny, wide first");
            tiny.set(1, 1, 0);
            tiny.set(2, 3, v);
            check_slice(tiny, 1, 2, 1, 3, 1, false, "tiny, wide last");
            tiny.set(2, 3, 0);
        }
        tiny.set(0, 0, INT64_MIN);
        check_slice(tiny, 0, 3, 0, 5, 3, false, "tiny, i64::MIN");
    }
    if (g_failed) {
        printf("pack_narrow: %d checks failed\n", g_failed);
        return 1;
    }
    printf("pack_narrow OK\n");
    return 0;
}
