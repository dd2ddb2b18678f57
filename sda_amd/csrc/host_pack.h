// host_pack.h -- packing host share rows into a dense staging tile (the streaming host path of engine_host.cpp).
// Header-only and HIP-free, so a plain C++ program can test it under a host sanitizer (tests/host_c).
#pragma once
#include <limits.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

namespace sda {

namespace host_pack_detail {

// run work(e0, e1) over [0, total) elements on up to `threads` threads (the caller's thread takes the first piece)
template <typename F>
void split_elements(uint64_t total, int threads, F work) {
    const uint64_t min_per_thread = 512 * 1024;             // elements (4 MiB): smaller pieces are not worth a thread
    const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)threads, total / min_per_thread));
    if (T <= 1) {
        work(0, total);
        return;
    }
    const uint64_t per = (total + T - 1) / T;
    std::vector<std::thread> ts;
    ts.reserve(T - 1);
    for (int t = 1; t < T; ++t) {
        const uint64_t e0 = std::min(total, (uint64_t)t * per), e1 = std::min(total, e0 + per);
        if (e0 < e1) ts.emplace_back(work, e0, e1);
    }
    work(0, std::min(per, total));
    for (auto& t : ts) t.join();
}

// byte address of element c of a row: rows are read through memcpy only, so they may sit at any address
inline const unsigned char* row_at(const int64_t* row, uint64_t c) {
    return reinterpret_cast<const unsigned char*>(row) + c * 8;
}

}  // namespace host_pack_detail

// copy the column slice [lo, lo + w) of rows [r0, r0 + R) into dst ([R][w], dense) on `threads` threads
inline void pack_rows(int64_t* dst, const int64_t* const* rows, uint64_t r0, uint64_t R, uint64_t lo, uint64_t w,
                      int threads) {
    const uint64_t total = R * w;
    auto work = [=](uint64_t e0, uint64_t e1) {
        while (e0 < e1) {
            const uint64_t r = e0 / w, c = e0 % w;
            const uint64_t n = std::min(e1 - e0, w - c);
            memcpy(dst + e0, host_pack_detail::row_at(rows[r0 + r], lo + c), n * 8);
            e0 += n;
        }
    };
    host_pack_detail::split_elements(total, threads, work);
}

// The same slice narrowed to int32 (dst [R][w], dense): true when every value fitted.  A thread that meets a
// value outside [-2^31, 2^31 - 1] stops (the others stop at their next row piece), and dst is then unspecified:
// the caller repacks the tile with pack_rows.
inline bool pack_rows32(int32_t* dst, const int64_t* const* rows, uint64_t r0, uint64_t R, uint64_t lo, uint64_t w,
                        int threads) {
    const uint64_t total = R * w;
    std::atomic<bool> wide(false);
    std::atomic<bool>* const wp = &wide;
    auto work = [=](uint64_t e0, uint64_t e1) {
        while (e0 < e1 && !wp->load(std::memory_order_relaxed)) {
            const uint64_t r = e0 / w, c = e0 % w;
            const uint64_t n = std::min(e1 - e0, w - c);
            const unsigned char* src = host_pack_detail::row_at(rows[r0 + r], lo + c);
            int32_t* d = dst + e0;
            // the high word of a value that fits is the sign extension of its low word: OR the differences, so
            // the loop has no branch and vectorises
            uint64_t bad = 0;
            for (uint64_t i = 0; i < n; ++i) {
                int64_t v;
                memcpy(&v, src + i * 8, 8);
                const int32_t t = (int32_t)(uint32_t)(uint64_t)v;
                bad |= (uint64_t)(v ^ (int64_t)t);
                d[i] = t;
            }
            if (bad) {
                wp->store(true, std::memory_order_relaxed);
                return;
            }
            e0 += n;
        }
    };
    host_pack_detail::split_elements(total, threads, work);
    return !wide.load();
}

}  // namespace sda
