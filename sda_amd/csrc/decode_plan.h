// decode_plan.h -- how one decoded reveal (sda_packed_reveal_decoded_dev) runs, decided once from three integers (no
// pointers, no HIP types, no environment: tests/host_c/decode_plan.cc builds it with a plain host compiler).
// launch_packed_decode (packed_decode.hip) and the entry points (engine_check.cpp) dispatch from the plan;
// tests/test_decode_plan.py restates it.
#pragma once
#include <stdint.h>

namespace sda {

enum DecodePath : uint32_t {
    kDecodeNothing = 0,       // fewer than k + t shares: no reveal
    kDecodeFirstPass = 1,     // the fused first pass alone (packed_repair_kernel<bucket>): nothing bad, or e_max == 0
    kDecodeDecoded = 2,       // the first pass, then packed_decode_kernel<rmax> over the bad batches
    kDecodeUnsupported = 3,   // more than 32 clerk results or k > 8: outside the fused first pass
};
struct PackedDecodePlan {
    uint32_t redundancy;      // r = n_idx - (k + t): the syndromes of a batch
    uint32_t radius;          // e_max = r / 2: the wrong shares per batch that are uniquely correctable
    uint32_t path;            // kDecodeNothing, kDecodeUnsupported, or the deepest path the call may take
    uint32_t bucket;          // 8 / 16 / 32 shares held by the first pass's kernel
    uint32_t rmax;            // the decode kernel's instantiation, the smallest of kDecodeRmax that is >= r; 0: no decode pass
    bool decode;              // e_max >= 1: bad batches are decoded
};

// The first pass is the checked reveal's fused kernel, so its scope is the decoded reveal's (repair_plan.h).
constexpr uint32_t kDecodeMaxShares = 32, kDecodeMaxK = 8;
// Syndromes, locator and evaluator of a batch live in registers at compile-time indices: one instantiation per bound
// on r.  12 is there for configs[2] from all 26 clerks (r = 11).
constexpr uint32_t kDecodeRmax[] = {4, 8, 12, 16, 32};

inline PackedDecodePlan packed_decode_plan(uint32_t n_idx, uint32_t k, uint32_t t) {
    PackedDecodePlan pl = {0, 0, kDecodeNothing, 0, 0, false};
    const uint64_t kt = (uint64_t)k + t;
    if (n_idx < kt) return pl;
    pl.redundancy = (uint32_t)(n_idx - kt);
    pl.radius = pl.redundancy / 2;
    if (n_idx > kDecodeMaxShares || k > kDecodeMaxK) {
        pl.path = kDecodeUnsupported;
        return pl;
    }
    pl.bucket = n_idx <= 8 ? 8 : n_idx <= 16 ? 16 : 32;
    pl.decode = pl.radius >= 1;
    pl.path = pl.decode ? kDecodeDecoded : kDecodeFirstPass;
    if (pl.decode)
        for (uint32_t m : kDecodeRmax)
            if (m >= pl.redundancy) { pl.rmax = m; break; }
    return pl;
}

}  // namespace sda
