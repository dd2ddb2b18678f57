// repair_plan.h -- how one checked reveal (sda_packed_reveal_checked_dev) runs, decided once from three integers (no
// pointers, no HIP types, no environment: tests/host_c/repair_plan.cc builds it with a plain host compiler).
// launch_packed_repair (packed_repair.hip) and the entry points (engine_check.cpp) dispatch from the plan;
// tests/test_repair_plan.py restates it.
#pragma once
#include <stdint.h>

namespace sda {

enum RepairPath : uint32_t {
    kRepairNothing = 0,       // fewer than k + t shares: no reveal
    kRepairFused = 1,         // packed_repair_kernel<bucket>: check and basis reveal in one pass over the shares
    kRepairComposed = 2,      // the share check, the CANONICAL reveal, then packed_repair_fix_kernel over the bad batches
};
struct PackedRepairPlan {
    uint32_t redundancy;      // r = n_idx - (k + t): the parity rows of a batch
    uint32_t path;            // RepairPath
    uint32_t bucket;          // 8 / 16 / 32 shares held by the fused kernel; 0 on the composed path
    bool locate;              // r >= 2: bad batches are located, and corrected when the wrong share is a basis share
};

// The fused kernel keeps the shares of a batch in registers (the check's buckets) and stages k <= 8 secrets per lane
// in LDS; everything else the reveal supports -- 33 ... 1023 shares, wide k, the workspace schemes -- is composed.
constexpr uint32_t kRepairFusedMaxShares = 32, kRepairFusedMaxK = 8;

inline PackedRepairPlan packed_repair_plan(uint32_t n_idx, uint32_t k, uint32_t t) {
    PackedRepairPlan pl = {0, kRepairNothing, 0, false};
    const uint64_t kt = (uint64_t)k + t;
    if (n_idx < kt) return pl;
    pl.redundancy = (uint32_t)(n_idx - kt);
    pl.locate = pl.redundancy >= 2;
    if (n_idx <= kRepairFusedMaxShares && k <= kRepairFusedMaxK) {
        pl.path = kRepairFused;
        pl.bucket = n_idx <= 8 ? 8 : n_idx <= 16 ? 16 : 32;
    } else {
        pl.path = kRepairComposed;
    }
    return pl;
}

}  // namespace sda
