// check_plan.h -- how one packed-Shamir share consistency check runs, decided once from three integers (no pointers,
// no HIP types, no environment: tests/host_c/check_plan.cc builds it with a plain host compiler).
// launch_packed_check (packed_check.hip) dispatches from the plan; tests/test_check_plan.py restates it.
#pragma once
#include <stdint.h>

namespace sda {

enum CheckPath : uint32_t {
    kCheckNothing = 0,        // fewer than k + t + 1 shares: no redundancy, nothing is launched
    kCheckRegisters = 1,      // packed_check_kernel<bucket>: the shares of a batch in registers
    kCheckLooped = 2,         // packed_check_loop_kernel: 33 ... 1023 shares, re-read per group of parity rows
};
struct PackedCheckPlan {
    uint32_t redundancy;      // r = n_idx - (k + t): the parity rows of a batch (0 when there are too few shares)
    uint32_t path;            // CheckPath
    uint32_t bucket;          // 8 / 16 / 32 shares held by the register kernel; 0 on the other paths
    bool locate;              // r >= 2: bad batches go on to packed_check_locate_kernel
};

inline PackedCheckPlan packed_check_plan(uint32_t n_idx, uint32_t k, uint32_t t) {
    PackedCheckPlan pl = {0, kCheckNothing, 0, false};
    const uint64_t kt = (uint64_t)k + t;
    if (n_idx <= kt) return pl;
    pl.redundancy = (uint32_t)(n_idx - kt);
    pl.locate = pl.redundancy >= 2;
    if (n_idx <= 32) {
        pl.path = kCheckRegisters;
        pl.bucket = n_idx <= 8 ? 8 : n_idx <= 16 ? 16 : 32;
    } else {
        pl.path = kCheckLooped;
    }
    return pl;
}

}  // namespace sda
