// reveal_plan.h -- how one packed-Shamir reveal runs, decided once from five integers (no pointers, no HIP types, no
// environment: tests/host_c/reveal_plan.cc builds it with a plain host compiler).  launch_packed_reveal dispatches
// from the plan and reveal_launch (packed_reveal.hip) launches what it names; tests/packed_dispatch.py restates it.
#pragma once
#include <stdint.h>

namespace sda {

// The register reveal kernels keep n_idx + 1 <= kRevealMaxPoints Newton points (n + 1 <= 81 gives n <= 80 clerks) and
// reveal up to kRevealMaxK secrets per batch.
constexpr int kRevealMaxPoints = 96;
constexpr int kRevealMaxK = 64;
// The exact packed kernels truncate lazily (packed_common.h: Trunc<true>, ZeroTrap) for primes at least this big.
constexpr uint32_t kLazyTruncMinP = 1u << 24;

enum RevealPath : uint32_t {
    kRevealRegisters = 0,     // the register kernels in the caller's mode
    kRevealWorkspace = 1,     // packed_wide.hip's workspace kernel (logs nothing; the fields from mm on stay 0)
    kRevealDetour = 2,        // CANONICAL from more than 32 shares: the exact register kernels, then launch_mod_canonical
                              // (CANONICAL = positive() of the exact reveal; DESIGN.md §4.2 on the wide Lagrange kernels)
};
enum RevealFixup : uint32_t { kRevealFixupNone = 0, kRevealFixupWave = 1, kRevealFixupLane = 2 };
struct PackedRevealPlan {
    uint32_t path;            // RevealPath
    int mode;                 // the mode the kernels run: 0 EXACT (also on the detour), 1 CANONICAL
    int mm;                   // the point bucket 8 / 16 / 32 / 64 / 96 (Makefile: REVEAL_PARTS)
    bool staged;              // results parked in LDS and written back coalesced: 256 * k * 8 B <= 32 KiB
    int ku;                   // 8: the evaluation over the k <= 8 secrets is unrolled; 0: a runtime loop
    bool lazy;                // the sign-bit kernel with its zero trap
    bool full;                // n_idx + 1 == mm: every `i < m` guard is a compile-time constant
    uint32_t fixup;           // the kernel that follows: one wave per logged batch (up to 64 points) or one lane
    bool logged;              // the launch zeroes the fix-up log and runs kernels that log into it
};

inline PackedRevealPlan packed_reveal_plan(uint32_t n_idx, uint32_t k, uint32_t t, uint32_t p, int mode) {
    PackedRevealPlan pl = {kRevealRegisters, mode, 0, false, 0, false, false, kRevealFixupNone, false};
    const uint32_t m = n_idx + 1;                     // the Newton points: the inserted (1, 0) first
    if (m > (uint32_t)kRevealMaxPoints || k > (uint32_t)kRevealMaxK) {
        pl.path = kRevealWorkspace;
        return pl;
    }
    if (mode == 1 && n_idx > 32) {
        pl.path = kRevealDetour;
        pl.mode = 0;
    }
    const uint32_t need = pl.mode == 0 ? m : n_idx;   // the Lagrange kernels keep the shares only
    pl.mm = need <= 8 ? 8 : need <= 16 ? 16 : need <= 32 ? 32 : need <= 64 ? 64 : kRevealMaxPoints;
    pl.staged = k <= 16;
    if (pl.mode == 1) return pl;                      // the Lagrange kernels reduce raw shares in the lane: no log
    pl.logged = true;
    pl.fixup = pl.mm <= 64 ? kRevealFixupWave : kRevealFixupLane;
    if (pl.mm <= 16 && k <= 8) {
        pl.ku = 8;
        // The sign-bit kernels are exact unless a residue on the way is 0.  From more than t + k shares the divided
        // differences past the polynomial's degree are 0 in EVERY batch: the launch would log all of its batches for
        // the fix-up.  From exactly t + k shares n_idx + 1 = k + t + 1 is a power of 2: 8 and 16 points are their
        // bucket's FULL kernel, 2 and 4 the 8-point bucket's partial one.
        const bool lazy = p >= kLazyTruncMinP && n_idx == k + t;
        pl.full = lazy && m == (uint32_t)pl.mm;
        pl.lazy = lazy && (pl.full || pl.mm == 8);
    }
    return pl;
}

}  // namespace sda
