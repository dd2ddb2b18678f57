#pragma once
// check_common.h -- device pieces shared by the share consistency check (packed_check.hip) and the checked reveal
// (packed_repair.hip): the counter block's layout, the exact residue of any share value, the residues of a batch as
// one register tuple, a parity / Lagrange row over them, and what a lane reports for a bad batch.
//
// Counter block (u64 words; `buf` of packed_check_buf_bytes()): [0] bad batches, [1] ~(first bad flat index) under
// atomicMax (0: none), [2] batches the checked reveal's fix-up rewrote, [kCheckHdr, +kCheckBlameCap) blame per
// position, then the log of bad flat indices vec * B + b.
#include "packed_common.h"

namespace sda {
namespace packed {

constexpr uint32_t kCheckHdr = 4, kCheckBlameCap = 1024;
static_assert(kRevealMaxShares < kCheckBlameCap, "one blame word per clerk position");

// the exact canonical residue of any share value
__device__ __forceinline__ uint32_t canon_exact(int64_t v, int64_t P, const Mod64& PM) {
    const int64_t r = trem64(v, PM);
    return (uint32_t)(r < 0 ? r + P : r);
}
template <class ST>
__device__ __forceinline__ uint32_t canon_any(ST v, uint32_t p, int64_t P, const Mod64& PM) {
    return share_in_range(v, p, P) ? canon32((int32_t)v, p) : canon_exact((int64_t)v, P, PM);
}

// The first thread id of the calling wave, as a uniform value (workgroups are 256 x 1 x 1: a wave's lanes are 64
// consecutive threads).
__device__ __forceinline__ uint32_t wave_first_thread() {
    return __builtin_amdgcn_readfirstlane(threadIdx.x) & ~63u;
}

// What a lane reports for its batch: the provisional verdict (0 / 0xFFFF; the location pass overwrites located ones),
// and per wave one add of its bad count, one max for the first bad index and a log slot per bad lane.
__device__ __forceinline__ void check_report(bool nonzero, uint32_t wave0, uint64_t B, uint16_t* __restrict__ verdict,
                                             unsigned long long* __restrict__ cnt, uint32_t cap) {
    // The batch's place is worked out here, after the arithmetic, from uniform values (wave0: taken before the
    // loads, a scalar) and the lane's number in its wave: no vector register carries it across the loads.
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t tid = wave0 + lane;
    const uint64_t b0 = (uint64_t)blockIdx.x * 256;
    const bool live = tid < B - b0;
    const bool bad = live && nonzero;
    const uint64_t flat = ((uint64_t)blockIdx.y * B + b0) + tid;
    const uint64_t mask = __ballot(bad);
    if (mask) {
        const uint32_t first = (uint32_t)__ffsll((unsigned long long)mask) - 1;
        uint32_t lo = 0, hi = 0;
        if (lane == first) {                     // lanes hold ascending batches of one vector: the wave's minimum
            const unsigned long long base = atomicAdd(cnt, (unsigned long long)__popcll(mask));
            atomicMax(cnt + 1, ~(unsigned long long)flat);
            lo = (uint32_t)base;
            hi = (uint32_t)(base >> 32);
        }
        lo = __shfl(lo, first);
        hi = __shfl(hi, first);
        if (bad) {
            const uint64_t slot = (((uint64_t)hi << 32) | lo) + __popcll(mask & ((1ull << lane) - 1));
            if (slot < cap) cnt[kCheckHdr + kCheckBlameCap + slot] = flat;
        }
    }
    if (verdict && live) verdict[flat] = bad ? (uint16_t)0xFFFF : (uint16_t)0;
}

// The canonical residues of a batch's n_idx <= NMAX shares as one register tuple (share kt + c of parity row c is
// then a uniform-index move, not a select); sh: the lane's share 0, the others B apart.  Every load is issued before
// the first wait and each share becomes its residue as it lands; raw i64 shares outside (-p, p) are reduced exactly
// in registers and reloaded (rare).
template <int NMAX>
using ShareTuple = uint32_t __attribute__((ext_vector_type(NMAX)));

template <class ST, int NMAX>
__device__ __forceinline__ ShareTuple<NMAX> load_residues(const ST* __restrict__ sh, uint64_t B, uint32_t n_idx,
                                                          uint32_t p) {
    auto share = [&](uint32_t i) { return sh[(uint64_t)i * B]; };
    const int64_t P = (int64_t)p;
    ShareTuple<NMAX> S;
    bool in_range = true;
    {
        ST v[NMAX];
        static_for<0, NMAX>([&](auto i) { v[i] = share((uint32_t)i < n_idx ? i : 0); });
        static_for<0, NMAX>([&](auto i) {
            in_range = in_range && ((uint32_t)i >= n_idx || share_in_range(v[i], p, P));
            S[(int)i] = (uint32_t)i < n_idx ? canon32((int32_t)v[i], p) : 0u;
        });
    }
    if (!in_range) {
        const Mod64 PM = make_mod64(P);
        for (uint32_t i = 0; i < n_idx; ++i) S[i & (NMAX - 1)] = canon_exact((int64_t)share(i), P, PM);
    }
    return S;
}

// sum_{s < kt} w[s] S[s] mod p for a row of Montgomery words w (uniform: scalar loads), two products per REDC
// (2 p^2 < p R); the row is padded with a zero word to an even length.
template <int NMAX>
__device__ __forceinline__ uint32_t row_mac(const uint32_t* __restrict__ w, const ShareTuple<NMAX>& S, uint32_t kt,
                                            const MontP& M) {
    const uint32_t p = M.p;
    uint32_t acc = 0;
    static_for<0, NMAX, 2>([&](auto i) {
        if ((uint32_t)i < kt) {
            uint64_t T = (uint64_t)w[i] * S[(int)i];
            if constexpr (i + 1 < NMAX) T += (uint64_t)w[i + 1] * S[(int)i + 1];     // the pad word past kt is 0
            acc = addm(acc, red1(redc_lazy(T, M), p), p);
        }
    });
    return acc;
}

}  // namespace packed
}  // namespace sda
