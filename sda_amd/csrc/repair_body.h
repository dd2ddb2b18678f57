#pragma once
// repair_body.h -- the fused first pass of the checked and decoded reveals as one device body, shared by its kernels:
// packed_repair_kernel / packed_repair32_kernel (packed_repair.hip) store the secrets as they are, and
// recipient_repair_kernel (recipient_repair.hip) subtracts the recipient's mask in the same write-back.
#include "check_common.h"

namespace sda {
namespace packed {

// One lane = one batch, in check_body's shape: the loads, the residues as one register tuple, the r syndrome rows,
// then k rows against lam into the workgroup's LDS block ([lane][k]), the report, and reveal_flush_with's coalesced
// write-back through `epi` (16-byte nontemporal stores when the block's output is 16-byte aligned, 8-byte ones
// otherwise; the tail batch is cut at `dimension` there).  Lanes past the last batch hold the last batch again;
// neither pass keeps them.
template <class ST, int NMAX, class Epi>
__device__ __forceinline__ void repair_body(const ST* __restrict__ shares, uint64_t B, uint64_t D,
                                            int64_t* __restrict__ out, uint32_t n_idx, uint32_t kt, uint32_t k,
                                            const uint32_t* __restrict__ tab, uint32_t ks, const MontP& M,
                                            uint16_t* __restrict__ verdict, unsigned long long* __restrict__ cnt,
                                            uint32_t cap, int64_t* lds_o, const Epi& epi) {
    const uint32_t wave0 = wave_first_thread();
    const uint64_t b0 = (uint64_t)blockIdx.x * 256, rest = B - b0;
    const ST* sh = shares + ((uint64_t)blockIdx.y * n_idx * B + b0) + (threadIdx.x < rest ? threadIdx.x : (uint32_t)rest - 1);
    const uint32_t p = M.p;
    const ShareTuple<NMAX> S = load_residues<ST, NMAX>(sh, B, n_idx, p);
    const uint32_t r = n_idx - kt;
    uint32_t nz = 0;
    for (uint32_t c = 0; c < r; ++c)
        nz |= addm(row_mac<NMAX>(tab + (size_t)c * ks, S, kt, M), S[(kt + c) & (NMAX - 1)], p);     // kt + c < n_idx <= NMAX
    const uint32_t* lam = tab + (size_t)r * ks;
    int64_t* dst = lds_o + threadIdx.x * k;
    for (uint32_t e = 0; e < k; ++e) dst[e] = (int64_t)row_mac<NMAX>(lam + (size_t)e * ks, S, kt, M);
    check_report(nz != 0, wave0, B, verdict, cnt, cap);
    reveal_flush_with(lds_o, out + (uint64_t)blockIdx.y * D, b0, B, D, k, epi);
}

// The exact canonical residue of any i64 value from the field's Montgomery constants alone: |v| = hi 2^32 + lo, and
// hi 2^32 mod p is one Montgomery product with R^2 mod p (R = 2^32).  Values in (-p, p) take canon32; the rest pay two
// 32-bit remainders (rare: a mask an engine call produced lies in (-p, p)).
__device__ __forceinline__ uint32_t canon_wide(int64_t v, const MontP& M) {
    const uint32_t p = M.p;
    if (share_in_range(v, p, (int64_t)p)) return canon32((int32_t)v, p);
    const uint64_t a = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;          // |i64::MIN| = 2^63: hi = 2^31
    const uint32_t r = addm(mont_mul(M.r2, (uint32_t)(a >> 32) % p, M), (uint32_t)a % p, p);
    return v < 0 && r ? p - r : r;
}

// The recipient's unmask + positive() where both moduli are the sharing prime: element j of the vector leaves as
// (secret_j - mask_j) mod p in [0, p), every i64 mask value reduced exactly.  mask: the vector's D values, 8-byte
// aligned; its alignment is independent of the output's, so a pair of mask values is one 16-byte load only where that
// address is 16-byte aligned, and two 8-byte loads otherwise.  Read once: nontemporal loads.
struct FlushSubMask {
    const int64_t* mask;
    MontP M;
    bool wide = false;
    __device__ __forceinline__ FlushSubMask at(uint64_t first) const {
        const int64_t* m = mask + first;
        return FlushSubMask{m, M, (reinterpret_cast<uintptr_t>(m) & 15) == 0};
    }
    __device__ __forceinline__ int64_t sub(int64_t v, int64_t m) const {
        return (int64_t)subm((uint32_t)v, canon_wide(m, M), M.p);
    }
    __device__ __forceinline__ int64_t one(int64_t v, uint32_t j) const {
        return sub(v, __builtin_nontemporal_load(mask + j));
    }
    __device__ __forceinline__ FlushPair pair(FlushPair v, uint32_t j) const {   // j even
        FlushPair m;
        if (wide) {
            m = __builtin_nontemporal_load(reinterpret_cast<const FlushPair*>(mask + j));
        } else {
            m.x = __builtin_nontemporal_load(mask + j);
            m.y = __builtin_nontemporal_load(mask + j + 1);
        }
        FlushPair o;
        o.x = sub(v.x, m.x);
        o.y = sub(v.y, m.y);
        return o;
    }
};

}  // namespace packed
}  // namespace sda
