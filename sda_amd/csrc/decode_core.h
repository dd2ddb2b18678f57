#pragma once
// decode_core.h -- the per-batch decoder of the decoded reveal (packed_decode.hip), written once over a field F so
// that it compiles for the device and for the host (tests/host_c/decode_core.cc runs it under the sanitizers).
//
// In: the r power-sum syndromes S_i = sum_{j in E} Y_j x_j^i of a word (decode_tables.h), Y_j = v_j err_j.  With
//   Lambda(z) = prod_{j in E} (1 - x_j z)      the locator, of degree nu = |E|,
//   Omega(z)  = S(z) Lambda(z) mod z^r         the evaluator, of degree < nu,
// the syndromes obey the recurrence Lambda spells, Berlekamp-Massey finds the shortest such recurrence, and it is
// Lambda (up to a factor) whenever 2 nu <= r.  The wrong positions are the j with Lambda(x_j^{-1}) = 0 and Forney
// gives  Y_j = -x_j Omega(x_j^{-1}) / Lambda'(x_j^{-1}),  err_j = Y_j / v_j.  A recurrence of length nu with nu
// distinct roots among the x_j^{-1} reproduces S_0 .. S_{r-1} from exactly those nu positions with every Y_j != 0
// (a zero Y_j would leave a shorter recurrence), so "nu <= r / 2 and nu roots found" is the whole acceptance test.
//
// Berlekamp-Massey runs inversion-free in its B <- z B form: step i takes Lambda <- b Lambda - d B with d the
// discrepancy and b the discrepancy at the last length change, so Lambda carries a nonzero factor, which the roots and
// Forney's quotient do not see.  Every array has compile-time indices (sfor over the template bound RMAX >= r): on
// the device S, Lambda, B and Omega are registers.  Lambda and B are kept to degree EMAX = RMAX / 2: deg Lambda <=
// the recurrence's length, which never shrinks, so a coefficient past EMAX is only ever nonzero in a word that is
// rejected for its length anyway.
//
// F: a field of u32 values with mul / add / sub, zero == 0 and one() (MontField: the values are a R mod p).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace sda {
namespace decode {

// pick(g, a, b) = g ? a : b for a mask g of all ones or all zeros, as one bit-field insert.  On the device the mask is
// made opaque first: as a comparison's result it would be kept as a lane mask in scalar registers across the whole
// update of Lambda and B, and the unrolled steps then spill scalar registers.
__host__ __device__ __forceinline__ uint32_t opaque_mask(bool c) {
    uint32_t g = 0u - (uint32_t)c;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(g));
#endif
    return g;
}
__host__ __device__ __forceinline__ uint32_t pick(uint32_t g, uint32_t a, uint32_t b) { return (a & g) | (b & ~g); }

template <int B, int E, typename Fn>
__host__ __device__ __forceinline__ void sfor(Fn&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        sfor<B + 1, E>(f);
    }
}

// Montgomery domain for odd p < 2^31, R = 2^32: modarith.h's redc, for host and device.
struct MontField {
    uint32_t p, pinv, r2, r1;     // r1 = R mod p, the field's one (make_field, or the caller's own copy of it)
    __host__ __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) const {
        const uint64_t T = (uint64_t)a * b;
        const uint32_t u = (uint32_t)T * pinv;
        const uint32_t t = (uint32_t)((T + (uint64_t)u * p) >> 32);
        return t >= p ? t - p : t;
    }
    __host__ __device__ __forceinline__ uint32_t add(uint32_t a, uint32_t b) const {
        const uint32_t s = a + b;
        return s >= p ? s - p : s;
    }
    __host__ __device__ __forceinline__ uint32_t sub(uint32_t a, uint32_t b) const { return a >= b ? a - b : a + p - b; }
    __host__ __device__ __forceinline__ uint32_t one() const { return r1; }
    __host__ __device__ __forceinline__ uint32_t enter(uint32_t canonical) const { return mul(canonical, r2); }
    __host__ __device__ __forceinline__ uint32_t leave(uint32_t a) const { return mul(a, 1u); }
};

__host__ __device__ __forceinline__ MontField make_field(uint32_t p, uint32_t pinv, uint32_t r2) {
    MontField f{p, pinv, r2, 0u};
    f.r1 = f.mul(r2, 1u);
    return f;
}

// a^(p - 2)
template <class F>
__host__ __device__ __forceinline__ uint32_t inverse(const F& f, uint32_t a, uint32_t p) {
    uint32_t acc = f.one();
    for (uint32_t e = p - 2; e; e >>= 1) {
        if (e & 1u) acc = f.mul(acc, a);
        a = f.mul(a, a);
    }
    return acc;
}

template <class F, int RMAX>
struct Decoder {
    static_assert(RMAX >= 2, "a decoder needs two syndromes");
    static constexpr int EMAX = RMAX / 2;
    uint32_t S[RMAX];             // in: the syndromes, S[i] = 0 for i >= r
    uint32_t lam[EMAX + 1];       // locator
    uint32_t om[EMAX];            // evaluator

    // Berlekamp-Massey over S[0 .. r): the length of the shortest recurrence (exact up to EMAX, and above EMAX
    // whenever the true length is).
    __host__ __device__ __forceinline__ uint32_t locator(const F& f, uint32_t r) {
        uint32_t bb[EMAX + 1];
        sfor<0, EMAX + 1>([&](auto l) { lam[l] = bb[l] = l == 0 ? f.one() : 0u; });
        uint32_t b = f.one(), len = 0;
        sfor<0, RMAX>([&](auto i) {
            // a step past r runs with d = 0: it scales Lambda and changes nothing else (no branch per step: nested
            // `i < r` branches each hold a saved lane mask on the device)
            sfor<0, EMAX>([&](auto l) { bb[EMAX - l] = bb[EMAX - 1 - l]; });      // B <- z B
            bb[0] = 0;
            uint32_t d = 0;
            sfor<0, (i < EMAX ? i : EMAX) + 1>([&](auto l) { d = f.add(d, f.mul(lam[l], S[i - l])); });
            d &= opaque_mask((uint32_t)i < r);
            const uint32_t grow = opaque_mask(d != 0 && 2 * len <= (uint32_t)i);
            sfor<0, EMAX + 1>([&](auto l) {
                const uint32_t next = f.sub(f.mul(b, lam[l]), f.mul(d, bb[l]));
                bb[l] = pick(grow, lam[l], bb[l]);
                lam[l] = next;
            });
            b = pick(grow, d, b);
            len = pick(grow, (uint32_t)i + 1 - len, len);
        });
        return len;
    }

    // Omega = S Lambda mod z^nu (its higher coefficients below z^r vanish by the recurrence), nu <= EMAX
    __host__ __device__ __forceinline__ void evaluator(const F& f, uint32_t nu) {
        sfor<0, EMAX>([&](auto i) {
            uint32_t acc = 0;
            sfor<0, i + 1>([&](auto l) { acc = f.add(acc, f.mul(lam[l], S[i - l])); });
            om[i] = (uint32_t)i < nu ? acc : 0u;
        });
    }

    // Lambda(xinv)
    __host__ __device__ __forceinline__ uint32_t locator_at(const F& f, uint32_t xinv) const {
        uint32_t acc = lam[EMAX];
        sfor<0, EMAX>([&](auto l) { acc = f.add(f.mul(acc, xinv), lam[EMAX - 1 - l]); });
        return acc;
    }

    // Forney at a root: err_j from x_j, x_j^{-1} and v_j^{-1}
    __host__ __device__ __forceinline__ uint32_t error_value(const F& f, uint32_t p, uint32_t x, uint32_t xinv,
                                                             uint32_t vinv) const {
        uint32_t val = 0, der = 0;                         // Lambda and Lambda' at xinv, one Horner pass
        sfor<0, EMAX + 1>([&](auto l) {
            der = f.add(f.mul(der, xinv), val);
            val = f.add(f.mul(val, xinv), lam[EMAX - l]);
        });
        uint32_t w = om[EMAX - 1];
        sfor<1, EMAX>([&](auto l) { w = f.add(f.mul(w, xinv), om[EMAX - 1 - l]); });
        const uint32_t y = f.mul(f.mul(x, w), inverse(f, der, p));
        return f.mul(f.sub(0u, y), vinv);
    }
};

// One word on the host: nu (0: every syndrome is zero), the bit mask of the wrong positions and err[j - 1] for each
// (field values, as the syndromes are).  false: undecodable -- nu > e_max = r / 2, or fewer than nu roots among the
// n_idx positions.  S: r syndromes; xinv, xs, vinv: n_idx field values each (decode_tables.h).
template <class F, int RMAX>
inline bool decode_word(const F& f, uint32_t p, uint32_t r, uint32_t n_idx, const uint32_t* S, const uint32_t* xinv,
                        const uint32_t* xs, const uint32_t* vinv, uint32_t* nu_out, uint32_t* wrong, uint32_t* err) {
    Decoder<F, RMAX> d;
    bool any = false;
    for (uint32_t i = 0; i < (uint32_t)RMAX; ++i) {
        d.S[i] = i < r ? S[i] : 0u;
        any = any || d.S[i] != 0;
    }
    *nu_out = 0;
    *wrong = 0;
    if (!any) return true;
    const uint32_t nu = d.locator(f, r);
    *nu_out = nu;
    if (nu > r / 2) return false;
    uint32_t mask = 0, roots = 0;
    for (uint32_t j = 0; j < n_idx; ++j)
        if (d.locator_at(f, xinv[j]) == 0) { mask |= 1u << j; ++roots; }
    if (roots != nu) return false;
    d.evaluator(f, nu);
    for (uint32_t j = 0; j < n_idx; ++j)
        if (mask >> j & 1u) err[j] = d.error_value(f, p, xs[j], xinv[j], vinv[j]);
    *wrong = mask;
    return true;
}

}  // namespace decode
}  // namespace sda
