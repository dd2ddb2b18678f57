#pragma once
// packed_common.h -- shared by packed_gen.hip / packed_reveal.hip: north-star kernel (2): packed-Shamir share generation and reveal.
//
// Reference call sites: client/src/crypto/sharing/packed_shamir.rs:40-43 (share) and :73-77
// (reconstruct), batched by client/src/crypto/sharing/batched.rs:19-53 / :69-97.  The
// arithmetic lives in threshold-secret-sharing 0.2 (absent from the reference tree):
//   share:       values = [0, secrets(k), randomness(t)]  (length L = k+t+1, a power of 2)
//                coeffs = fft2_inverse(values, omega_secrets)   recursive radix-2, `%` per op
//                points = fft3(coeffs ++ zeros, omega_shares)    recursive radix-3 over n+1
//                shares = points[1..=n]
//   reconstruct: Newton divided differences through (1,0) and (omega_shares^(i+1), share_i),
//                evaluated at omega_secrets^e, e = 1..k.
// Every intermediate is an i64 in (-p, p) whose SIGN depends on the exact operation order
// (Rust's truncated `%`).  The kernels reproduce them bit for bit: for each `(expr) % p` they
// compute (i) the canonical residue with 32-bit Montgomery products (R = 2^32, no 64-bit
// division) and (ii) the sign of the exact i64 expr with one 32x32->64 multiply-add, then
// recombine (trunc_from).  No MFMA: this is not a dense contraction (north star).
//
// One lane = one batch.  The in-place DIT on bit/digit-reversed registers performs exactly the
// butterflies of tss' recursion (same operands, same twiddles, same `%` points).  Batches whose
// inputs fall outside (-p, p) (raw i64 secrets / shares) take a generic exact path that mirrors
// the recursion with wrapping i64 arithmetic.
//
// Reveal comes in two modes: EXACT (Newton, tss' signed representatives; VALU-bound) and
// CANONICAL (Lagrange weights for the clerk-index set, residues in [0, p); HBM-bound), equal
// mod p and equal after RecipientOutput::positive (receive.rs:14-20).
#include <string.h>

#include <vector>

#include "kernels.h"

namespace sda {
namespace packed {

// ------------------------------------------------------------------------------------------
// host-side exact helpers (tss numtheory semantics: truncated `%`)
// ------------------------------------------------------------------------------------------
inline int64_t h_rem(int64_t a, int64_t p) { return a % p; }
inline int64_t h_powmod(int64_t x, uint32_t e, int64_t p) {      // numtheory::mod_pow
    int64_t acc = 1;
    while (e > 0) {
        if (e & 1u) acc = h_rem((int64_t)((uint64_t)acc * (uint64_t)x), p);
        x = h_rem((int64_t)((uint64_t)x * (uint64_t)x), p);
        e >>= 1;
    }
    return acc;
}
inline void h_egcd(int64_t a, int64_t b, int64_t* s, int64_t* t) {     // numtheory::gcd
    if (b == 0) { *s = 1; *t = 0; return; }
    int64_t n = a / b, c = a % b, s1, t1;
    h_egcd(b, c, &s1, &t1);
    *s = t1; *t = s1 - t1 * n;
}
inline int64_t h_modinv(int64_t k, int64_t p) {                 // numtheory::mod_inverse
    int64_t k2 = k % p, s, t, r;
    if (k2 < 0) { h_egcd(p, -k2, &s, &t); r = -t; } else { h_egcd(p, k2, &s, &t); r = t; }
    return (p + r) % p;
}
inline uint32_t to_mont(int64_t x, int64_t p) {            // canonical x -> x R mod p
    int64_t c = x % p; if (c < 0) c += p;
    return (uint32_t)((((unsigned __int128)c) << 32) % (uint64_t)p);
}

// ------------------------------------------------------------------------------------------
// generation tables (kernel argument, uniform => scalar loads)
// ------------------------------------------------------------------------------------------
struct GenTables {
    MontP M;
    uint32_t linv, linv_m;          // L^{-1} mod p (canonical, Montgomery)
    uint32_t tw2[64], tw2_m[64];    // radix-2 level len: entries [len/2 - 1, len - 1)
    uint32_t tw3[120], tw3_m[120];  // radix-3 level len: entries [(len-3)/2, (len-3)/2 + len)
    uint32_t sq3[120], sq3_m[120];  // x^2 % p per radix-3 entry
    // Sign-bit share-gen (packed_gen.hip, SIGNBIT): (u + w c) % p has the sign of c whenever |w c| >= p,
    // i.e. |c| >= ceil(p / w); big2 = the largest such bound over the non-unit radix-2 twiddles, big3 over
    // the radix-3 twiddles of the first radix-3 level (its groups are b + x c: d is zero padding).
    uint32_t big2, big3;
};

// The host twiddles of share generation for any L = k + t + 1 and N3 = n + 1, as i64 words in the layout of the
// workspace kernels' device table (packed_wide.hip): tw2[L - 1] (radix-2 level len: entries [len/2 - 1, len - 1)),
// linv = L^{-1} mod p, then tw3[W3] and sq3[W3] (radix-3 level len: x and x^2 % p at entries [(len-3)/2, (len-3)/2 +
// len)), W3 = (3 N3 - 3) / 2.  GenTables is the same table under its size caps.
inline std::vector<int64_t> make_gen_twiddles(uint32_t L, uint32_t N3, int64_t p, int64_t ws, int64_t wn) {
    const uint64_t W3 = (3ull * N3 - 3) / 2;
    std::vector<int64_t> h(L + 2 * W3, 0);
    // omega per level of a radix-r recursion over `size` points, top level (len = size) first: the recursion raises
    // omega to the r at each level (mod_pow(ω, r))
    auto levels = [p](int64_t om, uint32_t size, uint32_t r) {
        std::vector<int64_t> lv;
        for (uint32_t len = size; len >= r; len /= r) { lv.push_back(om); om = h_powmod(om, r, p); }
        return lv;
    };
    // fft2_inverse: fft2 over omega^-1
    std::vector<int64_t> lv = levels(h_modinv(ws, p), L, 2);
    int lvl = (int)lv.size() - 1;
    for (uint32_t len = 2; len <= L; len *= 2, --lvl)
        for (uint32_t i = 0; i < len / 2; ++i) h[len / 2 - 1 + i] = h_powmod(lv[lvl], i, p);
    h[L - 1] = h_modinv((int64_t)L, p);
    lv = levels(wn, N3, 3);
    lvl = (int)lv.size() - 1;
    for (uint32_t len = 3; len <= N3; len *= 3, --lvl)
        for (uint32_t j = 0; j < len; ++j) {
            const int64_t x = h_powmod(lv[lvl], j, p);
            h[L + (len - 3) / 2 + j] = x;
            h[L + W3 + (len - 3) / 2 + j] = h_rem(x * x, p);
        }
    return h;
}

inline GenTables make_gen_tables(uint32_t L, uint32_t N3, int64_t p, int64_t ws, int64_t wn) {
    GenTables T;
    memset(&T, 0, sizeof(T));
    T.M = make_mont((uint32_t)p);
    const std::vector<int64_t> h = make_gen_twiddles(L, N3, p, ws, wn);
    const uint32_t W3 = (3 * N3 - 3) / 2;
    for (uint32_t e = 0; e < L - 1; ++e) { T.tw2[e] = (uint32_t)h[e]; T.tw2_m[e] = to_mont(h[e], p); }
    T.linv = (uint32_t)h[L - 1];
    T.linv_m = to_mont(T.linv, p);
    for (uint32_t o = 0; o < W3; ++o) {
        const int64_t x = h[L + o], x2 = h[L + W3 + o];
        T.tw3[o] = (uint32_t)x; T.tw3_m[o] = to_mont(x, p);
        T.sq3[o] = (uint32_t)x2; T.sq3_m[o] = to_mont(x2, p);
    }
    T.big2 = 1;
    for (uint32_t e = 1; e < L - 1; ++e)
        if (T.tw2[e] > 1) { const uint64_t b = ((uint64_t)p + T.tw2[e] - 1) / T.tw2[e]; if (b > T.big2) T.big2 = (uint32_t)b; }
    T.big3 = 1;
    for (uint32_t j = 1; j < 3 && j < N3; ++j) {          // first radix-3 level: entries 1, 2 (len 3)
        const uint64_t b = ((uint64_t)p + T.tw3[j] - 1) / T.tw3[j];
        if (b > T.big3) T.big3 = (uint32_t)b;
    }
    return T;
}

// The host tables of a reveal from the clerk set `indices` (data independent; same ops as tss), as i64 words at stride
// m = n_idx + 1: packed_wide.hip uploads `h` as is, packed_reveal.hip packs it into its u32 / Montgomery layout.
//   pts[m]            the points: the inserted 1 first (points.insert(0, 1)), then omega_shares^(indices[i] + 1)
//   h[j m + i]        inv[j][i] = mod_inverse(points[i] - points[i-j]), 1 <= j <= i < m (store[i] covers [i-j, i])
//   h[m m + e m + i]  np[e][i], the signed Newton basis at omega_secrets^(e+1), e < k
//   duplicate         two of the m points coincide: no Lagrange form, so a CANONICAL reveal is refused
struct RevealTables { std::vector<int64_t> pts, h; bool duplicate = false; };
inline RevealTables make_reveal_tables(const uint64_t* indices, uint32_t n_idx, uint32_t k, int64_t p, int64_t ws,
                                       int64_t wn) {
    const uint32_t m = n_idx + 1;
    RevealTables T;
    T.pts.resize(m);
    T.h.assign((uint64_t)m * m + (uint64_t)k * m, 0);
    T.pts[0] = 1;
    for (uint32_t i = 0; i < n_idx; ++i) T.pts[i + 1] = h_powmod(wn, (uint32_t)(indices[i] + 1), p);
    for (uint32_t j = 1; j < m; ++j)
        for (uint32_t i = j; i < m; ++i) T.h[(uint64_t)j * m + i] = h_modinv(h_rem(T.pts[i] - T.pts[i - j], p), p);
    for (uint32_t a = 0; a < m && !T.duplicate; ++a)
        for (uint32_t c = a + 1; c < m; ++c)
            if (T.pts[a] == T.pts[c]) { T.duplicate = true; break; }
    int64_t* np = T.h.data() + (uint64_t)m * m;
    for (uint32_t e = 0; e < k; ++e) {
        const int64_t point = h_powmod(ws, e + 1, p);
        int64_t v = 1;
        for (uint32_t i = 0; i < m; ++i) {
            np[(uint64_t)e * m + i] = v;
            if (i + 1 < m) v = h_rem(v * h_rem(point - T.pts[i], p), p);
        }
    }
    return T;
}

// The parity weights of the share consistency check (packed_check.hip), from make_reveal_tables' points and inverses.
// A sharing polynomial has degree below L = kt + 1 (kt = k + t), so the first L points -- the inserted (1, 0) and
// shares 0 .. kt - 1 -- fix it, and each further share kt + c, c < r = n_idx - kt, must equal its value there:
//   syndrome_c = share_{kt+c} + sum_{s < kt} w[c kt + s] share_s  (mod p),  w[c kt + s] = -l_{s+1}(x_{L+c}),
// l_i the Lagrange basis over the first L points (point 0 carries the value 0, so it has no weight).  Canonical words;
// every one is nonzero (l_i vanishes at the other basis points only).  Distinct points only (!T.duplicate).
// den[i] = prod_{j < L, j != i} 1 / (x_i - x_j), 1 <= i < L: the Lagrange denominators over the first L of the m
// points, from the table's inverses (den[0] stays 1: point 0 has no weight).
inline std::vector<int64_t> basis_denominators(const RevealTables& T, uint32_t m, uint32_t L, int64_t p) {
    auto inv = [&](uint32_t a, uint32_t b) { return T.h[(uint64_t)(a - b) * m + a]; };   // 1 / (x_a - x_b), a > b
    std::vector<int64_t> den(L, 1);
    for (uint32_t i = 1; i < L; ++i)
        for (uint32_t j = 0; j < L; ++j) {
            if (j == i) continue;
            den[i] = den[i] * (j < i ? inv(i, j) : p - inv(j, i)) % p;
        }
    return den;
}

inline std::vector<int64_t> make_check_weights(const RevealTables& T, uint32_t n_idx, uint32_t kt, int64_t p) {
    const uint32_t m = n_idx + 1, L = kt + 1, r = n_idx - kt;
    auto inv = [&](uint32_t a, uint32_t b) { return T.h[(uint64_t)(a - b) * m + a]; };   // 1 / (x_a - x_b), a > b
    const std::vector<int64_t> den = basis_denominators(T, m, L, p);
    std::vector<int64_t> w((uint64_t)r * kt, 0);
    for (uint32_t c = 0; c < r; ++c) {
        int64_t num = 1;                                  // prod_{j < L} (x_{L+c} - x_j)
        for (uint32_t j = 0; j < L; ++j) {
            int64_t d = (T.pts[L + c] - T.pts[j]) % p; if (d < 0) d += p;
            num = num * d % p;
        }
        for (uint32_t i = 1; i < L; ++i) {
            const int64_t l = num * inv(L + c, i) % p * den[i] % p;
            w[(uint64_t)c * kt + (i - 1)] = (p - l) % p;
        }
    }
    return w;
}

// The tables of the checked reveal's correction (packed_repair.hip), from the same points and inverses.  Canonical
// words; distinct points only (!T.duplicate).
//   lam[e kt + s]  the basis Lagrange rows: l_{s+1}(omega_secrets^(e+1)) over the first L = kt + 1 points, e < k,
//                  s < kt -- the CANONICAL reveal's weights for indices[0 .. kt) alone (point 0 carries the value 0 and
//                  has no weight), so  secret_e = sum_s lam[e kt + s] share_s  for a consistent batch
//   winv[s]        1 / w[0][s] for parity row 0 of make_check_weights (`w`; r >= 1), else empty: a single error e at
//                  basis position s gives syndrome_0 = e w[0][s], so e = syndrome_0 winv[s]
// A secret's point is never a clerk's: omega_secrets has order 2^a, omega_shares order 3^b, and neither power is 1.
struct RepairTables { std::vector<int64_t> lam, winv; };
inline RepairTables make_repair_tables(const RevealTables& T, uint32_t n_idx, uint32_t k, uint32_t kt, int64_t p,
                                       int64_t ws, const std::vector<int64_t>& w) {
    const uint32_t m = n_idx + 1, L = kt + 1;
    const std::vector<int64_t> den = basis_denominators(T, m, L, p);
    RepairTables R;
    R.lam.assign((uint64_t)k * kt, 0);
    for (uint32_t e = 0; e < k; ++e) {
        const int64_t point = h_powmod(ws, e + 1, p);
        std::vector<int64_t> d(L);                        // X - x_j, canonical
        int64_t num = 1;
        for (uint32_t j = 0; j < L; ++j) {
            d[j] = (point - T.pts[j]) % p; if (d[j] < 0) d[j] += p;
            num = num * d[j] % p;
        }
        for (uint32_t i = 1; i < L; ++i) R.lam[(uint64_t)e * kt + (i - 1)] = num * h_modinv(d[i], p) % p * den[i] % p;
    }
    if (n_idx > kt) {
        R.winv.resize(kt);
        for (uint32_t s = 0; s < kt; ++s) R.winv[s] = h_modinv(w[s], p);
    }
    return R;
}

// The one device table of the share check and the checked reveal for a (scheme, clerk set), n_idx >= kt = k + t: u32
// words in Montgomery form, rows of ks = kt rounded up to even words, the pad word 0 (the kernels take the products
// of a row in pairs that share one REDC):
//   rows [0, r)       make_check_weights' parity rows w[c][s], r = n_idx - kt
//   rows [r, r + k)   make_repair_tables' lam[e][s]
//   row  r + k        its winv[s] (zeros when r == 0)
// duplicate: two points coincide, there is no systematic form and `words` is empty.
struct CheckTable { std::vector<uint32_t> words; bool duplicate = false; };
inline CheckTable make_check_table(const uint64_t* indices, uint32_t n_idx, uint32_t k, uint32_t t, int64_t p,
                                   int64_t ws, int64_t wn) {
    const uint32_t kt = k + t, r = n_idx - kt, ks = (kt + 1) & ~1u;
    const RevealTables T = make_reveal_tables(indices, n_idx, k, p, ws, wn);
    CheckTable C;
    C.duplicate = T.duplicate;
    if (T.duplicate) return C;
    const std::vector<int64_t> w = r ? make_check_weights(T, n_idx, kt, p) : std::vector<int64_t>();
    const RepairTables R = make_repair_tables(T, n_idx, k, kt, p, ws, w);
    C.words.assign((size_t)(r + k + 1) * ks, 0);
    auto row = [&](uint32_t at, const int64_t* src) {
        for (uint32_t i = 0; i < kt; ++i) C.words[(size_t)at * ks + i] = to_mont(src[i], p);
    };
    for (uint32_t c = 0; c < r; ++c) row(c, w.data() + (size_t)c * kt);
    for (uint32_t e = 0; e < k; ++e) row(r + e, R.lam.data() + (size_t)e * kt);
    if (r) row(r + k, R.winv.data());
    return C;
}

// Rust `v % p` from the canonical residue c and the sign word sw of the exact dividend v.
//   exact (LAZY = false): trunc_rep, 5 VALU ops incl. the c == 0 case (v < 0, v = 0 mod p -> 0);
//   LAZY: c - (p & sign), 3 ops, which gives -p instead of 0 exactly when v < 0 and v = 0 mod p
//   (a nonzero multiple of p: probability ~1/p per value; v == 0 itself is exact).  -p is the only
//   value outside (-p, p), so a running signed min over the outputs finds it (one v_min3 per two
//   values, as opaque asm so the compiler cannot reassociate the chain and stretch live ranges);
//   the batch is then logged and recomputed by the fix-up kernel launched behind it (share-gen: the generic
//   exact path; reveal: ZeroTrap below plays this part, and packed_reveal_fixup_wave_kernel / packed_reveal_fixup_kernel
//   rerun the batch with tss' truncation verbatim).  LAZY is launched only for p >= kLazyTruncMinP.
#ifndef SDA_TRAP_ASM
#define SDA_TRAP_ASM 1
#endif
template <bool LAZY>
struct Trunc {
    int32_t smin = 0x7FFFFFFF;
    int32_t pend = 0;             // note1: values are folded into smin two at a time (one v_min3)
    bool has_pend = false;        // (constant at every point of the unrolled code)
    __device__ __forceinline__ int32_t operator()(uint32_t c, uint32_t sw, uint32_t p) {
        if constexpr (LAZY) {
            return (int32_t)(c - (p & (uint32_t)((int32_t)sw >> 31)));
        }
        else return trunc_rep(c, sw, p);
    }
    __device__ __forceinline__ void note1(int32_t a) {
        if constexpr (LAZY) {
            if (has_pend) {
                note2(pend, a);
                has_pend = false;
            } else {
                pend = a;
                has_pend = true;
            }
        }
    }
    __device__ __forceinline__ void note2(int32_t a, int32_t b) {
        if constexpr (LAZY) {
#if SDA_TRAP_ASM
            asm("v_min3_i32 %0, %0, %1, %2" : "+v"(smin) : "v"(a), "v"(b));
#else
            smin = min(smin, min(a, b));
#endif
        }
    }
    static constexpr bool lazy = LAZY;
    __device__ __forceinline__ bool bad(uint32_t p) {
        if constexpr (LAZY) {
            if (has_pend) note2(pend, pend);
            has_pend = false;
            return smin == -(int32_t)p;
        }
        return false;
    }
};

// Sign-bit logic for the reveal's lazy path: only bit 31 of each operand matters (a sign).
//   maj3(a, b, c)    = MAJ(a, b, c)      one v_bitop3_b32
//   maj3_nb(a, b, c) = MAJ(a, ~b, c)
__device__ __forceinline__ uint32_t maj3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
}
__device__ __forceinline__ uint32_t maj3_nb(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0xB2);
}

// Running unsigned min of canonical residues, two per v_min3_u32 (opaque asm, as Trunc): the
// reveal's sign-bit path is exact unless some residue it produced is 0 (probability ~1/p each).
struct ZeroTrap {
    uint32_t zmin = 0xFFFFFFFFu;
    uint32_t pend = 0;
    bool has_pend = false;
    __device__ __forceinline__ void note2(uint32_t a, uint32_t b) {
        asm("v_min3_u32 %0, %0, %1, %2" : "+v"(zmin) : "v"(a), "v"(b));
    }
    __device__ __forceinline__ void note1(uint32_t a) {
        if (has_pend) {
            note2(pend, a);
            has_pend = false;
        } else {
            pend = a;
            has_pend = true;
        }
    }
    __device__ __forceinline__ void flush() {     // call where a runtime branch joins: keeps has_pend constant
        if (has_pend) note2(pend, pend);
        has_pend = false;
    }
    __device__ __forceinline__ bool bad() {
        flush();
        return zmin == 0;
    }
};

// Montgomery product with a uniform (SGPR) multiplier as a fixed instruction sequence:
// v_mad_u64_u32 (T = a' x [+ acc]), v_mul_lo_u32 (u = T pinv), v_mad_u64_u32 (T + u p) -> high word
// in [0, 2p).  (Left to isel, the exact kernel's lazy variant grew a dead mov + mad-by-0 after
// every reduction.)
__device__ __forceinline__ uint64_t mad_su(uint32_t s, uint32_t v, uint64_t acc) {
    uint64_t r, cy;
    asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(cy) : "s"(s), "v"(v), "v"(acc));
    return r;
}
__device__ __forceinline__ uint64_t mul_su(uint32_t s, uint32_t v) {
    uint64_t r, cy;
    asm("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(r), "=s"(cy) : "s"(s), "v"(v));
    return r;
}
__device__ __forceinline__ uint32_t redc_su(uint64_t T, const MontP& M) {
    const uint32_t u = (uint32_t)T * M.pinv;
    return (uint32_t)(mad_su(M.p, u, T) >> 32);
}
// a' x mod p in [0, p) (a' uniform, Montgomery form); ASM selects the fixed sequence above
// (used by the lazy kernel; the exact-trunc kernel keeps the compiler's, which allocates better).
template <bool ASM>
__device__ __forceinline__ uint32_t montu(uint32_t a_m, uint32_t x, const MontP& M) {
    if constexpr (ASM) return red1(redc_su(mul_su(a_m, x), M), M.p);
    else return red1(redc_lazy((uint64_t)a_m * x, M), M.p);
}
// (a' x + b' y) mod p in [0, p)   (a' x + b' y < 2 p^2 < p R)
template <bool ASM>
__device__ __forceinline__ uint32_t montu2(uint32_t a_m, uint32_t x, uint32_t b_m, uint32_t y, const MontP& M) {
    if constexpr (ASM) return red1(redc_su(mad_su(b_m, y, mul_su(a_m, x)), M), M.p);
    else return red1(redc_lazy((uint64_t)a_m * x + (uint64_t)b_m * y, M), M.p);
}

// A share v lies in (-p, p) (packed_reveal.hip, packed_check.hip).  An int32 share is checked in 32 bits: v + (p - 1)
// mod 2^32 lies in [0, 2p - 2] exactly for those v (above p - 1 the sum stays below 2^32, below -(p - 1) it is at
// least 2^31 + p - 1 > 2p - 2, as p < 2^31).
__device__ __forceinline__ bool share_in_range(int64_t v, uint32_t, int64_t P) {
    return (uint64_t)(v + (P - 1)) < (uint64_t)(2 * P - 1);
}
__device__ __forceinline__ bool share_in_range(int32_t v, uint32_t p, int64_t) {
    return (uint32_t)v + (p - 1) <= 2 * p - 2;
}

// The k secrets of a batch are adjacent in `out` (batched.rs:94 appends batch after batch), so a
// lane's own stores would stride by 8k bytes.  With STAGED the workgroup parks its results in
// LDS ([lane][k]) and writes the nb*k block back with coalesced stores.
// The results leave as nontemporal stores (written once, streamed out), 16 bytes per lane when the block's
// output is 16-byte aligned (lds_o is the dynamic LDS base, so 16-byte aligned too): canonical reveal -1.4 to
// -2.8 %, exact -0.7 to -1.1 % against 8-byte cached stores (in-process A/B on two boxes, profiles/r06ab, r06ac).
// What is stored is epi.at(first) applied to what was parked: at(first) binds the epilogue to the block's first
// element of the vector, and its one(v, j) / pair(v, j) give the value of element j (elements j, j + 1) of the
// block from the parked v.  FlushAsIs stores the results as they are.
using FlushPair = int64_t __attribute__((ext_vector_type(2)));
struct FlushAsIs {
    __device__ __forceinline__ FlushAsIs at(uint64_t) const { return *this; }
    __device__ __forceinline__ int64_t one(int64_t v, uint32_t) const { return v; }
    __device__ __forceinline__ FlushPair pair(FlushPair v, uint32_t) const { return v; }
};
template <class Epi>
__device__ __forceinline__ void reveal_flush_with(int64_t* lds_o, int64_t* o, uint64_t b0, uint64_t B, uint64_t D,
                                                  uint32_t k, const Epi& epilogue) {
    __syncthreads();
    const uint64_t first = b0 * k;
    const uint64_t last = (b0 + 256 < B ? b0 + 256 : B) * k;
    const uint32_t cnt = (uint32_t)((last < D ? last : D) - first);
    int64_t* dst = o + first;
    const auto epi = epilogue.at(first);
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const FlushPair* src2 = reinterpret_cast<const FlushPair*>(lds_o);
        FlushPair* dst2 = reinterpret_cast<FlushPair*>(dst);
        for (uint32_t j = threadIdx.x; j < cnt / 2; j += 256) __builtin_nontemporal_store(epi.pair(src2[j], 2 * j), dst2 + j);
        if ((cnt & 1) && threadIdx.x == 0) __builtin_nontemporal_store(epi.one(lds_o[cnt - 1], cnt - 1), dst + cnt - 1);
    } else {
        for (uint32_t j = threadIdx.x; j < cnt; j += 256) __builtin_nontemporal_store(epi.one(lds_o[j], j), dst + j);
    }
}
template <bool STAGED>
__device__ __forceinline__ void reveal_flush(int64_t* lds_o, int64_t* o, uint64_t b0, uint64_t B, uint64_t D,
                                             uint32_t k) {
    if constexpr (STAGED) reveal_flush_with(lds_o, o, b0, B, D, k, FlushAsIs{});
}

constexpr int ilog(int x, int b) { return x <= 1 ? 0 : 1 + ilog(x / b, b); }
constexpr int ipow(int b, int e) { return e == 0 ? 1 : b * ipow(b, e - 1); }
constexpr int rev_digits(int i, int base, int ndig) {
    int r = 0;
    for (int d = 0; d < ndig; ++d) { r = r * base + i % base; i /= base; }
    return r;
}

__device__ __forceinline__ int64_t wmul(int64_t a, int64_t b) { return (int64_t)((uint64_t)a * (uint64_t)b); }
__device__ __forceinline__ int64_t wadd(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
__device__ __forceinline__ int64_t wsub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }

}  // namespace packed
}  // namespace sda
