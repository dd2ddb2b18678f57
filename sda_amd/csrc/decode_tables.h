#pragma once
// decode_tables.h -- the host builder of the decoded reveal's table (packed_decode.hip), from make_reveal_tables'
// points.  tests/host_c/decode_table.cc builds it for the host alone.
//
// The shares of a batch and the inserted (1, 0) are the evaluations of a polynomial of degree < L = k + t + 1 at the
// m = n_idx + 1 distinct points x_0 = 1, x_j = omega_shares^(indices[j-1] + 1): a generalised Reed-Solomon code whose
// dual has the column multipliers v_j = 1 / prod_{l != j} (x_j - x_l), the product over all m points.  So a word y is
// a codeword iff its r = n_idx - (k + t) power-sum syndromes S_i = sum_j v_j x_j^i y_j, i < r, vanish; y_0 = 0 drops
// out of the sum.
//
// Table (u32 words, Montgomery form), n = n_idx:
//   rows [0, rmax) of n words   v_j x_j^i at i n + (j - 1); rows r .. rmax - 1 are zero (the kernel forms rmax sums;
//                               rmax >= r, the plan's instantiation)
//   then n words each           x_j^{-1},  x_j,  v_j^{-1}
#include "packed_common.h"

namespace sda {
namespace packed {

struct DecodeTable { std::vector<uint32_t> words; bool duplicate = false; };

inline size_t decode_table_words(uint32_t n_idx, uint32_t rmax) { return (size_t)(rmax + 3) * n_idx; }

inline DecodeTable make_decode_table(const uint64_t* indices, uint32_t n_idx, uint32_t k, uint32_t t, int64_t p,
                                     int64_t ws, int64_t wn, uint32_t rmax) {
    const uint32_t kt = k + t, r = n_idx - kt, m = n_idx + 1;
    const RevealTables T = make_reveal_tables(indices, n_idx, k, p, ws, wn);
    DecodeTable D;
    D.duplicate = T.duplicate;
    if (T.duplicate) return D;
    if (rmax < r) rmax = r;
    D.words.assign(decode_table_words(n_idx, rmax), 0);
    uint32_t* xinv = D.words.data() + (size_t)rmax * n_idx;
    uint32_t* xs = xinv + n_idx;
    uint32_t* vinv = xs + n_idx;
    for (uint32_t j = 1; j < m; ++j) {
        int64_t den = 1;                                   // prod_{l != j} (x_j - x_l), canonical
        for (uint32_t l = 0; l < m; ++l) {
            if (l == j) continue;
            int64_t d = (T.pts[j] - T.pts[l]) % p; if (d < 0) d += p;
            den = den * d % p;
        }
        int64_t x = T.pts[j] % p; if (x < 0) x += p;
        int64_t w = h_modinv(den, p);                      // v_j, then v_j x_j^i
        for (uint32_t i = 0; i < r; ++i) {
            D.words[(size_t)(j - 1) * rmax + i] = to_mont(w, p);
            w = w * x % p;
        }
        xinv[j - 1] = to_mont(h_modinv(x, p), p);
        xs[j - 1] = to_mont(x, p);
        vinv[j - 1] = to_mont(den, p);
    }
    return D;
}

}  // namespace packed
}  // namespace sda
