// make_check_table (sda_amd/csrc/packed_common.h) as a stand-alone program, for tests/test_check_table.py: the
// arguments are `k t p omega_secrets omega_shares n_idx index...`; prints whether the points repeat, then
// `rows <count> stride <ks>`, then per table word its raw (Montgomery) value and the canonical value it stands for,
// row by row, pad words included.  The program itself holds the canonical words against make_check_weights and
// make_repair_tables (exit status 3 on a difference).  Host code only: built for the host alone, with sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include "../../sda_amd/csrc/packed_common.h"

int main(int argc, char** argv) {
    using namespace sda::packed;
    if (argc < 7) return 2;
    const uint32_t k = (uint32_t)atoi(argv[1]), t = (uint32_t)atoi(argv[2]), n_idx = (uint32_t)atoi(argv[6]);
    const int64_t p = atoll(argv[3]), ws = atoll(argv[4]), wn = atoll(argv[5]);
    if ((uint32_t)argc != 7 + n_idx || n_idx < k + t) return 2;
    std::vector<uint64_t> idx;
    for (uint32_t i = 0; i < n_idx; ++i) idx.push_back((uint64_t)atoll(argv[7 + i]));
    const CheckTable tab = make_check_table(idx.data(), n_idx, k, t, p, ws, wn);
    printf("duplicate %d\n", (int)tab.duplicate);
    if (tab.duplicate) return tab.words.empty() ? 0 : 3;
    const uint32_t kt = k + t, r = n_idx - kt, ks = (kt + 1) & ~1u;
    printf("rows %llu stride %u\n", (unsigned long long)(tab.words.size() / ks), ks);
    if (tab.words.size() != (size_t)(r + k + 1) * ks) return 3;
    const int64_t rinv = h_modinv(((int64_t)1 << 32) % p, p);            // out of Montgomery form: x R^-1 mod p
    std::vector<int64_t> canon;
    for (uint32_t x : tab.words) {
        canon.push_back((int64_t)((unsigned __int128)x * (uint64_t)rinv % (uint64_t)p));
        printf("%u %lld\n", x, (long long)canon.back());
    }
    // the same words from the builders the table is made of
    const RevealTables T = make_reveal_tables(idx.data(), n_idx, k, p, ws, wn);
    const std::vector<int64_t> w = r ? make_check_weights(T, n_idx, kt, p) : std::vector<int64_t>();
    const RepairTables R = make_repair_tables(T, n_idx, k, kt, p, ws, w);
    for (uint32_t i = 0; i < kt; ++i) {
        for (uint32_t c = 0; c < r; ++c)
            if (canon[(size_t)c * ks + i] != w[(size_t)c * kt + i]) return 3;
        for (uint32_t e = 0; e < k; ++e)
            if (canon[(size_t)(r + e) * ks + i] != R.lam[(size_t)e * kt + i]) return 3;
        if (canon[(size_t)(r + k) * ks + i] != (r ? R.winv[i] : 0)) return 3;
    }
    return 0;
}
