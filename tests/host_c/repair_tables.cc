// make_repair_tables (sda_amd/csrc/packed_common.h) as a stand-alone program, for tests/test_repair_tables.py: the
// arguments are `k t p omega_secrets omega_shares n_idx index...`; prints whether the points repeat, then the
// k * (k + t) canonical basis Lagrange words lam[e][s], row by row, then the k + t inverse weights winv[s] (none when
// n_idx == k + t).  Host code only: it is built for the host alone, with sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include "../../sda_amd/csrc/packed_common.h"

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    const uint32_t k = (uint32_t)atoi(argv[1]), t = (uint32_t)atoi(argv[2]), n_idx = (uint32_t)atoi(argv[6]);
    const int64_t p = atoll(argv[3]), ws = atoll(argv[4]), wn = atoll(argv[5]);
    if ((uint32_t)argc != 7 + n_idx || n_idx < k + t) return 2;
    std::vector<uint64_t> idx;
    for (uint32_t i = 0; i < n_idx; ++i) idx.push_back((uint64_t)atoll(argv[7 + i]));
    const sda::packed::RevealTables T = sda::packed::make_reveal_tables(idx.data(), n_idx, k, p, ws, wn);
    printf("duplicate %d\n", (int)T.duplicate);
    if (T.duplicate) return 0;
    std::vector<int64_t> w;
    if (n_idx > k + t) w = sda::packed::make_check_weights(T, n_idx, k + t, p);
    const sda::packed::RepairTables R = sda::packed::make_repair_tables(T, n_idx, k, k + t, p, ws, w);
    for (int64_t x : R.lam) printf("%lld\n", (long long)x);
    for (int64_t x : R.winv) printf("%lld\n", (long long)x);
    return 0;
}
