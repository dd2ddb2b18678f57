// make_decode_table (sda_amd/csrc/decode_tables.h) as a stand-alone program, for tests/test_decode_table.py: the
// arguments are `k t p omega_secrets omega_shares rmax n_idx index...`; prints whether the points repeat, then every
// word of the table, one per line (Montgomery form, as the device reads them).  Host code only: it is built for the
// host alone, with sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include "../../sda_amd/csrc/decode_tables.h"

int main(int argc, char** argv) {
    if (argc < 8) return 2;
    const uint32_t k = (uint32_t)atoi(argv[1]), t = (uint32_t)atoi(argv[2]), rmax = (uint32_t)atoi(argv[6]);
    const uint32_t n_idx = (uint32_t)atoi(argv[7]);
    const int64_t p = atoll(argv[3]), ws = atoll(argv[4]), wn = atoll(argv[5]);
    if ((uint32_t)argc != 8 + n_idx || n_idx < k + t) return 2;
    std::vector<uint64_t> idx;
    for (uint32_t i = 0; i < n_idx; ++i) idx.push_back((uint64_t)atoll(argv[8 + i]));
    const sda::packed::DecodeTable T = sda::packed::make_decode_table(idx.data(), n_idx, k, t, p, ws, wn, rmax);
    printf("duplicate %d\n", (int)T.duplicate);
    for (uint32_t w : T.words) printf("%u\n", w);
    return 0;
}
