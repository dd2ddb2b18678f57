// The decoder core (sda_amd/csrc/decode_core.h) over the decode table (decode_tables.h) as a stand-alone program, for
// tests/test_decode_core.py.  Arguments: `k t p omega_secrets omega_shares n_idx index...`; stdin: one word per line,
// n_idx canonical residues.  The program does on the host what packed_decode_kernel's lane does: the rmax syndromes
// against the table's Montgomery words, then decode_word with the plan's RMAX instantiation.  Prints per word
// `ok nu wrong_mask err...` with one canonical err per set bit of the mask, ascending (ok 0: undecodable).  Host
// code only: it is built for the host alone, with sanitizers.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../sda_amd/csrc/decode_core.h"
#include "../../sda_amd/csrc/decode_plan.h"
#include "../../sda_amd/csrc/decode_tables.h"

template <int RMAX>
static int run(const sda::packed::DecodeTable& T, uint32_t p, uint32_t r, uint32_t n_idx) {
    const sda::MontP M = sda::make_mont(p);
    const sda::decode::MontField F = sda::decode::make_field(p, M.pinv, M.r2);
    const uint32_t* xinv = T.words.data() + (size_t)RMAX * n_idx;
    const uint32_t* xs = xinv + n_idx;
    const uint32_t* vinv = xs + n_idx;
    std::vector<uint32_t> y(n_idx), err(n_idx);
    for (;;) {
        for (uint32_t j = 0; j < n_idx; ++j)
            if (scanf("%" SCNu32, &y[j]) != 1) return j == 0 && feof(stdin) ? 0 : 1;
        uint32_t S[RMAX];
        for (int c = 0; c < RMAX; ++c) {
            uint32_t acc = 0;
            for (uint32_t j = 0; j < n_idx; ++j) acc = F.add(acc, F.mul(T.words[(size_t)j * RMAX + c], y[j]));
            S[c] = F.enter(acc);
        }
        uint32_t nu = 0, wrong = 0;
        const bool ok = sda::decode::decode_word<sda::decode::MontField, RMAX>(F, p, r, n_idx, S, xinv, xs, vinv, &nu,
                                                                               &wrong, err.data());
        printf("%d %" PRIu32 " %" PRIu32, (int)ok, nu, wrong);
        for (uint32_t j = 0; j < n_idx; ++j)
            if (wrong >> j & 1u) printf(" %" PRIu32, F.leave(err[j]));
        printf("\n");
    }
}

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    const uint32_t k = (uint32_t)atoi(argv[1]), t = (uint32_t)atoi(argv[2]), n_idx = (uint32_t)atoi(argv[6]);
    const int64_t p = atoll(argv[3]), ws = atoll(argv[4]), wn = atoll(argv[5]);
    if ((uint32_t)argc != 7 + n_idx) return 2;
    const sda::PackedDecodePlan pl = sda::packed_decode_plan(n_idx, k, t);
    if (!pl.decode) return 2;
    std::vector<uint64_t> idx;
    for (uint32_t i = 0; i < n_idx; ++i) idx.push_back((uint64_t)atoll(argv[7 + i]));
    const sda::packed::DecodeTable T = sda::packed::make_decode_table(idx.data(), n_idx, k, t, p, ws, wn, pl.rmax);
    if (T.duplicate) return 3;
    printf("rmax %" PRIu32 "\n", pl.rmax);
    switch (pl.rmax) {
        case 4: return run<4>(T, (uint32_t)p, pl.redundancy, n_idx);
        case 8: return run<8>(T, (uint32_t)p, pl.redundancy, n_idx);
        case 12: return run<12>(T, (uint32_t)p, pl.redundancy, n_idx);
        case 16: return run<16>(T, (uint32_t)p, pl.redundancy, n_idx);
        case 32: return run<32>(T, (uint32_t)p, pl.redundancy, n_idx);
    }
    return 2;
}
