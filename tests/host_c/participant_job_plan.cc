// Stand-alone check of sda_amd/csrc/participant_job_plan.h (HIP-free), built with a host sanitizer by
// tests/test_participant_job_plan.py: the payload bound against a scalar encoder over the extreme values, and the
// tile plan's ranges (they cover every secret once, in order, within the sizes the host job allocates).
#include "../../sda_amd/csrc/participant_job_plan.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

using namespace sda;

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

// the codec's encoder, one value (zigzag, 7 bits a byte)
static size_t encode(int64_t v, std::vector<uint8_t>* out) {
    uint64_t z = ((uint64_t)v << 1) ^ (uint64_t)(v >> 63);
    size_t n = 0;
    do {
        uint8_t b = z & 127;
        z >>= 7;
        out->push_back(z ? b | 128 : b);
        ++n;
    } while (z);
    return n;
}

int main() {
    const int64_t moduli[] = {1, 2, 64, 65, 433, 2147482801, (int64_t)1 << 31, ((int64_t)1 << 31) + 1,
                              ((int64_t)1 << 34), ((int64_t)1 << 34) + 1, 68719676673, 6148914691236517205,
                              INT64_MAX};
    std::vector<uint8_t> buf;
    for (int64_t m : moduli) {
        const uint32_t bound = varint_bound_mod(m);
        // the extremes of (-m, m) meet the bound or stay below it, and one of them reaches it
        const size_t hi = encode(m - 1, &buf), lo = encode(-(m - 1), &buf);
        CHECK(hi == varint_len(m - 1) && lo == varint_len(-(m - 1)));
        CHECK(hi <= bound && lo <= bound && (hi == bound || lo == bound));
        CHECK(encode(0, &buf) == 1 && varint_len(0) == 1);
        if (m <= ((int64_t)1 << 34)) CHECK(bound <= 5);
    }
    CHECK(varint_bound_mod(0) == 10 && varint_bound_mod(-433) == 10);
    CHECK(varint_len(INT64_MIN) == 10 && varint_len(INT64_MAX) == 10 && encode(INT64_MIN, &buf) == 10);
    CHECK(varint_bound_mod(433) == 2 && varint_bound_mod(2147482801) == 5 && varint_bound_mod(INT64_MAX) == 10);

    // bounds of whole jobs
    uint64_t row, mask;
    ParticipantJobShape packed{1, 2147482801, 0, true, 2147482801, 8, 26};
    CHECK(participant_job_bound(packed, 0, &row, &mask) && row == 0 && mask == 0);
    CHECK(participant_job_bound(packed, 9, &row, &mask) && row == 2 * 5 && mask == 9 * 5);
    ParticipantJobShape chacha{2, 433, 9, false, 433, 1, 3};
    CHECK(participant_job_bound(chacha, 100, &row, &mask) && row == 100 * 2 && mask == 9 * kSeedWordBytes);
    ParticipantJobShape none1{0, 0, 0, false, 433, 1, 1};    // one Additive clerk, no masking: the raw secret
    CHECK(participant_job_bound(none1, 7, &row, &mask) && row == 70 && mask == 0);
    ParticipantJobShape full1{1, 433, 0, false, 2147482801, 1, 1};
    CHECK(participant_job_bound(full1, 7, &row, &mask) && row == 14 && mask == 14);
    CHECK(!participant_job_bound(none1, UINT64_MAX / 4, &row, &mask));     // 10 bytes a value: past 64 bits

    // tile plans: every unit once, in order; no tile above the plan's size
    const uint64_t dims[] = {0, 1, 7, 8, 9, 2049, 3 * 2048 * 8 + 5};
    const uint64_t overrides[] = {0, 1, 2, 3, 2049, UINT64_MAX};
    for (const ParticipantJobShape& s : {packed, chacha, none1}) {
        const uint64_t k = s.packed ? s.k : 1;
        for (uint64_t D : dims)
            for (uint64_t ov : overrides)
                for (uint64_t stage : {(uint64_t)1, (uint64_t)4096, (uint64_t)256 << 20}) {
                    const ParticipantTilePlan p = participant_job_tiles(s, D, s.packed ? 4 : 8, stage, ov);
                    CHECK(p.units == (D + k - 1) / k && p.tile >= 1 && p.unit_bytes > 0);
                    CHECK((p.tiles == 0) == (D == 0));
                    if (ov && ov <= p.units) CHECK(p.tile == ov);
                    if (!ov && D) CHECK(p.tile == 1 || p.tile * p.unit_bytes <= stage || p.tile == p.units);
                    std::vector<uint8_t> seen(D, 0);
                    uint64_t next = 0;
                    for (uint64_t i = 0; i < p.tiles; ++i) {
                        const uint64_t u0 = i * p.tile, u1 = u0 + p.tile < p.units ? u0 + p.tile : p.units;
                        const uint64_t s0 = u0 * k, s1 = u1 * k < D ? u1 * k : D;
                        CHECK(u0 < u1 && s0 == next && s0 < s1 && u1 - u0 <= p.tile);
                        for (uint64_t e = s0; e < s1; ++e) seen[e]++;
                        next = s1;
                    }
                    CHECK(next == D);
                    for (uint64_t e = 0; e < D; ++e) CHECK(seen[e] == 1);
                }
    }
    printf("participant_job_plan OK\n");
    return 0;
}
