// packed_decode_plan (sda_amd/csrc/decode_plan.h) as a filter, for tests/test_decode_plan.py: reads lines of
// `n_idx k t` from stdin and prints, for each, the plan's `redundancy radius path bucket rmax decode` (path: nothing /
// first / decoded / unsupported).  Includes only the plan header.
#include <inttypes.h>
#include <stdio.h>

#include "../../sda_amd/csrc/decode_plan.h"

int main() {
    static const char* const kPath[] = {"nothing", "first", "decoded", "unsupported"};
    uint32_t n_idx, k, t;
    while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &n_idx, &k, &t) == 3) {
        const sda::PackedDecodePlan pl = sda::packed_decode_plan(n_idx, k, t);
        if (pl.path > sda::kDecodeUnsupported) return 2;
        printf("%" PRIu32 " %" PRIu32 " %s %" PRIu32 " %" PRIu32 " %d\n", pl.redundancy, pl.radius, kPath[pl.path],
               pl.bucket, pl.rmax, (int)pl.decode);
    }
    return feof(stdin) ? 0 : 1;       // a line that does not parse is an error, not the end
}
