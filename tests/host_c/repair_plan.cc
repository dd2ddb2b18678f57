// packed_repair_plan (sda_amd/csrc/repair_plan.h) as a filter, for tests/test_repair_plan.py: reads lines of
// `n_idx k t` from stdin and prints, for each, the plan's `redundancy path bucket locate` (path: nothing / fused /
// composed).  Includes only the plan header.
#include <inttypes.h>
#include <stdio.h>

#include "../../sda_amd/csrc/repair_plan.h"

int main() {
    static const char* const kPath[] = {"nothing", "fused", "composed"};
    uint32_t n_idx, k, t;
    while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &n_idx, &k, &t) == 3) {
        const sda::PackedRepairPlan pl = sda::packed_repair_plan(n_idx, k, t);
        if (pl.path > sda::kRepairComposed) return 2;
        printf("%" PRIu32 " %s %" PRIu32 " %d\n", pl.redundancy, kPath[pl.path], pl.bucket, (int)pl.locate);
    }
    return feof(stdin) ? 0 : 1;       // a line that does not parse is an error, not the end
}
