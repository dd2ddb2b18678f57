// packed_check_plan (sda_amd/csrc/check_plan.h) as a filter, for tests/test_check_plan.py: reads lines of
// `n_idx k t` from stdin and prints, for each, the plan's `redundancy path bucket locate` (path: nothing /
// registers / looped).  Includes only the plan header.
#include <inttypes.h>
#include <stdio.h>

#include "../../sda_amd/csrc/check_plan.h"

int main() {
    static const char* const kPath[] = {"nothing", "registers", "looped"};
    uint32_t n_idx, k, t;
    while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &n_idx, &k, &t) == 3) {
        const sda::PackedCheckPlan pl = sda::packed_check_plan(n_idx, k, t);
        if (pl.path > sda::kCheckLooped) return 2;
        printf("%" PRIu32 " %s %" PRIu32 " %d\n", pl.redundancy, kPath[pl.path], pl.bucket, (int)pl.locate);
    }
    return feof(stdin) ? 0 : 1;       // a line that does not parse is an error, not the end
}
