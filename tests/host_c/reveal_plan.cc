// packed_reveal_plan (sda_amd/csrc/reveal_plan.h) as a filter, for tests/test_reveal_plan.py: reads lines of
// `n_idx k t p mode` from stdin and prints, for each, the plan's
// `path mode MM staged KU lazy full fixup logged` (path: registers / workspace / detour; mode: the one the kernels
// run; fixup: none / wave / lane).  Includes only the plan header.
#include <inttypes.h>
#include <stdio.h>

#include "../../sda_amd/csrc/reveal_plan.h"

int main() {
    static const char* const kPath[] = {"registers", "workspace", "detour"};
    static const char* const kFixup[] = {"none", "wave", "lane"};
    uint32_t n_idx, k, t, p;
    int mode;
    while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %d", &n_idx, &k, &t, &p, &mode) == 5) {
        const sda::PackedRevealPlan pl = sda::packed_reveal_plan(n_idx, k, t, p, mode);
        if (pl.path > sda::kRevealDetour || pl.fixup > sda::kRevealFixupLane) return 2;
        printf("%s %d %d %d %d %d %d %s %d\n", kPath[pl.path], pl.mode, pl.mm, (int)pl.staged, pl.ku, (int)pl.lazy,
               (int)pl.full, kFixup[pl.fixup], (int)pl.logged);
    }
    return feof(stdin) ? 0 : 1;       // a line that does not parse is an error, not the end
}
