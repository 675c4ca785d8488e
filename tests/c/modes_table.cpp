// Prints the table of render_kernel's modes (csrc/rt_modes.h), one line per number 0 .. 14; tests/test_modes.py compares it with the
// expressions the table replaced.  A line:
//   mode=M pixels=P pass=S map=B log=B hits=B inverse=M words1=N words16=N words64=N built=<eight digits: block 256, 512, 768, 1024, each tex 0 then 1>
// pixels: 0 frame rows, 1 footprint list, 2 pixel list, 3 none; pass: 0 fused, 1 pass A, 2 pass B, 3 ray list, 4 camera hits.
#include "../../ray-tracing-fsharp_amd/csrc/rt_modes.h"

#include <cstdio>

int main() {
    printf("count=%d outside=%d,%d\n", (int) rtmode::MODE_COUNT, rtmode::mode_of(rtmode::mode_desc(-1)), rtmode::mode_of(rtmode::mode_desc(rtmode::MODE_COUNT)));
    for (int m = 0; m < rtmode::MODE_COUNT; ++m) {
        const rtmode::ModeDesc d = rtmode::mode_desc(m);
        printf("mode=%d pixels=%d pass=%d map=%d log=%d hits=%d inverse=%d words1=%u words16=%u words64=%u built=", m, (int) d.pixels, (int) d.pass, (int) d.map,
               (int) d.ray_log, (int) d.hits, rtmode::mode_of(d), rtmode::wave_words(m, 1u), rtmode::wave_words(m, 16u), rtmode::wave_words(m, 64u));
        for (int block = 256; block <= 1024; block += 256)
            for (int tex = 0; tex < 2; ++tex) printf("%d", (int) rtmode::is_built(m, block, tex != 0));
        printf(" every_block=%d textured=%d\n", (int) rtmode::built_for_every_block(m), (int) rtmode::has_textured_variant(m));
    }
    return 0;
}
