// The plan of the surface-record kernel (csrc/rt_surface_plan.h) on a CPU, for tests/test_surface_plan_cpp.py.  One line in, one out:
//   plan  slots cu_count scene_tex scene_prog want_tex_outputs
//   pred  kind style texture_id root_kind flipped        (the meta words are formed as the host forms them, rt_device.h's layout)
//   slot  hit_index n_hittables finite
#include "../../ray-tracing-fsharp_amd/csrc/rt_surface_plan.h"

#include <cstdio>
#include <iostream>
#include <string>

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "plan") {
            unsigned long long slots = 0;
            int cu = 0, tex = 0, prog = 0, want = 0;
            std::cin >> slots >> cu >> tex >> prog >> want;
            if (!std::cin) return 2;
            const rtsf::SurfacePlan pl = rtsf::plan(slots, cu, tex != 0, prog != 0, want != 0);
            printf("slots=%llu tile=%u block=%u tiles=%llu grid=%llu prog=%d tex_phase=%d\n", (unsigned long long) pl.slots, pl.tile, pl.block,
                   (unsigned long long) pl.tiles, (unsigned long long) pl.grid, (int) pl.prog, (int) pl.tex_phase);
        } else if (what == "pred") {
            int kind = 0, style = 0, texture = 0, flipped = 0;
            unsigned root = 0;
            std::cin >> kind >> style >> texture >> root >> flipped;
            if (!std::cin) return 2;
            const int32_t mx = (int32_t) ((unsigned) kind | ((unsigned) style << 2) | ((unsigned) flipped << 5));
            const int32_t my = (int32_t) (0x00123456u | ((unsigned) (texture + 1) << 24));
            printf("texture_of=%d phase=%d uv=%d emitter=%d\n", rtsf::texture_of(mx, my), (int) rtsf::needs_texture_phase(mx, my, root),
                   (int) rtsf::uv_filled(mx, my, root), (int) rtsf::emitter(mx));
        } else if (what == "slot") {
            long long hit = 0, n = 0;
            int finite = 0;
            std::cin >> hit >> n >> finite;
            if (!std::cin) return 2;
            printf("ok=%d none=%d\n", (int) rtsf::list_entry_ok((int32_t) hit, (int32_t) n), (int) rtsf::no_surface((int32_t) hit, (int32_t) n, finite != 0));
        } else return 2;
    }
    return 0;
}
