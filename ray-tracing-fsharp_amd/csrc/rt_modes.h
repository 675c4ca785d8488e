// rt_modes.h -- the ONE table of render_kernel's modes: what each number of its `int MODE` template parameter means, and everything
// that follows from the meaning alone (the wave's LDS scratch, which instantiations are built).  Plain C++17 with no HIP in it: the
// launch planner (rt_launch_plan.h, read by g++ in the CPU tests) chooses a mode from here, the kernel (rt_render_kernel.h) and the
// kernel table (rtfs_amd.hip) read its description from here.  tests/test_modes.py holds the table to the expressions it replaced.
//
// The NUMBERS are public: they are the q_mode / F_mode / A_mode / B_mode words of rt_dev_last_launch_plan (include/rtfs_amd.h), they are
// recorded in tests/golden/launch_plans.json, and they are part of every kernel's mangled name (profiles and scripts match on it).
//
// Per-pixel cost is heavy-tailed (a pixel on a glass sphere: ~20 rays per sample, 4 ms of one wave), so when a shard has only a few
// units per wave the fused kernel ends with most waves waiting for a few long units started late; A + sort + B removes that tail.
// Every mode computes the same integers: which wave traces which sample when has no effect (streams are per item).
#pragma once
#include "rt_launch_consts.h"

#include <cstdint>

namespace rtmode {

enum Mode : int {
    FRAME_FUSED = 0,           // a unit's pixels go through phase 1, the adaptive decision and phase 2 on one wave
    FRAME_PASS_A = 1,          // phase 1 and the decision for every pixel; pixels that continue are appended to `pairs` with the number of
                               // rays their 2k+1 samples took (a cost estimate), the others are final
    FRAME_PASS_B = 2,          // phase 2 for the pixels of `live_list`, which the host-side launch sequence has ordered by decreasing cost
                               // (longest job first); run_stream.  An extension (rt_render_extend) is this pass alone, with first_b set
    FRAME_FUSED_LOG = 3,       // FRAME_FUSED with the ray log of rt_scene_tune's probe compiled in (a dozen more scalar values live across
                               // the loop: kept out of the kernels that render frames)
    RAYS_TRACE = 4,            // the caller's rays through Scene.traceRay (run_rays, rt_trace_rays).  No pixels, so no per-wave LDS
                               // scratch: the LDS holds the scene (or the top of its tree) and the Lambert pools only
    RAYS_HIT = 5,              // the caller's rays through Scene.hitObject (run_rays, rt_hit_objects): nothing is shaded
    FOOTPRINTS_FUSED = 6,      // FRAME_FUSED / _PASS_A / _PASS_B over a caller's footprint list (rt_render_footprints): pixel i of
    FOOTPRINTS_PASS_A = 7,     // p.n_rows * p.cols is footprint i of p.rays ([n][12]: origin, base, du, dv), its stream that of
    FOOTPRINTS_PASS_B = 8,     // (seed, p.ray_base + i); a sample's ray is footprint_ray's; no pixel candidates.  Everything else -- units,
                               // accumulators, the decision, the compaction, pass B's ordered list -- is the frame's
    FRAME_PASS_B_MAP = 9,      // FRAME_PASS_B / FOOTPRINTS_PASS_B with per-pixel sample ranges (run_stream<.., MAP>): pass B of an
    FOOTPRINTS_PASS_B_MAP = 10, // extension by map (rt_render_extend_map)
    PIXELS_FUSED = 11,         // FRAME_FUSED / _PASS_A / _PASS_B over a caller's list of the FRAME's pixels (rt_render_pixels): entry i of
    PIXELS_PASS_A = 12,        // p.ray_n names the global pixel index g = p.pixel_list[i]; (row, col) = (g / cols, g % cols), the stream of
    PIXELS_PASS_B = 13,        // (seed, g), the frame's camera_ray AND its pixel candidates -- a frame's pixel in all but where it is stored,
                               // which is slot i.  An extension is PIXELS_PASS_B with first_b set
    CAMERA_HITS = 14,          // rt_camera_hits, run_camera_hits: the first object that sample s of a listed pixel's camera ray strikes -- the
                               // pixel modes' unit set-up (pix and candidate words) feeding RAYS_HIT's tail; nothing is shaded
    MODE_COUNT = 15
};

enum class Pixels { FRAME, FOOTPRINTS, LIST, NONE };               // frame rows; a footprint list; a list of the frame's pixels; a ray list
enum class Pass { FUSED, A, B, RAY_LIST, CAMERA_HITS };
struct ModeDesc {
    Pixels pixels; // where the mode's pixels come from
    Pass pass;     // which pass it is
    bool map = false;     // pass B with per-pixel sample ranges
    bool ray_log = false; // the ray log is compiled in
    bool hits = false;    // answers (hit, strike) instead of shading: no textured variant, nothing parked
};
constexpr bool operator==(const ModeDesc &a, const ModeDesc &b) {
    return a.pixels == b.pixels && a.pass == b.pass && a.map == b.map && a.ray_log == b.ray_log && a.hits == b.hits;
}

constexpr bool is_mode(int mode) { return mode >= 0 && mode < MODE_COUNT; }
// number -> description; for a number outside the table (ask is_mode) a row that no mode has, so that mode_of answers -1 for it
constexpr ModeDesc mode_desc(int mode) {
    switch (mode) {
    case FRAME_FUSED:           return {Pixels::FRAME, Pass::FUSED, false, false, false};
    case FRAME_PASS_A:          return {Pixels::FRAME, Pass::A, false, false, false};
    case FRAME_PASS_B:          return {Pixels::FRAME, Pass::B, false, false, false};
    case FRAME_FUSED_LOG:       return {Pixels::FRAME, Pass::FUSED, false, true, false};
    case RAYS_TRACE:            return {Pixels::NONE, Pass::RAY_LIST, false, false, false};
    case RAYS_HIT:              return {Pixels::NONE, Pass::RAY_LIST, false, false, true};
    case FOOTPRINTS_FUSED:      return {Pixels::FOOTPRINTS, Pass::FUSED, false, false, false};
    case FOOTPRINTS_PASS_A:     return {Pixels::FOOTPRINTS, Pass::A, false, false, false};
    case FOOTPRINTS_PASS_B:     return {Pixels::FOOTPRINTS, Pass::B, false, false, false};
    case FRAME_PASS_B_MAP:      return {Pixels::FRAME, Pass::B, true, false, false};
    case FOOTPRINTS_PASS_B_MAP: return {Pixels::FOOTPRINTS, Pass::B, true, false, false};
    case PIXELS_FUSED:          return {Pixels::LIST, Pass::FUSED, false, false, false};
    case PIXELS_PASS_A:         return {Pixels::LIST, Pass::A, false, false, false};
    case PIXELS_PASS_B:         return {Pixels::LIST, Pass::B, false, false, false};
    case CAMERA_HITS:           return {Pixels::LIST, Pass::CAMERA_HITS, false, false, true};
    default:                    return {Pixels::NONE, Pass::CAMERA_HITS, true, true, true};
    }
}
// description -> number; -1: no mode is that (the planner never asks for one: the static_asserts below cover what it asks for)
constexpr int mode_of(const ModeDesc &d) {
    for (int m = 0; m < MODE_COUNT; ++m)
        if (mode_desc(m) == d) return m;
    return -1;
}

// A wave's LDS scratch in 4-byte words, P = pixels per work unit (the layout: rt_render_kernel.h; the values: rt_launch_consts.h)
constexpr uint32_t wave_words(int mode, uint32_t P) {
    const ModeDesc d = mode_desc(mode);
    return !is_mode(mode) || d.pass == Pass::RAY_LIST ? 0u : d.pass == Pass::CAMERA_HITS ? RTD_WAVE_WORDS_CAM(P) : d.pass == Pass::A ? RTD_WAVE_WORDS_A(P) :
           d.map ? RTD_WAVE_WORDS_MAP(P) : RTD_WAVE_WORDS(P);
}

// The SET of instantiated render_kernel<...> is part of the build (compile time, code size).  Frames run at every block size (256,
// 512, 768, 1024 threads); the modes over a caller's list -- rays, footprints, pixels, camera hits -- are built for 256 and 1024 only (a
// launch asking for 512 or 768 runs at 1024: the block size never changes a result).  A mode that shades nothing evaluates no texture
// and has no textured variant.
constexpr bool built_for_every_block(int mode) { return is_mode(mode) && mode_desc(mode).pixels == Pixels::FRAME; }
constexpr bool has_textured_variant(int mode) { return is_mode(mode) && !mode_desc(mode).hits; }
constexpr bool is_built(int mode, int block, bool tex) {
    return is_mode(mode) && (built_for_every_block(mode) || block == 256 || block == 1024) && (!tex || has_textured_variant(mode));
}

// The variant with the arm of texture programs (render_prog_kernel, a scene that holds an RT_TEXTURE_PROGRAM record): every mode that has a
// textured variant, at blocks of 256 and 1024 threads only, as the list modes are -- frames too (a launch asking for 512 or 768 runs at 1024).
constexpr bool is_built_prog(int mode, int block) { return has_textured_variant(mode) && (block == 256 || block == 1024); }

constexpr bool round_trip(int m = 0) { return m == MODE_COUNT || (mode_of(mode_desc(m)) == m && round_trip(m + 1)); }
static_assert(round_trip(), "number -> description -> number holds for every mode: no two modes share a description");
static_assert(mode_of(mode_desc(MODE_COUNT)) == -1 && mode_of(mode_desc(-1)) == -1, "a number outside the table is no mode");
static_assert(FRAME_FUSED == 0 && FRAME_PASS_A == 1 && FRAME_PASS_B == 2 && FRAME_FUSED_LOG == 3 && RAYS_TRACE == 4 && RAYS_HIT == 5 &&
              FOOTPRINTS_FUSED == 6 && FOOTPRINTS_PASS_A == 7 && FOOTPRINTS_PASS_B == 8 && FRAME_PASS_B_MAP == 9 && FOOTPRINTS_PASS_B_MAP == 10 &&
              PIXELS_FUSED == 11 && PIXELS_PASS_A == 12 && PIXELS_PASS_B == 13 && CAMERA_HITS == 14 && MODE_COUNT == 15,
              "the numbers are public: plan words, recorded plans, kernel symbols");

} // namespace rtmode
