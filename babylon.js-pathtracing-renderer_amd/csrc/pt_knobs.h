// pt_knobs.h — the tunables a context takes from the environment when it is created (INTEGRATION.md lists
// them for users): one struct with the defaults and what was measured for them, and the one function that
// reads the PT_* variables. Plain host C++, no HIP: tests/test_knobs.py compiles it on its own.
#pragma once
#include <climits>
#include <cstdlib>
#include <cstring>

namespace pt {

constexpr int kDepthMax = 6;   // side streams: frames whose path tracing may be in flight at once
constexpr int kLagMax = 6;     // buffer sets beyond the side streams

struct Knobs {
    // Frame overlap of the megakernel's draws (PT_OVERLAP=0 turns it off): draw k's path tracing on side
    // stream k % depth beside the frames before it (pt_capi.cpp, Dev)
    int overlap = 1;
    // (PT_MOVING_SERIAL) frames drawn with uCameraIsMoving set run alone, one frame in flight: while the
    // camera moves, the user sees each frame as soon as it is done instead of two frames later
    int moving_serial = 1;
    // (PT_OVERLAP_DEPTH, 2-6) r05q: three frames in flight, with compaction, won on every workload but the bunny
    int depth = 3;
    bool depth_env = false;       // PT_OVERLAP_DEPTH given: the auto mode's default keeps it
    // (PT_OVERLAP_LAG, -1 = auto) auto is 2 for draws that trace fewer than lag_pixels pixels and 0 above: a
    // small frame (a rank's bands of an N-GPU frame) fills the chip only with more frames in flight, a 1080p
    // one lost 3-4 % to the extra lag (r05an: 260-520 kpx +4-10 %, 1 Mpx and up -3 %)
    int lag = -1;
    int lag_pixels = 800000;      // (PT_OVERLAP_LAG_PIXELS)
    // late-bounce compaction of the megakernel's mesh draws (PT_CONT: 0 off, 1 on, 2 auto); the bounce from
    // which, and the live lanes at or below which, a wave hands its paths on; the refill batch and pt_cont's
    // one-wave workgroups
    int cont_mode = 2;
    int cont_bounce = 2, cont_lanes = 48, cont_refill = 16, cont_waves = 2048;
    bool cont_waves_env = false;  // PT_CONT_WAVES given: it applies to every draw
    // pt_cont's waves for draws that trace at least cont_big_pixels (PT_CONT_WAVES_BIG, PT_CONT_BIG_PIXELS): beside
    // a 4K frame's path tracing fewer of them leave more wave slots to the next frames (dragon stand-in 4K
    // +3.2 to +3.9 %, helmet 4K +0.9 %, a rank's half of the 4K frame +1.5 %, 2560x1440 +1.1 %; 1080p keeps
    // 2048: 1536 there -1.8 %; profiles/r06bc_*, r06bd_*, r06be_*)
    int cont_waves_big = 1024;
    int cont_big_pixels = 3000000;
    int cont_auto_pixels = 2000000;   // (PT_CONT_AUTO_PIXELS) auto, before the trial: on from 2 MP traced (1080p)
    int cont_sort = 1;            // (PT_CONT_SORT) pt_cont takes its records ordered by a ray key (0: as stored)
    // (PT_CONT_SORT_GRID, 1-3) the key's cells per axis as bits; unset, draws that trace cont_big_pixels or more
    // take 3 (4K: dragon stand-in +0.4 %, helmet +1.1 %, profiles/r06bj_*; at 1080p the helmet lost 5.5 %)
    int cont_grid_bits = 2;
    bool cont_grid_env = false;   // PT_CONT_SORT_GRID given: it applies to every draw
    int persist_tiles = 4;        // persistent backend: 8x8 wave tiles per wave (PT_PERSIST_TILES)
    int persist_refill = 16;      // ... finished lanes that trigger a refill (PT_PERSIST_REFILL)
    // longest-first dispatch of the megakernel (PT_LPT=0 disables; 2: the order taken from both ends alternately)
    int lpt = 1, lpt_zig = 0;
    // (PT_LPT_ZIG_CONT) from both ends for compacting draws of up to lpt_flat_tiles tiles (dragon stand-in 1080p
    // +1.5 %, helmet +1.6 %, profiles/r06bo_*; uncompacted the bunny lost 1.4 %, at 4K the flattened order 1.9 %)
    int zig_cont = 1;
    int split_tiles = 32;         // (PT_SPLIT_TILES) at most this many of the slowest tiles shaded by 16-lane waves
    int split_near = 3;           // (PT_SPLIT_NEAR) ... those within this many cost buckets (1/8 octave) of the slowest
    int split_dominance = 8;      // ... when the slowest wave costs this many times the mean (PT_SPLIT_ALWAYS=1: 0)
    // (PT_LPT_FLAT, -1 = off) the tiles more than this many buckets below the slowest are dealt as one bucket, in
    // about row-major order (orderBuild). 6: dragon stand-in 4K +1.6-2.2 %, helmet 4K +8 %, sky + dragon 4K
    // +0.9 %, bunny 4K ±0 (profiles/r06g_frames_lpt_flat_4k.log); 1080p frames keep the whole order
    int lpt_flat = 6;
    int lpt_flat_tiles = 8192;    // (PT_LPT_FLAT_TILES) ... for frames of more than this many tiles
    int fuse_order = 1;           // (PT_FUSE_ORDER) the order build rides along with the next screenOutput; 0: alone
    // (PT_FUSE_BLEND) a megakernel draw's blend waits for the render loop's screenCopy and screenOutput and runs
    // folded into the output pass (pt_output_f1; frames of up to 8192 tiles), the copy target left stale (pt_plan.h MainPlan); 0: pt_blend
    // right after the draw, the copy riding along with the output
    int fuse_blend = 1;
    // (PT_MAIN_WAVES) pt_blend / pt_output as up to this many one-wave workgroups (0: 4-wave blocks) for frames
    // of up to 8192 tiles (r05bi: dragon stand-in 1080p +2 %, helmet +3 %; at 4K -4 %)
    int main_waves = 16384;
    // (PT_DRAW_EVENTS) per-draw events for pt_last_render_ms from the start: each hipEventRecord costs ~5 us of
    // stream time between two kernels (r02h: +1.7 % dragon stand-in, +3.8 % bunny)
    int draw_events = 0;
    int bvh_layout = 1;           // (PT_BVH_LAYOUT) reference 0 | pairs 1 | trail 2, as pt.h's pt_bvh_layout
};

// lo == hi == 0: a switch (any non-zero number is 1)
struct KnobRow { const char* name; int Knobs::*field; long lo, hi; };
constexpr KnobRow kKnobTable[] = {
    { "PT_OVERLAP", &Knobs::overlap, 0, 0 },
    { "PT_MOVING_SERIAL", &Knobs::moving_serial, 0, 0 },
    { "PT_OVERLAP_LAG", &Knobs::lag, -1, kLagMax },
    { "PT_OVERLAP_LAG_PIXELS", &Knobs::lag_pixels, 0, INT_MAX },
    { "PT_CONT", &Knobs::cont_mode, 0, 2 },
    { "PT_CONT_BOUNCE", &Knobs::cont_bounce, 2, INT_MAX },
    { "PT_CONT_LANES", &Knobs::cont_lanes, 1, 64 },
    { "PT_CONT_REFILL", &Knobs::cont_refill, 1, 64 },
    { "PT_CONT_WAVES_BIG", &Knobs::cont_waves_big, 1, INT_MAX },
    { "PT_CONT_BIG_PIXELS", &Knobs::cont_big_pixels, 0, INT_MAX },
    { "PT_CONT_AUTO_PIXELS", &Knobs::cont_auto_pixels, 0, INT_MAX },
    { "PT_CONT_SORT", &Knobs::cont_sort, 0, 0 },
    { "PT_PERSIST_TILES", &Knobs::persist_tiles, 1, INT_MAX },
    { "PT_PERSIST_REFILL", &Knobs::persist_refill, 1, 64 },
    { "PT_LPT_ZIG_CONT", &Knobs::zig_cont, 0, 0 },
    { "PT_SPLIT_TILES", &Knobs::split_tiles, 0, INT_MAX },
    { "PT_SPLIT_NEAR", &Knobs::split_near, 1, 128 },
    { "PT_LPT_FLAT", &Knobs::lpt_flat, -1, 127 },
    { "PT_LPT_FLAT_TILES", &Knobs::lpt_flat_tiles, 0, 1 << 21 },
    { "PT_FUSE_ORDER", &Knobs::fuse_order, 0, 0 },
    { "PT_MAIN_WAVES", &Knobs::main_waves, 0, INT_MAX },
    { "PT_DRAW_EVENTS", &Knobs::draw_events, 0, 0 },
};
// ... and the ones read_knobs writes out, by name (for listings)
constexpr const char* kKnobsWrittenOut[] = { "PT_LPT", "PT_OVERLAP_DEPTH", "PT_CONT_WAVES", "PT_CONT_SORT_GRID",
                                             "PT_SPLIT_ALWAYS", "PT_BVH_LAYOUT" };

// a variable's text as a number in lo..hi (no digits: 0, as atoi; too long for a long: the nearer end)
inline int knob_int(const char* text, long lo, long hi)
{
    const long v = std::strtol(text, nullptr, 10);   // (saturates at LONG_MIN / LONG_MAX)
    return (int)(v < lo ? lo : v > hi ? hi : v);
}

inline const char* knob_env(const char* name) { return std::getenv(name); }

// PT_TIMING_EVERY, read at every pt_timing_begin: the window brackets every k-th draw of a program kind
inline int knob_timing_every(int now) { const char* v = knob_env("PT_TIMING_EVERY"); return v ? knob_int(v, 1, INT_MAX) : now; }

inline void read_knobs(Knobs& k, const char* (*get)(const char*) = knob_env)
{
    for (const KnobRow& r : kKnobTable)
        if (const char* v = get(r.name)) k.*r.field = r.lo == 0 && r.hi == 0 ? knob_int(v, LONG_MIN, LONG_MAX) != 0 : knob_int(v, r.lo, r.hi);
    if (const char* v = get("PT_LPT")) {
        const int m = knob_int(v, INT_MIN, INT_MAX);
        k.lpt = m != 0;
        k.lpt_zig = m == 2;
    }
    if (const char* v = get("PT_OVERLAP_DEPTH")) { k.depth = knob_int(v, 2, kDepthMax); k.depth_env = true; }
    if (const char* v = get("PT_CONT_WAVES")) { k.cont_waves = knob_int(v, 1, INT_MAX); k.cont_waves_env = true; }
    if (const char* v = get("PT_CONT_SORT_GRID")) { k.cont_grid_bits = knob_int(v, 1, 3); k.cont_grid_env = true; }
    if (const char* v = get("PT_FUSE_BLEND")) k.fuse_blend = knob_int(v, LONG_MIN, LONG_MAX) != 0;   // a switch, as the table's
    if (const char* v = get("PT_SPLIT_ALWAYS")) k.split_dominance = knob_int(v, INT_MIN, INT_MAX) ? 0 : 8;
    if (const char* v = get("PT_BVH_LAYOUT"))   // reference | pairs | trail: the context's initial walk
        k.bvh_layout = !std::strcmp(v, "trail") ? 2 : !std::strcmp(v, "reference") ? 0 : 1;
}

}  // namespace pt
