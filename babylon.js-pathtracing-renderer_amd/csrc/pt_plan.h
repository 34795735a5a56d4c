// pt_plan.h — the draw schedule's arithmetic (pt_capi.cpp issues the HIP calls it decides): which bands a
// partition owns, how a buffer set's compaction slab is laid out, which buffer set / side stream / mark a
// megakernel draw takes, its grid, and the auto trial of late-bounce compaction. Plain host C++ over plain
// numbers, no HIP and no allocation: tests/test_plan.py compiles it on its own and checks it by hand-worked cases.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pt_knobs.h"

namespace pt {

constexpr int kBlock = 256;          // 4 waves; a block shades a 16x16 pixel tile
constexpr int kTile = 16;            // tile edge == row-band height used for sharding
// split tiles (pt_trace, longest-first): each 8x8 quadrant of a split 16x16 tile is shaded by this
// many waves of 64 / kSplitParts lanes (4x4-pixel waves of 16 lanes; one 2x2 quad per wave measured
// slower)
constexpr unsigned kSplitParts = 4;
constexpr unsigned kOrderHeld = 128;   // pt_order_build: tiles per thread kept in registers (a byte each)
constexpr int kSortBins = 8192;   // (PT_CONT_SORT) the record keys at most: light flag x 8 octants x 8^3 cells

constexpr size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// the 16-row bands of a frame of `height` rows that partition `part` of `parts` owns (band b: b % parts == part)
inline int bands_owned(int height, int parts, int part)
{
    const int nb = (height + kTile - 1) / kTile;
    return part < nb ? (nb - part + parts - 1) / parts : 0;
}

// the pixels a partition's draw traces: its owned bands (a bound on its compaction records) ...
inline size_t owned_pixels(int w, int h, int parts, int part)
{
    const size_t all = (size_t)w * h, own = (size_t)bands_owned(h, parts, part) * kTile * w;
    return own < all ? own : all;
}
// ... and about: what the measured thresholds (lag_pixels, cont_auto_pixels, cont_big_pixels) were taken with
inline size_t share_pixels(int w, int h, int parts) { return (size_t)w * h / (size_t)(parts > 1 ? parts : 1); }

// the overlap lag of a draw that traces `share` pixels (Knobs::lag): by default kLagSmall below lag_pixels, 0 above
constexpr int kLagSmall = 2;
inline int draw_lag(const Knobs& k, size_t share) { return k.lag >= 0 ? k.lag : share < (size_t)k.lag_pixels ? kLagSmall : 0; }

// One buffer set's slab of pt_cont's records, for `cap` records (a record per traced pixel at most): records
// [cap x 64 B] | pixels [x 4 B] | (PT_CONT_SORT: order [x 4 B] | ranks [x 4 B] | keys [x 2 B] | the keys'
// totals) | counter block. Byte offsets from the set's start; set p starts at p * bytes.
struct ContLayout {
    // the counter block's words: [kStored] records stored by the draw, [kHead] pt_cont's queue head (both zeroed
    // by the draw's pt_blend), [kTotal..+1] the set's 64-bit running total (pt_cont_stats)
    enum : size_t { kStored = 0, kHead = 1, kTotal = 2 };
    size_t rec, aux, perm, rank, key, bins, count, bytes;
    ContLayout(size_t cap, bool sort)
    {
        rec = 0;
        aux = cap * 64;
        perm = aux + align256(cap * 4);
        rank = sort ? perm + align256(cap * 4) : perm;   // (without the sort its arrays are empty)
        key = sort ? rank + align256(cap * 4) : perm;
        bins = sort ? key + align256(cap * 2) : perm;
        count = sort ? bins + (size_t)kSortBins * 4 : perm;
        bytes = count + 256;
    }
    size_t total() const { return count + kTotal * sizeof(unsigned); }
};

// Frame overlap of the megakernel's draws (pt_capi.cpp, Dev): the sequencing state. Draw k = mk_seq takes buffer
// set k % (depth + lag) and side stream k % depth, and its path tracing waits for the mark of draw
// k - depth - lag + 1, or of the oldest draw after everything it must wait for (mark_floor).
struct Overlap {
    unsigned mk_seq = 0;          // megakernel draws so far (the host counts a draw once it is enqueued)
    bool need_fresh = true;       // the next megakernel draw must wait for everything before it (a fresh mark)
    unsigned mark_floor = 0;      // no draw waits for a mark older than draw mark_floor's
    int depth_run = 3;            // the last megakernel draw's depth (<= Knobs::depth: the auto trial may pick 2)
    int lag_run = 0;              // the last megakernel draw's lag
    struct Slot {
        int set;      // buffer set: radiance, compaction records, longest-first cost / order
        int stream;   // side stream and spill slab
        int wait;     // the buffer set whose mark the path tracing waits for (-1: the draw is not overlapped)
    };
    // where draw mk_seq goes at `depth` frames in flight and `lag` buffer sets beyond them
    Slot slot(int depth, int lag) const
    {
        return Slot{ (int)(mk_seq % (unsigned)(depth + lag)), (int)(mk_seq % (unsigned)depth), -1 };
    }
    // ... and the next draw, if it keeps the last one's depth and lag
    Slot next() const { return slot(depth_run, lag_run); }
    // this draw: another depth or lag is another buffer-set cycle, so the draw waits for everything before it;
    // a draw that is not overlapped runs on the main stream, and the next one waits for it
    Slot step(int depth, int lag, bool overlap)
    {
        if (depth != depth_run || lag != lag_run) {
            depth_run = depth;
            lag_run = lag;
            need_fresh = true;
        }
        Slot s = slot(depth, lag);
        if (!overlap) {
            need_fresh = true;
            return s;
        }
        const unsigned k = mk_seq, D = (unsigned)(depth + lag);
        if (need_fresh) { mark_floor = k; need_fresh = false; }
        // the mark of draw k - sets + 1 (its state: draw k - sets' blend, order build and output), or of the
        // oldest draw after everything this draw must wait for; the draw k - depth before it on this stream is
        // ordered by the stream
        const unsigned w = k + 1 >= D && k + 1 - D > mark_floor ? k + 1 - D : mark_floor;
        s.wait = (int)(w % D);
        return s;
    }
};

// The megakernel's grid for gx x gy tiles. Longest-first: the wave durations of the buffer set's previous draw
// order this draw's workgroups when it drew the same grid, target and program (`same`); split tiles take 12 more
// workgroups each, in padding rows. A compacting draw (`cont`) splits none: their 16-lane waves would hand
// their slowest paths to pt_cont at once (r05j: dragon stand-in 4K with both 2222 Mpaths/s, with compaction
// alone 2762).
struct MegaGrid {
    size_t n;             // 16x16 tiles
    unsigned split_cap;   // the tiles the order build may mark for splitting (a multiple of 8, <= n)
    unsigned split;       // ... and the padding this draw's grid carries for them
    int gy_grid;          // rows of the grid with the padding rows
    size_t lanes;         // lanes of that grid (the spill slab's stride)
    bool one_wave;        // pt_blend as one-wave workgroups: up to 8192 tiles, as the output pass
    // 1: the order taken from both ends (runs of 8 tiles: the slowest, the cheapest, ...), also for compacting draws
    // whose order is not flattened: with the slowest tiles' late bounces handed to pt_cont, cheap tiles mixed in
    // early keep the slots full (dragon stand-in 1080p +1.5 %, its 20-frame run +1.7 %, helmet +1.6 %, three
    // rounds, profiles/r06bo_*; uncompacted the bunny lost 1.4 %, and at 4K the flattened order 1.9 %)
    unsigned order_zig;
    MegaGrid(int gx, int gy, bool same, bool cont, const Knobs& k)
    {
        n = (size_t)gx * gy;
        split_cap = (unsigned)((size_t)k.split_tiles < n ? (size_t)k.split_tiles : n) & ~7u;
        split = same && !cont ? split_cap : 0u;
        const unsigned extra = 4u * kSplitParts - 4u;   // more workgroups per split tile
        gy_grid = gy + (int)((extra * split + 4u * gx - 1) / (4u * gx));
        lanes = (size_t)gx * gy_grid * kBlock;
        one_wave = n <= kOrderHeld * 64u;
        order_zig = k.lpt_zig || (cont && k.zig_cont && n <= (size_t)k.lpt_flat_tiles) ? 1u : 0u;
    }
    // pt_cont's one-wave workgroups for a draw of `share` pixels (the sky composite keeps cont_waves: its sky
    // pixels store few records, and 1024 waves cost it 0.5 %)
    int cont_waves(const Knobs& k, size_t share, bool sky_composite) const
    {
        const bool big = !k.cont_waves_env && share >= (size_t)k.cont_big_pixels && !sky_composite;
        const size_t waves = (size_t)(big ? k.cont_waves_big : k.cont_waves);
        return (int)(waves < 4 * n ? waves : 4 * n);
    }
    // the record key's cells per axis, as bits: 8x8x8 for draws that trace cont_big_pixels or more (4K: dragon
    // stand-in +0.4 %, helmet +1.1 %, sky + dragon +0.6 %, three rounds, profiles/r06bj_*; at 1080p the helmet
    // lost 5.5 % with them, r06ao_*)
    static unsigned sort_grid_bits(const Knobs& k, size_t share)
    {
        return k.cont_grid_env || share < (size_t)k.cont_big_pixels ? (unsigned)k.cont_grid_bits : 3u;
    }
};

// Auto mode of late-bounce compaction (Knobs::cont_mode 2). Compaction pays on the heavy 4K frames (sky + dragon
// +19 %, dragon stand-in +10 %) and costs elsewhere (bunny 4K -22 %, helmet -9 %, rank-sized frames -29 %:
// profiles/r05i_*), which the draw's arguments do not tell apart. So the draws of one target / program /
// partition time it: after kContSkip draws (the last two compacting, to warm it up on the side streams), blocks
// of kContBlock draws with it on and off, kContMeasured draws inside each timed by events on the main stream; at
// the trial's end the host waits for it once, and compaction stays on only if its faster block took 2 % less
// time than the faster block without. Same bits either way.
// The blocks without compaction also try two frames in flight instead of three (on, off, off at depth 2 twice,
// off, on): the light frames that do not compact lost 2-5 % to the third frame (r05q: bunny 5365 vs 5228
// Mpaths/s, bunny16 -4.5 %), so the faster depth stays with "off".
// The trial starts at the 33rd draw of a target: short runs (the driver's 5 + 20 frames) stay in the default,
// longer ones settle on the measured best.
constexpr int kContSkip = 32, kContBlock = 10, kContSettle = 3, kContMeasured = 5, kContBlocks = 6;

struct ContTrial {
    struct Key { const void* target; int prog, part, parts, w, h; };
    struct Draw {
        bool on;      // the draw compacts
        int depth;    // its frames in flight
        int event;    // the trial event to record on the main stream before the draw (0 .. 2 * kContBlocks - 1), or -1
        bool ends;    // the trial ends at this draw: wait for its last event, then conclude()
        // what the draw did, for pt_queue_stats: 0 off, 1 auto decided off, 2 auto decided on, 3 forced on,
        // 4 auto trial, 5 / 6 the default before the trial on / off
        int code;
    };
    Key key = {};
    int seen = 0;                 // megakernel draws of this key so far
    bool decided = false, choice = false;
    int depth = 0;                // the frames in flight the decision keeps
    float ms_on = 0.0f, ms_off = 0.0f, ms_off2 = 0.0f;

    // Whether this draw compacts. `alone`: a moving-camera draw that runs alone never compacts and is no draw of
    // the trial - it leaves the state as it is (not counted, no event) and only takes the frames in flight a still
    // draw in its place would.
    Draw draw(const Key& now, bool eligible, bool alone, size_t share, const Knobs& k)
    {
        Draw d{ false, k.depth, -1, false, 0 };
        if (!eligible || k.cont_mode == 0) return d;
        if (k.cont_mode == 1) {
            d.on = !alone;
            d.code = d.on ? 3 : 0;
            return d;
        }
        bool same = key.target == now.target && key.prog == now.prog && key.part == now.part && key.parts == now.parts &&
                    key.w == now.w && key.h == now.h;
        if (!same && !alone) {
            *this = ContTrial();
            key = now;
            depth = k.depth;
            same = true;
        }
        const int i = (alone ? (same ? seen : 0) : seen++) - kContSkip;
        decide(d, i, same, alone, share, k);
        if (alone) {
            d.on = false;
            d.code = 0;
        } else if (!d.ends) {
            d.code = decided ? (choice ? 2 : 1) : seen > kContSkip ? 4 : d.on ? 5 : 6;
        }
        return d;
    }

    // the trial's end: the six blocks' times, by block. The faster block of each mode decides (one stray block
    // cannot); every later draw of this key takes the decision
    Draw conclude(const float ms[kContBlocks])
    {
        ms_on = ms_off = ms_off2 = 1e30f;
        for (int b = 0; b < kContBlocks; b++) {
            float& m = b == 0 || b == kContBlocks - 1 ? ms_on : b == 2 || b == 3 ? ms_off2 : ms_off;
            if (ms[b] < m) m = ms[b];
        }
        decided = true;
        const bool two = ms_off2 < ms_off;
        choice = ms_on < 0.98f * (two ? ms_off2 : ms_off);
        if (!choice && two && depth > 2) depth = 2;   // (depth: Knobs::depth since the trial began)
        return Draw{ choice, depth, -1, false, choice ? 2 : 1 };
    }

private:
    void decide(Draw& d, int i, bool same, bool alone, size_t share, const Knobs& k)
    {
        const int two = k.depth < 2 ? k.depth : 2;
        if (same && decided) {
            d.on = choice;
            d.depth = depth;
            return;
        }
        // before the trial, the default: on for frames of at least cont_auto_pixels (with three frames in
        // flight it won on every frame of 2 MP and more but the light bunny, and lost on the rank-sized one,
        // profiles/r05q_frames_depth_x_compaction.txt); the two draws before the trial compact, one per side
        // stream of the last two buffer sets, whatever the default: the first launch of a variant that needs
        // more scratch than any before it waits for the device to drain while the runtime grows its scratch
        // (r05k: the first trial block then took 2-8x the others)
        if (i < 0) {
            // (`share`, the pixels this partition traces: a rank's bands of an N-GPU frame are a small frame -
            // r05ao: 0.5-1 Mpx frames lost 33-41 % to compaction)
            d.on = share >= (size_t)k.cont_auto_pixels || i >= -2;
            // without compaction, frames of lag_pixels and more keep two frames in flight (r05aw: the
            // 4K frame's eighth at N = 8 +5.6 %; r05y: StanfordBunny 1080p +3.5 %), smaller ones three
            // and the lag (a 1920x136 frame: two lost a third, r05aa)
            if (!d.on && !k.depth_env && share >= (size_t)k.lag_pixels) d.depth = two;
            return;
        }
        // each block times draws S .. S + M - 1 of its own: an event on the main stream (the work before the
        // draw: the previous draw's blend, which waited for its path tracing) at the block's offsets S and
        // S + M. With up to `depth` frames in flight, S draws settle the switch (buffer sets whose
        // longest-first order came from the other mode's costs) and the block's last B - S - M draws keep the
        // next block's frames out of the timed ones.
        constexpr int B = kContBlock, S = kContSettle, M = kContMeasured, trial = kContBlocks * B;
        const int b = i / B, o = i % B;
        if (i < trial) {
            if ((o == S || o == S + M) && !alone) d.event = 2 * b + (o == S ? 0 : 1);
            d.on = b == 0 || b == kContBlocks - 1;   // on, off, off at depth 2 (twice), off, on
            if (b == 2 || b == 3) d.depth = two;
            return;
        }
        d.ends = !alone;   // (after the trial's draws, the next still draw ends it)
    }
};

}  // namespace pt
