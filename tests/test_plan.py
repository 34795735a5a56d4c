"""The draw schedule's arithmetic (csrc/pt_plan.h): bands and pixels of a partition, the carved slabs' layouts
(compaction records, the child-pair build's scratch and records, the wavefront buffers, the longest-first arrays,
the spill slabs), the overlap's buffer set / stream / mark, the megakernel's grid and the auto trial of late-bounce
compaction. Host C++ only: a small program over the header, no GPU. Every expectation is a literal worked out by
hand from the host code as it stood before the arithmetic moved into the header (pt_capi.cpp's render_trace,
cont_decide, cont_bytes; ensure_pairs, wf_reserve, lpt_cost / lpt_order / lpt_split, spill_reserve), not produced
by the header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "babylon.js-pathtracing-renderer_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "pt_plan.h"
static long num(const char* s) { return std::strtol(s, nullptr, 10); }
int main(int argc, char** argv)
{
    pt::Knobs k;
    pt::read_knobs(k);   // the tests set PT_* variables
    const char* cmd = argc > 1 ? argv[1] : "";
    if (!std::strcmp(cmd, "bands")) {          // bands height parts
        for (int p = 0; p < num(argv[3]); p++) std::printf("%d ", pt::bands_owned((int)num(argv[2]), (int)num(argv[3]), p));
    } else if (!std::strcmp(cmd, "pixels")) {  // pixels w h parts part
        std::printf("%zu %zu", pt::owned_pixels((int)num(argv[2]), (int)num(argv[3]), (int)num(argv[4]), (int)num(argv[5])),
                    pt::share_pixels((int)num(argv[2]), (int)num(argv[3]), (int)num(argv[4])));
    } else if (!std::strcmp(cmd, "lag")) {     // lag share...
        for (int i = 2; i < argc; i++) std::printf("%d ", pt::draw_lag(k, (size_t)num(argv[i])));
    } else if (!std::strcmp(cmd, "align")) {
        for (int i = 2; i < argc; i++) std::printf("%zu ", pt::align256((size_t)num(argv[i])));
    } else if (!std::strcmp(cmd, "layout")) {  // layout cap sort
        const pt::ContLayout L((size_t)num(argv[2]), num(argv[3]) != 0);
        std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d", L.bytes, L.rec, L.aux, L.perm, L.rank, L.key, L.bins, L.count,
                    L.total(), (int)pt::ContLayout::kStored, (int)pt::ContLayout::kHead, (int)pt::ContLayout::kTotal);
    } else if (!std::strcmp(cmd, "pairs")) {   // pairs texels n_inner n_leaf
        const pt::PairsLayout L((long long)num(argv[2]));
        const pt::PairsLayout::Records R((size_t)num(argv[3]), (size_t)num(argv[4]));
        std::printf("%u %u %zu %zu %zu %zu %zu %zu %zu %u %zu %zu %zu", L.nrec, L.nblk, L.inner, L.leafref, L.counts, L.code,
                    L.parent, L.refs, L.bytes, R.leaf_base, R.top_base, R.rec_bytes, R.alloc);
    } else if (!std::strcmp(cmd, "wf")) {      // wf tiles pixels blocks
        const unsigned cap = pt::WfLayout::shard_cap((int)num(argv[2]));
        const size_t slots = (size_t)cap * pt::kShards, spill = pt::WfLayout::spill_entries((int)num(argv[4]));
        const pt::WfLayout L(slots, (size_t)num(argv[3]), spill);
        std::printf("%u %zu %zu %zu %zu ", cap, slots, spill, L.end, L.bytes);
        std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu ", L.cnt, L.q[0][0], L.q[0][1], L.q[0][2], L.q[0][3], L.q[1][0], L.q[1][1],
                    L.q[1][2], L.q[1][3]);
        std::printf("%zu %zu %zu %zu %zu %zu %zu", L.hit[0], L.hit[1], L.gb[0], L.gb[1], L.rad, L.bvhq, L.spill);
    } else if (!std::strcmp(cmd, "lpt")) {     // lpt cap set
        const pt::LptLayout L{ (size_t)num(argv[2]) };
        const int p = (int)num(argv[3]);
        std::printf("%zu %zu %zu %zu %d", L.cost(p), L.order(p), L.split(p), L.words(), pt::kSetsMax);
    } else if (!std::strcmp(cmd, "spill")) {   // spill p lanes...
        std::printf("%zu ", pt::kSpillPerLane);
        for (int i = 3; i < argc; i++)
            std::printf("%d %zu ", (int)pt::spill_fits((size_t)std::strtoull(argv[i], nullptr, 10)),
                        pt::spill_slab((int)num(argv[2]), (size_t)std::strtoull(argv[i], nullptr, 10)));
    } else if (!std::strcmp(cmd, "overlap")) { // overlap depth,lag,overlapped[,f: memory grew before this draw] ...
        pt::Overlap o;
        for (int i = 2; i < argc; i++) {
            int d = 0, l = 0, ov = 0;
            char f = 0;
            std::sscanf(argv[i], "%d,%d,%d,%c", &d, &l, &ov, &f);
            const pt::Overlap::Slot at = o.slot(d, l);
            if (f == 'f') o.need_fresh = true;
            const pt::Overlap::Slot s = o.step(d, l, ov != 0);
            if (s.set != at.set || s.stream != at.stream) return 3;
            std::printf("%d %d %d %d %u\n", s.set, s.stream, s.wait, (int)o.need_fresh, o.mark_floor);
            o.mk_seq++;   // (the host counts the draw once it is enqueued)
        }
        std::printf("%d %d %d\n", o.next().set, o.depth_run, o.lag_run);
    } else if (!std::strcmp(cmd, "grid")) {    // grid gx gy same cont share sky
        const pt::MegaGrid g((int)num(argv[2]), (int)num(argv[3]), num(argv[4]) != 0, num(argv[5]) != 0, k);
        std::printf("%zu %u %u %d %zu %d %u %d %u", g.n, g.split_cap, g.split, g.gy_grid, g.lanes, (int)g.one_wave, g.order_zig,
                    g.cont_waves(k, (size_t)num(argv[6]), num(argv[7]) != 0), pt::MegaGrid::sort_grid_bits(k, (size_t)num(argv[6])));
    } else if (!std::strcmp(cmd, "trial")) {   // trial share ms0,..,ms5 draws...: s still, a alone, o / b the same of another
        pt::ContTrial t;                       // key, n not eligible; each with a count
        static int target_a, target_b;
        float ms[pt::kContBlocks] = {};
        std::sscanf(argv[3], "%f,%f,%f,%f,%f,%f", &ms[0], &ms[1], &ms[2], &ms[3], &ms[4], &ms[5]);
        for (int i = 4; i < argc; i++)
            for (long n = num(argv[i] + 1); n > 0; n--) {
                const char c = argv[i][0];
                const pt::ContTrial::Key key{ c == 'o' || c == 'b' ? (void*)&target_b : (void*)&target_a, 7, 0, 1, 1920, 1080 };
                pt::ContTrial::Draw d = t.draw(key, c != 'n', c == 'a' || c == 'b', (size_t)num(argv[2]), k);
                const int ev = d.event, ends = d.ends;
                if (d.ends) d = t.conclude(ms);
                std::printf("%c %d %d %d %d %d %d\n", c, (int)d.on, d.depth, ev, ends, d.code, t.seen);
            }
        std::printf("%d %d %d %g %g %g\n", (int)t.decided, (int)t.choice, t.depth, t.ms_on, t.ms_off, t.ms_off2);
    } else {
        return 2;
    }
    std::printf("\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("plan")
    (d / "plan_main.cpp").write_text(MAIN)
    exe = str(d / "plan_main")
    # only csrc on the include path: the header takes nothing from ROCm
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, str(d / "plan_main.cpp")],
                   check=True)

    def run(*args, **env):
        clean = {k: v for k, v in os.environ.items() if not k.startswith("PT_")}
        out = subprocess.run([exe, *[str(a) for a in args]], check=True, capture_output=True, text=True,
                             env=dict(clean, **env)).stdout
        rows = [[float(v) if "." in v or "e" in v else int(v) if v.lstrip("-").isdigit() else v for v in line.split()]
                for line in out.splitlines() if line.strip()]
        return rows[0] if len(rows) == 1 else rows
    return run


def test_header_is_host_only():
    text = open(os.path.join(CSRC, "pt_plan.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<cstddef>", "<cstdint>", '"pt_knobs.h"']
    for word in ("std::string", "std::vector", "std::map", "unordered_map", "malloc", "new "):
        assert word not in text, word   # the per-draw functions allocate nothing


def test_bands(plan):
    assert plan("bands", 200, 3) == [5, 4, 4]            # 13 bands
    assert plan("bands", 200, 8) == [2, 2, 2, 2, 2, 1, 1, 1]
    assert plan("bands", 1, 8) == [1, 0, 0, 0, 0, 0, 0, 0]
    assert plan("bands", 16, 1) == [1]
    assert plan("bands", 17, 1) == [2]
    assert plan("bands", 2160, 8) == [17, 17, 17, 17, 17, 17, 17, 16]   # 135 bands (added: by hand, (135 - p + 7) / 8)
    assert plan("align", 0, 1, 256, 257, 4000) == [0, 256, 256, 512, 4096]


def test_pixels(plan):
    assert plan("pixels", 1920, 136, 1, 0) == [261120, 261120]       # capped at w * h: nine bands would be 276480
    assert plan("pixels", 3840, 2160, 8, 0) == [1044480, 1036800]    # 17 bands x 16 x 3840; 8294400 / 8
    assert plan("pixels", 3840, 2160, 8, 7) == [983040, 1036800]     # (added) 16 bands x 16 x 3840
    assert plan("pixels", 1920, 8, 4, 1) == [0, 3840]                # (added) one band, part 1 owns none; 15360 / 4


def test_lag(plan):
    assert plan("lag", 0, 799999, 800000, 8294400) == [2, 2, 0, 0]
    assert plan("lag", 0, 799999, 800000, 8294400, PT_OVERLAP_LAG="4") == [4, 4, 4, 4]
    assert plan("lag", 99999, 100000, PT_OVERLAP_LAG_PIXELS="100000") == [2, 0]   # (added: the threshold is the knob)


# per draw: buffer set, stream, the set whose mark is waited for (-1: not overlapped)
def slots(rows):
    return [tuple(r[:3]) for r in rows[:-1]]


def test_overlap_depth3(plan):
    rows = plan("overlap", *["3,0,1"] * 12)
    # draw 0 its own mark, draw 1 draw 0's (the floor), draw k >= 2 draw k - 2's: set (k - 2) % 3
    want = [(k % 3, k % 3, 0 if k < 2 else (k - 2) % 3) for k in range(12)]
    assert want[:5] == [(0, 0, 0), (1, 1, 0), (2, 2, 0), (0, 0, 1), (1, 1, 2)]
    assert slots(rows) == want
    assert [r[3:] for r in rows[:-1]] == [[0, 0]] * 12   # need_fresh consumed by draw 0, the floor stays 0
    assert rows[-1] == [0, 3, 0]                          # the next draw: set 12 % 3


def test_overlap_depth3_lag2(plan):
    rows = plan("overlap", *["3,2,1"] * 12)
    want = [(k % 5, k % 3, 0 if k < 4 else (k - 4) % 5) for k in range(12)]
    assert want[3:7] == [(3, 0, 0), (4, 1, 0), (0, 2, 1), (1, 0, 2)]
    assert slots(rows) == want
    assert rows[-1] == [2, 3, 2]


def test_overlap_after_a_draw_that_is_not_overlapped(plan):
    rows = plan("overlap", *(["3,0,1"] * 5 + ["3,0,0"] + ["3,0,1"] * 6))
    assert slots(rows) == [(0, 0, 0), (1, 1, 0), (2, 2, 0), (0, 0, 1), (1, 1, 2),
                           (2, 2, -1),                      # draw 5 on the main stream
                           (0, 0, 0), (1, 1, 0), (2, 2, 0),  # draw 6 its own mark, 7 and 8 draw 6's
                           (0, 0, 1), (1, 1, 2), (2, 2, 0)]  # then draw k - 2's again
    assert rows[5][3:] == [1, 0]    # it sets need_fresh
    assert rows[6][3:] == [0, 6]    # ... which draw 6 takes: the floor is 6


def test_overlap_change_of_depth(plan):
    rows = plan("overlap", *(["3,0,1"] * 6 + ["2,0,1"] * 3))
    assert slots(rows)[5:] == [(2, 2, 0),                              # draw 5 waits for draw 3's
                               (0, 0, 0), (1, 1, 0), (0, 0, 1)]        # draw 6: set 6 % 2, its own mark; 7: 6's; 8: 7's
    assert [r[4] for r in rows[:-1]] == [0] * 6 + [6] * 3
    assert rows[-1] == [1, 2, 0]


def test_overlap_new_memory_and_change_of_lag(plan):
    # (added, by hand) a slab that grew before draw 3 sets need_fresh: draw 3 waits for its own mark, draw 4 for draw 3's
    rows = plan("overlap", "3,0,1", "3,0,1", "3,0,1", "3,0,1,f", "3,0,1", "3,0,1")
    assert slots(rows)[3:] == [(0, 0, 0), (1, 1, 0), (2, 2, 0)]
    assert [r[4] for r in rows[:-1]] == [0, 0, 0, 3, 3, 3]
    # (added, by hand) lag 0 -> 2 at draw 4: another cycle of sets, the floor is 4, set 4 % 5, stream 4 % 3
    rows = plan("overlap", *(["3,0,1"] * 4 + ["3,2,1"] * 2))
    assert slots(rows)[4:] == [(4, 1, 4), (0, 2, 4)]
    assert [r[4] for r in rows[:-1]] == [0, 0, 0, 0, 4, 4]


def test_cont_layout(plan):
    names = ("bytes", "rec", "aux", "perm", "rank", "key", "bins", "count", "total", "kStored", "kHead", "kTotal")
    got = dict(zip(names, plan("layout", 1000, 0)))
    assert got["bytes"] == 68352 and got["rec"] == 0 and got["aux"] == 64000 and got["count"] == 68096   # 64000 + 4096 + 256
    assert got["total"] == 68096 + 8
    assert (got["kStored"], got["kHead"], got["kTotal"]) == (0, 1, 2)
    got = dict(zip(names, plan("layout", 1000, 1)))
    assert got["bytes"] == 68352 + 2 * 4096 + 2048 + 8192 * 4 == 111360
    assert (got["aux"], got["perm"], got["rank"], got["key"], got["bins"], got["count"]) == (64000, 68096, 72192, 76288, 78336, 111104)
    assert got["total"] == 111112
    got = dict(zip(names, plan("layout", 0, 0)))
    assert got["bytes"] == 256 and got["aux"] == got["count"] == 0 and got["total"] == 8
    # (added, by hand) 100 records with the sort: 6400 | 512 | 512 | 512 | 256 | 32768 | 256
    got = dict(zip(names, plan("layout", 100, 1)))
    assert (got["aux"], got["perm"], got["rank"], got["key"], got["bins"], got["count"], got["bytes"]) == \
        (6400, 6912, 7424, 7936, 8192, 40960, 41216)


# ---- the other carved slabs. Each array starts where the one before it ends, rounded up to 256 B; none overlap
def check_carve(starts, sizes, end):
    """starts / sizes in carving order: array k + 1 starts at the end of array k rounded up to 256, the last ends at `end`"""
    assert len(starts) == len(sizes)
    for k, (at, size) in enumerate(zip(starts, sizes)):
        assert at % 256 == 0
        nxt = starts[k + 1] if k + 1 < len(starts) else end
        assert nxt == at + (size + 255) // 256 * 256, k      # (so no two overlap: every size is at most its rounding)


PAIRS = ("nrec", "nblk", "inner", "leafref", "counts", "code", "parent", "refs", "bytes", "leaf_base", "top_base", "rec_bytes", "alloc")


def test_pairs_layout_smallest(plan):
    # 2 texels: one node, one scan block; ensure_pairs: 2 al(1) + al(2 * 1 * 4) + al(1 * 4) + 2 al(1 * 4) = 6 x 256
    g = dict(zip(PAIRS, plan("pairs", 2, 0, 1)))
    assert (g["nrec"], g["nblk"]) == (1, 1)
    assert [g[k] for k in PAIRS[2:9]] == [0, 256, 512, 768, 1024, 1280, 1536]
    check_carve([g[k] for k in PAIRS[2:8]], [1, 1, 8, 4, 4, 4], g["bytes"])
    # no inner record: the one leaf record at byte 0, the jump table (4095 x 64 B) after its 48 B rounded up
    assert (g["leaf_base"], g["top_base"], g["rec_bytes"], g["alloc"]) == (0, 256, 256 + 262080, 256 + 262080 + 256)
    assert dict(zip(PAIRS, plan("pairs", 1, 0, 1)))["nrec"] == 1   # an odd texel count rounds up: (1 + 1) / 2


def test_pairs_layout_across_a_block_and_every_rounding(plan):
    # 2999 texels -> nrec 1500, two 1024-node blocks: flags 1500 -> 1536 B each, counts 16 -> 256 B, words 6000 -> 6144 B
    g = dict(zip(PAIRS, plan("pairs", 2999, 749, 750)))
    assert (g["nrec"], g["nblk"]) == (1500, 2)
    assert [g[k] for k in PAIRS[2:9]] == [0, 1536, 3072, 3328, 9472, 15616, 21760]
    check_carve([g[k] for k in PAIRS[2:8]], [1500, 1500, 16, 6000, 6000, 6000], g["bytes"])
    # 749 x 64 = 47936 -> 48128; 750 x 48 = 36000 -> 36096; + 4095 x 64 = 262080
    assert (g["leaf_base"], g["top_base"], g["rec_bytes"], g["alloc"]) == (48128, 84224, 346304, 346560)
    assert dict(zip(PAIRS, plan("pairs", 2048, 0, 1)))["nblk"] == 1 and dict(zip(PAIRS, plan("pairs", 2050, 0, 1)))["nblk"] == 2
    g = dict(zip(PAIRS, plan("pairs", 1 << 24, 1, 1)))                # the largest tree the host builds
    assert (g["nrec"], g["nblk"], g["bytes"]) == (1 << 23, 8192, 2 * (1 << 23) + 65536 + 3 * (1 << 25))


WF = ("cap", "slots", "spill_n", "end", "bytes", "cnt", "qA0", "qB0", "qC0", "qD0", "qA1", "qB1", "qC1", "qD1", "hit0", "hit1",
      "gb0", "gb1", "rad", "bvhq", "spill")


def wf_sizes(g, pixels):
    return [4096] + [g["slots"] * 16] * 10 + [pixels * 16] * 3 + [g["slots"] * 4, g["spill_n"] * 8]


def test_wf_layout_one_tile(plan):
    # one tile: a 256-slot shard x 16 shards; a 16 x 16 frame; 16 blocks: (28 - 7) x 16 x 256 stack entries
    g = dict(zip(WF, plan("wf", 1, 256, 16)))
    assert (g["cap"], g["slots"], g["spill_n"]) == (256, 4096, 86016)
    assert [g[k] for k in WF[5:]] == [0] + [4096 + 65536 * k for k in range(10)] + [659456, 663552, 667648, 671744, 688128]
    check_carve([g[k] for k in WF[5:]], wf_sizes(g, 256), g["end"])
    # wf_reserve: 4096 + 10 x 65536 + 3 x 4096 + 16384 + 688128 + 16 x 256; every size here is a multiple of 256
    assert g["bytes"] == 1380352 and g["end"] == 1376256 == g["bytes"] - 4096


def test_wf_layout_tiles_no_multiple_of_the_shards(plan):
    # 17 tiles: two tiles in shard 0, so 512 slots per shard; a 66 x 50 frame: 52800 B per plane -> 52992
    g = dict(zip(WF, plan("wf", 17, 3300, 16)))
    assert (g["cap"], g["slots"], g["spill_n"]) == (512, 8192, 86016)
    assert [g[k] for k in WF[5:]] == [0] + [4096 + 131072 * k for k in range(10)] + [1314816, 1367808, 1420800, 1473792, 1506560]
    check_carve([g[k] for k in WF[5:]], wf_sizes(g, 3300), g["end"])
    assert g["end"] == 2194688 and g["bytes"] == 2198208             # allocated: 256 B of slack for each of 16 arrays
    assert g["end"] <= g["bytes"]
    assert dict(zip(WF, plan("wf", 16, 256, 16)))["cap"] == 256 and dict(zip(WF, plan("wf", 32, 256, 16)))["cap"] == 512


def test_lpt_layout(plan):
    # 100 tiles, 12 buffer sets: cost 12 x 400 words | order 12 x 100 | split 12
    assert plan("lpt", 100, 0) == [0, 4800, 6000, 6012, 12]
    assert plan("lpt", 100, 11) == [4400, 5900, 6011, 6012, 12]       # the last set: its split is the last word
    assert plan("lpt", 100, 1)[:3] == [400, 4900, 6001]               # set 1 starts where set 0's 4 x cap / cap / 1 end
    assert plan("lpt", 8160, 11) == [359040, 481440, 489611, 489612, 12]


def test_spill_slab(plan):
    # 28 - 6 stack levels + 4 entries of G-buffer fields = 26 entries per lane; 2^32 / 26 = 165191049.8
    got = plan("spill", 2, 165191049, 165191050, 2088960)
    assert got[0] == 26
    assert got[1:3] == [1, 2 * 165191049 * 26] and 165191049 * 26 == 2 ** 32 - 22    # fits: the last index is below 2^32
    assert got[3:5] == [0, 2 * 165191050 * 26] and 165191050 * 26 == 2 ** 32 + 4     # does not
    assert got[5:7] == [1, 2 * 2088960 * 26]                                          # 120 x 68 tiles x 256 lanes, slab 2
    assert plan("spill", 0, 1000)[1:] == [1, 0]


GRID = ("n", "split_cap", "split", "gy_grid", "lanes", "one_wave", "order_zig", "cont_waves", "sort_bits")


def grid(plan, gx, gy, same, cont, share=2073600, sky=0, **env):
    return dict(zip(GRID, plan("grid", gx, gy, same, cont, share, sky, **env)))


def test_mega_grid(plan):
    g = grid(plan, 120, 68, 1, 0)
    assert (g["n"], g["split_cap"], g["split"], g["gy_grid"]) == (8160, 32, 32, 69)   # 68 + ceil(12 * 32 / 480)
    assert (g["lanes"], g["one_wave"], g["order_zig"]) == (120 * 69 * 256, 1, 0)
    g = grid(plan, 120, 68, 1, 1)
    assert (g["split_cap"], g["split"], g["gy_grid"], g["lanes"]) == (32, 0, 68, 120 * 68 * 256)
    assert (g["one_wave"], g["order_zig"]) == (1, 1)                                   # 8160 <= 8192
    g = grid(plan, 120, 68, 0, 0)
    assert (g["split"], g["gy_grid"], g["order_zig"]) == (0, 68, 0)                    # no order to reuse: no split tiles
    g = grid(plan, 8193, 1, 1, 1)
    assert (g["n"], g["one_wave"], g["order_zig"]) == (8193, 0, 0)
    assert grid(plan, 8192, 1, 1, 1)["one_wave"] == 1 and grid(plan, 8192, 1, 1, 1)["order_zig"] == 1
    assert grid(plan, 8193, 1, 1, 0, PT_LPT="2")["order_zig"] == 1                     # lpt_zig: every draw
    assert grid(plan, 120, 68, 1, 1, PT_LPT_ZIG_CONT="0")["order_zig"] == 0
    g = grid(plan, 5, 1, 1, 0)
    assert (g["n"], g["split_cap"], g["split"], g["gy_grid"]) == (5, 0, 0, 1)          # 5 & ~7
    # (added, by hand) 12 tiles: 12 & ~7 = 8 split tiles, 96 more workgroups in rows of 16: six padding rows
    g = grid(plan, 4, 3, 1, 0)
    assert (g["split_cap"], g["split"], g["gy_grid"], g["lanes"]) == (8, 8, 9, 4 * 9 * 256)
    assert grid(plan, 120, 68, 1, 0, PT_SPLIT_TILES="0")["gy_grid"] == 68


def test_cont_waves_and_sort_grid(plan):
    assert grid(plan, 120, 68, 1, 1, share=2999999)["cont_waves"] == 2048
    assert grid(plan, 120, 68, 1, 1, share=3000000)["cont_waves"] == 1024
    assert grid(plan, 120, 68, 1, 1, share=8294400, sky=1)["cont_waves"] == 2048
    assert grid(plan, 120, 68, 1, 1, share=100, sky=1)["cont_waves"] == 2048
    assert grid(plan, 10, 10, 1, 1, share=100)["cont_waves"] == 400                    # 4 n
    assert grid(plan, 10, 10, 1, 1, share=8294400)["cont_waves"] == 400
    assert grid(plan, 10, 30, 1, 1, share=8294400)["cont_waves"] == 1024               # 4 n = 1200
    for share in (100, 3000000, 8294400):
        assert grid(plan, 120, 68, 1, 1, share=share, PT_CONT_WAVES="512")["cont_waves"] == 512
        assert grid(plan, 120, 68, 1, 1, share=share, sky=1, PT_CONT_WAVES="512")["cont_waves"] == 512
    assert grid(plan, 120, 68, 1, 1, share=2999999)["sort_bits"] == 2
    assert grid(plan, 120, 68, 1, 1, share=3000000)["sort_bits"] == 3
    assert grid(plan, 120, 68, 1, 1, share=3000000, PT_CONT_SORT_GRID="1")["sort_bits"] == 1
    assert grid(plan, 120, 68, 1, 1, share=3000000, PT_CONT_SORT_GRID="2")["sort_bits"] == 2


# ---- the auto trial. Per draw: kind, on, depth, event, ends, code, seen; the last row decided, choice, depth, ms_on, ms_off, ms_off2
SHARE = 2073600
MS = "10,12,11,11,12,10"
# draws 33-92 by hand: blocks of 10 - on, off, off at depth 2, off at depth 2, off, on - with an event at the 4th
# draw of block b into slot 2b and at the 9th into slot 2b + 1
TRIAL = [(int(b in (0, 5)), 2 if b in (2, 3) else 3, {3: 2 * b, 8: 2 * b + 1}.get(o, -1)) for b in range(6) for o in range(10)]


def test_trial_listing_spot_checks():
    assert len(TRIAL) == 60
    assert TRIAL[0] == (1, 3, -1) and TRIAL[3] == (1, 3, 0) and TRIAL[8] == (1, 3, 1) and TRIAL[13] == (0, 3, 2)
    assert TRIAL[23] == (0, 2, 4) and TRIAL[38] == (0, 2, 7) and TRIAL[43] == (0, 3, 8) and TRIAL[58] == (1, 3, 11)
    assert [e for _, _, e in TRIAL if e >= 0] == list(range(12))


def test_trial_default_then_blocks_then_end(plan):
    rows = plan("trial", SHARE, MS, "s94")
    for n, r in enumerate(rows[:32], 1):
        assert r == ["s", 1, 3, -1, 0, 5, n]            # on (>= cont_auto_pixels), depth 3, no event, code 5
    for n, (r, (on, depth, event)) in enumerate(zip(rows[32:92], TRIAL), 33):
        assert r == ["s", on, depth, event, 0, 4, n]
    assert rows[92] == ["s", 1, 3, -1, 1, 2, 93]        # draw 93 ends the trial: on (10 < 0.98 * 11), depth 3
    assert rows[93] == ["s", 1, 3, -1, 0, 2, 94]        # ... and every later draw takes the decision
    assert rows[-1] == [1, 1, 3, 10, 12, 11]


@pytest.mark.parametrize("ms,choice,depth,blocks", [
    ("10,12,11,11,12,10", 1, 3, (10, 12, 11)),
    ("10.9,12,11,11,12,10.9", 0, 2, (10.9, 12, 11)),    # 10.9 >= 10.78: off; off2 < off: two frames in flight
    ("12,11,11.5,11.5,11,12", 0, 3, (12, 11, 11.5)),
    ("10,12,11,11,30,30", 1, 3, (10, 12, 11)),          # the faster block of each mode decides
    ("30,12,11,13,30,10", 1, 3, (10, 12, 11)),          # (added) whichever of the two it is
])
def test_trial_conclude(plan, ms, choice, depth, blocks):
    rows = plan("trial", SHARE, ms, "s94")
    assert rows[92] == ["s", choice, depth, -1, 1, 2 if choice else 1, 93]
    assert rows[93] == ["s", choice, depth, -1, 0, 2 if choice else 1, 94]
    assert rows[-1][:3] == [1, choice, depth]
    assert rows[-1][3:] == pytest.approx(blocks, rel=1e-6)


def test_trial_small_shares(plan):
    rows = plan("trial", 500000, MS, "s33")
    for n, r in enumerate(rows[:30], 1):
        assert r == ["s", 0, 3, -1, 0, 6, n]            # off; below lag_pixels: three frames in flight
    assert rows[30] == ["s", 1, 3, -1, 0, 5, 31] and rows[31] == ["s", 1, 3, -1, 0, 5, 32]   # the two warm-up draws
    assert rows[32] == ["s", 1, 3, -1, 0, 4, 33]
    rows = plan("trial", 1000000, MS, "s32")
    for n, r in enumerate(rows[:30], 1):
        assert r == ["s", 0, 2, -1, 0, 6, n]            # off, and from lag_pixels up two frames in flight
    assert rows[30] == ["s", 1, 3, -1, 0, 5, 31]
    rows = plan("trial", 1000000, MS, "s32", PT_OVERLAP_DEPTH="3")
    for n, r in enumerate(rows[:30], 1):
        assert r == ["s", 0, 3, -1, 0, 6, n]            # a given depth stays


def test_trial_alone_draws(plan):
    # ten alone draws among 92 still ones: before the trial, at both event offsets, in a depth-2 block, after the last block
    script = ["s5", "a1", "s27", "a1", "s3", "a2", "s5", "a1", "s12", "a2", "s40", "a3", "s2"]
    rows = plan("trial", SHARE, MS, *script)
    still = [r for r in rows[:-1] if r[0] == "s"]
    alone = [r for r in rows[:-1] if r[0] == "a"]
    assert len(still) == 94 and len(alone) == 10
    # the still draws are those of the run without alone draws
    assert still == plan("trial", SHARE, MS, "s94")[:-1]
    assert still[92][4] == 1 and still[92][6] == 93
    # never on, no event, code 0, seen as it was; the depth of the still draw that would stand there
    assert alone == [["a", 0, 3, -1, 0, 0, 5], ["a", 0, 3, -1, 0, 0, 32],
                     ["a", 0, 3, -1, 0, 0, 35], ["a", 0, 3, -1, 0, 0, 35],   # (the 4th draw of block 0 is next: its event waits)
                     ["a", 0, 3, -1, 0, 0, 40],                              # (the 9th)
                     ["a", 0, 2, -1, 0, 0, 52], ["a", 0, 2, -1, 0, 0, 52],   # block 2: depth 2
                     ["a", 0, 3, -1, 0, 0, 92], ["a", 0, 3, -1, 0, 0, 92], ["a", 0, 3, -1, 0, 0, 92]]   # the trial's draws are through
    # before the trial an alone draw of a 1 Mpx share takes the two frames in flight of the off default
    rows = plan("trial", 1000000, MS, "s5", "a1", "s1")
    assert rows[5] == ["a", 0, 2, -1, 0, 0, 5] and rows[6] == ["s", 0, 2, -1, 0, 6, 6]
    # after the decision it takes the decision's depth, and still does not compact
    rows = plan("trial", SHARE, "10.9,12,11,11,12,10.9", "s93", "a1")
    assert rows[93] == ["a", 0, 2, -1, 0, 0, 93]


def test_trial_other_keys(plan):
    rows = plan("trial", SHARE, MS, "s40", "b1", "s1", "o1", "s1")
    assert rows[40] == ["b", 0, 3, -1, 0, 0, 40]        # alone, another key: the trial goes on
    assert rows[41] == ["s", 1, 3, 1, 0, 4, 41]         # (the 9th draw of block 0: its event)
    assert rows[42] == ["o", 1, 3, -1, 0, 5, 1]         # still, another key: a new trial
    assert rows[43] == ["s", 1, 3, -1, 0, 5, 1]         # ... and again


def test_trial_forced_and_off(plan):
    rows = plan("trial", 100, MS, "s3", "a1", "n1", PT_CONT="1")
    assert rows[:3] == [["s", 1, 3, -1, 0, 3, 0]] * 3   # on, code 3, no trial state touched
    assert rows[3] == ["a", 0, 3, -1, 0, 0, 0] and rows[4] == ["n", 0, 3, -1, 0, 0, 0]
    assert rows[-1][:2] == [0, 0]
    rows = plan("trial", SHARE, MS, "s40", PT_CONT="0")
    assert rows[:-1] == [["s", 0, 3, -1, 0, 0, 0]] * 40
    rows = plan("trial", SHARE, MS, "s2", "n3", "s1")
    assert rows[2:5] == [["n", 0, 3, -1, 0, 0, 2]] * 3 and rows[5] == ["s", 1, 3, -1, 0, 5, 3]   # not eligible: off, not counted
