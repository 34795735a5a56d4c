"""The context's tunables (csrc/pt_knobs.h): defaults, clamps, and that INTEGRATION.md's table lists exactly
the PT_* variables the code reads. Host C++ only: a small program over the header, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "babylon.js-pathtracing-renderer_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <cstring>
#include "pt_knobs.h"
static const char* special_default(const pt::Knobs& k, const char* n)
{
    static char b[32];
    if (!std::strcmp(n, "PT_BVH_LAYOUT")) return k.bvh_layout == 2 ? "trail" : k.bvh_layout == 0 ? "reference" : "pairs";
    const int v = !std::strcmp(n, "PT_LPT") ? (k.lpt_zig ? 2 : k.lpt) : !std::strcmp(n, "PT_OVERLAP_DEPTH") ? k.depth
                : !std::strcmp(n, "PT_CONT_WAVES") ? k.cont_waves : !std::strcmp(n, "PT_CONT_SORT_GRID") ? k.cont_grid_bits
                : /* PT_SPLIT_ALWAYS */ k.split_dominance == 0;
    std::snprintf(b, sizeof b, "%d", v);
    return b;
}
int main(int argc, char** argv)
{
    pt::Knobs k;
    if (argc > 1 && !std::strcmp(argv[1], "--dump")) {   // every variable and its default
        for (const auto& r : pt::kKnobTable) std::printf("%s %d\n", r.name, k.*r.field);
        for (const char* n : pt::kKnobsWrittenOut) std::printf("%s %s\n", n, special_default(k, n));
        return 0;
    }
    pt::read_knobs(k);   // the real environment: every field
    for (const auto& r : pt::kKnobTable) std::printf("%s %d\n", r.name, k.*r.field);
    std::printf("lpt %d\nlpt_zig %d\ndepth %d\ndepth_env %d\ncont_waves %d\ncont_waves_env %d\n", k.lpt, k.lpt_zig, k.depth,
                (int)k.depth_env, k.cont_waves, (int)k.cont_waves_env);
    std::printf("cont_grid_bits %d\ncont_grid_env %d\nsplit_dominance %d\nbvh_layout %d\n", k.cont_grid_bits,
                (int)k.cont_grid_env, k.split_dominance, k.bvh_layout);
    std::printf("PT_TIMING_EVERY %d\n", pt::knob_timing_every(1));
    return 0;
}
"""

# the defaults of the Dev fields before they moved into pt::Knobs (pt_capi.cpp), by variable / field
DEFAULTS = {
    "PT_OVERLAP": 1, "PT_MOVING_SERIAL": 1, "PT_OVERLAP_LAG": -1, "PT_OVERLAP_LAG_PIXELS": 800000,
    "PT_CONT": 2, "PT_CONT_BOUNCE": 2, "PT_CONT_LANES": 48, "PT_CONT_REFILL": 16, "PT_CONT_WAVES_BIG": 1024,
    "PT_CONT_BIG_PIXELS": 3000000, "PT_CONT_AUTO_PIXELS": 2000000, "PT_CONT_SORT": 1, "PT_PERSIST_TILES": 4,
    "PT_PERSIST_REFILL": 16, "PT_LPT_ZIG_CONT": 1, "PT_SPLIT_TILES": 32, "PT_SPLIT_NEAR": 3, "PT_LPT_FLAT": 6,
    "PT_LPT_FLAT_TILES": 8192, "PT_FUSE_ORDER": 1, "PT_MAIN_WAVES": 16384, "PT_DRAW_EVENTS": 0,
    "lpt": 1, "lpt_zig": 0, "depth": 3, "depth_env": 0, "cont_waves": 2048, "cont_waves_env": 0,
    "cont_grid_bits": 2, "cont_grid_env": 0, "split_dominance": 8, "bvh_layout": 1, "PT_TIMING_EVERY": 1,
}
DUMP_DEFAULTS = {"PT_LPT": "1", "PT_OVERLAP_DEPTH": "3", "PT_CONT_WAVES": "2048", "PT_CONT_SORT_GRID": "2",
                 "PT_SPLIT_ALWAYS": "0", "PT_BVH_LAYOUT": "pairs"}
NOT_IN_KNOBS = {"PT_PEER", "PT_DEVICES", "PT_LIBPT", "PT_TIMING_EVERY"}   # read elsewhere (INTEGRATION.md says where)
INT_MAX = 2 ** 31 - 1
# the fields of the variables read_knobs writes out
FIELDS = {"PT_LPT": ("lpt", "lpt_zig"), "PT_OVERLAP_DEPTH": ("depth", "depth_env"), "PT_CONT_WAVES": ("cont_waves", "cont_waves_env"),
          "PT_CONT_SORT_GRID": ("cont_grid_bits", "cont_grid_env"), "PT_SPLIT_ALWAYS": ("split_dominance",),
          "PT_BVH_LAYOUT": ("bvh_layout",)}


@pytest.fixture(scope="module")
def knobs(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("knobs")
    (d / "knobs_main.cpp").write_text(MAIN)
    exe = str(d / "knobs_main")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, str(d / "knobs_main.cpp")],
                   check=True)

    def run(*args, **env):
        clean = {k: v for k, v in os.environ.items() if not k.startswith("PT_")}
        out = subprocess.run([exe, *args], check=True, capture_output=True, text=True, env=dict(clean, **env)).stdout
        return dict(line.split(" ", 1) for line in out.splitlines())
    return run


def test_defaults(knobs):
    got = knobs()
    assert {k: int(v) for k, v in got.items()} == DEFAULTS
    dump = knobs("--dump")
    assert dump == dict({k: str(v) for k, v in DEFAULTS.items() if k.startswith("PT_") and k != "PT_TIMING_EVERY"},
                        **DUMP_DEFAULTS)


@pytest.mark.parametrize("name,field,text,want", [
    ("PT_LPT_FLAT_TILES", None, "2097152", 2097152), ("PT_LPT_FLAT_TILES", None, "2097153", 2097152),
    ("PT_LPT_FLAT_TILES", None, "99999999999", 2097152), ("PT_LPT_FLAT_TILES", None, "99999999999999999999999", 2097152),
    ("PT_LPT_FLAT_TILES", None, "-5", 0), ("PT_LPT_FLAT_TILES", None, "0", 0), ("PT_LPT_FLAT_TILES", None, "100", 100),
    ("PT_CONT_LANES", None, "0", 1), ("PT_CONT_LANES", None, "1", 1), ("PT_CONT_LANES", None, "64", 64),
    ("PT_CONT_LANES", None, "65", 64), ("PT_CONT_LANES", None, "lots", 1),   # (no digits read as 0, as atoi did)
    ("PT_OVERLAP_DEPTH", "depth", "1", 2), ("PT_OVERLAP_DEPTH", "depth", "2", 2), ("PT_OVERLAP_DEPTH", "depth", "6", 6),
    ("PT_OVERLAP_DEPTH", "depth", "99", 6), ("PT_OVERLAP_DEPTH", "depth_env", "3", 1),
    ("PT_OVERLAP_LAG", None, "-7", -1), ("PT_OVERLAP_LAG", None, "-1", -1), ("PT_OVERLAP_LAG", None, "6", 6),
    ("PT_OVERLAP_LAG", None, "99", 6),
    ("PT_CONT_BOUNCE", None, "99999999999", INT_MAX), ("PT_CONT_BOUNCE", None, "1", 2),
    ("PT_CONT_WAVES", "cont_waves", "0", 1), ("PT_CONT_WAVES", "cont_waves_env", "7", 1),
    ("PT_CONT_SORT_GRID", "cont_grid_bits", "9", 3), ("PT_CONT_SORT_GRID", "cont_grid_env", "2", 1),
    ("PT_OVERLAP", None, "7", 1), ("PT_OVERLAP", None, "-1", 1), ("PT_OVERLAP", None, "0", 0), ("PT_OVERLAP", None, "no", 0),
    ("PT_LPT", "lpt", "2", 1), ("PT_LPT", "lpt_zig", "2", 1), ("PT_LPT", "lpt", "0", 0), ("PT_LPT", "lpt_zig", "1", 0),
    ("PT_SPLIT_ALWAYS", "split_dominance", "1", 0), ("PT_SPLIT_ALWAYS", "split_dominance", "0", 8),
    ("PT_BVH_LAYOUT", "bvh_layout", "trail", 2), ("PT_BVH_LAYOUT", "bvh_layout", "reference", 0),
    ("PT_BVH_LAYOUT", "bvh_layout", "anything", 1),
    ("PT_TIMING_EVERY", None, "0", 1), ("PT_TIMING_EVERY", None, "3", 3),
])
def test_clamps(knobs, name, field, text, want):
    got = knobs(**{name: text})
    assert int(got[field or name]) == want
    others = {k: int(v) for k, v in got.items() if k not in FIELDS.get(name, (name,))}
    assert all(DEFAULTS[k] == v for k, v in others.items()), others   # one variable moves nothing else


def test_integration_table_lists_the_knobs(knobs):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    first = [line.split("|")[1] for line in text.splitlines() if line.startswith("| `PT_")]
    listed = set(re.findall(r"PT_[A-Z0-9_]+", " ".join(first)))
    dumped = set(knobs("--dump"))
    assert dumped <= listed, sorted(dumped - listed)
    assert listed <= dumped | NOT_IN_KNOBS, sorted(listed - dumped - NOT_IN_KNOBS)
