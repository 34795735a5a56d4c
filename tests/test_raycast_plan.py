"""pt_cast_rays' slab and chunking arithmetic (csrc/pt_plan.h RaycastLayout), host C++ only, the way
tests/test_plan.py checks the other layouts: a small program over the header, every expectation a literal worked
out by hand.

A launch has one lane per ray, rounded up to whole waves of 64. The slab: origins | dirs (12 B per lane each) | hits
(64 B per lane) | the stack levels beyond LDS (28 - 6 = 22 levels x 8 B per lane, [level][lane]), every array on
256 B. A call of more than 262144 rays runs as chunks of that many through a slab of that many lanes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "babylon.js-pathtracing-renderer_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "pt_plan.h"
int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const size_t rays = (size_t)std::strtoull(argv[1], nullptr, 10);
    const pt::RaycastLayout L(rays);
    std::printf("%zu %zu %zu %zu %zu %zu %zu", L.lanes, L.origins, L.dirs, L.hits, L.spill, L.bytes, pt::RaycastLayout::chunks(rays));
    for (size_t i = 0; i < pt::RaycastLayout::chunks(rays); i++) std::printf(" %zu", pt::RaycastLayout::chunk_rays(rays, i));
    std::printf("\n%zu %zu %d %d\n", (size_t)pt::kRaycastChunk, (size_t)pt::kRaycastLevels, (int)pt::spill_fits(pt::kRaycastChunk),
                pt::kStackLevels - pt::kStackLdsMin);
    return 0;
}
"""


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("raycast_plan")
    (d / "main.cpp").write_text(MAIN)
    exe = str(d / "main")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, str(d / "main.cpp")], check=True)

    def run(rays):
        out = subprocess.run([exe, str(rays)], check=True, capture_output=True, text=True).stdout.split("\n")
        return [int(v) for v in out[0].split()], [int(v) for v in out[1].split()]
    return run


def test_constants(layout):
    _, k = layout(1)
    assert k == [262144, 22, 1, 22]   # the chunk (a multiple of 64), the levels beyond LDS, its slab index fits 32 bits
    assert 262144 % 64 == 0


@pytest.mark.parametrize("rays,expect", [
    # rays: lanes, origins, dirs, hits, spill, bytes, chunks, the chunks' rays
    (1, [64, 0, 768, 1536, 5632, 16896, 1, 1]),
    (63, [64, 0, 768, 1536, 5632, 16896, 1, 63]),
    (64, [64, 0, 768, 1536, 5632, 16896, 1, 64]),
    (65, [128, 0, 1536, 3072, 11264, 33792, 1, 65]),
    (130, [192, 0, 2304, 4608, 16896, 50688, 1, 130]),
    # 12 B x 100 lanes would not be a multiple of 256: 70 rays -> 128 lanes, 1536 B, as for 65
    (70, [128, 0, 1536, 3072, 11264, 33792, 1, 70]),
    (262144, [262144, 0, 3145728, 6291456, 23068672, 69206016, 1, 262144]),
    (262145, [262144, 0, 3145728, 6291456, 23068672, 69206016, 2, 262144, 1]),
    # the 1920 x 1080 camera rays: seven full chunks and 2073600 - 7 x 262144 = 238592
    (2073600, [262144, 0, 3145728, 6291456, 23068672, 69206016, 8] + [262144] * 7 + [238592]),
])
def test_layout_and_chunks(layout, rays, expect):
    got, _ = layout(rays)
    assert got == expect


def test_arrays_do_not_overlap_and_the_deepest_level_fits(layout):
    for rays in (1, 65, 1000, 262144):
        (lanes, origins, dirs, hits, spill, total, _, _), _ = layout(rays)
        assert origins + lanes * 12 <= dirs and dirs + lanes * 12 <= hits and hits + lanes * 64 <= spill
        # level 27 of the last lane: entry (27 - 6) * lanes + lanes - 1 of 8 bytes
        assert spill + ((27 - 6) * lanes + lanes - 1 + 1) * 8 <= total
        assert all(v % 256 == 0 for v in (origins, dirs, hits, spill, total))
