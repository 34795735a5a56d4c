"""The host half of pt_canvas_encode_jpeg (csrc/pt_jpeg_enc.h, and pt::JpegLayout in csrc/pt_plan.h): the file
header it writes, the quantisation tables of a quality, the Huffman codes derived at compile time and the
workspace's layout. Host C++ only: a small program over the two headers, no GPU. The header, tables and codes are
compared with tests/jpeg_enc_ref.py, which tests/test_jpeg_encode.py pins against libjpeg-turbo; the layout with
literals worked out by hand."""
import os
import shutil
import subprocess

import pytest

import jpeg_enc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "babylon.js-pathtracing-renderer_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "pt_plan.h"
#include "pt_jpeg_enc.h"
int main(int argc, char** argv)
{
    const char* cmd = argc > 1 ? argv[1] : "";
    if (!std::strcmp(cmd, "header") && argc == 5) {        // header w h quality -> hex
        std::vector<uint8_t> buf(4096);
        const size_t n = ptj::write_header(buf.data(), std::atoi(argv[2]), std::atoi(argv[3]),
                                           ptj::quant_tables(std::atoi(argv[4])));
        if (n != pt::kJpegHeader) return 3;
        for (size_t i = 0; i < n; i++) std::printf("%02x", buf[i]);
    } else if (!std::strcmp(cmd, "codes")) {               // table symbol code length, one per line
        constexpr ptj::HuffCodes h = ptj::make_codes();
        for (int t = 0; t < 2; t++) {
            for (int s = 0; s < 12; s++) std::printf("dc%d %d %u %u\n", t, s, h.dc[t][s] & 0xFFFFu, h.dc[t][s] >> 16);
            for (int s = 0; s < 256; s++)
                if (h.ac[t][s]) std::printf("ac%d %d %u %u\n", t, s, h.ac[t][s] & 0xFFFFu, h.ac[t][s] >> 16);
        }
    } else if (!std::strcmp(cmd, "layout") && argc == 4) {  // layout w h
        const pt::JpegLayout L(std::atoi(argv[2]), std::atoi(argv[3]));
        std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", L.blocks_row, L.rows, L.row_stride, L.tiles,
                    L.coef, L.bitoff, L.bits, L.tileoff, L.rowbits, L.rowlen, L.rowoff, L.total, L.bytes, L.stream_max());
    } else if (!std::strcmp(cmd, "room") && argc == 4) {    // room need stream_max
        std::printf("%zu", pt::jpeg_out_room((size_t)std::atoll(argv[2]), (size_t)std::atoll(argv[3])));
    } else {
        return 2;
    }
    std::printf("\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++")
                if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("jpeg_enc")
    (d / "main.cpp").write_text(MAIN)
    exe = str(d / "main")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, str(d / "main.cpp")], check=True)
    return lambda *a: subprocess.run([exe, *[str(v) for v in a]], check=True, capture_output=True, text=True).stdout


@pytest.mark.parametrize("w,h,q", [(1, 1, 1), (17, 9, 50), (1920, 1080, 75), (3840, 2160, 90), (65535, 65535, 100), (24, 80, 49)])
def test_header_is_the_references(enc, w, h, q):
    assert bytes.fromhex(enc("header", w, h, q).strip()) == R.header(w, h, q)


def test_codes_are_annex_c(enc):
    got = {}
    for line in enc("codes").split("\n"):
        if not line.strip():
            continue
        name, sym, code, length = line.split()
        got[(name, int(sym))] = (int(code), int(length))
    want = {}
    for t in range(2):
        want.update({("dc%d" % t, s): v for s, v in R.DC_TAB[t].items()})
        want.update({("ac%d" % t, s): v for s, v in R.AC_TAB[t].items()})
    assert got == want and len(got) == 2 * (12 + 162)


def test_stream_buffer_grows_with_headroom(enc):
    """a quarter more than the stream, 64 KiB at least, the canvas's bound at most; never less than the stream"""
    assert int(enc("room", 300000, 10 ** 9)) == 375000
    assert int(enc("room", 11, 10 ** 9)) == 65536
    assert int(enc("room", 11, 420)) == 420             # a bound below the floor
    assert int(enc("room", 7000, 7492)) == 7492         # 17x9 at its worst: capped, still >= the stream
    assert int(enc("room", 7492, 7492)) == 7492


def test_layout_by_hand(enc):
    # 17x9: 3 MCUs x 2 rows, 9 blocks a row of 208 B = 1872 B = 2 tiles; every array from a 256 B boundary
    L = [int(v) for v in enc("layout", 17, 9).split()]
    assert L[:4] == [9, 2, 1872, 2]
    coef, bitoff, bits, tileoff, rowbits, rowlen, rowoff, total, size, stream_max = L[4:]
    assert coef == 0 and bitoff == 2304           # 18 blocks x 128 B
    assert bits == 2304 + 256                     # 18 x 4 B
    assert tileoff == bits + 3840                 # 2 x 1872 = 3744 -> 3840
    assert (rowbits, rowlen, rowoff, total) == (tileoff + 256, tileoff + 512, tileoff + 768, tileoff + 1024)
    assert size == total + 256
    assert stream_max == 2 * (2 * 1872 + 2)
    # 3840x2160: 480 x 270 MCUs
    L = [int(v) for v in enc("layout", 3840, 2160).split()]
    assert L[:4] == [1440, 270, 299520, 293]
    assert L[4 + 2] == 1440 * 270 * 132           # coef and bitoff are multiples of 256 here
