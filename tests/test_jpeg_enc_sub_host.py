"""The host half of pt_canvas_encode_jpeg_sub (csrc/pt_jpeg_enc.h, and pt::JpegLayout in csrc/pt_plan.h) with Y
sampled 2x1 (4:2:2) and 2x2 (4:2:0): the file header and the workspace's layout. Host C++ only: a small program
over the two headers, no GPU. The header is compared with tests/jpeg_enc_sub_ref.py, which
tests/test_jpeg_encode_sub.py pins against libjpeg-turbo; the layout with literals worked out by hand."""
import os
import shutil
import subprocess

import pytest

import jpeg_enc_ref as R
import jpeg_enc_sub_ref as S

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
    if (argc != 6) return 2;
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), ss = std::atoi(argv[5]);
    const int hs = ptj::sampling_h(ss), vs = ptj::sampling_v(ss);
    if (!std::strcmp(cmd, "header")) {                     // header w h quality subsampling -> hex
        std::vector<uint8_t> buf(4096);
        const size_t n = ptj::write_header(buf.data(), w, h, ptj::quant_tables(std::atoi(argv[4])), hs, vs);
        if (n != pt::kJpegHeader) return 3;
        for (size_t i = 0; i < n; i++) std::printf("%02x", buf[i]);
    } else if (!std::strcmp(cmd, "layout")) {              // layout w h 0 subsampling
        const pt::JpegLayout L(w, h, hs, vs);
        std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", L.mcus_x, L.blocks_row, L.rows,
                    L.row_stride, L.tiles, L.coef, L.bitoff, L.bits, L.tileoff, L.rowbits, L.rowlen, L.rowoff, L.total,
                    L.bytes, L.stream_max());
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
    d = tmp_path_factory.mktemp("jpeg_enc_sub")
    (d / "main.cpp").write_text(MAIN)
    exe = str(d / "main")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, str(d / "main.cpp")], check=True)
    return lambda *a: subprocess.run([exe, *[str(v) for v in a]], check=True, capture_output=True, text=True).stdout


@pytest.mark.parametrize("ss", [1, 2], ids=["422", "420"])
@pytest.mark.parametrize("w,h,q", [(1, 1, 1), (17, 9, 50), (1920, 1080, 75), (65535, 65535, 100)])
def test_header_is_the_references(enc, w, h, q, ss):
    got = bytes.fromhex(enc("header", w, h, q, ss).strip())
    assert got == S.header(w, h, q, ss)
    # and it is the 4:4:4 header but for SOF0's Y sampling byte and DRI's count
    base = R.header(w, h, q)
    diff = [i for i in range(len(base)) if base[i] != got[i]]
    sof, dri = base.index(b"\xff\xc0"), base.index(b"\xff\xdd\x00\x04")
    assert set(diff) <= {sof + 11, dri + 4, dri + 5} and sof + 11 in diff
    assert got[sof + 11] == (0x21 if ss == 1 else 0x22)
    assert int.from_bytes(got[dri + 4:dri + 6], "big") == (w + 15) // 16


def test_subsampling_0_is_the_default(enc):
    assert bytes.fromhex(enc("header", 17, 9, 50, 0).strip()) == R.header(17, 9, 50)
    assert [int(v) for v in enc("layout", 17, 9, 0, 0).split()][:5] == [3, 9, 2, 1872, 2]


def test_layout_by_hand(enc):
    # 24x24 at 4:2:0: 2 x 2 MCUs of 16x16, 6 blocks each = 12 blocks a row of 208 B = 2496 B = 3 tiles; every
    # array from a 256 B boundary
    L = [int(v) for v in enc("layout", 24, 24, 0, 2).split()]
    assert L[:5] == [2, 12, 2, 2496, 3]
    coef, bitoff, bits, tileoff, rowbits, rowlen, rowoff, total, size, stream_max = L[5:]
    assert coef == 0 and bitoff == 3072            # 24 blocks x 128 B
    assert bits == 3072 + 256                      # 24 x 4 B
    assert tileoff == bits + 5120                  # 2 x 2496 = 4992 -> 5120
    assert (rowbits, rowlen, rowoff, total) == (tileoff + 256, tileoff + 512, tileoff + 768, tileoff + 1024)
    assert size == total + 256
    assert stream_max == 2 * (2 * 2496 + 2)
    # 24x16 at 4:2:2: 2 MCUs of 16x8, 4 blocks each, x 2 rows
    assert [int(v) for v in enc("layout", 24, 16, 0, 1).split()][:5] == [2, 8, 2, 1664, 2]
    # 3840x2160 at 4:2:0: 240 x 135 MCUs; at 4:2:2: 240 x 270 MCUs of 4 blocks
    L = [int(v) for v in enc("layout", 3840, 2160, 0, 2).split()]
    assert L[:5] == [240, 1440, 135, 299520, 293]
    # 194 400 blocks: coef 24 883 200 B (a multiple of 256), bitoff 777 600 B -> 3038 x 256 = 777 728
    assert L[5 + 1] == 24883200 and L[5 + 2] == 24883200 + 777728
    assert [int(v) for v in enc("layout", 3840, 2160, 0, 1).split()][:5] == [240, 960, 270, 199680, 195]
    # the widest and tallest: a row's stuffed bytes stay below 2^24 (pt_jpeg_scan_rows adds 256 of them in 32 bits)
    for ss, blocks in ((1, 4096 * 4), (2, 4096 * 6)):
        L = [int(v) for v in enc("layout", 65535, 65535, 0, ss).split()]
        assert L[1] == blocks and 2 * L[3] + 2 < 1 << 24
