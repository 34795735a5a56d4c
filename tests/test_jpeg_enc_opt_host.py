"""The host half of pt_canvas_encode_jpeg_opt with optimize = 1 (csrc/pt_jpeg_enc.h, and pt::JpegLayout /
pt::JpegOptLayout in csrc/pt_plan.h): the header that carries the frame's own Huffman tables, the bit packer that
host and kernels share, and the workspace's per-block bound. Host C++ only: a small program over the two headers, no
GPU. The header is compared with tests/jpeg_enc_opt_ref.py, which tests/test_jpeg_encode_opt.py pins against
libjpeg-turbo; the packer with a bit-by-bit restatement here.

Why the packer is tested apart from any image: with the Annex K tables a lane's share of a block (three ZRLs of 11
bits, a 16-bit code, 10 value bits) is at most 59 bits and fits one 64-bit word; with tables built for the frame
every code may be 16 bits long and the share 3 x 16 + 16 + 10 = 74. No frame of a size a test can afford reaches that
(tests/test_gpu_jpeg_encode_opt.py states what its frame reaches), so synthetic tables of 16-bit codes do."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_enc_opt_ref as O
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
static int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }
int main(int argc, char** argv)
{
    const char* cmd = argc > 1 ? argv[1] : "";
    if (!std::strcmp(cmd, "header") && argc == 7) {        // header w h quality subsampling tables-hex -> hex
        const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), ss = std::atoi(argv[5]);
        ptj::OptTables o;
        if (std::strlen(argv[6]) != 2 * sizeof(o)) return 3;
        for (size_t i = 0; i < sizeof(o); i++) ((uint8_t*)&o)[i] = (uint8_t)(hexval(argv[6][2 * i]) << 4 | hexval(argv[6][2 * i + 1]));
        for (int t = 0; t < 4; t++) if (ptj::opt_table_symbols(o, t) < 0) return 4;
        std::vector<uint8_t> buf(ptj::kOptHeaderMax + 64, 0xA5);
        const size_t n = ptj::write_header(buf.data(), w, h, ptj::quant_tables(std::atoi(argv[4])), ptj::sampling_h(ss),
                                           ptj::sampling_v(ss), o);
        if (n > ptj::kOptHeaderMax) return 5;
        for (size_t i = n; i < buf.size(); i++) if (buf[i] != 0xA5) return 6;
        for (size_t i = 0; i < n; i++) std::printf("%02x", buf[i]);
    } else if (!std::strcmp(cmd, "symbols") && argc == 3) {   // symbols tables-hex -> the four counts
        ptj::OptTables o;
        if (std::strlen(argv[2]) != 2 * sizeof(o)) return 3;
        for (size_t i = 0; i < sizeof(o); i++) ((uint8_t*)&o)[i] = (uint8_t)(hexval(argv[2][2 * i]) << 4 | hexval(argv[2][2 * i + 1]));
        for (int t = 0; t < 4; t++) std::printf("%d ", ptj::opt_table_symbols(o, t));
    } else if (!std::strcmp(cmd, "pack") && argc == 8) {
        // pack k v nonzero-mask-hex code-bits zrl-bits at salt: lane k holding v in a block whose non-zero lanes
        // are the mask, under a table whose every code is `code-bits` long (the ZRL `zrl-bits`) with the pattern
        // salt in it -> the symbols, the two lengths and the four words of the window at bit `at`
        const int k = std::atoi(argv[2]), v = std::atoi(argv[3]);
        const unsigned long long mask = std::strtoull(argv[4], nullptr, 16);
        const int cl = std::atoi(argv[5]), zl = std::atoi(argv[6]);
        const unsigned at = (unsigned)std::atoi(argv[7]);
        std::vector<uint32_t> tab(256);
        for (int s = 0; s < 256; s++) tab[s] = ((0xACE1u * (s + 1)) & ((1u << cl) - 1u)) | (uint32_t)cl << 16;
        const uint32_t zrl = (0xB5C3u & ((1u << zl) - 1u)) | (uint32_t)zl << 16;
        const ptj::LaneSyms s = ptj::lane_symbols(k, v, 0, mask);
        const ptj::LaneBits b = ptj::lane_bits(s, tab.data(), zrl);
        uint32_t w[4];
        ptj::lane_window(b, at, w);
        std::printf("%d %d %d %u %d %d %08x %08x %08x %08x", s.sym, s.zrls, s.n, s.val, b.zrl_len, b.code_len, w[0], w[1],
                    w[2], w[3]);
    } else if (!std::strcmp(cmd, "layout") && argc == 5) {   // layout w h subsampling
        const int ss = std::atoi(argv[4]);
        const pt::JpegLayout A(std::atoi(argv[2]), std::atoi(argv[3]), ptj::sampling_h(ss), ptj::sampling_v(ss));
        const pt::JpegLayout B(std::atoi(argv[2]), std::atoi(argv[3]), ptj::sampling_h(ss), ptj::sampling_v(ss),
                               pt::kJpegOptBlockBytes);
        const pt::JpegOptLayout O;
        std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", pt::kJpegBlockBytes,
                    pt::kJpegOptBlockBytes, A.blocks_row, A.row_stride, A.bytes, B.blocks_row, B.row_stride, B.tiles,
                    B.bits, B.tileoff, B.bytes, B.stream_max(), O.hist, O.codes, O.total, O.tables, O.bytes,
                    sizeof(ptj::OptTables));
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
    d = tmp_path_factory.mktemp("jpeg_enc_opt")
    (d / "main.cpp").write_text(MAIN)
    exe = str(d / "main")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, str(d / "main.cpp")], check=True)
    return lambda *a: subprocess.run([exe, *[str(v) for v in a]], check=True, capture_output=True, text=True).stdout


def tables_hex(tables):
    """ptj::OptTables: bits[4][16], then vals[4][256] zero-padded"""
    out = bytearray()
    for bits, _ in tables:
        out += bytes(bits)
    for _, vals in tables:
        out += bytes(vals) + bytes(256 - len(vals))
    return out.hex()


def frame(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 3 + yy, yy * 2, xx + yy * 3], -1) % 256
    return np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("ss", [0, 1, 2], ids=["444", "422", "420"])
@pytest.mark.parametrize("w,h,q", [(1, 1, 1), (17, 9, 50), (48, 40, 75), (64, 64, 100)])
def test_header_is_the_references(enc, w, h, q, ss):
    data, stats = O.encode_stats(frame(w, h, w + q), q, ss)
    want = O.header(w, h, q, ss, stats["tables"])
    assert data.startswith(want)
    got = bytes.fromhex(enc("header", w, h, q, ss, tables_hex(stats["tables"])).strip())
    assert got == want
    # the same segments in the same order as the standard header, which differs only inside the four DHTs
    std = S.header(w, h, q, ss)
    first, dri = std.index(b"\xff\xc4"), std.index(b"\xff\xdd\x00\x04")
    assert got[:first] == std[:first] and got[-(len(std) - dri):] == std[dri:]
    assert [int(v) for v in enc("symbols", tables_hex(stats["tables"])).split()] == [len(v) for _, v in stats["tables"]]


def test_header_of_full_tables_and_tables_it_refuses(enc):
    """256 AC symbols in both AC tables and 12 categories in both DC tables: the longest header; and tables the host
    must not write from: more than 256 symbols, a DC category past 11"""
    def full(n):
        bits = [0] * 16
        left = n
        for i in (7, 8, 15):
            take = min(left, 100 if i < 15 else 255)
            bits[i], left = take, left - take
        assert left == 0
        return bits, list(range(n))
    tables = [full(12), full(256), full(12), full(256)]
    got = bytes.fromhex(enc("header", 640, 480, 90, 2, tables_hex(tables)).strip())
    assert got == O.header(640, 480, 90, 2, tables)
    assert len(got) == 629 - 2 * (12 + 162) + 2 * (12 + 256)
    bad = [full(12), (([0] * 14) + [200, 100], list(range(256))), full(12), full(256)]
    assert enc("symbols", tables_hex(bad)).split() == ["12", "-1", "12", "256"]
    bad = [full(12), full(256), ([0, 2] + [0] * 14, [0, 12]), full(256)]
    assert enc("symbols", tables_hex(bad)).split() == ["12", "256", "-1", "256"]


def restated_window(pieces, at):
    """the pieces [(value, length)] written bit by bit from bit `at`, MSB first, into four 32-bit words"""
    w = [0, 0, 0, 0]
    pos = at & 31
    for value, length in pieces:
        for i in range(length - 1, -1, -1):
            if value >> i & 1:
                w[pos >> 5] |= 1 << (31 - (pos & 31))
            pos += 1
    assert pos <= 128
    return w


@pytest.mark.parametrize("run", [0, 15, 16, 47, 48, 62])
def test_packer_carries_74_bits(enc, run):
    """all-16-bit tables: a lane after `run` zeros holds run >> 4 ZRLs of 16 bits, a 16-bit code and 10 value bits,
    74 bits at run 48..62, at every bit offset of the first word"""
    k = run + 1
    mask = 1 | 1 << k                       # the DC and lane k alone are non-zero
    for v in (1023, -1023, 512, -1):
        n = abs(v).bit_length()
        val = (v - 1 if v < 0 else v) & ((1 << n) - 1)
        sym = (run & 15) << 4 | n
        code = (0xACE1 * (sym + 1)) & 0xFFFF
        zrl = 0xB5C3
        pieces = [(zrl, 16)] * (run >> 4) + [(code, 16), (val, n)]
        for at in (0, 1, 7, 31, 32 * 5 + 13, 32 * 1000 + 31):
            out = enc("pack", k, v, "%x" % mask, 16, 16, at).split()
            assert [int(x) for x in out[:6]] == [sym, run >> 4, n, val, 16 * (run >> 4), 16 + n]
            assert [int(x, 16) for x in out[6:]] == restated_window(pieces, at), (run, v, at)
    if run >= 48:
        assert 16 * (run >> 4) + 16 + 10 == 74


def test_packer_dc_eob_and_short_codes(enc):
    # the DC of lane 0 (its category's code and value), the EOB of lane 63, a zero lane, and codes of 1 and 11 bits
    for cl in (1, 11, 16):
        m = (1 << cl) - 1
        out = enc("pack", 0, -300, "1", cl, cl, 37).split()
        assert [int(x) for x in out[:6]] == [9, 0, 9, (-301) & 511, 0, cl + 9]
        assert [int(x, 16) for x in out[6:]] == restated_window([((0xACE1 * 10) & m, cl), ((-301) & 511, 9)], 37)
        out = enc("pack", 63, 0, "1", cl, cl, 95).split()
        assert [int(x) for x in out[:6]] == [0, 0, 0, 0, 0, cl]
        assert [int(x, 16) for x in out[6:]] == restated_window([(0xACE1 & m, cl)], 95)
        out = enc("pack", 40, 0, "1", cl, cl, 3).split()
        assert [int(x) for x in out[:6]] == [-1, 0, 0, 0, 0, 0] and [int(x, 16) for x in out[6:]] == [0] * 4
    # a run that starts behind another non-zero AC: lane 40 after lane 5 -> 34 zeros, two ZRLs and run 2
    out = enc("pack", 40, 3, "%x" % (1 | 1 << 5 | 1 << 40 | 1 << 50), 16, 11, 30).split()
    assert [int(x) for x in out[:6]] == [2 << 4 | 2, 2, 2, 3, 22, 18]
    z = 0xB5C3 & 0x7FF
    assert [int(x, 16) for x in out[6:]] == restated_window([(z, 11), (z, 11), ((0xACE1 * 0x23) & 0xFFFF, 16), (3, 2)], 30)


def test_block_bound_and_layouts(enc):
    L = [int(v) for v in enc("layout", 24, 24, 2).split()]
    std_block, opt_block, a_blocks, a_stride, a_bytes, b_blocks, b_stride, b_tiles, b_bits, b_tileoff, b_bytes, \
        b_stream, hist, codes, total, tables, obytes, sizeof_tables = L
    assert std_block == 208                                   # the standard path's bound is unchanged
    assert 8 * opt_block >= 63 * (16 + 10) + 16 + 11 == 1665  # every code 16 bits long
    assert 8 * std_block < 1665 and opt_block % 16 == 0 and opt_block == 224
    # 24x24 at 4:2:0 as in tests/test_jpeg_enc_sub_host.py: 12 blocks a row; the standard layout as it was
    assert (a_blocks, a_stride) == (12, 2496) and a_bytes == 3072 + 256 + 5120 + 256 * 5
    assert (b_blocks, b_stride, b_tiles) == (12, 12 * 224, 3)
    assert b_bits == 3072 + 256 and b_tileoff == b_bits + 5376 and b_stream == 2 * (2 * 2688 + 2)
    assert b_bytes == b_tileoff + 256 * 5
    # what the optimised tables add: 8 KiB of counts, the codes, and the length with the tables right behind it
    assert (hist, codes, total, tables) == (0, 8192, 8192 + 2304, 8192 + 2304 + 8)
    assert sizeof_tables == 4 * 16 + 4 * 256 and obytes == total + 1280
    # the widest rows stay below 2^24 stuffed bytes (pt_jpeg_scan_rows adds 256 of them in 32 bits)
    for ss in (0, 1, 2):
        b_stride = int(enc("layout", 65535, 65535, ss).split()[6])
        assert 2 * b_stride + 2 < 1 << 24
