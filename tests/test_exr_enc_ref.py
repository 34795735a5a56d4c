"""tests/exr_enc_ref.py against itself and against bytes written out by hand: the reference's own decoder returns the
converted samples of every case bit for bit, the head of a 2 x 2 file is the layout of include/pt.h spelt out, the
channels are sorted, the offsets and the bound hold, the half conversion in integers (a restatement of
pte::half_bits) agrees with numpy on the table, and every case's certificate says it reaches what it is for."""
import struct

import numpy as np
import pytest

import exr_enc_cases as C
import exr_enc_ref as R

CASES = C.cases()
SMALL = [n for n in CASES if n != "half-table"]


@pytest.fixture(scope="module")
def files():
    return {n: R.encode_stats(C.channels(CASES[n]), CASES[n][2]) for n in CASES}


@pytest.mark.parametrize("name", list(CASES))
def test_decode_returns_the_samples(files, name):
    chans = C.channels(CASES[name])
    data, st = files[name]
    got, attrs = R.decode(data)
    assert list(got) == [c[0] for c in R.sort_channels(chans)]
    for cname, tex, comp, scale, kind in chans:
        want = R.samples(tex, comp, scale, kind)[::-1]
        assert got[cname].dtype == want.dtype and np.array_equal(got[cname], want), cname
    assert attrs["compression"][1][0] == CASES[name][2]
    assert len(data) <= R.file_max(chans, CASES[name][2])
    assert st["header"] == 277 - 18 + sum(len(c[0]) + 17 for c in chans)
    # the offset table: absolute, increasing, each chunk right behind the one before it
    at = st["header"] + 8 * len(st["table"])
    for off in st["table"]:
        assert off == at
        at += 8 + struct.unpack_from("<i", data, off + 4)[0]
    assert at == len(data)


@pytest.mark.parametrize("compression", [R.NONE, R.ZIPS, R.ZIP])
def test_every_compression_of_the_small_cases(compression):
    for name in ("zip-3x17", "names", "scale-half", "noise-zips", "mixed-zips"):
        chans = C.channels(CASES[name])
        got, _ = R.decode(R.encode(chans, compression))
        for cname, tex, comp, scale, kind in chans:
            assert np.array_equal(got[cname], R.samples(tex, comp, scale, kind)[::-1])


def test_a_2x2_file_by_hand():
    tex = np.zeros((2, 2, 4), np.float32)
    tex[0, :, 0] = (1.0, 2.0)      # the bottom row: scanline 1
    tex[1, :, 0] = (-0.5, 0.0)     # the top row: scanline 0
    h = bytes.fromhex
    want = (h("762f3101 02000000")
            + b"channels\0chlist\0" + h("13000000") + b"R\0" + h("02000000 00000000 01000000 01000000") + h("00")
            + b"compression\0compression\0" + h("01000000 00")
            + b"dataWindow\0box2i\0" + h("10000000 00000000 00000000 01000000 01000000")
            + b"displayWindow\0box2i\0" + h("10000000 00000000 00000000 01000000 01000000")
            + b"lineOrder\0lineOrder\0" + h("01000000 00")
            + b"pixelAspectRatio\0float\0" + h("04000000 0000803f")
            + b"screenWindowCenter\0v2f\0" + h("08000000 00000000 00000000")
            + b"screenWindowWidth\0float\0" + h("04000000 0000803f")
            + h("00"))
    assert len(want) == 277
    want += h("2501000000000000 3501000000000000")                     # 277 + 16, + 8 + 8
    want += h("00000000 08000000 000000bf 00000000")                   # y 0: -0.5, 0.0
    want += h("01000000 08000000 0000803f 00000040")                   # y 1: 1.0, 2.0
    assert R.encode([("R", tex, 0, 1.0, R.FLOAT)], R.NONE) == want
    # the same as HALF under ZIPS: 4 raw bytes a scanline, which no zlib stream undercuts, so the data stay raw
    data = R.encode([("R", tex, 0, 1.0, R.HALF)], R.ZIPS)
    assert data[277 + 16:] == h("00000000 04000000 00b8 0000") + h("01000000 04000000 003c 0040")
    assert data[:277] == want[:277].replace(h("02000000 00000000 01000000 01000000"), h("01000000 00000000 01000000 01000000")) \
        .replace(b"compression\0" + h("01000000 00"), b"compression\0" + h("01000000 02"))


def test_the_predictor_by_hand():
    assert R.predict(bytes([1, 2, 3, 4, 5, 6])) == bytes([1, 130, 130, 125, 130, 130])   # 1 3 5 | 2 4 6
    assert R.predict(bytes([7, 7])) == bytes([7, 128])


def test_channels_are_sorted_as_unsigned_bytes(files):
    got, _ = R.decode(files["names"][0])
    assert list(got) == ["A", "B", "G", "R", "Z", "a", "id", "normal.X"]
    assert list(R.decode(files["chan-16"][0])[0]) == sorted(c[0] for c in CASES["chan-16"][1])


def half_bits_int(f):
    """pte::half_bits (csrc/pt_exr_enc.h) restated on numpy integers"""
    f = f.astype(np.uint64)
    sign, a = (f >> 16) & 0x8000, f & 0x7FFFFFFF
    r = a - 0x38000000
    normal = sign | ((r + 0xFFF + ((r >> 13) & 1)) >> 13)
    e = a >> 23
    shift = np.clip(126 - e.astype(np.int64), 14, 24).astype(np.uint64)
    m = (a & 0x7FFFFF) | 0x800000
    q = m >> shift
    rem, mid = m & ((np.uint64(1) << shift) - 1), np.uint64(1) << (shift - 1)
    q = q + ((rem > mid) | ((rem == mid) & (q & 1 == 1)))
    out = np.where(a > 0x7F800000, 0x7E00,
                   np.where(a >= 0x477FF000, sign | 0x7C00, np.where(a >= 0x38800000, normal, np.where(e < 102, sign, sign | q))))
    return out.astype(np.uint16)


def test_integer_half_conversion_matches_numpy_on_the_table():
    table, used = C.half_table()
    assert used >= 253000
    flat = table.reshape(-1)
    assert np.array_equal(half_bits_int(flat.view(np.uint32)), R.half_bits(flat))
    assert np.array_equal(half_bits_int(C.SPECIAL.view(np.uint32)), R.half_bits(C.SPECIAL))
    nan = np.isnan(flat)
    assert nan.sum() == 8 and (R.half_bits(flat)[nan] == 0x7E00).all()
    # every half value but the NaNs is hit, subnormals, both zeros and both infinities included
    assert len(np.unique(R.half_bits(flat))) == 2 * 0x7C01 + 1


def test_samples_by_hand():
    t = np.zeros((1, 6, 4), np.float32)
    t[0, :, 0] = C.bits([0x7FC12345, 0x00000001, 0x3F800000, 0xFF800000, 0x477FF000, 0x00800000])
    assert list(R.samples(t, 0, 1.0, R.FLOAT)[0]) == [0x7FC12345, 1, 0x3F800000, 0xFF800000, 0x477FF000, 0x00800000]
    assert list(R.samples(t, 0, 0.5, R.FLOAT)[0]) == [0x7FC00000, 0, 0x3F000000, 0xFF800000, 0x46FFF000, 0x00400000]
    assert list(R.samples(t, 0, -2.0, R.FLOAT)[0]) == [0x7FC00000, 0x80000002, 0xC0000000, 0x7F800000, 0xC7FFF000, 0x81000000]
    assert list(R.samples(t, 0, 1.0, R.HALF)[0]) == [0x7E00, 0, 0x3C00, 0xFC00, 0x7C00, 0]


def test_certificates(files):
    cert = {n: R.certificate(C.channels(CASES[n]), CASES[n][2]) for n in SMALL if CASES[n][2] != R.NONE}
    assert cert["zip-3x1"]["blocks"] == 1 and cert["zip-3x15"]["blocks"] == 1 and cert["zip-3x16"]["blocks"] == 1
    assert cert["zip-3x17"]["block_bytes"] == [288, 18] and cert["zip-3x33"]["block_bytes"] == [288, 288, 18]
    assert cert["zips-3x17"]["blocks"] == 17
    # a block of exactly one piece; a second piece of 32 and of 4 bytes; five pieces, and two in the short last block
    assert cert["piece-510"]["block_bytes"] == [R.PIECE] and cert["piece-510"]["pieces"] == [1]
    assert cert["piece-511"]["pieces"] == [2] and cert["piece-511"]["piece_tail"] == [32]
    assert cert["piece-4080"]["pieces"] == [1, 1] and cert["piece-4080"]["block_bytes"] == [R.PIECE] * 2
    assert cert["piece-4081"]["pieces"] == [2, 2] and cert["piece-4081"]["piece_tail"] == [4, 4]
    assert cert["pieces-5"]["pieces"] == [5, 2]
    # more blocks than a trip of the scan's loop; more pieces than that as well
    assert cert["scan-5x300"]["blocks"] > C.SCAN_TILE
    assert cert["scan-2100x260"]["blocks"] > C.SCAN_TILE and cert["scan-2100x260"]["pieces"][0] == 2
    # constant planes compress into long matches, across pieces; noise falls back everywhere; the mix does both
    assert cert["const-zip"]["pieces"] == [6, 6] and not any(cert["const-zip"]["fell_back"])
    assert len(files["const-zip"][0]) < sum(cert["const-zip"]["block_bytes"]) // 8
    assert all(cert["noise-zips"]["fell_back"]) and all(cert["noise-zip"]["fell_back"])
    assert cert["noise-zips"]["block_bytes"] == [800] * 3 and cert["noise-zip"]["block_bytes"] == [12800]
    assert cert["mixed-zips"]["block_bytes"] == [2000] * 8
    assert cert["mixed-zips"]["fell_back"] == [True, False] * 4       # (scanline 0 is row 7, all noise)
    types = set().union(*(c["types"] for c in cert.values()))
    assert types == {"stored", "fixed", "dynamic"}
    assert len(CASES["chan-16"][1]) == R.CHANNELS_MAX and len({s[1] for s in CASES["chan-16"][1]}) == 4
    assert {s[4] for s in CASES["chan-16"][1]} == {R.HALF, R.FLOAT}
