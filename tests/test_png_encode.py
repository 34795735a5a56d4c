"""The PNG reference itself (tests/png_enc_ref.py): the numpy filters, Python's zlib with the calls include/pt.h names,
struct and zlib.crc32 for the framing. For every case Pillow must decode the file to exactly the pixels, and the
chunk count and block types must be the ones named here; the block walker of png_enc_ref.py certifies what each case
reaches. The figures printed here are recorded in DESIGN.md section 6 as properties of the format."""
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import png_enc_cases as C
import png_enc_ref as P


def blocks_of(stats):
    """the file's deflate blocks, without the empty stored block of every full flush"""
    raw = b"".join(stats["payloads"])[2:-4]
    return [b for b in P.walk_blocks(raw) if not (b["type"] == "stored" and b["out"] == 0)]


def check(rows, colour, filt):
    data, stats = P.encode_stats(rows, colour, filt)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == ("RGBA" if colour == P.RGBA else "RGB") and im.info.get("interlace", 0) == 0
    assert np.array_equal(np.asarray(im), rows if colour == P.RGBA else rows[..., :3])
    h, w = rows.shape[:2]
    bpp = 4 if colour == P.RGBA else 3
    assert len(stats["stream"]) == h * (1 + bpp * w)
    assert len(stats["payloads"]) == -(-len(stats["stream"]) // P.CHUNK) and all(stats["payloads"])
    # the framing: signature, IHDR, one IDAT per chunk each with its own CRC, IEND; nothing else
    at, kinds = 8, []
    assert data[:8] == P.SIGNATURE
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(data[at + 4:at + 8 + n])
        kinds.append(kind)
        at += 12 + n
    assert kinds == [b"IHDR"] + [b"IDAT"] * len(stats["payloads"]) + [b"IEND"]
    # the stream framing: 78 01 before the first chunk, the Adler-32 of the whole stream behind the last, every
    # non-final chunk ends in the empty stored block, and every chunk inflates alone to its own bytes
    whole = b"".join(stats["payloads"])
    assert whole[:2] == b"\x78\x01" and whole[-4:] == struct.pack(">I", zlib.adler32(stats["stream"]))
    for i, p in enumerate(stats["payloads"]):
        last = i == len(stats["payloads"]) - 1
        body = p[2 if i == 0 else 0:len(p) - (4 if last else 0)]
        if not last:
            assert body.endswith(b"\x00\x00\xff\xff")
        assert zlib.decompressobj(-15).decompress(body) == stats["stream"][i * P.CHUNK:(i + 1) * P.CHUNK]
    return data, stats


def noise(w, h, seed=0):
    return np.random.default_rng(seed + w * 1009 + h).integers(0, 256, (h, w, 4), dtype=np.uint8)


def gradient(w, h, noisy, seed=0):
    rng = np.random.default_rng(seed + 5)
    yy, xx = np.mgrid[0:h, 0:w]
    px = np.empty((h, w, 4), np.uint8)
    base = np.stack([xx + yy // 2, 2 * yy + xx // 3, 255 - xx - yy // 4], -1)
    px[..., :3] = (base + (rng.integers(0, 4, (h, w, 3)) if noisy else 0)) % 256
    px[..., 3] = rng.integers(0, 256, (h, w))
    return px


def test_one_pixel_is_one_fixed_block():
    for colour in (P.RGB, P.RGBA):
        for filt in range(6):
            _, stats = check(noise(1, 1), colour, filt)
            assert [b["type"] for b in blocks_of(stats)] == ["fixed"]


def test_noise_is_two_stored_blocks():
    _, stats = check(noise(100, 100), P.RGB, P.NONE)
    assert [b["type"] for b in blocks_of(stats)] == ["stored"] * 2
    assert [len(p) for p in stats["payloads"]] == [P.CHUNK + 12, 100 * 301 - P.CHUNK + 9]


def test_flat_is_three_dynamic_blocks():
    px = np.zeros((120, 100, 4), np.uint8)
    data, stats = check(px, P.RGB, P.NONE)
    assert [b["type"] for b in blocks_of(stats)] == ["dynamic"] * 3
    assert all(b["matches"] == b["symbols"] - 1 or b["symbols"] - b["matches"] <= 3 for b in blocks_of(stats))


def test_gradient_plus_noise_and_the_clean_gradient(capsys):
    """six dynamic blocks; with noise the chunked Z_RLE stream is not longer than level-6 default zlib over the same
    filtered bytes by more than the framing, without noise it is many times longer: no match crosses a row"""
    figures, types = {}, {}
    for noisy in (True, False):
        _, stats = check(np.ascontiguousarray(gradient(200, 150, noisy)[::-1]), P.RGB, P.ADAPTIVE)
        assert [b["type"] for b in blocks_of(stats)] == ["dynamic"] * 6
        types[noisy] = set(stats["types"])
        ours, default = sum(len(p) for p in stats["payloads"]), len(zlib.compress(stats["stream"], 6))
        figures[noisy] = (ours, default)
    with capsys.disabled():
        print("\n200x150 gradient, adaptive, RGB: noisy %d B against %d B for zlib level 6; clean %d B against %d B"
              % (figures[True] + figures[False]))
    assert figures[True][0] < 1.05 * figures[True][1]
    assert figures[False][0] > 5 * figures[False][1]
    assert len(types[True]) >= 3   # (the canvas of tests/test_gpu_png_encode.py, top-down)


@pytest.mark.parametrize("h,chunks", [(1020, 1), (1021, 2), (2040, 2)])
def test_chunk_edges(h, chunks):
    _, stats = check(noise(5, h), P.RGB, P.NONE)
    assert len(stats["payloads"]) == chunks


def test_adaptive_takes_the_lowest_type_on_a_tie():
    px = np.empty((4, 1, 4), np.uint8)
    px[...] = (200, 7, 130, 99)
    assert P.encode_stats(px, P.RGB, P.ADAPTIVE)[1]["types"] == [P.NONE, P.UP, P.UP, P.UP]
    px = np.empty((4, 6, 4), np.uint8)
    px[...] = (200, 7, 130, 99)
    assert P.encode_stats(px, P.RGBA, P.ADAPTIVE)[1]["types"] == [P.SUB, P.UP, P.UP, P.UP]


def test_literal_codes_at_fifteen_bits():
    """zlib reaches a 15-bit literal code where an unlimited Huffman tree over the same counts is 17 deep: the case
    pins the overflow repair"""
    row = C.fibonacci_row()
    check(C.row_pixels(row), P.RGB, P.NONE)
    block = C.first_block(row)
    assert block["type"] == "dynamic" and block["maxlen"][0] == 15 and block["matches"] == 0
    assert C.unlimited_depth(C.literal_counts(row)) == 17


def test_code_length_codes_at_seven_bits():
    """The search asked for found one: a row whose header's code-length symbols would make an unlimited tree 8 deep,
    so zlib's repair runs on the code-length tree too, which comes out at its limit of 7 bits. The host program
    (tests/test_png_enc_host.py) and the GPU test run this row against zlib's bytes."""
    found = C.code_length_overflow_row()
    assert found is not None, "the seeded search finds a row within its tries"
    row, block = found
    assert C.unlimited_depth(block["clcounts"]) > 7 and block["maxlen"][2] == 7
    check(C.row_pixels(row), P.RGB, P.NONE)
