"""Inputs that drive zlib's trees to their code-length limits, shared by the PNG encoder's tests. Each is one row of
RGB pixels for filter None, so the filtered stream is a zero byte and the row's bytes, one chunk, one dynamic block."""
import heapq

import numpy as np

import png_enc_ref as P


def unlimited_depth(counts):
    """the depth of a Huffman tree over the non-zero counts with no length limit"""
    heap = [(c, 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def first_block(row_bytes):
    """the one deflate block of the row under filter None, as zlib writes it"""
    payloads = P.deflate_chunks(b"\x00" + row_bytes)
    assert len(payloads) == 1
    block, = P.walk_blocks(payloads[0][2:-4])
    return block


def fibonacci_row():
    """3,642 RGB pixels: 10,926 bytes of 17 values counted 1, 2, f(k-1) + f(k-2) + 1, equal bytes never adjacent (no
    run reaches a match). zlib's literal tree is cut to 15 bits where an unlimited one is 17 deep."""
    f = [1, 2]
    while len(f) < 17:
        f.append(f[-1] + f[-2] + 1)
    assert sum(f) == 10926 == 3 * 3642
    left = dict(enumerate(f))
    out = []
    while len(out) < 10926:   # always the most plentiful value that differs from the last byte
        v = next(v for v in sorted(left, key=lambda v: -left[v]) if left[v] and (not out or out[-1] != v))
        out.append(v)
        left[v] -= 1
    row = bytes(out)
    assert all(row[i] != row[i + 1] for i in range(len(row) - 1))
    return row


def literal_counts(row_bytes):
    counts = np.bincount(np.frombuffer(b"\x00" + row_bytes, np.uint8), minlength=257).tolist()
    counts[256] = 1   # the end-of-block symbol
    return counts


_found = {}


def code_length_overflow_row(tries=400):
    """A row whose dynamic header's code-length symbols would make an unlimited tree deeper than 7, so zlib's repair
    runs on the third tree: the first hit of a seeded search over rows of skewed byte distributions (power laws and
    exponentials over 20..255 values, 2,001..15,999 bytes in whole pixels). Returns (row bytes, its block)."""
    if "row" in _found:
        return _found["row"]
    rng = np.random.default_rng(1)
    for _ in range(tries):
        k, size = int(rng.integers(20, 256)), 3 * int(rng.integers(667, 5334))
        if rng.random() < 0.5:
            w = 1.0 / np.arange(1, k + 1) ** rng.uniform(0.2, 3)
        else:
            w = np.exp(-np.arange(k) * rng.uniform(0.01, 0.3))
        data = rng.choice(k, size=size, p=w / w.sum()).astype(np.uint8)
        if rng.random() < 0.5:
            data = rng.permutation(256)[data].astype(np.uint8)
        block = first_block(data.tobytes())
        if block["type"] == "dynamic" and unlimited_depth(block["clcounts"]) > 7:
            _found["row"] = (data.tobytes(), block)
            return _found["row"]
    return None


def row_pixels(row_bytes):
    """the row as a 1-row RGBA canvas (alpha 255)"""
    n = len(row_bytes) // 3
    px = np.full((1, n, 4), 255, np.uint8)
    px[0, :, :3] = np.frombuffer(row_bytes, np.uint8).reshape(n, 3)
    return px
