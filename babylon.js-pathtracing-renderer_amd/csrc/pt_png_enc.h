// pt_png_enc.h — what the host and the kernels of pt_canvas_encode_png share (pt_png_enc.hip, pt_capi.cpp): the PNG
// filters, deflate's length and distance code tables, the fixed trees, zlib's tree build with its tie-breaking and
// overflow repair, the block-size rule, the dynamic header's coding, an LSB-first bit packer, the CRC-32 table and
// its combination, the file's head and tail, and the kernels' argument block. Plain C++ over plain arrays, no HIP:
// the kernels call these functions, so a host program runs a whole chunk through them without a GPU
// (tests/test_png_enc_host.py). The format, stage by stage, is INTEGRATION.md "Encoding the canvas: PNG" and
// tests/png_enc_ref.py: every 16,320-byte chunk of the filtered stream is what zlib 1.2.11 writes for
// compressobj(6, DEFLATED, 15, 8, Z_RLE) fed that chunk and flushed with Z_FULL_FLUSH (Z_FINISH after the last).
//
// Out of scope: LZ77 matches beyond distance 1, 16-bit samples, palettes, interlace and ancillary chunks.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PTP_HD __host__ __device__
#else
#define PTP_HD
#endif

namespace ptp {

constexpr int kLanes = 64, kLaneBytes = 255;
constexpr int kChunk = kLanes * kLaneBytes;   // 16,320 filtered bytes: below zlib's 16,383 symbols, so one block
constexpr int kLCodes = 286, kDCodes = 30, kBlCodes = 19, kEndBlock = 256;
constexpr int kHeap = 2 * kLCodes + 1;
constexpr int kStored = 0, kFixed = 1, kDynamic = 2;   // BTYPE
constexpr int kMinMatch = 3, kMaxMatch = 258;
// what a chunk's payload adds to its filtered bytes at most: the zlib header (2), a stored block's header (5) and
// the empty stored block of a full flush (5), or the Adler-32 (4) in its place
constexpr int kChunkOverhead = 12;
constexpr size_t kHead = 33, kTail = 12;   // signature + IHDR; IEND

// ---- the filters (PNG specification 9.2 - 9.4) ----
PTP_HD inline int paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
// the filtered byte of x under `type` 0..4 with a the byte bpp to the left, b above, c above-left (0 outside)
PTP_HD inline uint8_t filter_byte(int type, int x, int a, int b, int c)
{
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (uint8_t)(x - pred);
}
// what the adaptive choice sums over a row: |byte as int8|
PTP_HD inline unsigned filter_cost(uint8_t f) { return f < 128 ? f : 256u - f; }

// ---- deflate's tables (RFC 1951 3.2.5; zlib trees.c extra_lbits, base_length, _length_code, bl_order) ----
PTP_HD inline int bit_width(unsigned a) { return a ? 32 - __builtin_clz(a) : 0; }
PTP_HD inline int extra_lbits(int code) { return code < 8 || code == 28 ? 0 : (code - 4) >> 2; }
PTP_HD inline int base_length(int code) { return code < 8 ? code : code == 28 ? 0 : (4 + (code & 3)) << extra_lbits(code); }
// the length code 0..28 of a match of lc + 3 bytes, lc 0..255
PTP_HD inline int length_code(int lc)
{
    if (lc < 8) return lc;
    if (lc == 255) return 28;
    const int extra = bit_width((unsigned)lc) - 3;
    return 4 * extra + 4 + ((lc >> extra) & 3);
}
PTP_HD inline int extra_dbits(int code) { return code < 2 ? 0 : (code >> 1) - 1; }
PTP_HD inline int extra_blbits(int code) { return code == 16 ? 2 : code == 17 ? 3 : code == 18 ? 7 : 0; }
PTP_HD inline int bl_order(int rank)
{
    static constexpr uint8_t t[kBlCodes] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
    return t[rank];
}
PTP_HD inline unsigned bit_reverse(unsigned code, int len)
{
    unsigned r = 0;
    for (int i = 0; i < len; i++, code >>= 1) r = r << 1 | (code & 1u);
    return r;
}
// the fixed trees (RFC 1951 3.2.6), codes as they go into the LSB-first stream
PTP_HD inline int static_llen(int n) { return n < 144 ? 8 : n < 256 ? 9 : n < 280 ? 7 : 8; }
PTP_HD inline unsigned static_lcode(int n)
{
    const int c = n < 144 ? 0x30 + n : n < 256 ? 0x190 + n - 144 : n < 280 ? n - 256 : 0xC0 + n - 280;
    return bit_reverse((unsigned)c, static_llen(n));
}
constexpr int kStaticDLen = 5;
PTP_HD inline unsigned static_dcode(int n) { return bit_reverse((unsigned)n, kStaticDLen); }

// ---- the trees (zlib trees.c build_tree, pqdownheap, gen_bitlen, gen_codes) ----
// One work area serves the three trees in turn: the nodes' frequencies, parents and lengths (leaves first, the
// internal nodes from `elems` up), zlib's heap (the priority queue from index 1, the nodes by frequency from the
// top down) and the subtree depths that break frequency ties.
struct TreeWork {
    uint16_t freq[kHeap], dad[kHeap], len[kHeap], heap[kHeap];
    uint8_t depth[kHeap];
};
constexpr int kTreeL = 0, kTreeD = 1, kTreeBl = 2;
PTP_HD inline int tree_max_length(int kind) { return kind == kTreeBl ? 7 : 15; }
PTP_HD inline int tree_extra(int kind, int n)
{
    return kind == kTreeL ? (n >= 257 ? extra_lbits(n - 257) : 0) : kind == kTreeD ? extra_dbits(n) : extra_blbits(n);
}
PTP_HD inline int tree_static_len(int kind, int n) { return kind == kTreeL ? static_llen(n) : kind == kTreeD ? kStaticDLen : 0; }

PTP_HD inline bool tree_smaller(const TreeWork& w, int n, int m)
{
    return w.freq[n] < w.freq[m] || (w.freq[n] == w.freq[m] && w.depth[n] <= w.depth[m]);
}
PTP_HD inline void tree_downheap(TreeWork& w, int heap_len, int k)
{
    const int v = w.heap[k];
    int j = k << 1;
    while (j <= heap_len) {
        if (j < heap_len && tree_smaller(w, w.heap[j + 1], w.heap[j])) j++;
        if (tree_smaller(w, v, w.heap[j])) break;
        w.heap[k] = w.heap[j];
        k = j;
        j <<= 1;
    }
    w.heap[k] = (uint16_t)v;
}
// The tree of `elems` counts: len[] and code[] by symbol (0 for an unused one), the largest used symbol returned,
// and the block's dynamic and fixed sizes in bits added to opt_len and static_len as zlib does (the wrap of the
// forced symbols' `opt_len--` included: the sums are taken modulo 2^32 and end small).
PTP_HD inline int build_tree(const uint16_t* freq, int elems, int kind, uint8_t* len, uint16_t* code, TreeWork& w,
                             uint32_t& opt_len, uint32_t& static_len)
{
    const int max_length = tree_max_length(kind);
    int heap_len = 0, heap_max = kHeap, max_code = -1;
    for (int n = 0; n < elems; n++) {
        w.freq[n] = freq[n];
        w.len[n] = 0;
        if (freq[n] != 0) {
            w.heap[++heap_len] = (uint16_t)(max_code = n);
            w.depth[n] = 0;
        }
    }
    while (heap_len < 2) {   // fewer than two used symbols: codes are forced into the tree
        const int node = max_code < 2 ? ++max_code : 0;
        w.heap[++heap_len] = (uint16_t)node;
        w.freq[node] = 1;
        w.depth[node] = 0;
        opt_len--;
        if (kind != kTreeBl) static_len -= (uint32_t)tree_static_len(kind, node);
    }
    for (int n = heap_len / 2; n >= 1; n--) tree_downheap(w, heap_len, n);
    int node = elems;
    do {
        const int n = w.heap[1];
        w.heap[1] = w.heap[heap_len--];
        tree_downheap(w, heap_len, 1);
        const int m = w.heap[1];
        w.heap[--heap_max] = (uint16_t)n;
        w.heap[--heap_max] = (uint16_t)m;
        w.freq[node] = (uint16_t)(w.freq[n] + w.freq[m]);
        w.depth[node] = (uint8_t)((w.depth[n] >= w.depth[m] ? w.depth[n] : w.depth[m]) + 1);
        w.dad[n] = w.dad[m] = (uint16_t)node;
        w.heap[1] = (uint16_t)node++;
        tree_downheap(w, heap_len, 1);
    } while (heap_len >= 2);
    w.heap[--heap_max] = w.heap[1];

    // gen_bitlen: lengths from the top down, clamped to max_length, and the repair of what the clamp broke
    uint16_t bl_count[16] = { 0 };
    int overflow = 0, h;
    w.len[w.heap[heap_max]] = 0;
    for (h = heap_max + 1; h < kHeap; h++) {
        const int n = w.heap[h];
        int bits = w.len[w.dad[n]] + 1;
        if (bits > max_length) { bits = max_length; overflow++; }
        w.len[n] = (uint16_t)bits;
        if (n > max_code) continue;   // not a leaf
        bl_count[bits]++;
        const uint32_t f = w.freq[n];
        opt_len += f * (uint32_t)(bits + tree_extra(kind, n));
        if (kind != kTreeBl) static_len += f * (uint32_t)(tree_static_len(kind, n) + tree_extra(kind, n));
    }
    if (overflow > 0) {
        do {
            int bits = max_length - 1;
            while (bl_count[bits] == 0) bits--;
            bl_count[bits]--;
            bl_count[bits + 1] = (uint16_t)(bl_count[bits + 1] + 2);
            bl_count[max_length]--;
            overflow -= 2;
        } while (overflow > 0);
        for (int bits = max_length; bits != 0; bits--) {
            int n = bl_count[bits];
            while (n != 0) {
                const int m = w.heap[--h];
                if (m > max_code) continue;
                if (w.len[m] != bits) {
                    opt_len += ((uint32_t)bits - w.len[m]) * w.freq[m];
                    w.len[m] = (uint16_t)bits;
                }
                n--;
            }
        }
    }
    // gen_codes
    uint16_t next_code[16];
    unsigned c = 0;
    next_code[0] = 0;
    for (int bits = 1; bits <= 15; bits++) {
        c = (c + bl_count[bits - 1]) << 1;
        next_code[bits] = (uint16_t)c;
    }
    for (int n = 0; n < elems; n++) {
        const int l = n <= max_code ? w.len[n] : 0;
        len[n] = (uint8_t)l;
        code[n] = l ? (uint16_t)bit_reverse(next_code[l]++, l) : (uint16_t)0;
    }
    return max_code;
}

// ---- a block: counts in, the three trees, the block type and the header out ----
struct Block {
    uint16_t lfreq[kLCodes], dfreq[kDCodes], blfreq[kBlCodes];
    uint16_t lcode[kLCodes], dcode[kDCodes], blcode[kBlCodes];
    uint8_t llen[kLCodes], dlen[kDCodes], bllen[kBlCodes];
    int lmax, dmax, blmax, type;
    uint32_t opt_len, static_len;   // bits of the dynamic and of the fixed form, without the 3 header bits
    TreeWork w;
};

// Runs of equal code lengths as the symbols 16, 17, 18 (scan_tree / send_tree): emit(symbol, extra value, extra
// bits) for every code-length symbol of the lengths len[0..max_code], zlib's guard behind the last one.
template <class Emit> PTP_HD inline void walk_tree(const uint8_t* len, int max_code, Emit&& emit)
{
    int prevlen = -1, nextlen = len[0], count = 0, max_count = 7, min_count = 4;
    if (nextlen == 0) { max_count = 138; min_count = 3; }
    for (int n = 0; n <= max_code; n++) {
        const int curlen = nextlen;
        nextlen = n + 1 <= max_code ? len[n + 1] : 0xffff;
        if (++count < max_count && curlen == nextlen) continue;
        if (count < min_count) {
            do emit(curlen, 0, 0); while (--count != 0);
        } else if (curlen != 0) {
            if (curlen != prevlen) { emit(curlen, 0, 0); count--; }
            emit(16, count - 3, 2);
        } else if (count <= 10) {
            emit(17, count - 3, 3);
        } else {
            emit(18, count - 11, 7);
        }
        count = 0;
        prevlen = curlen;
        if (nextlen == 0) { max_count = 138; min_count = 3; }
        else if (curlen == nextlen) { max_count = 6; min_count = 3; }
        else { max_count = 7; min_count = 4; }
    }
}

// From the counts in lfreq and dfreq (the end-of-block symbol is counted here): the trees, the sizes and the block
// type by zlib's rule (_tr_flush_block at level 6). A fixed block leaves the fixed trees in llen / lcode / dlen /
// dcode, so the tokens are coded alike in either case.
PTP_HD inline void plan_block(Block& b, unsigned stored_len)
{
    b.lfreq[kEndBlock] = 1;
    uint32_t opt = 0, stat = 0;
    b.lmax = build_tree(b.lfreq, kLCodes, kTreeL, b.llen, b.lcode, b.w, opt, stat);
    b.dmax = build_tree(b.dfreq, kDCodes, kTreeD, b.dlen, b.dcode, b.w, opt, stat);
    for (int i = 0; i < kBlCodes; i++) b.blfreq[i] = 0;
    auto count = [&](int sym, int, int) { b.blfreq[sym]++; };
    walk_tree(b.llen, b.lmax, count);
    walk_tree(b.dlen, b.dmax, count);
    build_tree(b.blfreq, kBlCodes, kTreeBl, b.bllen, b.blcode, b.w, opt, stat);
    for (b.blmax = kBlCodes - 1; b.blmax >= 3; b.blmax--)
        if (b.bllen[bl_order(b.blmax)] != 0) break;
    opt += 3u * ((uint32_t)b.blmax + 1u) + 5u + 5u + 4u;
    b.opt_len = opt;
    b.static_len = stat;
    uint32_t opt_lenb = (opt + 3 + 7) >> 3;
    const uint32_t static_lenb = (stat + 3 + 7) >> 3;
    if (static_lenb <= opt_lenb) opt_lenb = static_lenb;
    if (stored_len + 4 <= opt_lenb) {
        b.type = kStored;
    } else if (static_lenb == opt_lenb) {
        b.type = kFixed;
        for (int n = 0; n < kLCodes; n++) { b.llen[n] = (uint8_t)static_llen(n); b.lcode[n] = (uint16_t)static_lcode(n); }
        for (int n = 0; n < kDCodes; n++) { b.dlen[n] = kStaticDLen; b.dcode[n] = (uint16_t)static_dcode(n); }
    } else {
        b.type = kDynamic;
    }
}

// The header of a fixed or dynamic block through put(value, bits): BFINAL and BTYPE, and for a dynamic block
// HLIT, HDIST, HCLEN, the code-length code lengths in bl_order and the two trees' lengths (send_all_trees).
template <class Put> PTP_HD inline void block_header(const Block& b, int last, Put&& put)
{
    put((unsigned)(b.type << 1 | last), 3);
    if (b.type != kDynamic) return;
    put((unsigned)(b.lmax + 1 - 257), 5);
    put((unsigned)(b.dmax + 1 - 1), 5);
    put((unsigned)(b.blmax + 1 - 4), 4);
    for (int rank = 0; rank <= b.blmax; rank++) put(b.bllen[bl_order(rank)], 3);
    auto send = [&](int sym, int extra, int bits) {
        put(b.blcode[sym], b.bllen[sym]);
        if (bits) put((unsigned)extra, bits);
    };
    walk_tree(b.llen, b.lmax, send);
    walk_tree(b.dlen, b.dmax, send);
}

// ---- tokens (zlib deflate_rle: matches of distance 1 only) ----
// The byte at i of a chunk lies in the maximal run [s, e) of equal bytes. The run's first byte is a literal; the
// other e - s - 1 are taken greedily as matches of min(258, rest) bytes while rest >= 3, and what is left over is
// literals. Returns 0 when no token starts at i, 1 for a literal, otherwise the length of the match that starts here.
PTP_HD inline int token_at(unsigned i, unsigned s, unsigned e)
{
    const unsigned p = i - s;
    if (p == 0) return 1;
    const unsigned q = (p - 1) / kMaxMatch, o = (p - 1) % kMaxMatch, rest = e - s - 1 - kMaxMatch * q;
    if (rest < (unsigned)kMinMatch) return 1;
    return o ? 0 : (int)(rest < (unsigned)kMaxMatch ? rest : (unsigned)kMaxMatch);
}
// the literal / length symbol a token counts under
PTP_HD inline int token_symbol(int tok, uint8_t byte) { return tok == 1 ? byte : 257 + length_code(tok - kMinMatch); }
// a token's bits, right-aligned and LSB-first, `n` of them (at most 15 + 5 + 15)
PTP_HD inline unsigned long long token_bits(const Block& b, int tok, uint8_t byte, int& n)
{
    if (tok == 1) {
        n = b.llen[byte];
        return b.lcode[byte];
    }
    const int lc = tok - kMinMatch, c = length_code(lc), sym = 257 + c, extra = extra_lbits(c);
    unsigned long long v = b.lcode[sym];
    n = b.llen[sym];
    if (extra) {
        v |= (unsigned long long)(lc - base_length(c)) << n;
        n += extra;
    }
    v |= (unsigned long long)b.dcode[0] << n;   // distance 1: code 0, no extra bits
    n += b.dlen[0];
    return v;
}

// The LSB-first sibling of ptj::lane_window: `len` (1..64) right-aligned bits that start at bit `at` of a buffer of
// little-endian 32-bit words, as the words at at >> 5 and after with the bits in place and zeros elsewhere.
PTP_HD inline void lsb_window(unsigned long long bits, int len, unsigned long long at, uint32_t w[3])
{
    if (len < 64) bits &= (1ull << len) - 1ull;
    const unsigned sh = (unsigned)(at & 31u);
    const unsigned long long lo = bits << sh, hi = sh ? bits >> (64 - sh) : 0ull;
    w[0] = (uint32_t)lo;
    w[1] = (uint32_t)(lo >> 32);
    w[2] = (uint32_t)hi;
}

// ---- CRC-32 (PNG specification annex D) and Adler-32 ----
struct CrcTable {
    uint32_t t[256];
};
constexpr CrcTable make_crc_table()
{
    CrcTable c = {};
    for (uint32_t n = 0; n < 256; n++) {
        uint32_t v = n;
        for (int k = 0; k < 8; k++) v = v & 1u ? 0xEDB88320u ^ (v >> 1) : v >> 1;
        c.t[n] = v;
    }
    return c;
}
static_assert(make_crc_table().t[1] == 0x77073096u && make_crc_table().t[255] == 0x2D02EF8Du, "annex D");
// the running (inverted) register after one more byte; a CRC is ~ of the register started at ~0
PTP_HD inline uint32_t crc_step(uint32_t reg, uint8_t byte)
{
    static constexpr CrcTable T = make_crc_table();
    return T.t[(reg ^ byte) & 255u] ^ (reg >> 8);
}
PTP_HD inline uint32_t crc_bytes(const uint8_t* p, size_t n)
{
    uint32_t reg = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) reg = crc_step(reg, p[i]);
    return ~reg;
}
// a(x) b(x) modulo the CRC polynomial, bit-reflected (bit 31 is x^0)
PTP_HD inline uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = b & 1u ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
// x^(8 n) modulo the polynomial
PTP_HD inline uint32_t crc_shift(unsigned long long n)
{
    uint32_t p = 1u << 31, sq = 1u << 23;   // x^0, x^8
    for (; n; n >>= 1) {
        if (n & 1ull) p = crc_mul(sq, p);
        sq = crc_mul(sq, sq);
    }
    return p;
}
// the CRC of A followed by B from the CRCs of A and of B and B's length; by linearity the CRC of pieces P0 .. Pk is
// the XOR of crc_mul(crc_shift(bytes after Pi), crc(Pi)), which is how a wave combines its lanes' pieces
PTP_HD inline uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, unsigned long long len_b)
{
    return crc_mul(crc_shift(len_b), crc_a) ^ crc_b;
}
constexpr uint32_t kAdlerBase = 65521;

// ---- the file's head and tail ----
inline void put_be32(uint8_t* p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}
// the signature and IHDR (8 bits per sample, colour type 2 or 6 for colour 0 or 1, no interlace): kHead bytes
inline size_t write_png_head(uint8_t* dst, int width, int height, int colour)
{
    static const uint8_t sig[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
    for (int i = 0; i < 8; i++) dst[i] = sig[i];
    uint8_t* p = dst + 8;
    put_be32(p, 13);
    p[4] = 'I'; p[5] = 'H'; p[6] = 'D'; p[7] = 'R';
    put_be32(p + 8, (uint32_t)width);
    put_be32(p + 12, (uint32_t)height);
    p[16] = 8; p[17] = (uint8_t)(colour ? 6 : 2); p[18] = 0; p[19] = 0; p[20] = 0;
    put_be32(p + 21, crc_bytes(p + 4, 17));
    return kHead;
}
// IEND: kTail bytes
inline size_t write_png_tail(uint8_t* dst)
{
    put_be32(dst, 0);
    dst[4] = 'I'; dst[5] = 'E'; dst[6] = 'N'; dst[7] = 'D';
    put_be32(dst + 8, crc_bytes(dst + 4, 4));
    return kTail;
}

// ---- a whole chunk on the host (what pt_png_chunk does a lane per 255 bytes) ----
// The payload of the IDAT of chunk `in[0..n)`, n 1..kChunk, into `words` (zeroed, (n + kChunkOverhead + 11) / 4 words
// at least): the zlib header before the first chunk's block, the block, and the empty stored block of the full
// flush unless the chunk is the last, whose Adler-32 the caller appends. Returns the bytes written.
inline size_t deflate_chunk(const uint8_t* in, unsigned n, bool first, bool last, Block& b, uint32_t* words)
{
    for (int i = 0; i < kLCodes; i++) b.lfreq[i] = 0;
    for (int i = 0; i < kDCodes; i++) b.dfreq[i] = 0;
    auto tokens = [&](auto&& visit) {
        unsigned s = 0, e = 0;
        for (unsigned i = 0; i < n; i++) {
            if (i == e) {
                s = i;
                for (e = i + 1; e < n && in[e] == in[s]; e++) {}
            }
            const int tok = token_at(i, s, e);
            if (tok) visit(tok, in[i]);
        }
    };
    tokens([&](int tok, uint8_t byte) {
        b.lfreq[token_symbol(tok, byte)]++;
        if (tok != 1) b.dfreq[0]++;
    });
    plan_block(b, n);
    uint8_t* bytes = (uint8_t*)words;
    unsigned long long at = 0;
    auto put = [&](unsigned long long v, int len) {
        uint32_t w[3];
        lsb_window(v, len, at, w);
        for (int k = 0; k < 3; k++)
            if (w[k]) words[(at >> 5) + k] |= w[k];
        at += (unsigned)len;
    };
    if (first) { put(0x78, 8); put(0x01, 8); }
    if (b.type == kStored) {
        put(last ? 1u : 0u, 8);
        put(n & 0xFFFFu, 16);
        put(~n & 0xFFFFu, 16);
        for (unsigned i = 0; i < n; i++) bytes[(at >> 3) + i] = in[i];
        at += 8ull * n;
    } else {
        block_header(b, last ? 1 : 0, put);
        tokens([&](int tok, uint8_t byte) {
            int len;
            const unsigned long long v = token_bits(b, tok, byte, len);
            put(v, len);
        });
        put(b.lcode[kEndBlock], b.llen[kEndBlock]);
    }
    if (!last) put(0, 3);   // the full flush: an empty stored block, 00 00 FF FF behind the padding
    at = (at + 7) & ~7ull;
    if (!last) { put(0x0000, 16); put(0xFFFF, 16); }
    return (size_t)(at >> 3);
}

// ---- the kernels' arguments: the canvas (RGBA8, rows bottom-up) and the workspace arrays of pt::PngLayout ----
struct PngArgs {
    const uint32_t* canvas;
    int width, height;
    int bpp;                       // 3 (PT_PNG_RGB) or 4 (PT_PNG_RGBA)
    int filter;                    // 0..4 fixed, 5 adaptive
    unsigned long long row_bytes;  // bpp * width
    unsigned long long stream;     // height * (1 + row_bytes): the filtered stream's bytes
    unsigned long long chunks;     // ceil(stream / kChunk)
    size_t slot;                   // bytes of a chunk's slot in `slots`
    uint8_t* filtered;
    uint8_t* slots;
    uint32_t* meta;                // [chunks][4]: payload bytes, the IDAT's CRC, the Adler sums A and B mod 65521
    unsigned long long* off;       // [chunks] where the chunk's IDAT starts behind the head
    unsigned long long* total;     // the IDATs' bytes in all
    uint8_t* out;
};

}  // namespace ptp
