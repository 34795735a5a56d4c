// pt_jpeg_enc.h — what the host and the kernels of pt_canvas_encode_jpeg share (pt_jpeg_enc.hip, pt_capi.cpp): the
// Annex K tables of ITU-T T.81, the quantisation tables of a quality as libjpeg scales them, the Huffman codes
// derived from the tables at compile time, the file header, a lane's symbols and bits under tables built for the
// frame (optimised coding), and the kernels' argument block. Plain C++ over plain numbers, no HIP. The format, stage
// by stage, is INTEGRATION.md "Encoding the canvas" and tests/jpeg_enc_ref.py, jpeg_enc_sub_ref.py, jpeg_enc_opt_ref.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ptj {

constexpr uint8_t kZigzag[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
    62, 63 };

// K.1, K.2: luminance and chrominance, natural order
constexpr uint8_t kQBase[2][64] = {
    { 16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 },
    { 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
      47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 } };

// K.3 - K.6: codes per length 1..16, then the symbols in code order ([0] luminance, [1] chrominance)
constexpr uint8_t kDcBits[2][16] = { { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 },
                                     { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 } };
constexpr uint8_t kDcVals[12] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 };
constexpr uint8_t kAcBits[2][16] = { { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d },
                                     { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77 } };
constexpr uint8_t kAcVals[2][162] = {
    { 0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
      0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
      0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
      0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
      0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa },
    { 0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
      0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
      0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
      0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
      0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
      0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
      0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa } };

// The canonical codes (Annex C) by symbol, code | length << 16; 0 for a symbol the table does not have.
// dc[t][category 0..11], ac[t][run << 4 | category]: 0x00 is EOB, 0xF0 is ZRL.
struct HuffCodes {
    uint32_t dc[2][12];
    uint32_t ac[2][256];
};
constexpr HuffCodes make_codes()
{
    HuffCodes h = {};
    for (int t = 0; t < 2; t++) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; len++, code <<= 1)
            for (int i = 0; i < kDcBits[t][len - 1]; i++) h.dc[t][kDcVals[k++]] = code++ | (uint32_t)len << 16;
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; len++, code <<= 1)
            for (int i = 0; i < kAcBits[t][len - 1]; i++) h.ac[t][kAcVals[t][k++]] = code++ | (uint32_t)len << 16;
    }
    return h;
}

// the tables of `quality` 1..100 (jpeg_quality_scaling, baseline: entries 1..255), in zigzag order as DQT and
// the kernels' lanes take them; [0] luminance, [1] chrominance
struct QuantTables {
    uint16_t q[2][64];
};
inline QuantTables quant_tables(int quality)
{
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    QuantTables t;
    for (int i = 0; i < 2; i++)
        for (int k = 0; k < 64; k++) {
            const int v = (kQBase[i][kZigzag[k]] * s + 50) / 100;
            t.q[i][k] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
    return t;
}

// The four Huffman tables of a file coded with tables of its own (pt_canvas_encode_jpeg_opt with optimize = 1), as
// DHT carries them, in the header's order DC 0, AC 0, DC 1, AC 1: codes per length 1..16, then the symbols by length
// and value (sum of bits[t] of them). pt_jpeg_build_tables writes it, the host reads it back.
struct OptTables {
    uint8_t bits[4][16];
    uint8_t vals[4][256];
};
// the symbols of table t, or -1 where it is no table of this encoder (more than 256 symbols; a DC category past 11)
inline int opt_table_symbols(const OptTables& o, int t)
{
    int n = 0;
    for (int k = 0; k < 16; k++) n += o.bits[t][k];
    if (n > 256) return -1;
    if (!(t & 1))
        for (int i = 0; i < n; i++)
            if (o.vals[t][i] > 11) return -1;
    return n;
}

// SOI, APP0 (JFIF 1.1, no density unit, 1x1), DQT 0 and 1, SOF0 (8-bit, three components, Y sampled hs x vs and
// Cb, Cr 1x1, tables 0 1 1), DHT DC0 AC0 DC1 AC1, DRI (one MCU row of 8 hs pixel wide MCUs), SOS: the bytes before
// the entropy-coded data. Returns their count, which is pt::kJpegHeader for every size, quality and sampling with
// the Annex K tables (o == nullptr); with the tables of `o` the DHT segments carry those and the count varies.
inline size_t write_header_tables(uint8_t* dst, int width, int height, const QuantTables& qt, int hs, int vs,
                                  const OptTables* o)
{
    uint8_t* p = dst;
    auto put = [&](int b) { *p++ = (uint8_t)b; };
    auto put16 = [&](int v) { put(v >> 8); put(v & 255); };
    auto seg = [&](int marker, int body) { put(0xFF); put(marker); put16(body + 2); };
    put(0xFF); put(0xD8);
    seg(0xE0, 14);
    for (char ch : { 'J', 'F', 'I', 'F', '\0' }) put(ch);
    put(1); put(1); put(0); put16(1); put16(1); put(0); put(0);
    for (int i = 0; i < 2; i++) {
        seg(0xDB, 65);
        put(i);
        for (int k = 0; k < 64; k++) put(qt.q[i][k]);
    }
    seg(0xC0, 15);
    put(8); put16(height); put16(width); put(3);
    for (int c = 0; c < 3; c++) { put(c + 1); put(c ? 0x11 : hs << 4 | vs); put(c ? 1 : 0); }
    for (int t = 0; o && t < 4; t++) {
        const int syms = opt_table_symbols(*o, t);
        seg(0xC4, 1 + 16 + syms);
        put((t & 1) << 4 | t >> 1);
        for (int k = 0; k < 16; k++) put(o->bits[t][k]);
        for (int k = 0; k < syms; k++) put(o->vals[t][k]);
    }
    for (int i = 0; !o && i < 2; i++) {
        seg(0xC4, 1 + 16 + 12);
        put(0x00 | i);
        for (int k = 0; k < 16; k++) put(kDcBits[i][k]);
        for (int k = 0; k < 12; k++) put(kDcVals[k]);
        seg(0xC4, 1 + 16 + 162);
        put(0x10 | i);
        for (int k = 0; k < 16; k++) put(kAcBits[i][k]);
        for (int k = 0; k < 162; k++) put(kAcVals[i][k]);
    }
    seg(0xDD, 2);
    put16((width + 8 * hs - 1) / (8 * hs));
    seg(0xDA, 10);
    put(3); put(1); put(0x00); put(2); put(0x11); put(3); put(0x11); put(0); put(63); put(0);
    return (size_t)(p - dst);
}
inline size_t write_header(uint8_t* dst, int width, int height, const QuantTables& qt, int hs = 1, int vs = 1)
{
    return write_header_tables(dst, width, height, qt, hs, vs, nullptr);
}

// ---- optimised Huffman tables (pt_canvas_encode_jpeg_opt with optimize = 1; tests/jpeg_enc_opt_ref.py) ----
#if defined(__HIPCC__)
#define PTJ_HD __host__ __device__
#else
#define PTJ_HD
#endif

PTJ_HD inline int bit_width(unsigned a) { return a ? 32 - __builtin_clz(a) : 0; }

// Lane k's symbols of a block (libjpeg's htest_one_block, a coefficient a lane): v the lane's coefficient, prev_dc
// the DC the block is predicted from, `nonzero` the mask of lanes holding a non-zero coefficient. sym: the DC
// category for k = 0, (run & 15) << 4 | size for a non-zero AC after `run` zeros, 0x00 (EOB) for lane 63 holding a
// zero, -1 for no symbol; zrls: the run >> 4 ZRL symbols (0xF0) before an AC's own; n, val: the value bits.
struct LaneSyms {
    int sym, zrls, n;
    uint32_t val;
};
PTJ_HD inline LaneSyms lane_symbols(int k, int v, int prev_dc, unsigned long long nonzero)
{
    LaneSyms s = { -1, 0, 0, 0 };
    if (k == 0) {
        const int d = v - prev_dc;
        s.n = bit_width((unsigned)(d < 0 ? -d : d));
        s.sym = s.n;
        s.val = (uint32_t)(d < 0 ? d - 1 : d) & ((1u << s.n) - 1u);
    } else if (v != 0) {
        const unsigned long long below = nonzero & ((1ull << k) - 1ull) & ~1ull;
        const int run = k - 1 - (below ? 63 - __builtin_clzll(below) : 0);
        s.n = bit_width((unsigned)(v < 0 ? -v : v));
        s.zrls = run >> 4;
        s.sym = (run & 15) << 4 | s.n;
        s.val = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s.n) - 1u);
    } else if (k == 63) {
        s.sym = 0x00;
    }
    return s;
}

// A lane's share of a block's bits under tables of any code lengths up to 16: the ZRLs (at most 3 x 16 bits) apart
// from the code and value (at most 16 + 11), each right-aligned; 74 bits in all at most, which no 64-bit word holds.
struct LaneBits {
    unsigned long long zrl;
    uint32_t code;
    int zrl_len, code_len;
};
PTJ_HD inline LaneBits lane_bits(const LaneSyms& s, const uint32_t* table, uint32_t zrl)
{
    LaneBits b = { 0, 0, 0, 0 };
    if (s.sym < 0) return b;
    for (int i = 0; i < s.zrls; i++) {
        b.zrl = b.zrl << (zrl >> 16) | (zrl & 0xFFFFu);
        b.zrl_len += (int)(zrl >> 16);
    }
    const uint32_t e = table[s.sym];
    b.code = (e & 0xFFFFu) << s.n | s.val;
    b.code_len = (int)(e >> 16) + s.n;
    return b;
}
// ... and where it goes: the share starts at bit `at` of a buffer that is MSB-first in 32-bit words; w[0..3] are
// the words at at >> 5 and after with the share's bits in place and zeros elsewhere (31 + 74 bits <= 4 words)
PTJ_HD inline void lane_window(const LaneBits& b, unsigned at, uint32_t w[4])
{
    unsigned long long hi = 0, lo = 0;   // the window's first and second 64 bits
    auto place = [&](unsigned long long bits, int len, unsigned pos) {   // len 1..64 right-aligned bits to bit pos < 96
        const unsigned long long left = bits << (64 - len);
        if (pos < 64) {
            hi |= left >> pos;
            if (pos) lo |= left << (64 - pos);
        } else {
            lo |= left >> (pos - 64);
        }
    };
    const unsigned sh = at & 31;
    if (b.zrl_len) place(b.zrl, b.zrl_len, sh);
    if (b.code_len) place(b.code, b.code_len, sh + (unsigned)b.zrl_len);
    w[0] = (uint32_t)(hi >> 32); w[1] = (uint32_t)hi;
    w[2] = (uint32_t)(lo >> 32); w[3] = (uint32_t)lo;
}

// The header with the four DHT segments carrying `o` instead of Annex K: the same segments in the same order, its
// length what the tables' symbols make it (at most kOptHeaderMax). Every table of `o` must pass opt_table_symbols.
constexpr size_t kOptHeaderMax = 629 - 2 * (12 + 162) + 4 * 256;
inline size_t write_header(uint8_t* dst, int width, int height, const QuantTables& qt, int hs, int vs, const OptTables& o)
{
    return write_header_tables(dst, width, height, qt, hs, vs, &o);
}

// Y's sampling factors (Cb and Cr are 1 x 1) of a pt_jpeg_subsampling value 0..2: 4:4:4, 4:2:2, 4:2:0
inline int sampling_h(int subsampling) { return subsampling ? 2 : 1; }
inline int sampling_v(int subsampling) { return subsampling == 2 ? 2 : 1; }

// the kernels' arguments: the canvas (RGBA8, rows bottom-up), Y's sampling (an MCU is 8 hs x 8 vs pixels and
// hs vs + 2 blocks), the workspace arrays of pt::JpegLayout, and (for the last kernel) the stream buffer
struct EncArgs {
    const uint32_t* canvas;
    int width, height;
    int hs, vs;
    unsigned mcus_x, rows, blocks_row, tiles;
    size_t row_stride;             // bytes of `bits` per row
    int16_t* coef;
    uint32_t* bitoff;
    uint32_t* bits;
    uint32_t* tileoff;
    uint32_t* rowbits;
    uint32_t* rowlen;
    unsigned long long* rowoff;
    unsigned long long* total;
    uint8_t* out;
    QuantTables qt;
    // optimised tables only (pt::JpegOptLayout; all nullptr with the Annex K tables)
    unsigned long long* hist;      // [4][256] symbol counts: DC 0, AC 0, DC 1, AC 1
    HuffCodes* codes;              // the codes pt_jpeg_build_tables derives
    OptTables* tables;             // ... and the tables for the header, behind `total`
};

// pt_jpeg_ship's arguments (an encode job: pt_canvas_encode_jpeg_begin): the stream pt_jpeg_pack assembled in the
// job's device slot, the length and tables the length pass left, and where they go in the job's pinned host buffer
// (pt::JobLayout). `room` bytes of the stream at most are copied; both stream buffers are 16-byte aligned.
struct ShipArgs {
    const uint8_t* stream;
    const unsigned long long* total;
    const OptTables* tables;       // nullptr with the Annex K tables
    size_t room;
    uint8_t* host_stream;
    unsigned long long* host_total;
    OptTables* host_tables;
};

}  // namespace ptj
