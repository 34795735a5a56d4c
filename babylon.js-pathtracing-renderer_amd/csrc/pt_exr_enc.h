// pt_exr_enc.h — what the host and the kernels of pt_targets_encode_exr share (pt_exr_enc.hip, pt_capi.cpp): the
// sample conversion (binary32 to binary16 in integers only, so that no rounding or denormal mode can matter), where
// a sample lies in a block's raw bytes, the byte reorder and delta predictor of OpenEXR's ZIP, the combination of
// the pieces' Adler sums, the stream-or-raw rule, the header's writer and the kernels' argument block. Plain C++
// over plain arrays, no HIP: a host program runs whole blocks through them without a GPU
// (tests/test_exr_enc_host.py), with pt_png_enc.h's deflate_chunk for the pieces. The format is include/pt.h
// pt_targets_encode_exr and tests/exr_enc_ref.py: a single-part scanline OpenEXR file whose ZIP / ZIPS blocks are
// zlib streams cut like pt_canvas_encode_png's, a deflate block per 16,320-byte piece.
//
// Out of scope: tiles, multi-part and deep files, the other compressions, UINT and subsampled channels, long names.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "pt_png_enc.h"

namespace pte {

constexpr int kHalf = 1, kFloat = 2;             // OpenEXR's pixel types (PT_EXR_HALF, PT_EXR_FLOAT)
constexpr int kNone = 0, kZips = 2, kZip = 3;    // OpenEXR's compressions
constexpr int kChannelsMax = 16, kNameMax = 31;
constexpr int kPiece = ptp::kChunk;              // a deflate block's bytes
constexpr size_t kHeaderMax = 277 - 18 + kChannelsMax * (kNameMax + 17);

PTP_HD inline int lines_of(int compression) { return compression == kZip ? 16 : 1; }
PTP_HD inline int sample_bytes(int type) { return type == kHalf ? 2 : 4; }

// binary32 bits to binary16 bits, round to nearest even: subnormal halves are produced, what rounds past 65504 is
// +-inf, +-0 is kept, every NaN is 0x7E00
PTP_HD inline uint16_t half_bits(uint32_t f)
{
    const uint32_t sign = f >> 16 & 0x8000u, a = f & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return 0x7E00;
    if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);   // 65520, the midpoint to 2^16, and above
    if (a >= 0x38800000u) {                                      // a normal half: 2^-14 and above
        const uint32_t r = a - 0x38000000u;
        return (uint16_t)(sign | (r + 0xFFFu + (r >> 13 & 1u)) >> 13);   // (a carry into the exponent is the next half)
    }
    const uint32_t e = a >> 23;
    if (e < 102u) return (uint16_t)sign;                         // below 2^-25, float denormals included
    const uint32_t m = (a & 0x7FFFFFu) | 0x800000u, shift = 126u - e;   // in units of 2^-24: m >> shift, shift 14..24
    uint32_t q = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), mid = 1u << (shift - 1u);
    if (rem > mid || (rem == mid && (q & 1u))) q++;
    return (uint16_t)(sign | q);
}

PTP_HD inline uint32_t float_bits(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(v);
#else
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
#endif
}
PTP_HD inline float bits_float(uint32_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float v;
    memcpy(&v, &u, 4);
    return v;
#endif
}
// The stored bits of texel component x under scale: v = x * scale, one binary32 multiply (a scale of exactly 1
// takes x's bits untouched, payloads included). FLOAT stores v's bits, a NaN the multiply made or passed on as
// 0x7FC00000; HALF stores half_bits(v) in the low 16 bits.
PTP_HD inline uint32_t sample_bits(uint32_t x, float scale, int type)
{
    uint32_t v = x;
    if (scale != 1.0f) {
        v = float_bits(bits_float(x) * scale);
        if ((v & 0x7FFFFFFFu) > 0x7F800000u) v = 0x7FC00000u;
    }
    return type == kHalf ? half_bits(v) : v;
}

// byte i of the predicted block p from the raw block r[0..n), n even: the even bytes before the odd ones, then
// every byte but the first as its difference to the one before it plus 128
PTP_HD inline uint8_t reordered(const uint8_t* r, unsigned long long n, unsigned long long i)
{
    const unsigned long long h = n >> 1;
    return i < h ? r[2 * i] : r[2 * (i - h) + 1];
}
PTP_HD inline uint8_t predicted(const uint8_t* r, unsigned long long n, unsigned long long i)
{
    const uint8_t t = reordered(r, n, i);
    return i ? (uint8_t)(t - reordered(r, n, i - 1) + 128) : t;
}

// Adler-32 over pieces: a piece's sums are A = the bytes' sum and B = the sum of (bytes - i) x byte i, both mod
// 65521; `a` and `b` are the running checksum halves, which start at 1 and 0
PTP_HD inline void adler_piece(uint32_t& a, uint32_t& b, uint32_t piece_a, uint32_t piece_b, uint32_t bytes)
{
    b = (uint32_t)((b + piece_b + (unsigned long long)bytes * a) % ptp::kAdlerBase);
    a = (a + piece_a) % ptp::kAdlerBase;
}
// OpenEXR's rule: the stream when it is shorter than the block's n raw bytes, otherwise the raw bytes
PTP_HD inline bool keeps_stream(unsigned long long stream, unsigned long long n) { return stream < n; }

// ---- the header (host) ----
struct HeaderChan {
    char name[kNameMax + 1];
    int type;
};
inline bool name_ok(const char* s)
{
    if (!s) return false;
    size_t n = 0;
    for (; s[n]; n++)
        if (n >= (size_t)kNameMax || (unsigned char)s[n] < 0x21 || (unsigned char)s[n] > 0x7E) return false;
    return n >= 1;
}
inline void put_le32(uint8_t* p, uint32_t v)
{
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}
inline size_t header_bytes(const HeaderChan* ch, int n)
{
    size_t b = 277 - 18;
    for (int i = 0; i < n; i++) b += strlen(ch[i].name) + 17;
    return b;
}
// the magic, the version and the header of `n` channels sorted by name into dst (kHeaderMax bytes at most)
inline size_t write_header(uint8_t* dst, const HeaderChan* ch, int n, int width, int height, int compression)
{
    uint8_t* p = dst;
    auto str = [&](const char* s) { const size_t l = strlen(s) + 1; memcpy(p, s, l); p += l; };
    auto i32 = [&](uint32_t v) { put_le32(p, v); p += 4; };
    auto attr = [&](const char* name, const char* type, uint32_t size) { str(name); str(type); i32(size); };
    static const uint8_t magic[8] = { 0x76, 0x2F, 0x31, 0x01, 2, 0, 0, 0 };
    memcpy(p, magic, 8); p += 8;
    uint32_t chlist = 1;
    for (int i = 0; i < n; i++) chlist += (uint32_t)strlen(ch[i].name) + 17;
    attr("channels", "chlist", chlist);
    for (int i = 0; i < n; i++) {
        str(ch[i].name);
        i32((uint32_t)ch[i].type); i32(0); i32(1); i32(1);   // type, pLinear and 3 reserved bytes, x and y sampling
    }
    *p++ = 0;
    attr("compression", "compression", 1); *p++ = (uint8_t)compression;
    for (int k = 0; k < 2; k++) {
        attr(k ? "displayWindow" : "dataWindow", "box2i", 16);
        i32(0); i32(0); i32((uint32_t)(width - 1)); i32((uint32_t)(height - 1));
    }
    attr("lineOrder", "lineOrder", 1); *p++ = 0;
    attr("pixelAspectRatio", "float", 4); i32(0x3F800000u);
    attr("screenWindowCenter", "v2f", 8); i32(0); i32(0);
    attr("screenWindowWidth", "float", 4); i32(0x3F800000u);
    *p++ = 0;
    return (size_t)(p - dst);
}

// ---- the kernels' arguments (pt::ExrLayout's arrays) ----
struct ExrChan {
    const float* tex;          // RGBA32F, rows bottom-up
    int component, type;
    float scale;
    unsigned long long at;     // where the channel's samples start within a scanline's bytes
};
struct ExrArgs {
    ExrChan ch[kChannelsMax];  // sorted by name
    int channels, width, height, compression;
    int lines;                 // scanlines to a block
    int pieces;                // pieces of a full block
    unsigned long long line;   // a scanline's bytes
    unsigned long long blocks; // ceil(height / lines)
    unsigned long long stride; // bytes between the blocks in raw and pred
    unsigned long long header; // the file's bytes before the offset table
    uint8_t* raw;              // [blocks x stride]
    uint8_t* pred;             // [blocks x stride]
    uint8_t* slots;            // [blocks x pieces x pt::kPngSlot] each piece's deflate bytes
    uint32_t* meta;            // [blocks x pieces][4]: the piece's bytes, where they start in the chunk's data, Adler A, B
    uint32_t* bmeta;           // [blocks][4]: the chunk's data size, 1 when it is the stream, the Adler-32
    unsigned long long* off;   // [blocks] where the chunk starts in out
    unsigned long long* total; // out's bytes in all
    uint8_t* out;              // the offset table and the chunks: the file behind its header
};
// a block's scanlines and raw bytes
PTP_HD inline unsigned long long block_lines(const ExrArgs& a, unsigned long long b)
{
    const unsigned long long y0 = b * (unsigned long long)a.lines, left = (unsigned long long)a.height - y0;
    return left < (unsigned long long)a.lines ? left : (unsigned long long)a.lines;
}
PTP_HD inline unsigned long long block_bytes(const ExrArgs& a, unsigned long long b) { return block_lines(a, b) * a.line; }
PTP_HD inline unsigned block_pieces(unsigned long long n) { return (unsigned)((n + kPiece - 1) / kPiece); }

}  // namespace pte
