// pt_hdr_enc.h — what the host and the kernels of pt_target_encode_hdr share (pt_hdr_enc.hip, pt_capi.cpp): the
// texel -> RGBE conversion, the coding of one maximal run of a byte plane, a sequential coder of a whole plane built
// on it, the file's header and the kernels' argument block. Plain C++ over plain arrays, no HIP: the kernels call
// these functions, so a host program runs whole planes through them without a GPU (tests/test_hdr_enc_host.py). The
// format is include/pt.h pt_target_encode_hdr and tests/hdr_enc_ref.py: a Radiance picture, 32-bit_rle_rgbe, whose
// scanlines are coded plane by plane as Radiance's own writer parses them (MINRUN 4, counts below 128).
//
// A plane of W bytes is cut into maximal runs of equal bytes. A run of L bytes gives L / 127 run pieces of 127 and a
// remainder r = L % 127, which is a run piece when r >= 4 and r loose bytes otherwise, so a run *leads* (starts with
// a run piece) exactly when L >= 4. Consecutive loose bytes form a stretch; `at` below is the number of loose bytes
// of the stretch before the run's own. A stretch of 2 or 3 equal bytes (one run's loose bytes alone) is the short
// token 128 + n, b; any other is cut from its left into literals n, b_1 .. b_n of at most 128 bytes. A literal's
// count byte is written with its last byte, which alone knows n: by the byte at stretch offset 127 mod 128, or by the
// stretch's last.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PTH_HD __host__ __device__
#else
#define PTH_HD
#endif

namespace pth {

constexpr int kMinRun = 4, kMaxRun = 127, kMaxLiteral = 128;
constexpr int kFlatBelow = 8, kCodedMax = 32767;   // a scanline narrower or wider than these is flat
constexpr int kStep = 64;                          // bytes, then runs, a wave takes per step
constexpr unsigned kWaves = 2048;                  // waves of the plane kernels at most (4 per block)
constexpr unsigned kPlaneGrid = 4096;              // blocks of 256 lanes of pt_hdr_planes at most: 2^20 texels a trip

PTH_HD inline bool flat_width(int w) { return w < kFlatBelow || w > kCodedMax; }

PTH_HD inline uint32_t float_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
PTH_HD inline float bits_float(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// R | G << 8 | B << 16 | E << 24 of a texel: Radiance's setcolr with the factor 256 / 2^e taken exactly. Every step
// is one binary32 operation or exact: v > 0 is false for NaN, negatives and -0; the cap is the largest value RGBE
// holds, (255 / 256) 2^127; a multiply by a power of two is exact, and where it underflows the floor is 0 either way.
PTH_HD inline uint32_t rgbe(float r, float g, float b, float scale)
{
    const float cap = bits_float(0x7EFF0000u);   // 255 x 2^119
    const float v[3] = { r * scale, g * scale, b * scale };
    float c[3];
    for (int k = 0; k < 3; k++) c[k] = v[k] > 0.0f ? (v[k] < cap ? v[k] : cap) : 0.0f;
    float m = c[0] > c[1] ? c[0] : c[1];
    m = m > c[2] ? m : c[2];
    if (m < 1e-32f) return 0u;
    const int e = (int)(float_bits(m) >> 23 & 255u) - 126;   // m = f 2^e, f in [0.5, 1); e in -106..127
    const float f = bits_float((uint32_t)(8 - e + 127) << 23);   // 2^(8 - e), 2^-119 .. 2^114: a normal number
    uint32_t out = (uint32_t)(e + 128) << 24;
    for (int k = 0; k < 3; k++) out |= (uint32_t)(int)(c[k] * f) << (8 * k);   // (c >= 0: the cast floors)
    return out;
}

// ---- one maximal run ----
struct Run {
    int pieces;   // run pieces of 127
    int rem;      // the remainder as a run piece, 4..126, or 0
    int loose;    // the remainder as loose bytes, 1..3, or 0
};
PTH_HD inline Run run_of(int L)
{
    const int r = L % kMaxRun;
    return Run{ L / kMaxRun, r >= kMinRun ? r : 0, r >= kMinRun ? 0 : r };
}
PTH_HD inline bool run_leads(int L) { return L >= kMinRun; }
// the run's loose bytes are a short token: 2 or 3 of them, alone in their stretch
PTH_HD inline bool run_short(const Run& r, int at, bool ends) { return r.loose >= 2 && at == 0 && ends; }
// the bytes the run codes to; `at` loose bytes of its stretch precede its own, `ends`: the stretch ends with them
PTH_HD inline int run_bytes(const Run& r, int at, bool ends)
{
    int n = 2 * (r.pieces + (r.rem ? 1 : 0));
    if (!r.loose) return n;
    if (run_short(r, at, ends)) return n + 2;
    for (int t = 0; t < r.loose; t++) n += 1 + ((at + t) % kMaxLiteral == 0);
    return n;
}
// ... and those bytes, of value b, at out; the count byte of a literal that one of the run's loose bytes closes lies
// up to 128 bytes before out, among the bytes of the runs before this one. Returns run_bytes.
PTH_HD inline int run_emit(const Run& r, uint8_t b, int at, bool ends, uint8_t* out)
{
    uint8_t* p = out;
    for (int i = 0; i < r.pieces; i++) { p[0] = (uint8_t)(128 + kMaxRun); p[1] = b; p += 2; }
    if (r.rem) { p[0] = (uint8_t)(128 + r.rem); p[1] = b; p += 2; }
    if (!r.loose) return (int)(p - out);
    if (run_short(r, at, ends)) {
        p[0] = (uint8_t)(128 + r.loose); p[1] = b;
        return (int)(p - out) + 2;
    }
    for (int t = 0; t < r.loose; t++) {
        const int m = (at + t) % kMaxLiteral;
        if (m == 0) p++;   // the literal's count byte
        *p = b;
        if (m == kMaxLiteral - 1 || (ends && t == r.loose - 1)) p[-(m + 1)] = (uint8_t)(m + 1);
        p++;
    }
    return (int)(p - out);
}

// A whole plane, run by run from the left: what the kernels compute with a run per lane. `out` holds
// plane_max(w) bytes; returns the coded length.
PTH_HD inline size_t plane_max(size_t w) { return w + (w + kMaxLiteral - 1) / kMaxLiteral; }
PTH_HD inline size_t code_plane(const uint8_t* in, int w, uint8_t* out)
{
    size_t n = 0;
    int at = 0;
    for (int s = 0; s < w;) {
        int e = s + 1;
        while (e < w && in[e] == in[s]) e++;
        int e2 = e + 1;   // the next run, as far as its first four bytes
        while (e2 < w && e2 - e < kMinRun && in[e2] == in[e]) e2++;
        const bool ends = e >= w || run_leads(e2 - e);
        const Run r = run_of(e - s);
        if (run_leads(e - s)) at = 0;
        n += (size_t)run_emit(r, in[s], at, ends, out + n);
        at += r.loose;
        s = e;
    }
    return n;
}

// The same from the list of run starts, as the kernels hold a plane: what a lane knows of run j of nr without its
// neighbours' help. The loose bytes before it in its stretch are a segmented sum over the runs, restarted where a
// run leads (the kernels: a wave scan with a carry from step to step; plane_from_starts: a loop).
struct RunAt {
    int s;        // where the run starts
    Run r;
    bool leads;   // it starts with a run piece: the stretch before it ends
    bool ends;    // its loose bytes, if any, end their stretch
};
PTH_HD inline RunAt run_at(const uint16_t* starts, unsigned nr, int w, unsigned j)
{
    const int s = j < nr ? (int)starts[j] : w, e = j + 1 < nr ? (int)starts[j + 1] : w,
              e2 = j + 2 < nr ? (int)starts[j + 2] : w;
    return RunAt{ s, run_of(e - s), run_leads(e - s), e >= w || run_leads(e2 - e) };
}
PTH_HD inline unsigned find_starts(const uint8_t* in, int w, uint16_t* starts)
{
    unsigned nr = 0;
    for (int i = 0; i < w; i++)
        if (i == 0 || in[i] != in[i - 1]) starts[nr++] = (uint16_t)i;
    return nr;
}
PTH_HD inline size_t plane_from_starts(const uint8_t* in, int w, const uint16_t* starts, unsigned nr, uint8_t* out)
{
    size_t n = 0;
    int sum = 0;
    for (unsigned j = 0; j < nr; j++) {
        const RunAt a = run_at(starts, nr, w, j);
        if (a.leads) sum = 0;
        n += (size_t)run_emit(a.r, in[a.s], sum, a.ends, out + n);
        sum += a.r.loose;
    }
    return n;
}

// ---- the file ----
constexpr size_t kHeaderMax = 80;
// "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y H +X W\n"; returns its length (<= kHeaderMax)
inline size_t write_header(uint8_t* dst, int width, int height)
{
    static const char head[] = "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y ";
    size_t n = sizeof(head) - 1;
    memcpy(dst, head, n);
    auto number = [&](unsigned v) {
        char d[10];
        int k = 0;
        do { d[k++] = (char)('0' + v % 10); v /= 10; } while (v);
        while (k) dst[n++] = (uint8_t)d[--k];
    };
    number((unsigned)height);
    memcpy(dst + n, " +X ", 4);
    n += 4;
    number((unsigned)width);
    dst[n++] = '\n';
    return n;
}
inline size_t header_bytes(int width, int height)
{
    uint8_t h[kHeaderMax];
    return write_header(h, width, height);
}

// the kernels' arguments (pt::HdrLayout's arrays)
struct HdrArgs {
    const float* tex;            // RGBA32F, rows bottom-up
    int width, height;
    float scale;
    uint8_t* planes;             // [height x 4 x width] scanline y's R, G, B, E planes
    uint16_t* starts;            // [height x 4 x width] a plane's run starts, in order
    uint32_t* runs;              // [height x 4] how many
    uint32_t* len;               // [height x 4] a plane's coded bytes
    unsigned long long* off;     // [height x 4] where it starts in out (plane 0: its scanline's four head bytes)
    unsigned long long* total;   // out's bytes in all
    uint8_t* out;                // the scanlines, coded
};

}  // namespace pth
