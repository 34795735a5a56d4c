// pt_jpeg_enc.hip — the canvas as a baseline JPEG, on the device (include/pt.h pt_canvas_encode_jpeg_opt; the
// format, stage by stage, is INTEGRATION.md "Encoding the canvas" and tests/jpeg_enc_ref.py, jpeg_enc_sub_ref.py).
// Integer arithmetic only, so the bytes are libjpeg-turbo's. A wave is one MCU of 8 hs x 8 vs pixels (Y sampled
// hs x vs: 4:4:4 1x1, 4:2:2 2x1, 4:2:0 2x2) and takes its hs vs + 2 blocks (Y row-major, Cb, Cr) in turn; lane k is
// zigzag coefficient k. The workspace is pt::JpegLayout (pt_plan.h). The first three kernels are instances per
// sampling, so the 4:4:4 ones are the code they were before the other two.
//
//   pt_jpeg_dct          a wave per MCU: colour conversion with the edges repeated, Cb and Cr of a lane's hs x vs
//                        pixels summed with jcsample's bias, jfdctint's two passes through
//                        LDS (a lane computes its own output of the 8-point transform, the column pass at the
//                        lane's zigzag position, so the zigzag costs nothing), quantisation; the coefficients as
//                        int16 (128 B per block, one store per wave) and the block's AC bit count. A Y block
//                        outside the image (a dummy) is the DC of the block before it and no AC.
//   pt_jpeg_scan_blocks  a block per MCU row: the DC category of every block against its predecessor, an exclusive
//                        scan of the block lengths -> every block's first bit in its row and the row's bit count;
//                        then it zeroes the words of the row's bit buffer that the row will use.
//   pt_jpeg_emit         a wave per MCU: lane k's bits (ZRLs, code, value) from the ballot of non-zero lanes and a
//                        wave prefix sum of lengths, ORed into the row's bit buffer (integer atomicOr, at most
//                        three words per lane; the buffer is MSB-first in big-endian 32-bit words).
//   pt_jpeg_count_ff     a block per MCU row: the 0xFF bytes before each kJpegTile-byte tile of the row's bytes
//                        (the last byte padded with 1-bits), and the row's stuffed length with its marker.
//   pt_jpeg_scan_rows    one block: the exclusive scan of the row lengths, and the stream's length.
//   pt_jpeg_pack         a block per tile: every byte to its place in the stream, a 0x00 after every 0xFF, RSTm
//                        after every row but the last and EOI after that one.
// With optimised tables (pt_canvas_encode_jpeg_opt, optimize = 1; tests/jpeg_enc_opt_ref.py) three kernels run
// between pt_jpeg_dct and pt_jpeg_scan_blocks, and that one and pt_jpeg_emit are their OPT instances, which read
// the tables built on the device (pt::JpegOptLayout) where the others read the Annex K codes:
//   pt_jpeg_hist         a wave per MCU: the symbols the emitter will write, counted per table in LDS and then in
//                        the four global histograms.
//   pt_jpeg_build_tables a wave per table: libjpeg's jpeg_gen_optimal_table, the tables for the header and the codes.
//   pt_jpeg_block_bits   a wave per MCU: every block's AC bit count again, under those codes.
// An encode job (pt_canvas_encode_jpeg_begin) runs the same kernels with pt_jpeg_pack writing into the job's own
// device slot of stream_max() bytes, so that the host need not know the length first, and one more behind them:
//   pt_jpeg_ship         the stream, its length and the tables into the job's pinned host buffer, 16 bytes a lane.
// No kernel writes outside the workspace whatever the pixels: a block's bits are bounded by kJpegBlockBytes, or
// kJpegOptBlockBytes under tables of any code lengths up to 16 (pt_plan.h), because the quantiser clamps to the
// categories the tables have, and the stream buffer is allocated from the length pt_jpeg_scan_rows computed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_jpeg_enc.h"
#include "pt_plan.h"

namespace ptj {

__device__ const HuffCodes kCodes = make_codes();
static_assert(make_codes().ac[0][0xF0] == (0x7F9u | 11u << 16) && make_codes().ac[1][0x00] == (0u | 2u << 16), "Annex K");

constexpr int kWaves = 4;   // MCUs per block of pt_jpeg_dct / pt_jpeg_emit

// jfdctint ("islow", CONST_BITS 13, PASS1_BITS 2): output `idx` of the 8-point transform of d[0..7]; ROW: the first
// pass (outputs scaled up by 4), otherwise the second (the scaling removed, so the result is 8 x the DCT)
template <bool ROW> __device__ inline int fdct8(const int* d, int idx)
{
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = ROW ? 11 : 15, r = 1 << (n - 1);
    const int o0 = ROW ? (t10 + t11) << 2 : (t10 + t11 + 2) >> 2;
    const int o4 = ROW ? (t10 - t11) << 2 : (t10 - t11 + 2) >> 2;
    const int ze = (t12 + t13) * 4433;
    const int o2 = (ze + t13 * 6270 + r) >> n, o6 = (ze - t12 * 15137 + r) >> n;
    const int z5 = (t4 + t6 + t5 + t7) * 9633;
    const int z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995;
    const int z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
    const int o7 = (t4 * 2446 + z1 + z3 + r) >> n, o5 = (t5 * 16819 + z2 + z4 + r) >> n;
    const int o3 = (t6 * 25172 + z2 + z3 + r) >> n, o1 = (t7 * 12299 + z1 + z4 + r) >> n;
    const int lo = idx & 2 ? (idx & 1 ? o3 : o2) : (idx & 1 ? o1 : o0);
    const int hi = idx & 2 ? (idx & 1 ? o7 : o6) : (idx & 1 ? o5 : o4);
    return idx & 4 ? hi : lo;
}

// Lane k's share of a block's entropy-coded bits, right-aligned in `bits`, `len` of them (at most 3 x 11 + 16 + 10):
// k = 0 the DC difference; a non-zero AC its ZRLs, code and value, the zero run read from the mask of non-zero
// lanes; lane 63 the EOB when it holds a zero; nothing otherwise.
__device__ inline void lane_code(int k, int v, int prev_dc, unsigned long long nonzero, int table,
                                 unsigned long long& bits, int& len)
{
    bits = 0;
    len = 0;
    if (k == 0) {
        const int d = v - prev_dc, n = 32 - __clz(d < 0 ? -d : d);
        const uint32_t e = kCodes.dc[table][n];
        bits = (unsigned long long)(e & 0xFFFFu) << n | (unsigned)((d < 0 ? d - 1 : d) & ((1 << n) - 1));
        len = (int)(e >> 16) + n;
    } else if (v != 0) {
        const unsigned long long below = nonzero & ((1ull << k) - 1ull) & ~1ull;
        const int run = k - 1 - (below ? 63 - __clzll((long long)below) : 0);
        const int n = 32 - __clz(v < 0 ? -v : v);
        const uint32_t zrl = kCodes.ac[table][0xF0], e = kCodes.ac[table][(run & 15) << 4 | n];
        for (int i = 0; i < (run >> 4); i++) {
            bits = bits << (zrl >> 16) | (zrl & 0xFFFFu);
            len += (int)(zrl >> 16);
        }
        bits = (bits << (e >> 16) | (e & 0xFFFFu)) << n | (unsigned)((v < 0 ? v - 1 : v) & ((1 << n) - 1));
        len += (int)(e >> 16) + n;
    } else if (k == 63) {
        const uint32_t e = kCodes.ac[table][0x00];
        bits = e & 0xFFFFu;
        len = (int)(e >> 16);
    }
}

__device__ inline int wave_sum(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// inclusive prefix sum over the wave's 64 lanes
__device__ inline int wave_scan(int v, int lane)
{
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}
// exclusive prefix sum over a 256-thread block, and the block's total; `sh` holds 4 words (two barriers)
__device__ inline unsigned block_scan(unsigned v, unsigned* sh, unsigned& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned inc = (unsigned)wave_scan((int)v, lane);
    __syncthreads();   // (the previous call's reads of sh)
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    unsigned base = 0;
    total = 0;
    for (int i = 0; i < 4; i++) {
        if (i < w) base += sh[i];
        total += sh[i];
    }
    return base + inc - v;
}

// jccolor's fixed point, F(x) = int(x 65536 + 0.5), of an RGBA8 pixel
__device__ inline int luma(uint32_t p)
{
    const int r = p & 255, g = p >> 8 & 255, b = p >> 16 & 255;
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
}
__device__ inline void chroma(uint32_t p, int& cb, int& cr)
{
    const int r = p & 255, g = p >> 8 & 255, b = p >> 16 & 255;
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// How far back in its row the block at position j of an MCU of NY Y blocks finds the block its DC is predicted
// from: a Y block the Y block before it, which for j = 0 is the last one of the MCU before (NY - 1 + 2 chroma
// blocks back = 3 whatever NY), a chroma block its own component in the MCU before. The first MCU of a row has no
// such block where that reaches past the row's start: the prediction is 0 there.
template <int NY> __device__ inline unsigned dc_back(unsigned j) { return j >= NY ? NY + 2 : j ? 1 : 3; }

// HS x VS is Y's sampling: the wave's MCU is 8 HS x 8 VS pixels, its blocks the VS rows of HS Y blocks, Cb, Cr.
template <int HS, int VS> __global__ __launch_bounds__(64 * kWaves) void pt_jpeg_dct(EncArgs a)
{
    constexpr int NY = HS * VS;
    __shared__ int s_in[kWaves][64], s_mid[kWaves][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t n_mcu = (size_t)a.mcus_x * a.rows;
    size_t m = (size_t)blockIdx.x * kWaves + w;
    const bool live = m < n_mcu;   // (a wave past the end works on the last MCU and stores nothing: the barriers)
    if (!live) m = n_mcu - 1;
    const unsigned row = (unsigned)(m / a.mcus_x), mx = (unsigned)(m % a.mcus_x);
    const int x = lane & 7, y = lane >> 3;
    // scanline 0 is the top canvas row; the edges repeat
    auto pixel = [&](int px, int py) {
        return a.canvas[(size_t)(a.height - 1 - min(py, a.height - 1)) * a.width + min(px, a.width - 1)];
    };
    // every sample of the lane before the first barrier: s[0 .. NY) the Y blocks, s[NY] Cb, s[NY + 1] Cr
    int s[NY + 2];
    bool real[NY];   // (the same in every lane) a Y block outside the image's ceil(W / 8) x ceil(H / 8) is a dummy
#pragma unroll
    for (int j = 0; j < NY; j++) {
        const int bx = (int)mx * HS + j % HS, by = (int)row * VS + j / HS;
        real[j] = NY == 1 || (bx < (a.width + 7) >> 3 && by < (a.height + 7) >> 3);   // (1x1: no MCU has one)
        s[j] = real[j] ? luma(pixel(bx * 8 + x, by * 8 + y)) : 0;
    }
    {
        // jcsample's h2v1 / h2v2 over the converted samples: the right edge repeats before the downsampling, the
        // bottom edge up to a multiple of VS rows before it and in downsampled rows after it; the bias alternates
        // with the output column (x's parity is the column's: an MCU starts at an even one)
        const int cx = (int)mx * 8 + x, cy = min((int)row * 8 + y, (a.height + VS - 1) / VS - 1);
        int cb = 0, cr = 0;
#pragma unroll
        for (int i = 0; i < NY; i++) {
            int pb, pr;
            chroma(pixel(cx * HS + i % HS, cy * VS + i / HS), pb, pr);
            cb += pb;
            cr += pr;
        }
        constexpr int sh = NY == 4 ? 2 : NY == 2 ? 1 : 0;
        const int bias = NY == 4 ? 1 + (x & 1) : NY == 2 ? x & 1 : 0;
        s[NY] = (cb + bias) >> sh;
        s[NY + 1] = (cr + bias) >> sh;
    }
    const int nat = kZigzag[lane], u = nat >> 3, v = nat & 7;
    int prev_dc = 0;   // the quantised DC of the block before, for a dummy
#pragma unroll
    for (int c = 0; c < NY + 2; c++) {
        const bool is_real = c < NY ? real[c] : true;   // (a dummy keeps the barriers and skips the transform)
        const int table = c < NY ? 0 : 1;
        if (is_real) s_in[w][lane] = s[c] - 128;
        __syncthreads();
        int d[8];
        if (is_real) {
            for (int j = 0; j < 8; j++) d[j] = s_in[w][y * 8 + j];
            s_mid[w][lane] = fdct8<true>(d, x);
        }
        __syncthreads();
        int q = lane ? 0 : prev_dc;
        if (is_real) {
            for (int j = 0; j < 8; j++) d[j] = s_mid[w][j * 8 + v];
            const int f = fdct8<false>(d, u);
            // jcdctmgr's quantiser: divide by 8 t, rounding half away from zero. The clamp never binds for 8-bit
            // samples (|DC| <= 1024, |AC| <= 1020 at t = 1); it holds the block to the categories the tables have.
            const int t8 = 8 * (int)a.qt.q[table][lane];
            q = (f < 0 ? -f : f) + (t8 >> 1);
            q = q >= t8 ? q / t8 : 0;
            q = f < 0 ? -min(q, lane ? 1023 : 1024) : min(q, 1023);
        }
        if (c + 1 < NY) prev_dc = __shfl(q, 0);
        unsigned long long bits;
        int len;
        lane_code(lane, q, 0, __ballot(q != 0), table, bits, len);
        const int ac_bits = wave_sum(lane ? len : 0);   // (a dummy's: the EOB)
        if (live) {
            const size_t blk = (size_t)row * a.blocks_row + mx * (NY + 2) + c;
            a.coef[blk * 64 + lane] = (int16_t)q;
            if (lane == 0) a.bitoff[blk] = (uint32_t)ac_bits;
        }
    }
}

// ---- optimised tables: the statistics, the tables, and every block's AC bit count under them ----

// Block c of MCU mx of `row`: lane k's coefficient and the DC the block is predicted from (0 at the row's start)
template <int NY> __device__ inline void load_block(const EncArgs& a, unsigned row, unsigned mx, int c, int lane,
                                                     size_t& blk, int& v, int& prev)
{
    blk = (size_t)row * a.blocks_row + mx * (NY + 2) + c;
    v = a.coef[blk * 64 + lane];
    const unsigned at_row = mx * (NY + 2) + c, back = dc_back<NY>((unsigned)c);
    prev = at_row >= back ? a.coef[(blk - back) * 64] : 0;
}
// lane k's bits under the tables pt_jpeg_build_tables derived
__device__ inline LaneBits lane_code_opt(const HuffCodes* codes, int k, int v, int prev, unsigned long long nonzero, int table)
{
    return lane_bits(lane_symbols(k, v, prev, nonzero), k ? codes->ac[table] : codes->dc[table], codes->ac[table][0xF0]);
}

constexpr unsigned kHistBlocks = 1024;   // pt_jpeg_hist's grid at most: each block adds its counts to the global ones once

// A wave per MCU, MCUs in a grid-stride loop: the symbols the emitter will write (libjpeg's htest_one_block), counted
// in LDS and added to a.hist once per block. Integer counts: the result does not depend on the order. A block's LDS
// counter stays in 32 bits: at most 2^26 MCUs x 6 blocks x 63 symbols / kHistBlocks.
template <int NY> __global__ __launch_bounds__(64 * kWaves) void pt_jpeg_hist(EncArgs a)
{
    __shared__ unsigned s_hist[4 * 256];
    for (unsigned i = threadIdx.x; i < 4 * 256; i += 64 * kWaves) s_hist[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const size_t n_mcu = (size_t)a.mcus_x * a.rows;
    for (size_t m = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6); m < n_mcu; m += (size_t)gridDim.x * kWaves) {
        const unsigned row = (unsigned)(m / a.mcus_x), mx = (unsigned)(m % a.mcus_x);
        for (int c = 0; c < NY + 2; c++) {
            size_t blk;
            int v, prev;
            load_block<NY>(a, row, mx, c, lane, blk, v, prev);
            const LaneSyms s = lane_symbols(lane, v, prev, __ballot(v != 0));
            unsigned* h = s_hist + ((c < NY ? 0 : 2) + (lane ? 1 : 0)) * 256;   // (a DC category is at most 11)
            if (s.sym >= 0) atomicAdd(h + s.sym, 1u);
            if (s.zrls) atomicAdd(h + 0xF0, (unsigned)s.zrls);
        }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < 4 * 256; i += 64 * kWaves)
        if (const unsigned n = s_hist[i]) atomicAdd(a.hist + i, (unsigned long long)n);
}

// the wave's two least of every lane's a <= b, in every lane (the keys differ but for the "none" key)
__device__ inline void wave_min2(unsigned long long& a, unsigned long long& b)
{
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long c = __shfl_xor(a, o), d = __shfl_xor(b, o);
        const unsigned long long hi = a < c ? c : a, next = b < d ? b : d;
        a = a < c ? a : c;
        b = hi < next ? hi : next;
    }
}

// A wave (a block of one) per table, blockIdx.x = DC 0, AC 0, DC 1, AC 1: libjpeg's jpeg_gen_optimal_table.
// Slot j of a lane is symbol 64 j + lane; slot 4 is symbol 256 in lane 0, the reserved one with count 1, so that no
// real symbol gets the all-ones code. The merge loop: c1 the non-zero count that is least, the largest symbol on a
// tie, c2 the same among the rest (one wave reduction that keeps the two least of count << 9 | 511 - symbol); c2's count goes to c1 and
// every symbol of either tree gets a bit longer and c1's tree id, which is libjpeg's walk of the others[] chains.
// Then the counts per length, libjpeg's limiting loop to 16 bits and the reserved code's removal (lane 0; libjpeg
// gives up on a length past 32, the loop itself holds for any, and kMaxLen = 256 is what 257 symbols can reach),
// huffval by length then value (ballots), and the canonical codes of Annex C in the layout of HuffCodes.
constexpr int kMaxLen = 256;
__global__ __launch_bounds__(64) void pt_jpeg_build_tables(EncArgs a)
{
    __shared__ int s_raw[kMaxLen + 1], s_bits[kMaxLen + 1];   // symbols per length: as merged, and limited
    __shared__ int s_cum[18];                                  // [l] the symbols shorter than l (1..17)
    __shared__ uint32_t s_first[17];                           // [l] the first code of length l
    __shared__ uint32_t s_code[256];
    __shared__ uint8_t s_vals[256];
    const int lane = threadIdx.x, t = blockIdx.x;
    constexpr unsigned long long kNone = ~0ull;
    unsigned long long freq[5];
    int tree[5], size[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        freq[j] = j < 4 ? a.hist[t * 256 + 64 * j + lane] : lane == 0 ? 1ull : 0ull;
        tree[j] = 64 * j + lane;
        size[j] = 0;
    }
    for (;;) {
        unsigned long long k1 = kNone, k2 = kNone;   // the lane's two least keys, then the wave's
#pragma unroll
        for (int j = 0; j < 5; j++) {
            const unsigned long long k = freq[j] ? freq[j] << 9 | (unsigned long long)(511 - (64 * j + lane)) : kNone;
            k2 = k < k1 ? k1 : k < k2 ? k : k2;
            k1 = k < k1 ? k : k1;
        }
        wave_min2(k1, k2);
        if (k2 == kNone) break;   // (the same in every lane)
        const int c1 = 511 - (int)(k1 & 511), c2 = 511 - (int)(k2 & 511);
#pragma unroll
        for (int j = 0; j < 5; j++) {
            if (64 * j + lane == c1) freq[j] += k2 >> 9;
            if (64 * j + lane == c2) freq[j] = 0;
            if (tree[j] == c1 || tree[j] == c2) {
                size[j]++;
                tree[j] = c1;
            }
        }
    }
    for (int i = lane; i <= kMaxLen; i += 64) s_raw[i] = 0;
    for (int i = lane; i < 256; i += 64) {
        s_code[i] = 0;
        s_vals[i] = 0;
    }
    __syncthreads();
    int longest = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        if (size[j]) atomicAdd(&s_raw[size[j]], 1);   // (size <= 256: a merge lengthens a tree of at most 257 symbols)
        longest = max(longest, size[j]);
    }
    for (int o = 32; o > 0; o >>= 1) longest = max(longest, __shfl_xor(longest, o));
    __syncthreads();
    for (int i = lane; i <= kMaxLen; i += 64) s_bits[i] = s_raw[i];
    __syncthreads();
    if (lane == 0) {
        for (int i = longest; i > 16; i--)
            while (s_bits[i] > 0) {
                int j = i - 2;
                while (j > 0 && s_bits[j] == 0) j--;   // (the codes are complete, so a shorter length has a symbol)
                s_bits[i] -= 2;
                s_bits[i - 1]++;
                s_bits[j + 1] += 2;
                s_bits[j]--;
            }
        int i = 16;
        while (i > 0 && s_bits[i] == 0) i--;   // (symbol 256 and one real symbol at least: some length 1..16 has codes)
        s_bits[i]--;
        uint32_t code = 0;
        int cum = 0;
        for (int l = 1; l <= 16; l++) {
            s_first[l] = code;
            s_cum[l] = cum;
            code = (code + (uint32_t)s_bits[l]) << 1;
            cum += s_bits[l];
        }
        s_cum[17] = cum;
    }
    // huffval: the symbols 0..255 by raw length, then by value (slot-major, then lane)
    int at = 0;
    for (int l = 1; l <= longest; l++) {
        if (!s_raw[l]) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned long long mask = __ballot(size[j] == l);
            if (size[j] == l) s_vals[at + __popcll(mask & ((1ull << lane) - 1ull))] = (uint8_t)(64 * j + lane);
            at += __popcll(mask);
        }
    }
    __syncthreads();
    const int syms = s_cum[17];   // == at: the limiting loop moves codes between lengths and keeps their number
    const bool dc = !(t & 1);
    for (int p = lane; p < syms; p += 64) {
        int l = 1;
        while (p >= s_cum[l + 1]) l++;
        const int sym = s_vals[p];
        if (!dc || sym < 12) s_code[sym] = (s_first[l] + (uint32_t)(p - s_cum[l])) | (uint32_t)l << 16;
    }
    __syncthreads();
    uint32_t* out = dc ? a.codes->dc[t >> 1] : a.codes->ac[t >> 1];
    for (int i = lane; i < (dc ? 12 : 256); i += 64) out[i] = s_code[i];
    for (int i = lane; i < 256; i += 64) a.tables->vals[t][i] = s_vals[i];
    if (lane < 16) a.tables->bits[t][lane] = (uint8_t)s_bits[lane + 1];
}

// A wave per MCU: every block's AC bit count under the built tables, where pt_jpeg_dct left the Annex K one
template <int NY> __global__ __launch_bounds__(64 * kWaves) void pt_jpeg_block_bits(EncArgs a)
{
    const int lane = threadIdx.x & 63;
    const size_t m = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (m >= (size_t)a.mcus_x * a.rows) return;
    const unsigned row = (unsigned)(m / a.mcus_x), mx = (unsigned)(m % a.mcus_x);
    for (int c = 0; c < NY + 2; c++) {
        size_t blk;
        int v, prev;
        load_block<NY>(a, row, mx, c, lane, blk, v, prev);
        const LaneBits b = lane_code_opt(a.codes, lane, v, prev, __ballot(v != 0), c < NY ? 0 : 1);
        const int ac_bits = wave_sum(lane ? b.zrl_len + b.code_len : 0);
        if (lane == 0) a.bitoff[blk] = (uint32_t)ac_bits;
    }
}

// OPT: the tables pt_jpeg_build_tables derived (a.codes) in place of the Annex K ones
template <int NY, bool OPT> __global__ __launch_bounds__(256) void pt_jpeg_scan_blocks(EncArgs a)
{
    __shared__ unsigned sh[4];
    const unsigned row = blockIdx.x;
    const size_t base = (size_t)row * a.blocks_row;
    unsigned carry = 0;
    for (unsigned b0 = 0; b0 < a.blocks_row; b0 += 256) {
        const unsigned b = b0 + threadIdx.x;
        unsigned len = 0;
        if (b < a.blocks_row) {
            const unsigned j = b % (NY + 2), back = dc_back<NY>(j);
            const int dc = a.coef[(base + b) * 64], prev = b >= back ? a.coef[(base + b - back) * 64] : 0;
            const int d = dc - prev, n = 32 - __clz(d < 0 ? -d : d);
            if constexpr (OPT) len = a.bitoff[base + b] + (a.codes->dc[j < NY ? 0 : 1][n] >> 16) + n;
            else len = a.bitoff[base + b] + (kCodes.dc[j < NY ? 0 : 1][n] >> 16) + n;
        }
        unsigned total;
        const unsigned at = carry + block_scan(len, sh, total);
        if (b < a.blocks_row) a.bitoff[base + b] = at;
        carry += total;
    }
    if (threadIdx.x == 0) a.rowbits[row] = carry;
    // the row's words of the bit buffer that pt_jpeg_emit will OR into (carry <= 8 row_stride, a multiple of 128)
    uint4* z = (uint4*)((char*)a.bits + (size_t)row * a.row_stride);
    for (unsigned i = threadIdx.x; i < (carry + 127) / 128; i += 256) z[i] = make_uint4(0, 0, 0, 0);
}

// OPT: the built tables, under which a lane's share may be 74 bits: the ZRLs apart from the code, in a four-word window
template <int NY, bool OPT> __global__ __launch_bounds__(64 * kWaves) void pt_jpeg_emit(EncArgs a)
{
    const int lane = threadIdx.x & 63;
    const size_t m = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (m >= (size_t)a.mcus_x * a.rows) return;   // (a whole wave: no block barrier below)
    const unsigned row = (unsigned)(m / a.mcus_x), mx = (unsigned)(m % a.mcus_x);
    uint32_t* words = (uint32_t*)((char*)a.bits + (size_t)row * a.row_stride);
    for (int c = 0; c < NY + 2; c++) {
        const size_t blk = (size_t)row * a.blocks_row + mx * (NY + 2) + c;
        const int v = a.coef[blk * 64 + lane];
        const unsigned at_row = mx * (NY + 2) + c, back = dc_back<NY>((unsigned)c);
        const int prev = at_row >= back ? a.coef[(blk - back) * 64] : 0;   // the prediction restarts with every row
        if constexpr (OPT) {
            const LaneBits b = lane_code_opt(a.codes, lane, v, prev, __ballot(v != 0), c < NY ? 0 : 1);
            const int len = b.zrl_len + b.code_len;
            const unsigned at = a.bitoff[blk] + (unsigned)(wave_scan(len, lane) - len);
            if (len) {
                uint32_t w[4];
                lane_window(b, at, w);
                uint32_t* dst = words + (at >> 5);   // (a word past the row's bits is zero here and is not touched)
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (w[i]) atomicOr(dst + i, w[i]);
            }
            continue;
        }
        unsigned long long bits;
        int len;
        lane_code(lane, v, prev, __ballot(v != 0), c < NY ? 0 : 1, bits, len);
        const unsigned at = a.bitoff[blk] + (unsigned)(wave_scan(len, lane) - len);
        if (len) {
            // the lane's bits left-aligned in 64, then shifted to bit `at & 31` of a three-word window
            const unsigned long long left = bits << (64 - len);
            const unsigned sh = at & 31;
            const unsigned long long two = left >> sh;
            const uint32_t w0 = (uint32_t)(two >> 32), w1 = (uint32_t)two, w2 = sh ? (uint32_t)left << (32 - sh) : 0u;
            uint32_t* dst = words + (at >> 5);
            if (w0) atomicOr(dst, w0);
            if (w1) atomicOr(dst + 1, w1);
            if (w2) atomicOr(dst + 2, w2);
        }
    }
}

// word i of a row's bit buffer as the stream has it: the bits after the row's last one, up to the byte's end, set
__device__ inline uint32_t row_word(const uint32_t* words, unsigned i, unsigned rowbits)
{
    uint32_t w = words[i];
    const unsigned pad = (8 - (rowbits & 7)) & 7;
    if (pad && i == rowbits >> 5) w |= ((1u << pad) - 1u) << (32 - (rowbits & 31) - pad);
    return w;
}
// the bytes of word i that the row has (of its `nbytes`), and how many of them are 0xFF
__device__ inline int word_bytes(unsigned i, unsigned nbytes) { return (int)min(4u, nbytes - min(nbytes, 4 * i)); }
__device__ inline unsigned count_ff(uint32_t w, int n)
{
    unsigned c = 0;
    for (int j = 0; j < n; j++) c += (w >> (24 - 8 * j) & 255u) == 255u;
    return c;
}

__global__ __launch_bounds__(256) void pt_jpeg_count_ff(EncArgs a)
{
    __shared__ unsigned sh[4];
    const unsigned row = blockIdx.x, rowbits = a.rowbits[row], nbytes = (rowbits + 7) / 8;
    const uint32_t* words = (const uint32_t*)((const char*)a.bits + (size_t)row * a.row_stride);
    unsigned before = 0;
    for (unsigned t = 0; t * pt::kJpegTile < nbytes; t++) {   // (t < a.tiles: nbytes <= row_stride)
        const unsigned i = t * 256 + threadIdx.x;
        const int n = word_bytes(i, nbytes);
        const unsigned ff = n ? count_ff(row_word(words, i, rowbits), n) : 0u;
        unsigned total;
        block_scan(ff, sh, total);
        if (threadIdx.x == 0) a.tileoff[(size_t)row * a.tiles + t] = before;
        before += total;
    }
    if (threadIdx.x == 0) a.rowlen[row] = nbytes + before + 2;
}

__global__ __launch_bounds__(256) void pt_jpeg_scan_rows(EncArgs a)
{
    __shared__ unsigned sh[4];
    unsigned long long carry = 0;
    for (unsigned r0 = 0; r0 < a.rows; r0 += 256) {
        // a tile of 256 rows in 32 bits: a row is below 2^24 bytes (4:4:4 65535 / 8 MCUs x 3 blocks x 2 x 208 + 2 =
        // 10 223 618; 4:2:0 65535 / 16 MCUs x 6 x 2 x 208 + 2 the same, 4:2:2 x 4 x 2 x 208 + 2 = 6 815 746)
        const unsigned r = r0 + threadIdx.x, len = r < a.rows ? a.rowlen[r] : 0u;
        unsigned total;
        const unsigned at = block_scan(len, sh, total);
        if (r < a.rows) a.rowoff[r] = carry + at;
        carry += total;
    }
    if (threadIdx.x == 0) *a.total = carry;
}

__global__ __launch_bounds__(256) void pt_jpeg_pack(EncArgs a)
{
    __shared__ unsigned sh[4];
    const unsigned row = blockIdx.y, rowbits = a.rowbits[row], nbytes = (rowbits + 7) / 8;
    const uint32_t* words = (const uint32_t*)((const char*)a.bits + (size_t)row * a.row_stride);
    uint8_t* out = a.out + a.rowoff[row];
    for (unsigned t = blockIdx.x; t * pt::kJpegTile < nbytes; t += gridDim.x) {
        const unsigned i = t * 256 + threadIdx.x;
        const int n = word_bytes(i, nbytes);
        const uint32_t w = n ? row_word(words, i, rowbits) : 0u;
        unsigned total;
        unsigned at = 4 * i + a.tileoff[(size_t)row * a.tiles + t] + block_scan(n ? count_ff(w, n) : 0u, sh, total);
        for (int j = 0; j < n; j++) {
            const unsigned byte = w >> (24 - 8 * j) & 255u;
            out[at++] = (uint8_t)byte;
            if (byte == 255u) out[at++] = 0;
        }
        if (n && 4 * i + n == nbytes) {   // the row's last byte: RSTm, or EOI after the last row
            out[at] = 0xFF;
            out[at + 1] = (uint8_t)(row + 1 < a.rows ? 0xD0 + (row & 7) : 0xD9);
        }
    }
}

// An encode job's stream from its device slot to the job's pinned host buffer: min(length, room) bytes, a uint4 per
// lane and consecutive lanes consecutive addresses (a block moves 4 KiB per turn), the last length % 16 bytes one
// by one; block 0 also leaves the length and, with optimised tables, the tables in the buffer's result block. The
// host reads the buffer after the event recorded behind this kernel, whose release is system-scope.
constexpr unsigned kShipBlocks = 256;
__global__ __launch_bounds__(256) void pt_jpeg_ship(ShipArgs a)
{
    const unsigned long long length = *a.total;
    const size_t n = length < a.room ? (size_t)length : a.room;
    const uint4* src = (const uint4*)a.stream;
    uint4* dst = (uint4*)a.host_stream;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n / 16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
    if (blockIdx.x != 0) return;
    const size_t tail = (n & ~(size_t)15) + threadIdx.x;
    if (threadIdx.x < 16 && tail < n) a.host_stream[tail] = a.stream[tail];
    if (threadIdx.x == 0) *a.host_total = length;
    // (the tables stand right behind a length on either side, so they are 8-byte aligned and no more)
    static_assert(sizeof(OptTables) % 8 == 0 && sizeof(OptTables) / 8 <= 256, "the tables in one turn of 8-byte lanes");
    if (a.tables && threadIdx.x < sizeof(OptTables) / 8)
        ((unsigned long long*)a.host_tables)[threadIdx.x] = ((const unsigned long long*)a.tables)[threadIdx.x];
}

}  // namespace ptj

// the three kernels that know the MCU's blocks, at Y's sampling HS x VS
template <int HS, int VS> static void launch_blocks(const ptj::EncArgs* a, hipStream_t s)
{
    const size_t n_mcu = (size_t)a->mcus_x * a->rows;
    const dim3 mcus((unsigned)((n_mcu + ptj::kWaves - 1) / ptj::kWaves));
    hipLaunchKernelGGL((ptj::pt_jpeg_dct<HS, VS>), mcus, dim3(64 * ptj::kWaves), 0, s, *a);
    if (a->codes) {   // optimised tables: count the symbols (a->hist is zero), build the tables, measure with them
        const dim3 some(mcus.x < ptj::kHistBlocks ? mcus.x : ptj::kHistBlocks);
        hipLaunchKernelGGL((ptj::pt_jpeg_hist<HS * VS>), some, dim3(64 * ptj::kWaves), 0, s, *a);
        hipLaunchKernelGGL(ptj::pt_jpeg_build_tables, dim3(4), dim3(64), 0, s, *a);
        hipLaunchKernelGGL((ptj::pt_jpeg_block_bits<HS * VS>), mcus, dim3(64 * ptj::kWaves), 0, s, *a);
        hipLaunchKernelGGL((ptj::pt_jpeg_scan_blocks<HS * VS, true>), dim3(a->rows), dim3(256), 0, s, *a);
        hipLaunchKernelGGL((ptj::pt_jpeg_emit<HS * VS, true>), mcus, dim3(64 * ptj::kWaves), 0, s, *a);
        return;
    }
    hipLaunchKernelGGL((ptj::pt_jpeg_scan_blocks<HS * VS, false>), dim3(a->rows), dim3(256), 0, s, *a);
    hipLaunchKernelGGL((ptj::pt_jpeg_emit<HS * VS, false>), mcus, dim3(64 * ptj::kWaves), 0, s, *a);
}

// colour conversion .. the stream's length: what runs before the host can size the stream buffer
extern "C" hipError_t pt_launch_jpeg_measure(const ptj::EncArgs* a, hipStream_t s)
{
    if (a->hs == 1 && a->vs == 1) launch_blocks<1, 1>(a, s);
    else if (a->hs == 2 && a->vs == 1) launch_blocks<2, 1>(a, s);
    else if (a->hs == 2 && a->vs == 2) launch_blocks<2, 2>(a, s);
    else return hipErrorInvalidValue;   // (no kernel for any other sampling)
    hipLaunchKernelGGL(ptj::pt_jpeg_count_ff, dim3(a->rows), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(ptj::pt_jpeg_scan_rows, dim3(1), dim3(256), 0, s, *a);
    return hipGetLastError();
}

// ... and the stream into a->out, which holds the length that pass computed
extern "C" hipError_t pt_launch_jpeg_pack(const ptj::EncArgs* a, hipStream_t s)
{
    hipLaunchKernelGGL(ptj::pt_jpeg_pack, dim3(a->tiles < 32u ? a->tiles : 32u, a->rows), dim3(256), 0, s, *a);
    return hipGetLastError();
}

// ... and, for an encode job, from the job's device slot to its pinned host buffer with the length and the tables
extern "C" hipError_t pt_launch_jpeg_ship(const ptj::ShipArgs* a, hipStream_t s)
{
    const size_t turns = (a->room + 4095) / 4096;
    const unsigned blocks = turns < 1 ? 1u : turns < ptj::kShipBlocks ? (unsigned)turns : ptj::kShipBlocks;
    hipLaunchKernelGGL(ptj::pt_jpeg_ship, dim3(blocks), dim3(256), 0, s, *a);
    return hipGetLastError();
}
