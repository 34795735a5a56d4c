// pt_jpeg_enc.hip — the canvas as a baseline JPEG, on the device (include/pt.h pt_canvas_encode_jpeg; the format,
// stage by stage, is INTEGRATION.md "Encoding the canvas" and tests/jpeg_enc_ref.py). Integer arithmetic only, so
// the bytes are libjpeg-turbo's. A wave is one 8x8 MCU and takes its three blocks (Y, Cb, Cr) in turn; lane k is
// zigzag coefficient k. The workspace is pt::JpegLayout (pt_plan.h).
//
//   pt_jpeg_dct          a wave per MCU: colour conversion with the edges repeated, jfdctint's two passes through
//                        LDS (a lane computes its own output of the 8-point transform, the column pass at the
//                        lane's zigzag position, so the zigzag costs nothing), quantisation; the coefficients as
//                        int16 (128 B per block, one store per wave) and the block's AC bit count.
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
// No kernel writes outside the workspace whatever the pixels: a block's bits are bounded by kJpegBlockBytes
// (pt_plan.h) because the quantiser clamps to the categories the tables have, and the stream buffer is allocated
// from the length pt_jpeg_scan_rows computed.
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

__global__ __launch_bounds__(64 * kWaves) void pt_jpeg_dct(EncArgs a)
{
    __shared__ int s_in[kWaves][64], s_mid[kWaves][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t n_mcu = (size_t)a.mcus_x * a.rows;
    size_t m = (size_t)blockIdx.x * kWaves + w;
    const bool live = m < n_mcu;   // (a wave past the end works on the last MCU and stores nothing: the barriers)
    if (!live) m = n_mcu - 1;
    const unsigned row = (unsigned)(m / a.mcus_x), mx = (unsigned)(m % a.mcus_x);
    const int x = lane & 7, y = lane >> 3;
    const int px = min((int)mx * 8 + x, a.width - 1), py = min((int)row * 8 + y, a.height - 1);
    const uint32_t p = a.canvas[(size_t)(a.height - 1 - py) * a.width + px];   // scanline 0 is the top canvas row
    const int r = p & 255, g = p >> 8 & 255, b = p >> 16 & 255;
    // jccolor's fixed point, F(x) = int(x 65536 + 0.5)
    int s[3];
    s[0] = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    s[1] = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    s[2] = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
    const int nat = kZigzag[lane], u = nat >> 3, v = nat & 7;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        s_in[w][lane] = s[c] - 128;
        __syncthreads();
        int d[8];
        for (int j = 0; j < 8; j++) d[j] = s_in[w][y * 8 + j];
        s_mid[w][lane] = fdct8<true>(d, x);
        __syncthreads();
        for (int j = 0; j < 8; j++) d[j] = s_mid[w][j * 8 + v];
        const int f = fdct8<false>(d, u);
        // jcdctmgr's quantiser: divide by 8 t, rounding half away from zero. The clamp never binds for 8-bit
        // samples (|DC| <= 1024, |AC| <= 1020 at t = 1); it holds the block to the categories the tables have.
        const int t8 = 8 * (int)a.qt.q[c ? 1 : 0][lane];
        int q = (f < 0 ? -f : f) + (t8 >> 1);
        q = q >= t8 ? q / t8 : 0;
        q = f < 0 ? -min(q, lane ? 1023 : 1024) : min(q, 1023);
        unsigned long long bits;
        int len;
        lane_code(lane, q, 0, __ballot(q != 0), c ? 1 : 0, bits, len);
        const int ac_bits = wave_sum(lane ? len : 0);
        if (live) {
            const size_t blk = (size_t)row * a.blocks_row + mx * 3 + c;
            a.coef[blk * 64 + lane] = (int16_t)q;
            if (lane == 0) a.bitoff[blk] = (uint32_t)ac_bits;
        }
    }
}

__global__ __launch_bounds__(256) void pt_jpeg_scan_blocks(EncArgs a)
{
    __shared__ unsigned sh[4];
    const unsigned row = blockIdx.x;
    const size_t base = (size_t)row * a.blocks_row;
    unsigned carry = 0;
    for (unsigned b0 = 0; b0 < a.blocks_row; b0 += 256) {
        const unsigned b = b0 + threadIdx.x;
        unsigned len = 0;
        if (b < a.blocks_row) {
            const int dc = a.coef[(base + b) * 64], prev = b >= 3 ? a.coef[(base + b - 3) * 64] : 0;
            const int d = dc - prev, n = 32 - __clz(d < 0 ? -d : d);
            len = a.bitoff[base + b] + (kCodes.dc[b % 3 ? 1 : 0][n] >> 16) + n;
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

__global__ __launch_bounds__(64 * kWaves) void pt_jpeg_emit(EncArgs a)
{
    const int lane = threadIdx.x & 63;
    const size_t m = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (m >= (size_t)a.mcus_x * a.rows) return;   // (a whole wave: no block barrier below)
    const unsigned row = (unsigned)(m / a.mcus_x), mx = (unsigned)(m % a.mcus_x);
    uint32_t* words = (uint32_t*)((char*)a.bits + (size_t)row * a.row_stride);
    for (int c = 0; c < 3; c++) {
        const size_t blk = (size_t)row * a.blocks_row + mx * 3 + c;
        const int v = a.coef[blk * 64 + lane];
        const int prev = mx ? a.coef[(blk - 3) * 64] : 0;   // the prediction restarts with every row
        unsigned long long bits;
        int len;
        lane_code(lane, v, prev, __ballot(v != 0), c ? 1 : 0, bits, len);
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
        // a tile of 256 rows in 32 bits: a row is below 2^24 bytes (65535 / 8 MCUs x 3 x 2 x 208 + 2)
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

}  // namespace ptj

// colour conversion .. the stream's length: what runs before the host can size the stream buffer
extern "C" hipError_t pt_launch_jpeg_measure(const ptj::EncArgs* a, hipStream_t s)
{
    const size_t n_mcu = (size_t)a->mcus_x * a->rows;
    const dim3 mcus((unsigned)((n_mcu + ptj::kWaves - 1) / ptj::kWaves));
    hipLaunchKernelGGL(ptj::pt_jpeg_dct, mcus, dim3(64 * ptj::kWaves), 0, s, *a);
    hipLaunchKernelGGL(ptj::pt_jpeg_scan_blocks, dim3(a->rows), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(ptj::pt_jpeg_emit, mcus, dim3(64 * ptj::kWaves), 0, s, *a);
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
