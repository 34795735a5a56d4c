// pt_png_enc.hip — the canvas as a PNG, on the device (include/pt.h pt_canvas_encode_png; the format is
// INTEGRATION.md "Encoding the canvas: PNG" and tests/png_enc_ref.py). Lossless: the filtered scanlines, deflated
// chunk by chunk to the bytes zlib 1.2.11 writes for each chunk under Z_RLE at level 6 with a full flush behind it.
// What host and kernels share (the tables, zlib's tree build, the block-size rule, the header coding, the packer,
// the CRC) is pt_png_enc.h; the workspace is pt::PngLayout (pt_plan.h).
//
//   pt_png_filter   a block per scanline (a bounded grid loops over them): the row's five |int8| sums by a block
//                   reduction when the filter is adaptive, then the filter byte and the filtered bytes into the
//                   stream. Row y reads rows y and y - 1 of the canvas, never the stream, so rows are independent.
//   pt_png_chunk    a one-wave block per chunk of 16,320 bytes, 255 bytes per lane, the chunk and its payload in LDS:
//                   run boundaries across the lanes, the tokens (literals and distance-1 matches), the 286 + 1
//                   counts by LDS atomics, the three trees and the three candidate sizes by lane 0 (the chunks are
//                   what runs in parallel), then the chosen block: the header by lane 0, the tokens by a prefix sum
//                   of the lanes' bit counts and LDS atomic ORs, or the stored bytes. It leaves the payload in the
//                   chunk's slot, and its length, the IDAT's CRC-32 (the lanes' pieces combined by linearity) and the
//                   chunk's Adler sums reduced mod 65521.
//   pt_png_scan     one block: the exclusive scan of the IDAT lengths, the Adler-32 of the whole stream from the
//                   chunks' sums, which it appends to the last chunk's payload (length and CRC with it), the total.
//   pt_png_pack     a block per chunk: length, "IDAT", payload, CRC to their place behind the file's head.
//
// The host writes the signature, IHDR and IEND, reads the total and copies that many bytes. Every global store is
// an ordinary vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_png_enc.h"
#include "pt_plan.h"

namespace ptp {

static_assert(kChunk == (int)pt::kPngChunk && kChunk % 4 == 0 && pt::kPngSlot % 4 == 0, "");
static_assert(pt::PngLayout::payload_max(pt::kPngChunk) <= pt::kPngSlot, "");

constexpr unsigned kFilterGrid = 4096;   // blocks of pt_png_filter at most
constexpr int kSlotWords = (int)(pt::kPngSlot / 4);

__device__ inline int channel(uint32_t px, int ch) { return (int)(px >> (8 * ch) & 255u); }

template <class T> __device__ inline T wave_sum(T v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// inclusive prefix sum over the wave's 64 lanes
__device__ inline unsigned wave_scan(unsigned v, int lane)
{
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}
// exclusive prefix sum over a 256-thread block, and the block's total; `sh` holds 4 values (two barriers)
template <class T> __device__ inline T block_scan(T v, T* sh, T& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    __syncthreads();   // (the previous call's reads of sh)
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    T base = 0;
    total = 0;
    for (int i = 0; i < 4; i++) {
        if (i < w) base += sh[i];
        total += sh[i];
    }
    return base + inc - v;
}

__global__ __launch_bounds__(256) void pt_png_filter(PngArgs a)
{
    __shared__ unsigned long long sums[4][5];
    const int W = a.width, H = a.height, bpp = a.bpp;
    for (unsigned long long y = blockIdx.x; y < (unsigned long long)H; y += gridDim.x) {
        // scanline y is canvas row H - 1 - y; the row above it the canvas row after that
        const uint32_t* cur = a.canvas + ((size_t)H - 1 - y) * (size_t)W;
        const uint32_t* up = cur + W;
        int type = a.filter;
        if (type == 5) {
            unsigned long long cost[5] = { 0, 0, 0, 0, 0 };
            for (int p = threadIdx.x; p < W; p += 256) {
                const uint32_t x = cur[p], pa = p ? cur[p - 1] : 0u, pb = y ? up[p] : 0u, pc = y && p ? up[p - 1] : 0u;
                for (int ch = 0; ch < bpp; ch++)
                    for (int t = 0; t < 5; t++)
                        cost[t] += filter_cost(filter_byte(t, channel(x, ch), channel(pa, ch), channel(pb, ch), channel(pc, ch)));
            }
            __syncthreads();   // (the previous row's reads of sums)
            for (int t = 0; t < 5; t++) {
                const unsigned long long s = wave_sum(cost[t]);
                if ((threadIdx.x & 63) == 0) sums[threadIdx.x >> 6][t] = s;
            }
            __syncthreads();
            unsigned long long best = ~0ull;
            for (int t = 0; t < 5; t++) {
                const unsigned long long s = sums[0][t] + sums[1][t] + sums[2][t] + sums[3][t];
                if (s < best) { best = s; type = t; }   // the lowest type on a tie
            }
        }
        uint8_t* out = a.filtered + y * (1ull + a.row_bytes);
        if (threadIdx.x == 0) out[0] = (uint8_t)type;
        for (int p = threadIdx.x; p < W; p += 256) {
            const uint32_t x = cur[p], pa = p ? cur[p - 1] : 0u, pb = y ? up[p] : 0u, pc = y && p ? up[p - 1] : 0u;
            for (int ch = 0; ch < bpp; ch++)
                out[1 + (size_t)p * bpp + ch] =
                    filter_byte(type, channel(x, ch), channel(pa, ch), channel(pb, ch), channel(pc, ch));
        }
    }
}

// the lanes' walk over the tokens that start in [lo, hi) of the chunk `in[0..n)`: s0 the start of the run that
// holds lo, nb the first run boundary at or after hi
template <class Visit>
__device__ inline void lane_tokens(const uint8_t* in, unsigned lo, unsigned hi, unsigned n, unsigned s0, unsigned nb, Visit&& visit)
{
    auto run_end = [&](unsigned i) {
        unsigned e = i + 1;
        while (e < hi && in[e] == in[e - 1]) e++;
        return e == hi && hi < n ? nb : e;
    };
    if (lo >= hi) return;
    unsigned s = s0, e = run_end(lo);
    for (unsigned i = lo; i < hi; i++) {
        if (i == e) { s = i; e = run_end(i); }
        const int tok = token_at(i, s, e);
        if (!tok) continue;
        visit(tok, in[i]);
        if (tok > 1) i += (unsigned)tok - 1;   // (the match ends within its run)
    }
}

__global__ __launch_bounds__(64) void pt_png_chunk(PngArgs a)
{
    __shared__ uint32_t s_in[kChunk / 4];
    __shared__ uint32_t s_out[kSlotWords];
    __shared__ unsigned s_cnt[kLCodes + 1];    // the literal / length counts, and the matches
    __shared__ int s_first[kLanes], s_last[kLanes];
    __shared__ unsigned s_at;
    __shared__ Block s_b;

    const unsigned long long c = blockIdx.x;
    const int lane = threadIdx.x;
    const unsigned long long base = c * (unsigned long long)kChunk;
    const unsigned n = (unsigned)(a.stream - base < (unsigned long long)kChunk ? a.stream - base : (unsigned long long)kChunk);
    const bool first = c == 0, last = c + 1 == a.chunks;
    const uint32_t* gin = (const uint32_t*)(a.filtered + base);   // (the chunks start on 64 B)
    for (unsigned i = lane; i < (n + 3) / 4; i += kLanes) s_in[i] = gin[i];
    for (int i = lane; i < kSlotWords; i += kLanes) s_out[i] = 0u;
    for (int i = lane; i < kLCodes + 1; i += kLanes) s_cnt[i] = 0u;
    __syncthreads();

    // run boundaries: a lane's first and last, and its Adler sums on the way
    const uint8_t* in = (const uint8_t*)s_in;
    const unsigned lo = min((unsigned)lane * kLaneBytes, n), hi = min(lo + kLaneBytes, n);
    int fb = (int)n, lb = -1;
    unsigned long long sa = 0, sb = 0;
    for (unsigned i = lo; i < hi; i++) {
        const unsigned d = in[i];
        if (i == 0 || d != in[i - 1]) {
            if (lb < 0) fb = (int)i;
            lb = (int)i;
        }
        sa += d;
        sb += (unsigned long long)(n - i) * d;
    }
    s_first[lane] = fb;
    s_last[lane] = lb;
    __syncthreads();
    unsigned s0 = 0, nb = n;
    for (int l = 0; l < lane; l++)
        if (s_last[l] >= 0) s0 = (unsigned)s_last[l];
    if (fb == (int)lo) s0 = lo;
    for (int l = kLanes - 1; l > lane; l--)
        if (s_first[l] < (int)nb) nb = (unsigned)s_first[l];

    // the counts
    lane_tokens(in, lo, hi, n, s0, nb, [&](int tok, uint8_t byte) {
        atomicAdd(&s_cnt[token_symbol(tok, byte)], 1u);
        if (tok != 1) atomicAdd(&s_cnt[kLCodes], 1u);
    });
    __syncthreads();
    for (int i = lane; i < kLCodes; i += kLanes) s_b.lfreq[i] = (uint16_t)s_cnt[i];
    if (lane < kDCodes) s_b.dfreq[lane] = lane == 0 ? (uint16_t)s_cnt[kLCodes] : (uint16_t)0;
    __syncthreads();

    // the trees, the sizes, the block type and the header: one lane over LDS arrays
    uint8_t* ob = (uint8_t*)s_out;
    if (lane == 0) {
        plan_block(s_b, n);
        unsigned at = 0;
        if (first) { ob[0] = 0x78; ob[1] = 0x01; at = 16; }
        if (s_b.type == kStored) {
            uint8_t* p = ob + (at >> 3);
            p[0] = last ? 1 : 0;
            p[1] = (uint8_t)n; p[2] = (uint8_t)(n >> 8);
            p[3] = (uint8_t)~n; p[4] = (uint8_t)(~n >> 8);
            at += 40;
        } else {
            block_header(s_b, last ? 1 : 0, [&](unsigned long long v, int len) {
                uint32_t w[3];
                lsb_window(v, len, at, w);
                const unsigned k = at >> 5;   // (a header is below 5000 bits)
                s_out[k] |= w[0];
                s_out[k + 1] |= w[1];
                at += (unsigned)len;
            });
        }
        s_at = at;
    }
    __syncthreads();

    unsigned at = s_at;
    if (s_b.type == kStored) {
        for (unsigned i = lo; i < hi; i++) ob[(at >> 3) + i] = in[i];
        at += 8 * n;
    } else {
        unsigned mine = 0;
        lane_tokens(in, lo, hi, n, s0, nb, [&](int tok, uint8_t byte) {
            int len;
            token_bits(s_b, tok, byte, len);
            mine += (unsigned)len;
        });
        const unsigned inc = wave_scan(mine, lane);
        unsigned pos = at + inc - mine;
        auto put = [&](unsigned long long v, int len) {
            uint32_t w[3];
            lsb_window(v, len, pos, w);
            const unsigned k = pos >> 5;
            for (int j = 0; j < 3; j++)
                if (w[j] && k + j < (unsigned)kSlotWords) atomicOr(&s_out[k + j], w[j]);
            pos += (unsigned)len;
        };
        lane_tokens(in, lo, hi, n, s0, nb, [&](int tok, uint8_t byte) {
            int len;
            const unsigned long long v = token_bits(s_b, tok, byte, len);
            put(v, len);
        });
        at += __shfl(inc, kLanes - 1);
        if (lane == 0) {
            pos = at;
            put(s_b.lcode[kEndBlock], s_b.llen[kEndBlock]);
        }
        at += s_b.llen[kEndBlock];
    }
    // a full flush behind every chunk but the last: an empty stored block, 00 00 FF FF after the padding
    if (!last) at += 3;
    at = (at + 7u) & ~7u;
    __syncthreads();
    if (!last) {
        if (lane == 0) { ob[(at >> 3) + 2] = 0xFF; ob[(at >> 3) + 3] = 0xFF; }
        at += 32;
    }
    const unsigned len = at >> 3;   // the payload's bytes: n + 12 at most
    __syncthreads();
    uint32_t* slot = (uint32_t*)(a.slots + (size_t)c * a.slot);
    for (unsigned i = lane; i < (len + 3) / 4 && i < (unsigned)kSlotWords; i += kLanes) slot[i] = s_out[i];

    // the IDAT's CRC over "IDAT" and the payload: a piece per lane, combined by linearity
    const unsigned piece = (len + kLanes - 1) / kLanes;
    const unsigned p0 = min((unsigned)lane * piece, len), p1 = min(p0 + piece, len);
    uint32_t reg = 0xFFFFFFFFu;
    if (lane == 0) {
        reg = crc_step(reg, 'I'); reg = crc_step(reg, 'D'); reg = crc_step(reg, 'A'); reg = crc_step(reg, 'T');
    }
    for (unsigned i = p0; i < p1; i++) reg = crc_step(reg, ob[i]);
    uint32_t crc = lane == 0 || p1 > p0 ? ~reg : 0u;
    crc = crc_mul(crc_shift(len - p1), crc);
    for (int o = 32; o > 0; o >>= 1) crc ^= __shfl_xor(crc, o);
    sa = wave_sum(sa);
    sb = wave_sum(sb);
    if (lane == 0) {
        uint32_t* m = a.meta + 4 * c;
        m[0] = len;
        m[1] = crc;
        m[2] = (uint32_t)(sa % kAdlerBase);
        m[3] = (uint32_t)(sb % kAdlerBase);
    }
}

__global__ __launch_bounds__(256) void pt_png_scan(PngArgs a)
{
    __shared__ unsigned long long sh64[4];
    __shared__ unsigned sh32[4];
    unsigned long long carry = 0, bsum = 0;
    unsigned acarry = 1;   // Adler's a before the tile's first chunk, mod 65521
    for (unsigned long long c0 = 0; c0 < a.chunks; c0 += 256) {
        const unsigned long long c = c0 + threadIdx.x;
        const bool in = c < a.chunks;
        const unsigned long long len = in ? a.meta[4 * c] + 12ull : 0ull;
        const unsigned sa = in ? a.meta[4 * c + 2] : 0u, sb = in ? a.meta[4 * c + 3] : 0u;
        unsigned long long total;
        const unsigned long long at = block_scan(len, sh64, total);
        if (in) a.off[c] = carry + at;
        carry += total;
        unsigned atotal;
        const unsigned before = (acarry + block_scan(sa, sh32, atotal)) % kAdlerBase;
        acarry = (acarry + atotal) % kAdlerBase;
        // the chunk's bytes: b grows by bytes x (a before the chunk) + the chunk's own weighted sum
        const unsigned long long bytes = c + 1 < a.chunks ? (unsigned long long)kChunk : a.stream - (a.chunks - 1) * kChunk;
        if (in) bsum += (sb + bytes * before) % kAdlerBase;
    }
    unsigned long long btotal;
    block_scan(bsum, sh64, btotal);
    if (threadIdx.x != 0) return;
    // the Adler-32 of the whole filtered stream behind the last chunk's block, in the same IDAT
    const uint32_t adler = (uint32_t)(btotal % kAdlerBase) << 16 | acarry;
    const unsigned long long lastc = a.chunks - 1;
    uint32_t* m = a.meta + 4 * lastc;
    uint8_t* p = a.slots + (size_t)lastc * a.slot + m[0];
    uint32_t reg = 0xFFFFFFFFu;
    for (int i = 0; i < 4; i++) {
        p[i] = (uint8_t)(adler >> (24 - 8 * i));
        reg = crc_step(reg, p[i]);
    }
    m[1] = crc_combine(m[1], ~reg, 4);
    m[0] += 4;
    *a.total = carry + 4;
}

__global__ __launch_bounds__(256) void pt_png_pack(PngArgs a)
{
    const unsigned long long c = blockIdx.x;
    const uint32_t len = a.meta[4 * c], crc = a.meta[4 * c + 1];
    uint8_t* out = a.out + a.off[c];
    const uint32_t* slot = (const uint32_t*)(a.slots + (size_t)c * a.slot);
    if (threadIdx.x < 4) {
        static constexpr char type[5] = "IDAT";
        out[threadIdx.x] = (uint8_t)(len >> (24 - 8 * threadIdx.x));
        out[4 + threadIdx.x] = (uint8_t)type[threadIdx.x];
        out[8 + (size_t)len + threadIdx.x] = (uint8_t)(crc >> (24 - 8 * threadIdx.x));
    }
    out += 8;
    for (unsigned i = threadIdx.x; 4 * i < len; i += 256) {
        const uint32_t w = slot[i];
        for (unsigned j = 0; j < 4 && 4 * i + j < len; j++) out[4 * i + j] = (uint8_t)(w >> (8 * j));
    }
}

}  // namespace ptp

// filter .. the IDATs' total: what runs before the host can size the output buffer
extern "C" hipError_t pt_launch_png_measure(const ptp::PngArgs* a, hipStream_t s)
{
    // (a block per chunk: 2^26 one-wave blocks are a filtered stream of a terabyte, which no device holds)
    if (a->chunks < 1 || a->chunks >= (1ull << 26) || a->height < 1) return hipErrorInvalidValue;
    const unsigned rows = (unsigned)a->height < ptp::kFilterGrid ? (unsigned)a->height : ptp::kFilterGrid;
    hipLaunchKernelGGL(ptp::pt_png_filter, dim3(rows), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(ptp::pt_png_chunk, dim3((unsigned)a->chunks), dim3(ptp::kLanes), 0, s, *a);
    hipLaunchKernelGGL(ptp::pt_png_scan, dim3(1), dim3(256), 0, s, *a);
    return hipGetLastError();
}

// ... and the IDATs into a->out, which holds the total that pass computed
extern "C" hipError_t pt_launch_png_pack(const ptp::PngArgs* a, hipStream_t s)
{
    hipLaunchKernelGGL(ptp::pt_png_pack, dim3((unsigned)a->chunks), dim3(256), 0, s, *a);
    return hipGetLastError();
}
