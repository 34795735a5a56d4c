// pt_exr_enc.hip — render targets as a multi-channel OpenEXR file, on the device (include/pt.h
// pt_targets_encode_exr; the format is tests/exr_enc_ref.py). Named HALF / FLOAT channels, each one component of one
// RGBA32F target times a scale; scanline blocks raw (NONE) or as zlib streams (ZIPS, ZIP) whose deflate blocks are
// the bytes zlib 1.2.11 writes under Z_RLE at level 6 with a full flush behind every 16,320-byte piece, exactly as
// pt_canvas_encode_png's chunks. What host and kernels share is pt_exr_enc.h and, for the coder (the trees, the
// block-size rule, the tokens, the packer), pt_png_enc.h; the workspace is pt::ExrLayout (pt_plan.h).
//
//   pt_exr_convert   a lane per texel: one float4 load per texture the channels name (channels that share a texture
//                    share the load), the samples into the block's raw bytes in 16-bit stores. Under NONE the raw
//                    bytes, the chunk heads and the offset table go straight into the file: nothing else runs.
//   pt_exr_predict   a lane per 4 predicted bytes: the reorder and the delta, pointwise from the raw bytes.
//   pt_exr_piece     a one-wave block per (block, piece), pt_png_chunk's scheme: 255 bytes per lane, the piece and its
//                    deflate bytes in LDS, the counts by LDS atomics, the trees and the block type by lane 0, the
//                    tokens by a prefix sum of the lanes' bit counts. `first` and `last` are per block; it leaves
//                    the piece's length and Adler sums.
//   pt_exr_scan      one block, a lane per block of scanlines: the pieces' lengths and places, the Adler-32, the
//                    stream-or-raw choice; then the exclusive scan of the chunk sizes, the offset table, the total.
//   pt_exr_pack      a block per (block, piece): the chunk's head, the piece's deflate bytes (the Adler-32 behind the
//                    last) or its share of the raw bytes into place.
//
// The host writes the magic and the header, reads the total and copies that many bytes. Every global store is an
// ordinary vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_exr_enc.h"
#include "pt_plan.h"

namespace pte {

using namespace ptp;

static_assert(kPiece == (int)pt::kPngChunk && kPiece % 64 == 0 && pt::kPngSlot % 4 == 0, "");
constexpr int kSlotWords = (int)(pt::kPngSlot / 4);

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

__device__ inline void store_le(uint8_t* p, unsigned long long v, int bytes)
{
    for (int i = 0; i < bytes; i++) p[i] = (uint8_t)(v >> (8 * i));
}

__global__ __launch_bounds__(256) void pt_exr_convert(ExrArgs a)
{
    const unsigned long long W = (unsigned long long)a.width, H = (unsigned long long)a.height;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= W * H) return;
    const unsigned long long y = i / W, x = i - y * W;   // scanline y is the targets' row H - 1 - y
    const unsigned long long texel = (H - 1 - y) * W + x;
    uint8_t* row;
    if (a.compression == kNone) {
        uint8_t* chunk = a.out + 8 * H + y * (8 + a.line);
        if (x == 0) {
            store_le(a.out + 8 * y, a.header + 8 * H + y * (8 + a.line), 8);
            store_le(chunk, y, 4);
            store_le(chunk + 4, a.line, 4);
        }
        if (i == 0) *a.total = 8 * H + H * (8 + a.line);
        row = chunk + 8;
    } else {
        const unsigned long long b = y / (unsigned long long)a.lines;
        row = a.raw + b * a.stride + (y - b * (unsigned long long)a.lines) * a.line;
    }
    const float* last = nullptr;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = 0; c < a.channels; c++) {
        const ExrChan& ch = a.ch[c];
        if (ch.tex != last) {   // (uniform over the grid)
            t = ((const float4*)ch.tex)[texel];
            last = ch.tex;
        }
        const float v = ch.component == 0 ? t.x : ch.component == 1 ? t.y : ch.component == 2 ? t.z : t.w;
        const uint32_t s = sample_bits(__float_as_uint(v), ch.scale, ch.type);
        // a scanline's bytes and a channel's start in it are even: 16-bit stores are aligned, 32-bit ones need not be
        uint16_t* p = (uint16_t*)(row + ch.at + x * (unsigned long long)sample_bytes(ch.type));
        p[0] = (uint16_t)s;
        if (ch.type != kHalf) p[1] = (uint16_t)(s >> 16);
    }
}

__global__ __launch_bounds__(256) void pt_exr_predict(ExrArgs a)
{
    const unsigned long long words = a.stride / 4;   // of a block
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.blocks * words) return;
    const unsigned long long b = i / words, w = i - b * words, n = block_bytes(a, b);
    if (4 * w >= n) return;
    const uint8_t* r = a.raw + b * a.stride;
    uint32_t v = 0;
    for (unsigned k = 0; k < 4; k++)
        if (4 * w + k < n) v |= (uint32_t)predicted(r, n, 4 * w + k) << (8 * k);
    ((uint32_t*)(a.pred + b * a.stride))[w] = v;
}

// the lanes' walk over the tokens that start in [lo, hi) of the piece `in[0..n)`: s0 the start of the run that
// holds lo, nb the first run boundary at or after hi (pt_png_enc.hip's)
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

__global__ __launch_bounds__(64) void pt_exr_piece(ExrArgs a)
{
    __shared__ uint32_t s_in[kPiece / 4];
    __shared__ uint32_t s_out[kSlotWords];
    __shared__ unsigned s_cnt[kLCodes + 1];    // the literal / length counts, and the matches
    __shared__ int s_first[kLanes], s_last[kLanes];
    __shared__ unsigned s_at;
    __shared__ Block s_b;

    const unsigned long long g = blockIdx.x, blk = g / (unsigned)a.pieces;
    const unsigned k = (unsigned)(g - blk * (unsigned)a.pieces);
    const unsigned long long nblk = block_bytes(a, blk);
    const unsigned pieces = block_pieces(nblk);
    if (k >= pieces) return;   // (the last block may have fewer pieces; uniform over the wave)
    const int lane = threadIdx.x;
    const unsigned long long base = (unsigned long long)k * kPiece;
    const unsigned n = (unsigned)(nblk - base < (unsigned long long)kPiece ? nblk - base : (unsigned long long)kPiece);
    const bool first = k == 0, last = k + 1 == pieces;
    const uint32_t* gin = (const uint32_t*)(a.pred + blk * a.stride + base);   // (blocks and pieces start on 64 B)
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
                const unsigned j = at >> 5;   // (a header is below 5000 bits)
                s_out[j] |= w[0];
                s_out[j + 1] |= w[1];
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
            const unsigned j = pos >> 5;
            for (int q = 0; q < 3; q++)
                if (w[q] && j + q < (unsigned)kSlotWords) atomicOr(&s_out[j + q], w[q]);
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
    // a full flush behind every piece but the block's last: an empty stored block, 00 00 FF FF after the padding
    if (!last) at += 3;
    at = (at + 7u) & ~7u;
    __syncthreads();
    if (!last) {
        if (lane == 0) { ob[(at >> 3) + 2] = 0xFF; ob[(at >> 3) + 3] = 0xFF; }
        at += 32;
    }
    const unsigned len = at >> 3;   // the piece's deflate bytes: n + 12 at most
    __syncthreads();
    uint32_t* slot = (uint32_t*)(a.slots + (size_t)g * pt::kPngSlot);
    for (unsigned i = lane; i < (len + 3) / 4 && i < (unsigned)kSlotWords; i += kLanes) slot[i] = s_out[i];
    sa = wave_sum(sa);
    sb = wave_sum(sb);
    if (lane == 0) {
        uint32_t* m = a.meta + 4 * g;
        m[0] = len;
        m[1] = 0u;
        m[2] = (uint32_t)(sa % kAdlerBase);
        m[3] = (uint32_t)(sb % kAdlerBase);
    }
}

__global__ __launch_bounds__(256) void pt_exr_scan(ExrArgs a)
{
    __shared__ unsigned long long sh[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long carry = 8 * a.blocks;   // the offset table comes first
    for (unsigned long long b0 = 0; b0 < a.blocks; b0 += 256) {
        const unsigned long long b = b0 + threadIdx.x;
        const bool in = b < a.blocks;
        unsigned long long v = 0;
        if (in) {
            const unsigned long long n = block_bytes(a, b);
            const unsigned pieces = block_pieces(n);
            uint32_t* m = a.meta + 4 * b * (unsigned)a.pieces;
            unsigned long long stream = 0;
            uint32_t aa = 1, ab = 0;
            for (unsigned k = 0; k < pieces; k++, m += 4) {
                m[1] = (uint32_t)stream;
                stream += m[0];
                const unsigned long long at = (unsigned long long)k * kPiece;
                adler_piece(aa, ab, m[2], m[3], (uint32_t)(n - at < (unsigned long long)kPiece ? n - at : (unsigned long long)kPiece));
            }
            stream += 4;   // the Adler-32
            const bool keep = keeps_stream(stream, n);
            uint32_t* bm = a.bmeta + 4 * b;
            bm[0] = (uint32_t)(keep ? stream : n);
            bm[1] = keep ? 1u : 0u;
            bm[2] = ab << 16 | aa;
            v = 8 + bm[0];
        }
        unsigned long long inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        __syncthreads();   // (the previous tile's reads of sh)
        if (lane == 63) sh[wv] = inc;
        __syncthreads();
        unsigned long long base = 0, total = 0;
        for (int i = 0; i < 4; i++) {
            if (i < wv) base += sh[i];
            total += sh[i];
        }
        if (in) {
            const unsigned long long at = carry + base + inc - v;
            a.off[b] = at;
            ((unsigned long long*)a.out)[b] = a.header + at;   // (out starts on 256 B)
        }
        carry += total;
    }
    if (threadIdx.x == 0) *a.total = carry;
}

__global__ __launch_bounds__(256) void pt_exr_pack(ExrArgs a)
{
    const unsigned long long g = blockIdx.x, blk = g / (unsigned)a.pieces;
    const unsigned k = (unsigned)(g - blk * (unsigned)a.pieces);
    const unsigned long long nblk = block_bytes(a, blk);
    const unsigned pieces = block_pieces(nblk);
    if (k >= pieces) return;
    const uint32_t* bm = a.bmeta + 4 * blk;
    const uint32_t size = bm[0], adler = bm[2];
    uint8_t* chunk = a.out + a.off[blk];
    if (k == 0 && threadIdx.x < 8) {
        const unsigned long long head = blk * (unsigned long long)a.lines | (unsigned long long)size << 32;
        chunk[threadIdx.x] = (uint8_t)(head >> (8 * threadIdx.x));
    }
    uint8_t* data = chunk + 8;
    if (bm[1]) {
        const uint32_t* m = a.meta + 4 * g;
        const uint32_t len = m[0];
        uint8_t* out = data + m[1];
        const uint32_t* slot = (const uint32_t*)(a.slots + (size_t)g * pt::kPngSlot);
        for (unsigned i = threadIdx.x; 4 * i < len; i += 256) {
            const uint32_t w = slot[i];
            for (unsigned j = 0; j < 4 && 4 * i + j < len; j++) out[4 * i + j] = (uint8_t)(w >> (8 * j));
        }
        if (k + 1 == pieces && threadIdx.x < 4) out[len + threadIdx.x] = (uint8_t)(adler >> (24 - 8 * threadIdx.x));
    } else {
        const unsigned long long base = (unsigned long long)k * kPiece;
        const unsigned n = (unsigned)(nblk - base < (unsigned long long)kPiece ? nblk - base : (unsigned long long)kPiece);
        const uint32_t* r = (const uint32_t*)(a.raw + blk * a.stride + base);
        uint8_t* out = data + base;
        for (unsigned i = threadIdx.x; 4 * i < n; i += 256) {
            const uint32_t w = r[i];
            for (unsigned j = 0; j < 4 && 4 * i + j < n; j++) out[4 * i + j] = (uint8_t)(w >> (8 * j));
        }
    }
}

}  // namespace pte

// The whole encode of a->ch into a->out, which holds pt::ExrLayout::out_max bytes, and the length into a->total:
// nothing here needs a length from the host. Every grid is exact, so a file whose texels, words or pieces do not fit
// a grid of 2^31 - 1 blocks is refused.
extern "C" hipError_t pt_launch_exr_encode(const pte::ExrArgs* a, hipStream_t s)
{
    if (a->width < 1 || a->height < 1 || a->channels < 1 || a->channels > pte::kChannelsMax) return hipErrorInvalidValue;
    const unsigned long long kGridMax = 0x7FFFFFFFull;
    const unsigned long long texels = (unsigned long long)a->width * (unsigned long long)a->height;
    const unsigned long long tb = (texels + 255) / 256;
    // (a block's bytes and a chunk's size are 32-bit fields of the file)
    if (tb > kGridMax || a->lines < 1 || (unsigned long long)a->lines * a->line >= (1ull << 31)) return hipErrorInvalidValue;
    if (a->compression == pte::kNone) {
        hipLaunchKernelGGL(pte::pt_exr_convert, dim3((unsigned)tb), dim3(256), 0, s, *a);
        return hipGetLastError();
    }
    const unsigned long long wb = (a->blocks * (a->stride / 4) + 255) / 256;
    const unsigned long long pieces = a->blocks * (unsigned long long)a->pieces;
    if (wb > kGridMax || pieces < 1 || pieces > kGridMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pte::pt_exr_convert, dim3((unsigned)tb), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(pte::pt_exr_predict, dim3((unsigned)wb), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(pte::pt_exr_piece, dim3((unsigned)pieces), dim3(pte::kLanes), 0, s, *a);
    hipLaunchKernelGGL(pte::pt_exr_scan, dim3(1), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(pte::pt_exr_pack, dim3((unsigned)pieces), dim3(256), 0, s, *a);
    return hipGetLastError();
}
