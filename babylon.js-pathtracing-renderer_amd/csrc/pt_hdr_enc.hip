// pt_hdr_enc.hip — a render target as a Radiance HDR picture, on the device (include/pt.h pt_target_encode_hdr; the
// format is tests/hdr_enc_ref.py). RGBE texels, every scanline coded plane by plane with the tokens Radiance's own
// writer parses its scanlines into. What host and kernels share (the conversion, the coding of a run) is
// pt_hdr_enc.h; the workspace is pt::HdrLayout (pt_plan.h).
//
//   pt_hdr_planes    a lane per texel (a bounded grid loops over them): texel -> RGBE, into the scanline's four byte
//                    planes, or, for a flat width, straight into the file.
//   pt_hdr_measure   a wave per plane (a bounded grid loops over them). Steps of 64 bytes: the run starts by a
//                    ballot, compacted into the plane's list with an mbcnt prefix. Then steps of 64 runs, a run per
//                    lane: its pieces, remainder and neighbours from the list; the loose bytes before it in its
//                    stretch by a segmented wave scan with a carry from step to step; its coded bytes; a wave scan
//                    of those. Leaves the plane's run count and length.
//   pt_hdr_scan      one block: the exclusive scan of the plane lengths (and the scanlines' four head bytes) into
//                    64-bit offsets, the total.
//   pt_hdr_emit      a wave per plane again: the same steps over the runs, and every lane writes its run's tokens
//                    (pth::run_emit); lanes 0..3 of a scanline's first plane write its head.
//
// The host writes the file's header, reads the total and copies that many bytes. Every global store is an ordinary
// vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_hdr_enc.h"
#include "pt_plan.h"

namespace pth {

static_assert(kStep == 64 && kWaves % 4 == 0, "a step is a wave's lanes; four waves to a block");

// inclusive prefix sum over the wave's 64 lanes
__device__ inline unsigned wave_scan(unsigned v, int lane)
{
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

__global__ __launch_bounds__(256) void pt_hdr_planes(HdrArgs a)
{
    const unsigned long long W = (unsigned long long)a.width, H = (unsigned long long)a.height, n = W * H;
    const bool flat = flat_width(a.width);
    const float4* tex = (const float4*)a.tex;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const unsigned long long y = i / W, x = i - y * W;   // scanline y is the target's row H - 1 - y
        const float4 t = tex[(H - 1 - y) * W + x];
        const uint32_t u = rgbe(t.x, t.y, t.z, a.scale);
        if (flat) {
            ((uint32_t*)a.out)[i] = u;   // R G B E in memory order
        } else {
            uint8_t* p = a.planes + y * 4 * W + x;
            for (int k = 0; k < 4; k++) p[k * W] = (uint8_t)(u >> (8 * k));
        }
    }
    if (flat && blockIdx.x == 0 && threadIdx.x == 0) *a.total = 4 * n;
}

// the steps over a plane's nr runs: returns its coded bytes; with Emit writes them at out
template <bool Emit>
__device__ inline unsigned walk_runs(const uint8_t* in, const uint16_t* starts, unsigned nr, int w, int lane, uint8_t* out)
{
    unsigned done = 0;   // the bytes of the runs before this step
    int carry = 0;       // the loose bytes of the stretch that is open behind the last step's last run
    for (unsigned j0 = 0; j0 < nr; j0 += kStep) {
        const unsigned j = j0 + lane;
        const bool on = j < nr;
        const RunAt r = run_at(starts, nr, w, j);   // (past the list: an empty run at w)
        // the loose bytes up to and with this run's, restarted where a run leads
        int sum = r.r.loose, cut = r.leads;
        for (int o = 1; o < 64; o <<= 1) {
            const int us = __shfl_up(sum, o), uc = __shfl_up(cut, o);
            if (lane >= o) {
                if (!cut) sum += us;
                cut |= uc;
            }
        }
        if (!cut) sum += carry;
        const int at = sum - r.r.loose;
        const unsigned bytes = on ? (unsigned)run_bytes(r.r, at, r.ends) : 0u;
        const unsigned inc = wave_scan(bytes, lane);
        if (Emit && on) run_emit(r.r, in[r.s], at, r.ends, out + done + inc - bytes);
        done += __shfl(inc, 63);
        carry = __shfl(sum, 63);
    }
    return done;
}

__global__ __launch_bounds__(256) void pt_hdr_measure(HdrArgs a)
{
    const int lane = threadIdx.x & 63, w = a.width;
    const unsigned long long planes = 4ull * (unsigned long long)a.height;
    for (unsigned long long p = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6); p < planes; p += (unsigned long long)gridDim.x * 4) {
        const uint8_t* in = a.planes + p * (unsigned long long)w;
        uint16_t* starts = a.starts + p * (unsigned long long)w;
        unsigned nr = 0;
        for (int i0 = 0; i0 < w; i0 += kStep) {
            const int i = i0 + lane;
            const bool start = i < w && (i == 0 || in[i] != in[i - 1]);
            const unsigned long long m = __ballot(start);
            const unsigned before = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (start) starts[nr + before] = (uint16_t)i;   // (at most one run per byte: below w)
            nr += (unsigned)__popcll(m);
        }
        // The list is read back by other lanes of this same wave, never by another wave (a wave owns its plane):
        // the fence completes the wave's stores before its loads issue, and both go through this CU's cache. A
        // plane shared between waves would need a barrier here.
        __threadfence_block();
        const unsigned len = walk_runs<false>(in, starts, nr, w, lane, nullptr);
        if (lane == 0) { a.runs[p] = nr; a.len[p] = len; }
    }
}

__global__ __launch_bounds__(256) void pt_hdr_scan(HdrArgs a)
{
    __shared__ unsigned long long sh[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long planes = 4ull * (unsigned long long)a.height;
    unsigned long long carry = 0;
    for (unsigned long long p0 = 0; p0 < planes; p0 += 256) {
        const unsigned long long p = p0 + threadIdx.x;
        const unsigned long long v = p < planes ? a.len[p] + ((p & 3) == 0 ? 4ull : 0ull) : 0ull;
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
        if (p < planes) a.off[p] = carry + base + inc - v;
        carry += total;
    }
    if (threadIdx.x == 0) *a.total = carry;
}

__global__ __launch_bounds__(256) void pt_hdr_emit(HdrArgs a)
{
    const int lane = threadIdx.x & 63, w = a.width;
    const unsigned long long planes = 4ull * (unsigned long long)a.height;
    for (unsigned long long p = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6); p < planes; p += (unsigned long long)gridDim.x * 4) {
        uint8_t* out = a.out + a.off[p];
        if ((p & 3) == 0) {   // the scanline's head: 02 02 and the width, big-endian
            if (lane < 4) out[lane] = lane < 2 ? (uint8_t)2 : lane == 2 ? (uint8_t)(w >> 8) : (uint8_t)(w & 255);
            out += 4;
        }
        walk_runs<true>(a.planes + p * (unsigned long long)w, a.starts + p * (unsigned long long)w, a.runs[p], w, lane, out);
    }
}

}  // namespace pth

// The whole encode of a->tex into a->out, which holds pt::HdrLayout::out_max bytes, and the length into a->total:
// nothing here needs a length from the host.
extern "C" hipError_t pt_launch_hdr_encode(const pth::HdrArgs* a, hipStream_t s)
{
    if (a->width < 1 || a->height < 1) return hipErrorInvalidValue;
    const unsigned long long n = (unsigned long long)a->width * (unsigned long long)a->height;
    const unsigned long long tb = (n + 255) / 256;
    hipLaunchKernelGGL(pth::pt_hdr_planes, dim3((unsigned)(tb < pth::kPlaneGrid ? tb : pth::kPlaneGrid)), dim3(256), 0, s, *a);
    if (pth::flat_width(a->width)) return hipGetLastError();
    const unsigned long long pb = (unsigned long long)a->height;   // 4 planes, 4 waves to a block
    const dim3 grid((unsigned)(pb < pth::kWaves / 4 ? pb : pth::kWaves / 4));
    hipLaunchKernelGGL(pth::pt_hdr_measure, grid, dim3(256), 0, s, *a);
    hipLaunchKernelGGL(pth::pt_hdr_scan, dim3(1), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(pth::pt_hdr_emit, grid, dim3(256), 0, s, *a);
    return hipGetLastError();
}
