// pt_denoise.hip — the edge-avoiding à-trous denoiser over the feature buffers (include/pt.h pt_denoise;
// the formula, operation by operation, is INTEGRATION.md "Denoising" and tests/denoise_ref.py).
//
//   pt_denoise_prep         per pixel: beauty, normal + id and albedo + weight (48 B) -> two float4 planes,
//                           colour = {d.xyz, id} and guide = {n.xyz, valid} (32 B), so that a tap costs 32 B.
//   pt_denoise_pass<S,LAST> one 5x5 pass at tap spacing S = 1, 2, 4 from LDS: a 256-thread block filters a 16x16
//                           tile from its (16 + 4S)^2 neighbourhood of both planes (12.5 / 18 / 32 KiB), each texel
//                           read from L2 once instead of by up to 25 taps (reuse 16x / 11x / 6x). A fixed grid walks
//                           the tiles gridDim.x apart with the next tile's neighbourhood in flight in registers, as
//                           pt_output does (one LDS buffer, so two barriers per tile).
//   pt_denoise_far<LAST>    the pass at S = 8, 16 through L2: a tile's neighbourhood would be 48^2 / 80^2 texels for
//                           256 pixels (reuse 2.8x / 1x), so every lane fetches its own 25 taps; a block is 64 x 4
//                           pixels, a wave one row of 64: 1 KiB contiguous per tap.
// LAST: the pass writes dst, remodulated and back in the accumulation's scale, instead of the next colour plane.
// Texels outside the image are staged as invalid (guide.w = 0): they are skipped like any invalid tap.
// Every access is one float4 per lane, consecutive lanes along a row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_args.h"
#include "pt_glsl.h"

using namespace ptg;

namespace pt {

__global__ __launch_bounds__(256) void pt_denoise_prep(DenoiseArgs a, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 b = a.beauty[i], ni = a.normal_id[i], aw = a.albedo_weight[i];
    const float w = aw.w;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, ni.w), g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (w > 0.0f) {
        const float iw = 1.0f / w;
        g = make_float4(ni.x * iw, ni.y * iw, ni.z * iw, 1.0f);
        c.x = b.x * iw; c.y = b.y * iw; c.z = b.z * iw;
        if (a.demodulate) {
            c.x = c.x / gmax(aw.x * iw, 1e-3f);
            c.y = c.y / gmax(aw.y * iw, 1e-3f);
            c.z = c.z / gmax(aw.z * iw, 1e-3f);
        }
    }
    a.colour[0][i] = c;
    a.guide[i] = g;
}

// the filtered colour of the pixel whose planes hold (cp, gp); at(dx, dy, cq, gq) fetches the tap at
// p + S * (dx, dy), invalid (gq.w == 0) outside the image. Taps in row-major order, one IEEE operation each.
template <class F>
PT_D float4 denoisePixel(const float4 cp, const float4 gp, float inv_n, float inv_c, F at)
{
    constexpr float K[3] = { 0.375f, 0.25f, 0.0625f };
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, ws = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            float4 cq, gq;
            at(dx, dy, cq, gq);
            if (gq.w != 0.0f && !(cq.w != cp.w)) {
                const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
                const float dn2 = (nx * nx + ny * ny) + nz * nz;
                const float cx = cp.x - cq.x, cy = cp.y - cq.y, cz = cp.z - cq.z;
                const float dc2 = (cx * cx + cy * cy) + cz * cz;
                const float e = dn2 * inv_n + dc2 * inv_c;
                const float k = K[dx < 0 ? -dx : dx] * K[dy < 0 ? -dy : dy];
                const float wt = k * gexp(-e);
                sx += cq.x * wt; sy += cq.y * wt; sz += cq.z * wt;
                ws += wt;
            }
        }
    }
    if (gp.w == 0.0f) return make_float4(0.0f, 0.0f, 0.0f, cp.w);
    return make_float4(sx / ws, sy / ws, sz / ws, cp.w);
}

// what the last pass writes for a pixel of filtered colour d: remodulated, times the weight; an invalid pixel 0
PT_D float4 denoiseFinal(const DenoiseArgs& a, long long i, const float4 d, bool valid)
{
    const float4 aw = a.albedo_weight[i];
    const float w = aw.w;
    if (!valid) return make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    float rx = d.x, ry = d.y, rz = d.z;
    if (a.demodulate) {
        const float iw = 1.0f / w;
        rx = rx * gmax(aw.x * iw, 1e-3f);
        ry = ry * gmax(aw.y * iw, 1e-3f);
        rz = rz * gmax(aw.z * iw, 1e-3f);
    }
    return make_float4(rx * w, ry * w, rz * w, 1.0f);
}

template <int S, bool LAST>
__global__ __launch_bounds__(256) void pt_denoise_pass(DenoiseArgs a, const float4* in, float4* out, float inv_c,
                                                       int tiles_x, int ntiles)
{
    constexpr int R = 16 + 4 * S, N = R * R, NF = (N + 255) / 256;
    __shared__ float4 sc[N], sg[N];
    const int tid = threadIdx.x;
    const int lx = tid & 15, ly = tid >> 4;
    float4 fc[NF], fg[NF];
    auto load = [&](int t) {
        const int x0 = (t % tiles_x) * 16 - 2 * S, y0 = (t / tiles_x) * 16 - 2 * S;
#pragma unroll
        for (int j = 0; j < NF; j++) {
            const int k = tid + 256 * j;
            const int x = x0 + k % R, y = y0 + k / R;
            fc[j] = fg[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (k < N && x >= 0 && y >= 0 && x < a.width && y < a.height) {
                const long long i = (long long)y * a.width + x;
                fc[j] = in[i];
                fg[j] = a.guide[i];
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < NF; j++) {
            const int k = tid + 256 * j;
            if (k < N) { sc[k] = fc[j]; sg[k] = fg[j]; }
        }
    };
    int t = (int)blockIdx.x;
    if (t >= ntiles) return;
    load(t);
    store();
    __syncthreads();
    for (;;) {
        const int tn = t + (int)gridDim.x;
        if (tn < ntiles) load(tn);
        const int x = (t % tiles_x) * 16 + lx, y = (t / tiles_x) * 16 + ly;
        if (x < a.width && y < a.height) {
            const int p = (ly + 2 * S) * R + lx + 2 * S;
            const float4 cp = sc[p], gp = sg[p];
            const float4 d = denoisePixel(cp, gp, a.inv_n, inv_c, [&](int dx, int dy, float4& cq, float4& gq) {
                cq = sc[p + (dy * R + dx) * S];
                gq = sg[p + (dy * R + dx) * S];
            });
            const long long i = (long long)y * a.width + x;
            if (LAST) a.dst[i] = denoiseFinal(a, i, d, gp.w != 0.0f);
            else out[i] = d;
        }
        if (tn >= ntiles) break;
        __syncthreads();
        store();
        __syncthreads();
        t = tn;
    }
}

template <bool LAST>
__global__ __launch_bounds__(256) void pt_denoise_far(DenoiseArgs a, const float4* in, float4* out, float inv_c, int s)
{
    const int x = (int)blockIdx.x * 64 + (threadIdx.x & 63), y = (int)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    const long long i = (long long)y * a.width + x;
    const float4 cp = in[i], gp = a.guide[i];
    const float4 d = denoisePixel(cp, gp, a.inv_n, inv_c, [&](int dx, int dy, float4& cq, float4& gq) {
        const int qx = x + dx * s, qy = y + dy * s;
        cq = gq = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (qx >= 0 && qy >= 0 && qx < a.width && qy < a.height) {
            const long long q = (long long)qy * a.width + qx;
            cq = in[q];
            gq = a.guide[q];
        }
    });
    if (LAST) a.dst[i] = denoiseFinal(a, i, d, gp.w != 0.0f);
    else out[i] = d;
}

template <int S>
static void launch_pass(const DenoiseArgs& a, bool last, const float4* in, float4* out, float inv_c, hipStream_t s)
{
    const int tx = (a.width + 15) / 16, ntiles = tx * ((a.height + 15) / 16);
    // persistent blocks as pt_output's: about four tiles each, 4096..8192
    const int blocks = ntiles / 4 < 4096 ? 4096 : ntiles / 4 > 8192 ? 8192 : ntiles / 4;
    const dim3 grid(ntiles < blocks ? ntiles : blocks);
    if (last) hipLaunchKernelGGL((pt_denoise_pass<S, true>), grid, dim3(256), 0, s, a, in, out, inv_c, tx, ntiles);
    else hipLaunchKernelGGL((pt_denoise_pass<S, false>), grid, dim3(256), 0, s, a, in, out, inv_c, tx, ntiles);
}

} // namespace pt

// The whole filter on stream s: prep, then a->iterations passes; pass i reads colour[i & 1] and writes the other
// plane, the last one dst. The arguments are checked by the caller (dev_denoise).
extern "C" hipError_t pt_launch_denoise(const pt::DenoiseArgs* a, hipStream_t s)
{
    const long long n = (long long)a->width * a->height;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pt::pt_denoise_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, *a, n);
    for (int i = 0; i < a->iterations; i++) {
        const bool last = i == a->iterations - 1;
        const float4* in = a->colour[i & 1];
        float4* out = a->colour[(i & 1) ^ 1];
        const float inv_c = a->inv_c0 * (float)(1 << (2 * i));   // exact: the colour sigma halves every pass
        switch (i) {
        case 0: pt::launch_pass<1>(*a, last, in, out, inv_c, s); break;
        case 1: pt::launch_pass<2>(*a, last, in, out, inv_c, s); break;
        case 2: pt::launch_pass<4>(*a, last, in, out, inv_c, s); break;
        default: {
            const dim3 grid((a->width + 63) / 64, (a->height + 3) / 4);
            if (last) hipLaunchKernelGGL(pt::pt_denoise_far<true>, grid, dim3(256), 0, s, *a, in, out, inv_c, 1 << i);
            else hipLaunchKernelGGL(pt::pt_denoise_far<false>, grid, dim3(256), 0, s, *a, in, out, inv_c, 1 << i);
        }
        }
    }
    return hipGetLastError();
}
