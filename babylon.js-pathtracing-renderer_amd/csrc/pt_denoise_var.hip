// pt_denoise_var.hip — the variance-guided à-trous denoiser (include/pt.h pt_denoise_variance; the formula,
// operation by operation, is INTEGRATION.md "Denoising" and tests/denoise_var_ref.py). pt_denoise's filter with the
// colour edge-stop replaced by a luminance one that scales with each pixel's own variance, estimated from the
// accumulated luminance moments (pt_set_moment_target) and filtered along with the colour.
//
//   pt_dvar_prep            a 256-thread block per 16x16 tile: stages the 22x22 neighbourhood of {moments.x,
//                           moments.y, valid ? moments.w : 0, id} in LDS (7.6 KiB) for the 7x7 spatial estimate, and
//                           writes colour = {d.xyz, id}, guide = {n.xyz, valid} and var (36 B per pixel).
//   pt_dvar_pass<S,LAST>    one 5x5 pass at tap spacing S = 1, 2, 4 from LDS, tiled as pt_denoise_pass: the
//                           (16 + 4S)^2 neighbourhood of the three planes (14 / 20.3 / 36 KiB), persistent blocks, the
//                           next tile in flight in registers. The centre's 3x3 variance mean at spacing 1 reads the
//                           same staged neighbourhood (its +-1 lies inside the 2S halo).
//   pt_dvar_far<LAST>       the pass at S = 8, 16 through L2, as pt_denoise_far: every lane fetches its own taps.
// LAST: the pass writes dst, remodulated and in the accumulation's scale, and no variance.
// Texels outside the image are staged as invalid (guide.w = 0). Every access is one float4 (or, for the variance
// plane and a neighbour's id / valid word, one float) per lane, consecutive lanes along a row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_args.h"
#include "pt_glsl.h"

using namespace ptg;

namespace pt {

PT_D float dvarLum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

__global__ __launch_bounds__(256) void pt_dvar_prep(DenoiseVarArgs a, int tiles_x)
{
    constexpr int R = 22, N = R * R;
    __shared__ float4 sm[N];
    const int tid = threadIdx.x;
    const int tx = (int)blockIdx.x % tiles_x, ty = (int)blockIdx.x / tiles_x;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int k = tid + 256 * j;
        const int x = tx * 16 - 3 + k % R, y = ty * 16 - 3 + k / R;
        float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (k < N && x >= 0 && y >= 0 && x < a.width && y < a.height) {
            const long long i = (long long)y * a.width + x;
            const float4 mo = a.moments[i];
            const float w = ((const float*)&a.albedo_weight[i])[3];
            const float id = ((const float*)&a.normal_id[i])[3];
            m = make_float4(mo.x, mo.y, (w > 0.0f && mo.w > 0.0f) ? mo.w : 0.0f, id);
        }
        if (k < N) sm[k] = m;
    }
    __syncthreads();
    const int lx = tid & 15, ly = tid >> 4;
    const int x = tx * 16 + lx, y = ty * 16 + ly;
    if (x >= a.width || y >= a.height) return;
    const long long i = (long long)y * a.width + x;
    const int p = (ly + 3) * R + lx + 3;
    const float4 b = a.beauty[i], ni = a.normal_id[i], aw = a.albedo_weight[i];
    const float4 mp = sm[p];
    const float w = aw.w, mw = mp.z;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, ni.w), g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float var = 0.0f;
    if (mw > 0.0f) {   // valid: w > 0 && moments.w > 0
        const float iw = 1.0f / w;
        g = make_float4(ni.x * iw, ni.y * iw, ni.z * iw, 1.0f);
        c.x = b.x * iw; c.y = b.y * iw; c.z = b.z * iw;
        const float dx_ = gmax(aw.x * iw, 1e-3f), dy_ = gmax(aw.y * iw, 1e-3f), dz_ = gmax(aw.z * iw, 1e-3f);
        if (a.demodulate) { c.x = c.x / dx_; c.y = c.y / dy_; c.z = c.z / dz_; }
        // the temporal estimate, from this pixel's own moments
        const float mu1 = mp.x / mw, mu2 = mp.y / mw;
        float vt = mu2 - mu1 * mu1;
        vt = vt > 0.0f ? vt : 0.0f;
        // the spatial one, over the kept taps of the 7x7 window (row-major, the centre included)
        float S1 = 0.0f, S2 = 0.0f, SW = 0.0f;
#pragma unroll
        for (int dy = -3; dy <= 3; dy++) {
#pragma unroll
            for (int dx = -3; dx <= 3; dx++) {
                const float4 q = sm[p + dy * R + dx];
                if (q.z > 0.0f && !(q.w != mp.w)) { S1 += q.x; S2 += q.y; SW += q.z; }
            }
        }
        const float s1 = S1 / SW, s2 = S2 / SW;
        float vs = s2 - s1 * s1;
        vs = vs > 0.0f ? vs : 0.0f;
        const float v = mw < 4.0f ? vs : vt;
        var = v / mw;
        if (a.demodulate) {
            const float l = dvarLum(dx_, dy_, dz_);
            var = var / (l * l);
        }
    }
    a.colour[0][i] = c;
    a.guide[i] = g;
    a.var[0][i] = var;
}

struct DvarOut { float4 d; float var; };

// the filtered colour and variance of the pixel whose planes hold (cp, gp). at(dx, dy, cq, gq, vq) fetches the tap
// at p + S * (dx, dy), near(dx, dy, idq, validq, vq) the one at p + (dx, dy); both invalid outside the image. Taps
// in row-major order, one IEEE operation each.
template <class F, class G>
PT_D DvarOut dvarPixel(const float4 cp, const float4 gp, float inv_n, float sl2, F at, G near)
{
    constexpr float K[3] = { 0.375f, 0.25f, 0.0625f };
    constexpr float B[2] = { 0.5f, 0.25f };
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            float idq, validq, vq;
            near(dx, dy, idq, validq, vq);
            if (validq != 0.0f && !(idq != cp.w)) {
                const float k = B[dx < 0 ? -dx : dx] * B[dy < 0 ? -dy : dy];
                gs += k * vq;
                gw += k;
            }
        }
    }
    const float gv = gs / gw;
    const float inv_l = 1.0f / (sl2 * gv + 1e-8f);
    const float lp = dvarLum(cp.x, cp.y, cp.z);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, ws = 0.0f, sv = 0.0f;
    // (the rows are not unrolled: with all 25 taps' LDS reads hoisted the S = 4 pass took 149 VGPRs, 3 waves per
    // SIMD; a row at a time it takes 105 and 4, and measured 2-3 % faster. ky * K[|dx|] is the same exact product.)
#pragma unroll 1
    for (int dy = -2; dy <= 2; dy++) {
        const float ky = dy == 0 ? K[0] : (dy == 1 || dy == -1) ? K[1] : K[2];
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            float4 cq, gq;
            float vq;
            at(dx, dy, cq, gq, vq);
            if (gq.w != 0.0f && !(cq.w != cp.w)) {
                const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
                const float dn2 = (nx * nx + ny * ny) + nz * nz;
                const float dl = lp - dvarLum(cq.x, cq.y, cq.z);
                const float e = dn2 * inv_n + (dl * dl) * inv_l;
                const float k = K[dx < 0 ? -dx : dx] * ky;
                const float wt = k * gexp(-e);
                sx += cq.x * wt; sy += cq.y * wt; sz += cq.z * wt;
                ws += wt;
                sv += (wt * wt) * vq;
            }
        }
    }
    DvarOut o;
    if (gp.w == 0.0f) { o.d = make_float4(0.0f, 0.0f, 0.0f, cp.w); o.var = 0.0f; return o; }
    o.d = make_float4(sx / ws, sy / ws, sz / ws, cp.w);
    o.var = sv / (ws * ws);
    return o;
}

// what the last pass writes for a pixel of filtered colour d: remodulated, times the weight; an invalid pixel 0
PT_D float4 dvarFinal(const DenoiseVarArgs& a, long long i, const float4 d, bool valid)
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
__global__ __launch_bounds__(256) void pt_dvar_pass(DenoiseVarArgs a, const float4* in, float4* out, const float* vin,
                                                    float* vout, int tiles_x, int ntiles)
{
    constexpr int R = 16 + 4 * S, N = R * R, NF = (N + 255) / 256;
    __shared__ float4 sc[N], sg[N];
    __shared__ float sv[N];
    const int tid = threadIdx.x;
    const int lx = tid & 15, ly = tid >> 4;
    float4 fc[NF], fg[NF];
    float fv[NF];
    auto load = [&](int t) {
        const int x0 = (t % tiles_x) * 16 - 2 * S, y0 = (t / tiles_x) * 16 - 2 * S;
#pragma unroll
        for (int j = 0; j < NF; j++) {
            const int k = tid + 256 * j;
            const int x = x0 + k % R, y = y0 + k / R;
            fc[j] = fg[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            fv[j] = 0.0f;
            if (k < N && x >= 0 && y >= 0 && x < a.width && y < a.height) {
                const long long i = (long long)y * a.width + x;
                fc[j] = in[i];
                fg[j] = a.guide[i];
                fv[j] = vin[i];
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < NF; j++) {
            const int k = tid + 256 * j;
            if (k < N) { sc[k] = fc[j]; sg[k] = fg[j]; sv[k] = fv[j]; }
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
            const DvarOut o = dvarPixel(cp, gp, a.inv_n, a.sl2,
                [&](int dx, int dy, float4& cq, float4& gq, float& vq) {
                    const int q = p + (dy * R + dx) * S;
                    cq = sc[q]; gq = sg[q]; vq = sv[q];
                },
                [&](int dx, int dy, float& idq, float& validq, float& vq) {
                    const int q = p + dy * R + dx;
                    idq = sc[q].w; validq = sg[q].w; vq = sv[q];
                });
            const long long i = (long long)y * a.width + x;
            if (LAST) a.dst[i] = dvarFinal(a, i, o.d, gp.w != 0.0f);
            else { out[i] = o.d; vout[i] = o.var; }
        }
        if (tn >= ntiles) break;
        __syncthreads();
        store();
        __syncthreads();
        t = tn;
    }
}

template <bool LAST>
__global__ __launch_bounds__(256) void pt_dvar_far(DenoiseVarArgs a, const float4* in, float4* out, const float* vin,
                                                   float* vout, int s)
{
    const int x = (int)blockIdx.x * 64 + (threadIdx.x & 63), y = (int)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    const long long i = (long long)y * a.width + x;
    const float4 cp = in[i], gp = a.guide[i];
    const DvarOut o = dvarPixel(cp, gp, a.inv_n, a.sl2,
        [&](int dx, int dy, float4& cq, float4& gq, float& vq) {
            const int qx = x + dx * s, qy = y + dy * s;
            cq = gq = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            vq = 0.0f;
            if (qx >= 0 && qy >= 0 && qx < a.width && qy < a.height) {
                const long long q = (long long)qy * a.width + qx;
                cq = in[q];
                gq = a.guide[q];
                vq = vin[q];
            }
        },
        [&](int dx, int dy, float& idq, float& validq, float& vq) {
            const int qx = x + dx, qy = y + dy;
            idq = validq = vq = 0.0f;
            if (qx >= 0 && qy >= 0 && qx < a.width && qy < a.height) {
                const long long q = (long long)qy * a.width + qx;
                idq = ((const float*)&in[q])[3];
                validq = ((const float*)&a.guide[q])[3];
                vq = vin[q];
            }
        });
    if (LAST) a.dst[i] = dvarFinal(a, i, o.d, gp.w != 0.0f);
    else { out[i] = o.d; vout[i] = o.var; }
}

template <int S>
static void launch_dvar_pass(const DenoiseVarArgs& a, bool last, const float4* in, float4* out, const float* vin,
                             float* vout, hipStream_t s)
{
    const int tx = (a.width + 15) / 16, ntiles = tx * ((a.height + 15) / 16);
    // persistent blocks as pt_denoise_pass's: about four tiles each, 4096..8192
    const int blocks = ntiles / 4 < 4096 ? 4096 : ntiles / 4 > 8192 ? 8192 : ntiles / 4;
    const dim3 grid(ntiles < blocks ? ntiles : blocks);
    if (last) hipLaunchKernelGGL((pt_dvar_pass<S, true>), grid, dim3(256), 0, s, a, in, out, vin, vout, tx, ntiles);
    else hipLaunchKernelGGL((pt_dvar_pass<S, false>), grid, dim3(256), 0, s, a, in, out, vin, vout, tx, ntiles);
}

} // namespace pt

// The whole filter on stream s: prep, then a->iterations passes; pass i reads colour[i & 1] and var[i & 1] and
// writes the other planes, the last one dst. The arguments are checked by the caller (dev_denoise_variance).
extern "C" hipError_t pt_launch_denoise_var(const pt::DenoiseVarArgs* a, hipStream_t s)
{
    const long long n = (long long)a->width * a->height;
    if (n <= 0) return hipSuccess;
    const int tx = (a->width + 15) / 16, ty = (a->height + 15) / 16;
    hipLaunchKernelGGL(pt::pt_dvar_prep, dim3((unsigned)(tx * ty)), dim3(256), 0, s, *a, tx);
    for (int i = 0; i < a->iterations; i++) {
        const bool last = i == a->iterations - 1;
        const float4* in = a->colour[i & 1];
        float4* out = a->colour[(i & 1) ^ 1];
        const float* vin = a->var[i & 1];
        float* vout = a->var[(i & 1) ^ 1];
        switch (i) {
        case 0: pt::launch_dvar_pass<1>(*a, last, in, out, vin, vout, s); break;
        case 1: pt::launch_dvar_pass<2>(*a, last, in, out, vin, vout, s); break;
        case 2: pt::launch_dvar_pass<4>(*a, last, in, out, vin, vout, s); break;
        default: {
            const dim3 grid((a->width + 63) / 64, (a->height + 3) / 4);
            if (last) hipLaunchKernelGGL(pt::pt_dvar_far<true>, grid, dim3(256), 0, s, *a, in, out, vin, vout, 1 << i);
            else hipLaunchKernelGGL(pt::pt_dvar_far<false>, grid, dim3(256), 0, s, *a, in, out, vin, vout, 1 << i);
        }
        }
    }
    return hipGetLastError();
}
