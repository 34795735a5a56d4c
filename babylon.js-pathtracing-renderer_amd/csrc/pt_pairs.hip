// pt_pairs.hip — the child-pair BVH records and the restart trail's jump table of a (tAABBTexture,
// tTriangleTexture) pair: the seven kernels of the build and the host sequence that runs them (pairs_build,
// pt_pairs.h). The scratch and the record array are laid out by pt::PairsLayout (pt_plan.h, with kPairsBlock, the
// nodes per scan block: 256 threads x 4).
#include <vector>

#include "pt_device.h"   // fetch32, pairLineWrite; pt_args.h (pairCode), pt_plan.h (PairsLayout)
#include "pt_pairs.h"

namespace pt {
// ------------------------------------------------------------------------------ child-pair BVH records
// Built once per (tAABBTexture, tTriangleTexture) upload; walked by bvhWalkPairs (pt_device.h).
// Every value is read from the reference textures with the same fetch32 / float index arithmetic
// the reference walk uses, so the boxes, codes and triangles equal what that walk would fetch.
//   pass 1  kinds: inner node (idObject < 0); leaf referenced as a child of an inner node (or the
//           root); `bad` flags links the records cannot express (right child not an exact integer
//           in [0, nrec), left child n+1 beyond the texture) -> the host keeps the reference walk
//   pass 2  per 1024-node block counts; the host scans them
//   pass 3  dense ranks -> rank codes: inner rank, or -1 - leaf rank
//   pass 4  inner records (64 B): A.min.xyz A.max.x | A.max.yz B.min.xy | B.min.z B.max.xyz |
//           codeA codeB (pairLineWrite; pairCode: record byte offsets, float bits); leaf records (48 B):
//           v0, e1 = v1 - v0, e2 = v2 - v0, idObject

__global__ __launch_bounds__(256) void pt_pairs_kinds(const float4* aabb, long long texels, unsigned nrec,
                                                      unsigned char* inner, unsigned char* leafref, unsigned* bad)
{
    const unsigned n = blockIdx.x * 256u + threadIdx.x;
    if (n >= nrec) return;
    const float fn = (float)n;   // exact: nrec <= 2^23
    const float4 c0 = fetch32(aabb, texels, fn * 2.0f), c1 = fetch32(aabb, texels, fn * 2.0f + 1.0f);
    const bool in = c0.x < 0.0f;
    inner[n] = in ? 1 : 0;
    // boxFast needs NaN-free boxes
    if (c0.y != c0.y || c0.z != c0.z || c0.w != c0.w || c1.y != c1.y || c1.z != c1.z || c1.w != c1.w) atomicOr(bad, 1u);
    if (n == 0 && !in) leafref[0] = 1;
    if (!in) return;
    const float idA = fn + 1.0f, idB = c1.x;
    const bool ok = idB >= 0.0f && idB < (float)nrec && floorf(idB) == idB && n + 1u < nrec;
    if (!ok) { atomicOr(bad, 1u); return; }
    const float4 a0 = fetch32(aabb, texels, idA * 2.0f), b0 = fetch32(aabb, texels, idB * 2.0f);
    if (!(a0.x < 0.0f)) leafref[n + 1u] = 1;
    if (!(b0.x < 0.0f)) leafref[(unsigned)idB] = 1;
}

__global__ __launch_bounds__(256) void pt_pairs_count(const unsigned char* inner, const unsigned char* leafref,
                                                      unsigned nrec, unsigned* counts)
{
    __shared__ unsigned si[256], sl[256];
    unsigned ci = 0, cl = 0;
    for (int k = 0; k < 4; k++) {
        const unsigned n = blockIdx.x * kPairsBlock + threadIdx.x * 4u + k;
        if (n < nrec) { ci += inner[n]; cl += leafref[n]; }
    }
    si[threadIdx.x] = ci; sl[threadIdx.x] = cl;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { si[threadIdx.x] += si[threadIdx.x + o]; sl[threadIdx.x] += sl[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { counts[2 * blockIdx.x] = si[0]; counts[2 * blockIdx.x + 1] = sl[0]; }
}

__global__ __launch_bounds__(256) void pt_pairs_rank(const unsigned char* inner, const unsigned char* leafref,
                                                     unsigned nrec, const unsigned* offsets, float* code)
{
    __shared__ unsigned si[256], sl[256];
    unsigned fi[4], fl[4], ci = 0, cl = 0;
    for (int k = 0; k < 4; k++) {
        const unsigned n = blockIdx.x * kPairsBlock + threadIdx.x * 4u + k;
        fi[k] = n < nrec ? inner[n] : 0u;
        fl[k] = n < nrec ? leafref[n] : 0u;
        ci += fi[k]; cl += fl[k];
    }
    si[threadIdx.x] = ci; sl[threadIdx.x] = cl;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {   // inclusive Hillis-Steele scan
        unsigned vi = threadIdx.x >= (unsigned)o ? si[threadIdx.x - o] : 0u;
        unsigned vl = threadIdx.x >= (unsigned)o ? sl[threadIdx.x - o] : 0u;
        __syncthreads();
        si[threadIdx.x] += vi; sl[threadIdx.x] += vl;
        __syncthreads();
    }
    unsigned ri = offsets[2 * blockIdx.x] + si[threadIdx.x] - ci;
    unsigned rl = offsets[2 * blockIdx.x + 1] + sl[threadIdx.x] - cl;
    for (int k = 0; k < 4; k++) {
        const unsigned n = blockIdx.x * kPairsBlock + threadIdx.x * 4u + k;
        if (n >= nrec) break;
        float cd = 0.0f;
        if (fi[k]) cd = (float)ri;
        else if (fl[k]) cd = -1.0f - (float)rl;
        code[n] = cd;
        ri += fi[k]; rl += fl[k];
    }
}

__global__ __launch_bounds__(256) void pt_pairs_build(const float4* aabb, long long texels, const float4* tri,
                                                      long long tri_texels, unsigned nrec, const float* code,
                                                      float4* inner_rec, float4* leaf_rec,
                                                      const unsigned char* inner, const unsigned char* leafref,
                                                      unsigned leaf_base)
{
    const unsigned n = blockIdx.x * 256u + threadIdx.x;
    if (n >= nrec) return;
    const float fn = (float)n;
    if (inner[n]) {
        const float4 c1 = fetch32(aabb, texels, fn * 2.0f + 1.0f);
        const float idA = fn + 1.0f, idB = c1.x;
        const float4 a0 = fetch32(aabb, texels, idA * 2.0f), a1 = fetch32(aabb, texels, idA * 2.0f + 1.0f);
        const float4 b0 = fetch32(aabb, texels, idB * 2.0f), b1 = fetch32(aabb, texels, idB * 2.0f + 1.0f);
        float4* o = inner_rec + 4ull * (unsigned)code[n];
        pairLineWrite(o, a0, a1, b0, b1);
        o[3] = make_float4(__uint_as_float(pairCode(code[n + 1u], leaf_base)),
                           __uint_as_float(pairCode(code[(unsigned)idB], leaf_base)), 0.0f, 0.0f);
    } else if (leafref[n]) {
        const float hdr = fetch32(aabb, texels, fn * 2.0f).x;
        const float id = 8.0f * hdr;
        const float4 t0 = fetch32(tri, tri_texels, id), t1 = fetch32(tri, tri_texels, id + 1.0f),
                     t2 = fetch32(tri, tri_texels, id + 2.0f);
        // edges e1 = v1 - v0, e2 = v2 - v0 are the walk's first two IEEE subtractions, done here once
        const f3 v0 = mk(t0.x, t0.y, t0.z), e1 = mk(t0.w, t1.x, t1.y) - v0, e2 = mk(t1.z, t1.w, t2.x) - v0;
        float4* o = leaf_rec + 3ull * (unsigned)(-1.0f - code[n]);
        o[0] = make_float4(v0.x, v0.y, v0.z, e1.x);
        o[1] = make_float4(e1.y, e1.z, e2.x, e2.y);
        o[2] = make_float4(e2.z, hdr, 0.0f, 0.0f);
    }
}

// Restart-trail prerequisites (PROG_TRAIL, bvhWalkTrail in pt_device.h), after the records:
//   links  every child link of an inner node counted (refs) and its parent noted; a node linked twice,
//          or the root linked at all, is no tree -> *flag
//   depth  every linked node climbs its parents to the root within kTrailMaxDepth steps, else *flag
//          (the trail has one bit per depth; unreachable runs are skipped)
//   top    the jump table: for each depth p <= kTopLevels and path (p A/B bits, heap order) the
//          inner record the path reaches, copied (64 B); zero where the path meets a leaf first
__global__ __launch_bounds__(256) void pt_pairs_links(const float4* aabb, long long texels, unsigned nrec,
                                                      const unsigned char* inner, unsigned* parent, unsigned* refs,
                                                      unsigned* flag)
{
    const unsigned n = blockIdx.x * 256u + threadIdx.x;
    if (n >= nrec || !inner[n]) return;
    const unsigned c[2] = { n + 1u, (unsigned)fetch32(aabb, texels, (float)n * 2.0f + 1.0f).x };   // exact: checked by pass 1
    for (int k = 0; k < 2; k++) {
        const unsigned old = atomicAdd(&refs[c[k]], 1u);
        parent[c[k]] = n;
        if (old != 0u || c[k] == 0u) atomicOr(flag, 1u);
    }
}

__global__ __launch_bounds__(256) void pt_pairs_depth(unsigned nrec, const unsigned* parent, const unsigned* refs,
                                                      unsigned* flag)
{
    const unsigned n = blockIdx.x * 256u + threadIdx.x;
    if (n >= nrec || n == 0u || refs[n] == 0u) return;
    unsigned m = n;
    for (int d = 1; d <= kTrailMaxDepth; d++) {
        m = parent[m];
        if (m == 0u) return;
        if (refs[m] == 0u) return;   // a run that is not reached from the root
    }
    atomicOr(flag, 1u);
}

__global__ __launch_bounds__(256) void pt_pairs_top(const float4* rec, uint32_t root, float4* top)
{
    for (unsigned idx = threadIdx.x; idx < kTopEntries; idx += blockDim.x) {
        const int p = 31 - __builtin_clz(idx + 1u);
        const unsigned prefix = idx + 1u - (1u << p);
        uint32_t code = root;
        bool ok = true;
        for (int j = 0; j < p && ok; j++) {
            if (code & kLeafBit) { ok = false; break; }
            const float4 c = rec[code / 16u + 3u];
            code = __float_as_uint(((prefix >> (p - 1 - j)) & 1u) ? c.y : c.x);
        }
        if (code & kLeafBit) ok = false;
        for (int q = 0; q < 4; q++) top[4u * idx + q] = ok ? rec[code / 16u + q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}
}  // namespace pt

// ------------------------------------------------------------------------------ the host sequence
// kinds, count | the host scans the per-block counts | rank, build, links, depth | the host reads the root and the
// trail's flag | top. One host round trip per build and one for the trail. `bad` (after count): the records cannot
// express the tree, nothing more is built and ok stays false; `notrail` (after depth): the records stand, without
// a jump table (top 0).
hipError_t pairs_build(const float4* aabb, long long texels, const float4* tri, long long tri_texels, unsigned* d_flags,
                       hipStream_t s, PairsTree* out)
{
    out->ok = false;
    out->top = 0;
    const pt::PairsLayout L(texels);
    const unsigned nrec = L.nrec;
    const dim3 nodes((nrec + 255) / 256), blocks(L.nblk), b256(256);
    DevMem scratch;   // (freed on every return)
    std::vector<unsigned> h(2 * L.nblk);
    unsigned bad = 0, notrail = 0;
#define PT_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)
#define PT_PASS(kernel, grid, ...) \
    do { hipLaunchKernelGGL(pt::kernel, grid, b256, 0, s, __VA_ARGS__); PT_TRY(hipGetLastError()); } while (0)
    auto run = [&]() -> hipError_t {
        PT_TRY(scratch.alloc(L.bytes));
        char* const m = scratch.as<char>();
        unsigned char *inner = (unsigned char*)(m + L.inner), *leafref = (unsigned char*)(m + L.leafref);
        unsigned* counts = (unsigned*)(m + L.counts);
        float* code = (float*)(m + L.code);
        unsigned *parent = (unsigned*)(m + L.parent), *refs = (unsigned*)(m + L.refs);   // restart-trail checks
        PT_TRY(hipMemsetAsync(leafref, 0, nrec, s));
        PT_TRY(hipMemsetAsync(refs, 0, nrec * sizeof(unsigned), s));
        PT_TRY(hipMemsetAsync(d_flags, 0, 2 * sizeof(unsigned), s));
        PT_PASS(pt_pairs_kinds, nodes, aabb, texels, nrec, inner, leafref, d_flags);
        PT_PASS(pt_pairs_count, blocks, inner, leafref, nrec, counts);
        PT_TRY(hipMemcpyAsync(h.data(), counts, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        PT_TRY(hipMemcpyAsync(&bad, d_flags, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        PT_TRY(hipStreamSynchronize(s));
        if (bad) return hipSuccess;
        size_t n_inner = 0, n_leaf = 0;
        for (unsigned b = 0; b < L.nblk; b++) {   // exclusive scan of the per-block counts
            unsigned ci = h[2 * b], cl = h[2 * b + 1];
            h[2 * b] = (unsigned)n_inner; h[2 * b + 1] = (unsigned)n_leaf;
            n_inner += ci; n_leaf += cl;
        }
        const pt::PairsLayout::Records R(n_inner, n_leaf);
        PT_TRY(out->mem.alloc(R.alloc));
        float4* const rec = out->mem.as<float4>();
        float4* const top = (float4*)(out->mem.as<char>() + R.top_base);
        out->inner = rec;
        out->leaf = (const float4*)(out->mem.as<char>() + R.leaf_base);
        PT_TRY(hipMemcpyAsync(counts, h.data(), h.size() * sizeof(unsigned), hipMemcpyHostToDevice, s));
        PT_PASS(pt_pairs_rank, blocks, inner, leafref, nrec, counts, code);
        PT_PASS(pt_pairs_build, nodes, aabb, texels, tri, tri_texels, nrec, code, rec, (float4*)out->leaf, inner, leafref,
                R.leaf_base);
        PT_PASS(pt_pairs_links, nodes, aabb, texels, nrec, inner, parent, refs, d_flags + 1);
        PT_PASS(pt_pairs_depth, nodes, nrec, parent, refs, d_flags + 1);
        float root = 0.0f, node0[8] = {};
        PT_TRY(hipMemcpyAsync(&root, code, sizeof(float), hipMemcpyDeviceToHost, s));
        PT_TRY(hipMemcpyAsync(node0, aabb, sizeof(node0), hipMemcpyDeviceToHost, s));
        PT_TRY(hipMemcpyAsync(&notrail, d_flags + 1, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        PT_TRY(hipStreamSynchronize(s));
        out->root = pt::pairCode(root, R.leaf_base);
        const float box6[6] = { node0[1], node0[2], node0[3], node0[5], node0[6], node0[7] };
        for (int k = 0; k < 6; k++) out->root_box[k] = box6[k];
        out->bytes = (uint32_t)R.rec_bytes;
        // the restart trail's jump table, for trees it can walk (one parent per node, depth <= 28)
        if (!notrail) {
            PT_PASS(pt_pairs_top, dim3(1), rec, out->root, top);
            out->top = (uint32_t)R.top_base;
        }
        return hipSuccess;
    };
#undef PT_PASS
#undef PT_TRY
    const hipError_t e = run();
    if (scratch.p) hipStreamSynchronize(s);   // (the passes queued so far use it)
    if (e != hipSuccess) out->mem.release();
    out->ok = e == hipSuccess && !bad;
    return e;
}
