// pt_raycast.hip — pt_cast_rays and pt_cast_rays_ex (include/pt.h): SceneIntersect of the bound scene on caller-given rays.
// pt_raycast<PROG> runs sceneIntersect (pt_trace.h) as the path kernels do - the same analytic tests, the same
// walk of the same BVH data, closest hit - and stores what it leaves as one 64-B record per ray; nothing of
// CalculateRadiance runs. One ray per lane, one-wave workgroups of 64 like pt_trace's, so a walk's LDS stack is
// sized and addressed exactly as there; the stack levels beyond LDS go to the call's own slab [level][lane of the
// grid] (pt_plan.h RaycastLayout), never to the draws' slabs.
#include "pt_raycast.h"
#include "pt_trace.h"

namespace pt {

// The lanes past the last ray of the last wave trace a copy of that ray and store nothing: the walks read wave-level
// values (the buffer descriptor's readfirstlane, laneNow) and index LDS by lane, so every lane of the wave goes
// through sceneIntersect with a defined ray and none leaves early.
// SLIM = kWaveBaseOf, as pt_trace and pt_cont instantiate it: `deep` is then the wave's base in the slab and
// MegaStack::at() adds the lane id, else it is the lane's own index. The result does not depend on it.
template <int PROG>
__global__ __launch_bounds__(kTraceBlock, kMinWaves<PROG>) void pt_raycast(TraceArgs a, RaycastArgs q)
{
    __shared__ float2 lds_stack[kHasMesh<PROG> ? kWalkSlotsOf<PROG> * kTraceBlock : 1];
    const unsigned lane = threadIdx.x;
    const unsigned i = blockIdx.x * kTraceBlock + lane;
    const unsigned r = min(i, q.n - 1u);
    const f3 ro = mk(q.origins[3u * r], q.origins[3u * r + 1u], q.origins[3u * r + 2u]);
    const f3 rd = mk(q.dirs[3u * r], q.dirs[3u * r + 1u], q.dirs[3u * r + 2u]);
    const unsigned deep = blockIdx.x * kTraceBlock + (kWaveBaseOf<PROG> ? 0u : lane);
    Cnt cnt = { 0, 0, 0, 0, 0, 0, 0 };
    // what SceneIntersect does not write stays +0: the kernels' Hit is not initialised, a record is
    Hit h;
    h.normal = mk(0.0f, 0.0f, 0.0f); h.color = mk(0.0f, 0.0f, 0.0f);
    h.u = 0.0f; h.v = 0.0f;
    BvhResult br = { 0.0f, 0.0f, 0.0f, false, 0u, 0u, 0u };
    sceneIntersect<PROG, false, kTraceBlock, kWaveBaseOf<PROG>>(a, ro, rd, h, lds_stack, lane, deep, cnt, false, &br);
    if (i >= q.n) return;
    // streamed once: non-temporal stores, as radianceOut's
    typedef float nt4 __attribute__((ext_vector_type(4)));
    const bool mesh = kHasMesh<PROG> && br.lookup;
    const int tri = mesh ? (int)(br.triID * 0.125f) : -1;   // (triID = 8 x the leaf's triangle: the texel of its vertices)
    const nt4 o0 = { h.t, __int_as_float(h.id), __int_as_float(h.type), __int_as_float(tri) };
    const nt4 o1 = { h.normal.x, h.normal.y, h.normal.z, mesh ? br.triU : 0.0f };
    const nt4 o2 = { h.color.x, h.color.y, h.color.z, mesh ? br.triV : 0.0f };
    const nt4 o3 = { h.u, h.v, 0.0f, 0.0f };
    nt4* const o = (nt4*)(q.hits + 4ull * i);
    __builtin_nontemporal_store(o0, o);
    __builtin_nontemporal_store(o1, o + 1);
    __builtin_nontemporal_store(o2, o + 2);
    __builtin_nontemporal_store(o3, o + 3);
}

// pt_cast_rays_ex's kernels: the bounded closest hit (MODE RAYS_CLOSEST) and the occlusion flag (RAYS_OCCLUDED).
// SceneIntersect with hitT starting at min(INFINITY, t_max[i]) - the GLSL's min, y < x ? y : x, so a NaN, an
// infinite or any t_max >= INFINITY is no bound - plumbed through sceneIntersect's `start`: the analytic tests and the
// walk see the lower hitT as they see any other, so the bound culls boxes too, as the GLSL with that start would.
// CLOSEST stores pt_raycast's record; a ray that takes no object (h.id < 0, h.t still the bound) gets the miss
// record, t = INFINITY. OCCLUDED stores one byte, whether the bounded closest hit takes an object: with
// kOccludedFirstHit the pairs walk stops at the first triangle it accepts (sceneIntersect's firstHit, the shadow
// rays' walk; it has visited the full walk's nodes up to there in the same order, so the flag is the full walk's),
// and the mesh hit needs no lookup; the trail and reference walks have no early out and run the bounded closest
// walk. Tail lanes as in pt_raycast: every lane of the wave goes through sceneIntersect.
constexpr bool kOccludedFirstHit = true;   // (DESIGN.md §6 "Ray queries": kept while it measures no slower)
template <int PROG, int MODE>
__global__ __launch_bounds__(kTraceBlock, kMinWaves<PROG>) void pt_raycast_q(TraceArgs a, RaycastArgs q)
{
    __shared__ float2 lds_stack[kHasMesh<PROG> ? kWalkSlotsOf<PROG> * kTraceBlock : 1];
    const unsigned lane = threadIdx.x;
    const unsigned i = blockIdx.x * kTraceBlock + lane;
    const unsigned r = min(i, q.n - 1u);
    const f3 ro = mk(q.origins[3u * r], q.origins[3u * r + 1u], q.origins[3u * r + 2u]);
    const f3 rd = mk(q.dirs[3u * r], q.dirs[3u * r + 1u], q.dirs[3u * r + 2u]);
    float start = kINF;
    if (q.t_max) {   // (wave-uniform)
        const float m = q.t_max[r];
        start = m < kINF ? m : kINF;
    }
    const unsigned deep = blockIdx.x * kTraceBlock + (kWaveBaseOf<PROG> ? 0u : lane);
    Cnt cnt = { 0, 0, 0, 0, 0, 0, 0 };
    Hit h;
    h.normal = mk(0.0f, 0.0f, 0.0f); h.color = mk(0.0f, 0.0f, 0.0f);
    h.u = 0.0f; h.v = 0.0f;
    BvhResult br = { 0.0f, 0.0f, 0.0f, false, 0u, 0u, 0u };
    sceneIntersect<PROG, false, kTraceBlock, kWaveBaseOf<PROG>>(a, ro, rd, h, lds_stack, lane, deep, cnt,
                                                                 MODE == RAYS_OCCLUDED && kOccludedFirstHit, &br, start);
    if (i >= q.n) return;
    if (MODE == RAYS_OCCLUDED) {
        q.flags[i] = h.id >= 0 ? 1 : 0;
        return;
    }
    typedef float nt4 __attribute__((ext_vector_type(4)));
    const bool mesh = kHasMesh<PROG> && br.lookup;
    const int tri = mesh ? (int)(br.triID * 0.125f) : -1;
    const nt4 o0 = { h.id < 0 ? kINF : h.t, __int_as_float(h.id), __int_as_float(h.type), __int_as_float(tri) };
    const nt4 o1 = { h.normal.x, h.normal.y, h.normal.z, mesh ? br.triU : 0.0f };
    const nt4 o2 = { h.color.x, h.color.y, h.color.z, mesh ? br.triV : 0.0f };
    const nt4 o3 = { h.u, h.v, 0.0f, 0.0f };
    nt4* const o = (nt4*)(q.hits + 4ull * i);
    __builtin_nontemporal_store(o0, o);
    __builtin_nontemporal_store(o1, o + 1);
    __builtin_nontemporal_store(o2, o + 2);
    __builtin_nontemporal_store(o3, o + 3);
}

template <int P>
hipError_t launchRaycast(const TraceArgs* a, const RaycastArgs* q, hipStream_t s)
{
    hipLaunchKernelGGL((pt_raycast<P>), dim3((q->n + kTraceBlock - 1) / kTraceBlock), dim3(kTraceBlock), 0, s, *a, *q);
    return hipGetLastError();
}

template <int P, int MODE>
hipError_t launchRaycastQ(const TraceArgs* a, const RaycastArgs* q, hipStream_t s)
{
    hipLaunchKernelGGL((pt_raycast_q<P, MODE>), dim3((q->n + kTraceBlock - 1) / kTraceBlock), dim3(kTraceBlock), 0, s, *a, *q);
    return hipGetLastError();
}

}  // namespace pt

extern "C" hipError_t pt_launch_raycast(int prog, const pt::TraceArgs* a, const pt::RaycastArgs* q, hipStream_t s)
{
    using namespace pt;
    if (!q->n) return hipSuccess;
    prog = resolveProgram(prog, a->uses_albedo || a->uses_bump, a->bvh_walk);
#define PT_CASE(P) case P: return launchRaycast<P>(a, q, s);
    switch (prog) {
        PT_FOR_EACH_PROG(PT_CASE)
    default: return hipErrorInvalidValue;
    }
#undef PT_CASE
}

extern "C" hipError_t pt_launch_raycast_q(int prog, int mode, const pt::TraceArgs* a, const pt::RaycastArgs* q, hipStream_t s)
{
    using namespace pt;
    if (!q->n) return hipSuccess;
    if (mode != RAYS_CLOSEST && mode != RAYS_OCCLUDED) return hipErrorInvalidValue;
    prog = resolveProgram(prog, a->uses_albedo || a->uses_bump, a->bvh_walk);
#define PT_CASE(P) case P: return mode == RAYS_OCCLUDED ? launchRaycastQ<P, RAYS_OCCLUDED>(a, q, s) : launchRaycastQ<P, RAYS_CLOSEST>(a, q, s);
    switch (prog) {
        PT_FOR_EACH_PROG(PT_CASE)
    default: return hipErrorInvalidValue;
    }
#undef PT_CASE
}
