// pt_trace_feat_inst.h — the FEAT instantiations of pt_trace (pt_trace.h: a draw with feature targets bound
// also stages its G-buffer) for the program variants of one BVH walk, and their launcher; included by
// pt_trace_feat_<walk>.hip with PT_WALK_NAME / PT_WALK_PROGS set, as pt_trace_inst.h is by pt_trace_walk_<walk>.hip:
// translation units of their own, so that the build stays parallel and a plain draw's kernels are untouched.
#include "pt_trace.h"

#define PT_CAT2(a, b) a##b
#define PT_CAT(a, b) PT_CAT2(a, b)

namespace pt {
// the timed megakernel variant of a feature draw, with or without late-bounce compaction (mesh programs)
template <int P>
hipError_t launchTraceFeat(bool cont, const TraceArgs* a, dim3 grid, dim3 block, hipStream_t s)
{
    if constexpr (kHasMesh<P>) {
        if (cont) hipLaunchKernelGGL((pt_trace<P, false, true, true>), grid, block, 0, s, *a);
        else hipLaunchKernelGGL((pt_trace<P, false, false, true>), grid, block, 0, s, *a);
    } else hipLaunchKernelGGL((pt_trace<P, false, false, true>), grid, block, 0, s, *a);
    return hipGetLastError();
}
} // namespace pt

hipError_t PT_CAT(pt_launch_trace_feat_, PT_WALK_NAME)(int prog, const pt::TraceArgs* a, dim3 grid, dim3 block,
                                                       hipStream_t s)
{
    using namespace pt;
    const bool cont = a->cont_rec != nullptr;
#define PT_CASE(P) case P: return launchTraceFeat<P>(cont, a, grid, block, s);
    switch (prog) {
        PT_WALK_PROGS(PT_CASE)
    default: return hipErrorInvalidValue;
    }
#undef PT_CASE
}
