// pt_raycast.h — pt_cast_rays' kernel arguments and launcher (pt_raycast.hip), shared with the host (pt_capi.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "pt_args.h"

namespace pt {

// One launch: rays [0, n) of the staged arrays, one per lane of ceil(n / 64) one-wave workgroups. The scene comes as
// the effect's TraceArgs (pt_capi.cpp scene_args), whose spill / spill_stride are the call's own slab
// (pt_plan.h RaycastLayout) with the launch's lanes as the stride.
struct RaycastArgs {
    const float* origins;   // [n x 3]
    const float* dirs;      // [n x 3]
    float4* hits;           // [n x 4]: the pt_ray_hit records (include/pt.h)
    unsigned n;
};

}  // namespace pt

// `prog`: the effect's scene program (PROG_*); the variant is resolved here as pt_launch_trace resolves it
extern "C" hipError_t pt_launch_raycast(int prog, const pt::TraceArgs* a, const pt::RaycastArgs* q, hipStream_t s);
