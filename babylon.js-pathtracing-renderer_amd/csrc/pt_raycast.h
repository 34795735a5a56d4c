// pt_raycast.h — the ray queries' kernel arguments and launchers (pt_raycast.hip), shared with the host (pt_capi.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "pt_args.h"

namespace pt {

// One launch: rays [0, n) of the arrays given, one per lane of ceil(n / 64) one-wave workgroups. The arrays are the
// call's staged copies (the host route) or the caller's own device memory at the chunk's offset (the device route).
// The scene comes as the effect's TraceArgs (pt_capi.cpp scene_args), whose spill / spill_stride are the call's own
// slab (pt_plan.h RaycastLayout / RaycastStackLayout) with the launch's lanes as the stride.
struct RaycastArgs {
    const float* origins;   // [n x 3]
    const float* dirs;      // [n x 3]
    float4* hits;           // [n x 4]: the pt_ray_hit records (include/pt.h); closest hit
    unsigned n;
    const float* t_max;     // [n], or null: no bound (pt_raycast_q alone reads it)
    unsigned char* flags;   // [n]: 1 or 0; the occlusion query
};

// pt_raycast_q's MODE (include/pt.h PT_RAYS_CLOSEST / PT_RAYS_OCCLUDED)
enum { RAYS_CLOSEST = 0, RAYS_OCCLUDED = 1 };

}  // namespace pt

// `prog`: the effect's scene program (PROG_*); the variant is resolved here as pt_launch_trace resolves it
extern "C" hipError_t pt_launch_raycast(int prog, const pt::TraceArgs* a, const pt::RaycastArgs* q, hipStream_t s);
// ... the bounded closest hit (`mode` RAYS_CLOSEST, into q->hits) or the occlusion flag (RAYS_OCCLUDED, into q->flags)
extern "C" hipError_t pt_launch_raycast_q(int prog, int mode, const pt::TraceArgs* a, const pt::RaycastArgs* q, hipStream_t s);
