// pt_pairs.h — the child-pair / restart-trail records of a BVH texture (pt_pairs.hip builds them, bvhWalkPairs and
// bvhWalkTrail of pt_device.h walk them). pt_capi.cpp decides when a tree is built and how long it is valid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_devmem.h"

struct PairsTree {
    DevMem mem;                    // one record array (pt::PairsLayout::Records): inner records,
    const float4* inner = nullptr;
    const float4* leaf = nullptr;  // ... the leaf records from here on, then the jump table
    uint32_t root = 0;             // pairCode of node 0
    uint32_t bytes = 0;            // of the records with the jump table
    uint32_t top = 0;              // byte offset of the restart-trail jump table; 0: the tree is not walkable by the trail
    float root_box[6] = {};
    bool ok = false;               // false: the records cannot express the tree, the reference walk must be used
};

// Builds `out` (whose memory the caller has released) from the BVH texture `aabb` and the triangle texture `tri`
// on stream `s`, which it waits for twice; `d_flags`: two words of device memory for the passes' flags. On an
// error no memory is left allocated.
hipError_t pairs_build(const float4* aabb, long long texels, const float4* tri, long long tri_texels, unsigned* d_flags,
                       hipStream_t s, PairsTree* out);
