// pt_devmem.h — one owner for a device allocation: the pointer, and its size in the owner's units (pixels, lanes,
// records; 0 while there is none). Freed when the owner goes out of scope, so a temporary is freed on every error
// return; a context's growing slabs are released by name of their array, before its streams go (dev_ctx_destroy).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct Dev;
enum SlabWait { WAIT_MAIN, WAIT_ALL };

struct DevMem {
    void* p = nullptr;
    size_t size = 0;
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { release(); }
    template <class T> T* as() const { return (T*)p; }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    void release() { if (p) hipFree(p); p = nullptr; size = 0; }
    // Grow a slab of context `c` (pt_capi.cpp): wait for the streams whose work may still use the old one, free
    // it, allocate `bytes` and record its new size. WAIT_ALL: the side streams' path tracing uses it too.
    // `fresh`: the megakernel's draws use it, so the next one waits for everything before it (new memory).
    int grow(Dev* c, size_t new_size, size_t bytes, SlabWait wait, bool fresh);
};
