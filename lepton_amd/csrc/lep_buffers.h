// lep_buffers.h -- what the host runtime (lep_gpu.hip, lep_batch.hip) keeps its memory in: a grow-only device buffer and a grow-only
// pinned host buffer (the layout of a packed descriptor block, and the block: lep_block.h).  A buffer owns its pointer and its capacity
// together: both change in set() and nowhere else, so a capacity never outlives its allocation (the next allocation may fail).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "lep_block.h"

namespace lepbuf {

// An owned virtual address range with physical chunks mapped into its front (lep_gpu.hip "workspaces": the codec object's large
// buffers; the chunks come from and go back to that object's pool).  Empty for every other buffer.
struct VRange { char* va = nullptr; size_t reserved = 0, mapped = 0; std::vector<hipMemGenericAllocationHandle_t> chunks; };

typedef hipError_t (*DevAlloc)(void** p, size_t bytes);
inline hipError_t dev_malloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }

// Grow-only device buffer; T is what the pointer reads as.  Growing does not keep the contents: every user fills its buffer anew.
template <class T = void>
struct DevBuf {
    static constexpr bool pinned = false;
    void* p = nullptr;
    size_t cap = 0;   // bytes
    VRange v;         // the memory is v's (p == v.va, cap == v.mapped) once the buffer has turned virtual, else a plain allocation
    operator T*() const { return (T*)p; }
    template <class U> U* at(size_t off) const { return (U*)((char*)p + off); }
    void set(void* q, size_t n) { p = q; cap = n; }
    // a plain allocation given back (a virtual one is lep_gpu.hip's to unmap)
    hipError_t release() {
        const hipError_t e = p && !v.va ? hipFree(p) : hipSuccess;
        if (!v.va) set(nullptr, 0);
        return e;
    }
    // at least `need` bytes; a buffer that grows asks for `head` bytes more, and for `need` alone where it cannot have them
    hipError_t ensure(size_t need, size_t head = 0, DevAlloc alloc = dev_malloc) {
        if (cap >= need) return hipSuccess;
        hipError_t e = release();
        if (e != hipSuccess) return e;
        void* q = nullptr;
        e = alloc(&q, need + head);
        if (e != hipSuccess && head) { (void)hipGetLastError(); head = 0; e = alloc(&q, need); }
        if (e == hipSuccess) set(q, need + head);
        return e;
    }
};

// Grow-only pinned host buffer (hipHostFree waits for the device: not for a buffer that is replaced while kernels run)
template <class T = void>
struct PinBuf {
    static constexpr bool pinned = true;
    void* p = nullptr;
    size_t cap = 0;
    operator T*() const { return (T*)p; }
    void set(void* q, size_t n) { p = q; cap = n; }
    hipError_t release() {
        const hipError_t e = p ? hipHostFree(p) : hipSuccess;
        set(nullptr, 0);
        return e;
    }
    hipError_t ensure(size_t need, size_t head = 0) {
        if (cap >= need) return hipSuccess;
        hipError_t e = release();
        if (e != hipSuccess) return e;
        void* q = nullptr;
        e = hipHostMalloc(&q, need + head, hipHostMallocDefault);
        if (e == hipSuccess) set(q, need + head);
        return e;
    }
};

}  // namespace lepbuf
