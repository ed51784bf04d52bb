// Grow-only buffer in device or pinned host memory, shared by the host units that stage data (gmc_kernels.hip, shopformer_host.hip).
// The owner says what it needs and, where it keeps slack, what to allocate instead; what a reallocation invalidates is the owner's
// business too: buf_grow tells it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace mi355 {

struct Buf {
    bool pinned = false;
    uint8_t* p = nullptr; size_t cap = 0;
};
inline void buf_free(Buf& b) {
    if (b.p) (void)(b.pinned ? hipHostFree(b.p) : hipFree(b.p));
    b.p = nullptr; b.cap = 0;
}
// 0 = large enough as it is, 1 = reallocated at max(need, alloc) bytes (the contents are gone), -2 = HIP error (the buffer is empty)
inline int buf_grow(Buf& b, size_t need, size_t alloc = 0) {
    if (b.cap >= need) return 0;
    buf_free(b);
    alloc = std::max(alloc, need);
    if ((b.pinned ? hipHostMalloc(&b.p, alloc) : hipMalloc(&b.p, alloc)) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return -2; }
    b.cap = alloc;
    return 1;
}

}  // namespace mi355
