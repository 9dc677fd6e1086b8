// tools/emul/hip_stub/hip/hip_runtime.h — TEST INFRASTRUCTURE: a stand-in for the HIP runtime header with the types and the
// calls that lachain_amd/csrc/lcb_ctx.hpp and host_call.hpp use, for tools/emul/host_call_emul.cpp.  Device memory is
// the heap at its exact size, so AddressSanitizer reports any overrun of a "device" buffer; copies and fills run at once.
// hip_emul::fail_in makes a chosen allocation fail; the counters let a test see that a call touched nothing.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct ihipStream_t *hipStream_t;
typedef struct ihipEvent_t *hipEvent_t;
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };

namespace hip_emul {
inline long fail_in = -1;          // >= 0: that many allocations succeed, the next one fails (once)
inline long allocs = 0, frees = 0, copies = 0, fills = 0;
}  // namespace hip_emul

inline hipError_t hipMalloc(void **p, size_t n) {
    if (hip_emul::fail_in == 0) {
        hip_emul::fail_in = -1;
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    if (hip_emul::fail_in > 0) hip_emul::fail_in--;
    hip_emul::allocs++;
    *p = malloc(n);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t hipFree(void *p) {
    hip_emul::frees++;
    free(p);
    return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind, hipStream_t) {
    hip_emul::copies++;
    memcpy(dst, src, n);
    return hipSuccess;
}
inline hipError_t hipMemsetAsync(void *dst, int v, size_t n, hipStream_t) {
    hip_emul::fills++;
    memset(dst, v, n);
    return hipSuccess;
}
inline hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
