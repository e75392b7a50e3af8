// capi_util.h -- what the host files of the C ABI (capi.cpp, create.cpp, layouts.cpp, multi.cpp)
// share: the error reporting behind sm_last_error, the device guard and the post-launch check.
#pragma once

#include <hip/hip_runtime.h>

#include "sparsematrix.h"

namespace smamd {

// Sets the calling thread's sm_last_error text (one string, defined in capi.cpp); returns `s`.
sm_status fail(sm_status s, const char *fmt, ...);

inline sm_status hip_fail(hipError_t e, const char *what) {
    return fail(e == hipErrorOutOfMemory ? SM_ERR_OUT_OF_MEMORY : SM_ERR_HIP, "%s: %s (%d)", what,
                hipGetErrorString(e), (int)e);
}

#define SM_TRY_HIP(call)                                           \
    do {                                                           \
        hipError_t e_ = (call);                                    \
        if (e_ != hipSuccess) return smamd::hip_fail(e_, #call);   \
    } while (0)

// Makes `dev` current for the scope and restores the caller's device.  Default-constructed it
// does nothing until enter() (a constructor checks the device's number first: create.cpp).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    DeviceGuard() = default;
    explicit DeviceGuard(int dev) { enter(dev); }
    void enter(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// SM_DEBUG_SYNC=1: synchronise after every launch and report the failing call
// (fault attribution; it changes no result, only the timing).
hipError_t after_launch(hipError_t e, hipStream_t s, const char *what);

}  // namespace smamd
