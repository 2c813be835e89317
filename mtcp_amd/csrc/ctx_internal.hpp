// ctx_internal.hpp — what the library's translation units (mtcp_gpu.hip,
// rxq.hip) share besides the C ABI: not exported from libmtcp_gpu.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

struct mtcp_gpu_ctx;

// The context gave up on GPU work at a deadline (mtcp_gpu_set_wait_limit):
// nothing may be issued on it or waited for without a bound again.
extern "C" __attribute__((visibility("hidden"))) bool mg_ctx_abandoned(const mtcp_gpu_ctx *ctx);

namespace {   // per translation unit: nothing here is exported from the library

// MTCP_GPU_DEBUG=1 in the environment: report every failing HIP call.
bool hip_ok(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    static const bool debug = getenv("MTCP_GPU_DEBUG") != nullptr;
    if (debug) fprintf(stderr, "mtcp_gpu: %s -> %s\n", what, hipGetErrorString(e));
    return false;
}
#define HIP_OK(x) hip_ok((x), #x)

// Makes `device` current for one ABI call and restores the caller's device
// on return: an mTCP thread (or a torch process) keeps the device it chose.
struct DeviceGuard {
    int prev = -1;
    bool ok = false, switched = false;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev == device) {
            ok = true;
        } else {
            ok = HIP_OK(hipSetDevice(device));
            switched = ok && prev >= 0;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

}  // namespace
