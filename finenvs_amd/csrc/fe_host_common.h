// fe_host_common.h -- host-side launch helpers of the library's smaller translation units (fe_mlp_critic.hip,
// fe_mlp_sac.hip, fe_evo.hip), included after the unit's kernel header (it needs kBlock, fail and hip_fail of fe_device_common.h).
// They restate helpers of fe_env.hip, which keeps its own (its host code names its kernels in an order its device code
// object depends on; nothing there moves).  Host code only: no unit's device code sees this file's contents.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace {

constexpr int64_t kMaxGrid = 8 * 256;
constexpr size_t kMaxLds = 160 * 1024;

[[maybe_unused]] const auto kHostFastDiv = &make_fastdiv;  // fe_device_common.h's host helper; no host code of these units divides

[[maybe_unused]] int64_t capped_grid(int64_t tiles) { return tiles < kMaxGrid ? tiles : kMaxGrid; }

[[maybe_unused]] int grid_for(int64_t work_items) {
    const int64_t g = (work_items + kBlock - 1) / kBlock;
    return (int)(g < 1 ? 1 : capped_grid(g));
}

// "<who> launch: <HIP error>"; after hipLaunchKernelGGL, which returns nothing, the one-argument form asks hipGetLastError
[[maybe_unused]] int launched(const char *who, hipError_t he = hipGetLastError()) {
    return he == hipSuccess ? FE_OK : fail(FE_ERR_HIP, "%s launch: %s", who, hipGetErrorString(he));
}

// "<who>: <what> launch: <HIP error>"
[[maybe_unused]] int launched(const char *who, const char *what, hipError_t he) {
    return he == hipSuccess ? FE_OK : fail(FE_ERR_HIP, "%s: %s launch: %s", who, what, hipGetErrorString(he));
}

// Makes a device current for the duration of a call (fe_env.hip's DeviceGuard).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        if (device < 0) {
            err = hipErrorInvalidDevicePointer;
            return;
        }
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) {
            err = hipSetDevice(device);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    int status(const char *what = "hipSetDevice") const { return err == hipSuccess ? FE_OK : hip_fail(err, what); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// Device a caller-owned pointer lives on (-1 if it is not device memory; fe_env.hip's device_of).
[[maybe_unused]] int device_of(const void *ptr) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged) return -1;
    return attr.device;
}

// f(std::integral_constant<int, NT>) for NT = H / 32 at H = 32 / 64 / 128 (the caller has refused every other H)
template <class F>
auto with_nt(int32_t H, F &&f) {
    return H == 32 ? f(std::integral_constant<int, 1>{}) : (H == 64 ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 4>{}));
}

}  // namespace
