// lscqp_device.hpp — how the host objects of the library (plan, grid, record, map, worlds) own device memory and report a HIP failure.
// Host only: the units that keep such objects include it, the kernels-only units do not.  Nothing here allocates by policy, pools or
// copies: lscqp_staging.hpp is the pool, with its own rules.
#ifndef LSCQP_DEVICE_HPP
#define LSCQP_DEVICE_HPP

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <memory>
#include <string>

#include "lscqp_internal.hpp"

namespace lscqp {

// LSCQP_ERR_HIP with the text "<what>: <what the runtime says>"
inline int hip_fail(hipError_t e, const char* what) {
    return lscqp_set_error_(LSCQP_ERR_HIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}

// an object's device made current for a scope; the previous one comes back at its end only if the scope changed it
struct OnDevice {
    int prev = -1;
    explicit OnDevice(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~OnDevice() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    OnDevice(const OnDevice&) = delete;
    OnDevice& operator=(const OnDevice&) = delete;
};

struct DeviceFree {
    void operator()(void* p) const { (void)hipFree(p); }
};
struct PinnedFree {
    void operator()(void* p) const { (void)hipHostFree(p); }
};
// device memory (hipMalloc) and pinned host memory (hipHostMalloc) that free themselves; an owner is freed with its device current
template <class T>
using dev_ptr = std::unique_ptr<T, DeviceFree>;
template <class T>
using pinned_ptr = std::unique_ptr<T, PinnedFree>;

// `count` elements for `out`, zeroed if asked; on failure `out` is empty and the error is hip_fail's with the caller's text
template <class T>
int dev_alloc(dev_ptr<T>& out, size_t count, const char* what, bool zeroed = false) {
    out.reset();
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e != hipSuccess) return hip_fail(e, what);
    out.reset(static_cast<T*>(p));
    if (zeroed && (e = hipMemset(p, 0, count * sizeof(T))) != hipSuccess) {
        out.reset();
        return hip_fail(e, what);
    }
    return LSCQP_OK;
}

}  // namespace lscqp

#endif  // LSCQP_DEVICE_HPP
