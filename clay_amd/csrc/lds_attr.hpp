// lds_attr.hpp -- hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device), for
// every launcher of a kernel with more dynamic LDS than the default limit.  Host only.
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>
#include <set>
#include <utility>

namespace clay {

// The lock is held across the HIP call: a second thread's first launch waits for the attribute.
inline hipError_t lds_attr_once(const void *fn, int bytes, int dev) {
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({fn, dev})) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.insert({fn, dev});
    return e;
}

}  // namespace clay
