// More than 64 KB of dynamic LDS is a per-DEVICE opt-in of every kernel that asks for it (hipFuncSetAttribute).  Host code only.
#pragma once
#include "ag_common.h"

#include <atomic>
#include <initializer_list>

namespace ag {

// A launch site keeps its own `static std::atomic<unsigned long long> done{0}` - one bit per device ordinal it has served - and
// hands it over with its byte budget and its kernels.  The attribute is set once per device and kernel; for an ordinal >= 64 there
// is no bit to keep, so it is set again on every call.  The first error is returned, and the device then stays unmarked.
template <typename... K>
hipError_t lds_opt_in(std::atomic<unsigned long long>& done, int bytes, K*... kernels) {
    int dev_id = 0;
    if (hipGetDevice(&dev_id) != hipSuccess) dev_id = 0;
    if (dev_id < 64 && (done.load(std::memory_order_acquire) >> dev_id & 1ull)) return hipSuccess;
    for (const void* k : {reinterpret_cast<const void*>(kernels)...}) {
        hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
    }
    if (dev_id < 64) done.fetch_or(1ull << dev_id, std::memory_order_release);
    return hipSuccess;
}

}  // namespace ag
