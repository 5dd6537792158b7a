// abi_host.hpp -- the host half the C-ABI entries of every side module share (envgpu, envimg, pergpu, plangpu, mapgpu, dqngpu):
// the error slot behind a *_last_error export and the two HIP calls that stand around a launch.  An entry reads
//     checks -> fail(...);  if (on_device(slot, device)) return -1;  hipLaunchKernelGGL(...);  return launched(slot, "... launch");
// Each *_last_error export keeps a thread_local slot of its own: a refusal through one entry leaves every other slot's text alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace abi {

struct ErrorSlot {
    std::string text;
    // stores `what`, or `what: <HIP's words for e>`; -1, so that an entry can `return slot.fail(...)`
    int fail(const char* what, hipError_t e = hipSuccess) {
        text = what;
        if (e != hipSuccess) text.append(": ").append(hipGetErrorString(e));
        return -1;
    }
};

inline int on_device(ErrorSlot& slot, int32_t device) {
    const hipError_t e = hipSetDevice(device);
    return e == hipSuccess ? 0 : slot.fail("hipSetDevice", e);
}

// after the launches of an entry: 0, or the launch error under `what`
inline int launched(ErrorSlot& slot, const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : slot.fail(what, e);
}

}  // namespace abi
