// vmask_host.h - the host-side plumbing that every translation unit behind include/vmask.h shares: the one error macro, the
// one owner of device allocations, and the copies between a caller's host or device arrays and the device.  Host code only;
// everything has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vrg.h"
#include "vmask_common.h"

namespace {

#define VMASK_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { vmask::set_error(std::string(#x) + ": " + hipGetErrorString(e_)); return VRG_E_INTERNAL; } } while (0)

// The device allocations of one call.  Whatever was grabbed and not dropped is freed when the owner leaves scope, so a
// function that allocates only through it has no return path that leaks.
struct DevMem {
    std::vector<void*> owned;
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { for (void* p : owned) (void)hipFree(p); }
    // *p (re)allocated for max(1, count) elements; what it held before, if it came from here, is freed first
    template <class T> int grab(T** p, size_t count, const char* what) {
        drop(*p);
        *p = nullptr;
        void* q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(1, count) * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            vmask::set_error(std::string("out of device memory (") + what + ")");
            return VRG_E_MEM;
        }
        owned.push_back(q);
        *p = (T*)q;
        return VRG_OK;
    }
    // one allocation freed early (a pointer that is not owned here is left alone)
    void drop(const void* p) {
        const auto it = std::find(owned.begin(), owned.end(), p);
        if (it == owned.end()) return;
        (void)hipFree(*it);
        owned.erase(it);
    }
};
// (in a function that returns a VRG_* code and calls its DevMem `mem`)
#define VMASK_GRAB(p, count, what) do { int rc_ = mem.grab(&(p), (count), (what)); if (rc_) return rc_; } while (0)

// a caller's array that the kernels read: itself when it lives on the device, a device copy otherwise
template <class T> int bring(DevMem& mem, const T* p, size_t n, const char* what, const T** dev) {
    if (!n || vmask::is_device_pointer(p)) { *dev = p; return VRG_OK; }
    T* d = nullptr;
    const int rc = mem.grab(&d, n, what);
    if (rc) return rc;
    VMASK_TRY(hipMemcpy(d, p, n * sizeof(T), hipMemcpyHostToDevice));
    *dev = d;
    return VRG_OK;
}
// a host array to a new device array
template <class T> int send(DevMem& mem, const std::vector<T>& v, const char* what, const T** dev) {
    T* d = nullptr;
    const int rc = mem.grab(&d, v.size(), what);
    if (rc) return rc;
    if (!v.empty()) VMASK_TRY(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *dev = d;
    return VRG_OK;
}
// a caller's array that the kernels write: itself when it lives on the device, a device copy otherwise
template <class T> struct Out {
    T* user = nullptr; T* dev = nullptr; size_t count = 0;
    int open(DevMem& mem, T* p, size_t n, const char* what) {
        user = p; count = n;
        if (vmask::is_device_pointer(p)) { dev = p; return VRG_OK; }
        return mem.grab(&dev, n, what);
    }
    int close() {
        if (dev != user && count) VMASK_TRY(hipMemcpy(user, dev, count * sizeof(T), hipMemcpyDeviceToHost));
        return VRG_OK;
    }
};
// a caller's small array on the host
template <class T> int fetch(const T* p, size_t n, std::vector<T>& out) {
    out.resize(n);
    if (!n) return VRG_OK;
    if (vmask::is_device_pointer(p)) VMASK_TRY(hipMemcpy(out.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    else std::copy(p, p + n, out.begin());
    return VRG_OK;
}
inline int put(int64_t* dst, const int64_t* src, size_t count) {       // host values to a host or device array
    if (vmask::is_device_pointer(dst)) VMASK_TRY(hipMemcpy(dst, src, count * sizeof(int64_t), hipMemcpyHostToDevice));
    else std::copy(src, src + count, dst);
    return VRG_OK;
}

}  // namespace
