// Thread-local last-error string behind the C ABI (include/rvc_amd.h: rvc_last_error), and the host helpers common.h declares.
#include <stdarg.h>

#include <map>
#include <mutex>
#include <unordered_map>

#include "common.h"

namespace rvc {

static thread_local char g_err[1024] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

// What the library learns or sets once per DEVICE (common.h), keyed by hipGetDevice on the calling thread: a kernel attribute
// belongs to the current device's function object, so a process that drives several devices (a thread per device) needs it on each.
namespace {
struct DeviceState {
    int cus = 0;                                       // 0: not asked yet
    std::unordered_map<const void *, int> lds;         // kernel -> largest dynamic-LDS byte count granted so far
};
std::mutex g_dev_mu;
std::map<int, DeviceState> g_dev;
}  // namespace

int reserve_lds(const void *kernel, int bytes, const char *what) {
    int dev = 0;
    RVC_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(g_dev_mu);
    int &granted = g_dev[dev].lds[kernel];
    if (bytes <= granted) return 0;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return fail("%s: cannot reserve %d bytes of LDS on device %d: %s", what, bytes, dev, hipGetErrorString(e));
    granted = bytes;
    return 0;
}

int cu_count() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    std::lock_guard<std::mutex> g(g_dev_mu);
    DeviceState &d = g_dev[dev];
    if (!d.cus) d.cus = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0 ? cus : 256;
    return d.cus;
}

int upload_packed(const char *fn, const void *host, size_t bytes, void *dev, void *stream) {
    hipError_t e = hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail("%s: %s", fn, hipGetErrorString(e));
    return 0;
}

}  // namespace rvc

extern "C" int rvc_abi_version(void) { return RVC_AMD_ABI_VERSION; }
extern "C" const char *rvc_last_error(void) { return rvc::g_err; }
