// host.h -- host-side helpers every entry-point file of the library shares: the thread-local error message, the HIP
// call check, the device guard and the 256-thread grid size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Stores the formatted message for siggan_last_error() and returns `code` (defined in siggan.hip).
int siggan_set_error(int code, const char* fmt, ...);
#define FAIL(...) siggan_set_error(__VA_ARGS__)
#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) return FAIL(SIGGAN_E_HIP, "%s -> %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Entry points run on the context's device and put the caller's current device back on return (a process whose
// torch current device is another GPU must not find it switched behind its back).
struct DevGuard {
    int prev = -1, dev;
    hipError_t err = hipSuccess;
    explicit DevGuard(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev);
    }
    ~DevGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
};

static inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
// ceil(log2(v)); the extents it is used on are powers of two
static inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
