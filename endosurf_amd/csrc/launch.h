// Host-side launch helpers shared by the translation units of libendosurf_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

namespace es {

constexpr int ST_OK = 0;
constexpr int ST_BAD_ARG = 1;
constexpr int ST_HIP_ERROR = 2;

inline char* last_error_buf() {
    static char buf[512] = {0};
    return buf;
}
inline int fail(int code, const char* what, const char* detail) {
    snprintf(last_error_buf(), 512, "%s: %s", what, detail ? detail : "");
    return code;
}
inline int hip_last(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ST_HIP_ERROR, what, hipGetErrorString(e));
    return ST_OK;
}
#define ES_HIP(call)                                                                      \
    do {                                                                                  \
        const hipError_t e__ = (call);                                                    \
        if (e__ != hipSuccess) return ::es::fail(::es::ST_HIP_ERROR, #call, hipGetErrorString(e__)); \
    } while (0)
#define ES_REQUIRE(cond, msg)                                             \
    do {                                                                  \
        if (!(cond)) return ::es::fail(::es::ST_BAD_ARG, msg, #cond);     \
    } while (0)

// a caller's scratch buffer: the regions below are carved at multiples of 16 bytes (uint4 loads rely on it)
#define ES_SCRATCH_OK(ptr, what) \
    ES_REQUIRE(ptr && reinterpret_cast<uintptr_t>(ptr) % 16 == 0, what " must be a 16-byte aligned device buffer")

constexpr unsigned MAX_GRID = 1u << 16;          // workgroups of a grid-stride launch
inline unsigned grid_for(long long n, int per_wg = 256) {
    const long long wg = (n + per_wg - 1) / per_wg;
    return (unsigned)(wg < 1 ? 1 : (wg < MAX_GRID ? wg : MAX_GRID));
}

inline long long up16(long long b) { return (b + 15) / 16 * 16; }
// A scratch layout is written once, as a sequence of take() calls: with the caller's buffer it carves, with a null base it only
// measures, so the size a caller is told and the pointers the kernels get cannot disagree.
struct Carver {
    char* base;
    long long off = 0;
    explicit Carver(const void* scratch) : base(static_cast<char*>(const_cast<void*>(scratch))) {}
    template <class T>
    T* take(long long n) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += up16((long long)sizeof(T) * n);
        return p;
    }
};

// opt a kernel into > 64 KiB of dynamic LDS (once per kernel)
template <class K>
inline int allow_big_lds(K kernel, int bytes) {
    ES_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return ST_OK;
}

// Per-device "has this one-time setup run yet" flag: hipFuncSetAttribute and __constant__ uploads are per device, so a
// process that drives several GPUs (one Engine per device) must repeat them on each.  Keyed by the CURRENT device
// (callers run under hipSetDevice / torch.cuda.device of their engine).  Not thread-safe: one host thread per device handle.
struct DeviceOnce {
    unsigned long long mask[4] = {0, 0, 0, 0};
    int dev = 0;
    bool first() {
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 256) dev = 0;
        return !((mask[dev >> 6] >> (dev & 63)) & 1ull);
    }
    void done() { mask[dev >> 6] |= 1ull << (dev & 63); }
};

// A launcher keeps the instantiations of its kernel in one array, indexed by the template switches: this opts every entry into big LDS
// once per device, and the launcher then launches the one entry its arguments select.
template <class K, int N>
inline int allow_big_lds_once(DeviceOnce& once, K* const (&kernels)[N], int bytes) {
    if (!once.first()) return ST_OK;
    for (K* k : kernels)
        if (int e = allow_big_lds(k, bytes)) return e;
    once.done();
    return ST_OK;
}

// The launch of a lean-tile kernel (one workgroup of 256 threads per tile of ``pts`` points, ``lds_bytes`` of dynamic LDS), written
// once: every entry of ``kernels`` is opted into big LDS once per device, then entry ``which`` runs on ceil(rows / pts) workgroups.
template <class K, int N, class... Args>
inline int launch_lean(K* const (&kernels)[N], DeviceOnce& once, int which, int lds_bytes, long long rows, int pts, hipStream_t st,
                       const char* name, const Args&... args) {
    if (int e = allow_big_lds_once(once, kernels, lds_bytes)) return e;
    const dim3 grid((unsigned)((rows + pts - 1) / pts)), block(256);
    hipLaunchKernelGGL(kernels[which], grid, block, lds_bytes, st, args...);
    return hip_last(name);
}

}  // namespace es
