// hip_host.h — what the host side of both handles (isingmc_batch: batch.hip.h, isingmc_classical: classical_handle.h) shares: the error
// macro, an owner of device memory, the device probe of the create functions, bytes <-> state words, and the plain copies of the
// accessors.  Host code only, plain C++17: no kernels, no __device__ code, so a host compiler takes it (tests/test_host_buffers_cpu.py
// runs DevBuf and the bit packing over stand-ins of the runtime, under the sanitizers).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include "../../include/isingmc_hip.h" // the return codes

// for any handle with an `err` string
#define HIP_TRY(h, expr)                                                                              \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                             \
            return ISINGMC_ENODEVICE;                                                                 \
        }                                                                                             \
    } while (0)

// One hipMalloc block and its size; freed when the owner goes.  Move-only.  Failures come back as hipError_t: the callers word them.
// (The device the block lives on must be current when it is freed: the destroy functions set it before they delete the handle.)
class DevBuf {
    void *p_ = nullptr;
    size_t bytes_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }

    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; bytes_ = 0;
    }
    // a fresh block of `bytes` (what was held is freed first); empty after a failure
    hipError_t alloc(size_t bytes) {
        reset();
        const hipError_t e = hipMalloc(&p_, bytes);
        if (e != hipSuccess) p_ = nullptr; else bytes_ = bytes;
        return e;
    }
    // scratch that only grows: at least `bytes`, contents not kept.  A block that is large enough stays, and nothing waits; a smaller
    // one is freed behind the work of `drain`, which may still use it.  Empty after a failure.
    hipError_t reserve(size_t bytes, hipStream_t drain) {
        if (p_ && bytes_ >= bytes) return hipSuccess;
        if (p_) (void)hipStreamSynchronize(drain);
        return alloc(bytes);
    }
    template <class T> T *as() const { return static_cast<T *>(p_); }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
};

// The prologue of the create functions: is there a device, which one (wish < 0: the current one), make it current, and the LDS of one
// of its workgroups (64 KB where the runtime does not say).  Returns nullptr, or why there is no device to create on.
inline const char *probe_device(int wish, int *dev, int *lds_bytes) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return "no HIP device available (this library has no CPU fallback)";
    *dev = wish;
    if (*dev < 0 && hipGetDevice(dev) != hipSuccess) *dev = 0;
    if (hipSetDevice(*dev) != hipSuccess) return "hipSetDevice failed";
    *lds_bytes = 0;
    if (hipDeviceGetAttribute(lds_bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, *dev) != hipSuccess || *lds_bytes <= 0) *lds_bytes = 65536;
    return nullptr;
}

// states as the ABI passes them, [rows][N] bytes (non-zero = up), and as the device keeps them, [rows][nwords] words (bit v & 31 of word
// v >> 5; the bits past N are zero)
inline void pack_bits(const uint8_t *in, size_t rows, uint32_t N, uint32_t nwords, uint32_t *out) {
    for (size_t i = 0; i < rows * nwords; ++i) out[i] = 0u;
    for (size_t r = 0; r < rows; ++r)
        for (uint32_t v = 0; v < N; ++v)
            if (in[r * N + v]) out[r * nwords + (v >> 5)] |= 1u << (v & 31u);
}
inline void unpack_bits(const uint32_t *in, size_t rows, uint32_t N, uint32_t nwords, uint8_t *out) {
    for (size_t r = 0; r < rows; ++r)
        for (uint32_t v = 0; v < N; ++v) out[r * N + v] = (uint8_t)((in[r * nwords + (v >> 5)] >> (v & 31u)) & 1u);
}

// The plain accessors: null checks, hipSetDevice, `count` elements copied down or up with a blocking copy, behind the work of the
// handle's stream where `drain` asks
template <class H, class T>
int copy_down(H *h, T *out, const T *src, size_t count, bool drain = false) {
    if (!h || !out) return ISINGMC_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    if (drain) HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(out, src, sizeof(T) * count, hipMemcpyDeviceToHost));
    return ISINGMC_OK;
}
template <class H, class T>
int copy_up(H *h, T *dst, const T *in, size_t count, bool drain = false) {
    if (!h || !in) return ISINGMC_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    if (drain) HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(dst, in, sizeof(T) * count, hipMemcpyHostToDevice));
    return ISINGMC_OK;
}
