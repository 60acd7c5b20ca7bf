// The one place where host code lays device memory out and grows it ("Host side").  The carver is plain C++17 (g++ compiles it alone:
// tests/test_arena_cpu.py); the owners need the HIP runtime and exist under hipcc only.
//   VhCarver: a layout is ONE function of a carver, called with a null base for the size and with the block for the pointers: the two cannot disagree.
//   VhBlock:  the owner of one device (or pinned host) block and the one grow rule of every scratch that grows on demand.
#pragma once
#include <stddef.h>
#include <stdint.h>

static inline size_t vh_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
#define VH_CARVE_OVERFLOW SIZE_MAX  // bytes() of a layout whose size does not fit size_t: no allocation of that size can succeed

struct VhCarver {
    char* base;  // null: sizes only, every take returns null
    size_t align, off;
    bool overflow;
    explicit VhCarver(void* base_, size_t align_ = 256) : base(static_cast<char*>(base_)), align(align_), off(0), overflow(false) {}
    // `count` objects of T at the current offset, which then advances by their bytes rounded up to the alignment.  A count of 0 takes no space: it returns
    // the current position and leaves the offset where it was (match_carve: level 0 of a frame has no image of its own).
    template <class T>
    T* take(size_t count)
    {
        overflow = overflow || count > (SIZE_MAX - off - (align - 1)) / sizeof(T);  // (off + the rounded bytes would wrap)
        if (overflow) return nullptr;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += vh_align_up(count * sizeof(T), align);
        return p;
    }
    size_t bytes() const { return overflow ? VH_CARVE_OVERFLOW : off; }
};

#ifdef __HIPCC__
#include <stdio.h>
#include "vh_common.hpp"
int vh_fail(int code, const char* msg);

// One block, allocated whole or not at all: {p, bytes} is a live block of that size or {nullptr, 0}.  Plain data: zero-initialised is the empty owner.
template <bool PINNED>
struct VhBlock {
    char* p;
    size_t bytes;
    void release() { (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; bytes = 0; }
    // THE grow rule.  Nothing to do when the block holds `need` bytes already (it never shrinks).  Otherwise: never inside a stream capture (-6: "<what> must
    // grow inside a stream capture: <remedy>"); work queued on `s` may still use the old block, so the stream is waited for before it is freed; then the new
    // block, cleared when `zero`.  A failure after the free leaves the owner empty ("hipMalloc(<what>)" or "hipMemset(<what>)" in vh_last_error).
    int reserve(size_t need, hipStream_t s, const char* what, const char* remedy, bool zero = false)
    {
        if (need <= bytes) return 0;
        if (need == VH_CARVE_OVERFLOW) return vh_fail(-1, "the size of a device block overflows size_t");
        char msg[256];
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
            snprintf(msg, sizeof(msg), "%s must grow inside a stream capture: %s", what, remedy);
            return vh_fail(-6, msg);
        }
        if (p) VH_CHECK(hipStreamSynchronize(s));
        release();
        hipError_t e = PINNED ? hipHostMalloc((void**)&p, need, hipHostMallocDefault) : hipMalloc((void**)&p, need);
        const bool made = e == hipSuccess;
        if (made && zero) e = hipMemset(p, 0, need);
        snprintf(msg, sizeof(msg), "%s(%s)", made ? "hipMemset" : "hipMalloc", what);  // vh_last_error names the call that failed, as it always did
        if (e != hipSuccess) { vh_set_error(msg, e, __FILE__, __LINE__); release(); return (int)e; }
        bytes = need;
        return 0;
    }
};
typedef VhBlock<false> VhDeviceBlock;
typedef VhBlock<true> VhPinnedBlock;
#endif  // __HIPCC__
