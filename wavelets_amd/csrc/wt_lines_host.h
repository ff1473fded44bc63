// Host text the two 1-D units share (wt_signals.hip, wt_along.hip): releasing a stack, the end of a create, the row
// copy, the choice of a kernel by element type and family, and the 1 / tau rule.  What differs on purpose stays in
// the units: the layouts of the threshold tables, how they are staged, and the signal unit's padding.
#pragma once
#include <type_traits>

#include "wt_host.h"

// hipFree of the device buffers of a stack that were allocated; *bad = 1 where one could not be released
static inline void lines_free(std::initializer_list<void *> dev, int *bad)
{
    for (void *q : dev)
        if (q && hipFree(q) != hipSuccess) *bad = 1;
}

// the end of `who` = wt_..._create after its allocations gave `e`: the stack to *out, or released with HIP's words
template <typename B>
static int lines_created(B *b, B **out, hipError_t e, const char *who, void (*release)(B *, int *))
{
    if (e != hipSuccess) {
        int bad = 0;
        release(b, &bad);
        delete b;
        wt_set_error("%s: HIP error %d (%s)", who, (int)e, hipGetErrorString(e));
        return 2;
    }
    *out = b;
    return 0;
}

// `who` = wt_..._destroy: behind the stream, and a buffer that HIP does not take back is reported
template <typename B>
static int lines_destroy(B *b, const char *who, void (*release)(B *, int *))
{
    if (!b) return 0;
    WtGuard guard_(b->ctx);
    (void)hipStreamSynchronize(b->ctx->stream);
    int bad = 0;
    release(b, &bad);
    delete b;
    if (bad) WT_FAIL("%s: a device buffer could not be released", who);
    return 0;
}

// `rows` rows of `w` bytes between device rows dpitch and host rows hpitch bytes apart, on the stream, NOT synchronised:
// one linear copy where both pitches are the width, a 2-D copy otherwise
static int lines_copy(hipStream_t st, void *dev, size_t dpitch, void *host, size_t hpitch, size_t w, size_t rows, bool up)
{
    const bool linear = dpitch == w && hpitch == w;
    if (up) {
        if (linear) WT_HIP(hipMemcpyAsync(dev, host, w * rows, hipMemcpyHostToDevice, st));
        else WT_HIP(hipMemcpy2DAsync(dev, dpitch, host, hpitch, w, rows, hipMemcpyHostToDevice, st));
    } else {
        if (linear) WT_HIP(hipMemcpyAsync(host, dev, w * rows, hipMemcpyDeviceToHost, st));
        else WT_HIP(hipMemcpy2DAsync(host, hpitch, dev, dpitch, w, rows, hipMemcpyDeviceToHost, st));
    }
    return 0;
}

// f(T()) with the element type of `itemsize` bytes; f(T(), K) with the taps of `family` too (K::value: 5 or 3)
template <typename F>
static inline void lines_by_type(int itemsize, F f) { itemsize == 4 ? f(float()) : f(double()); }
template <typename F>
static inline void lines_by_type_family(int itemsize, int family, F f)
{
    const bool b3 = family == WT_B3SPLINE;
    lines_by_type(itemsize, [&](auto t) { b3 ? f(t, std::integral_constant<int, 5>()) : f(t, std::integral_constant<int, 3>()); });
}

// 1 / tau of a float64 threshold: the host's IEEE division, as wt64_denoise_sum; 0 where the significance is one
static inline double lines_inv_tau(double t) { return t > 0.0 ? 1.0 / t : 0.0; }

// `flags` of the ..._ex entries: bit 0 = Anscombe, any other bit refused.  A mode of the CALL, never of the stack: stacks
// are cached and reused, and a mode left behind on one would silently change the next caller's result.
#define WT_LINES_ANSCOMBE 1
static inline int lines_flags(int flags, const char *who)
{
    if (flags & ~WT_LINES_ANSCOMBE) WT_FAIL("%s: flags %d (bit 0 = Anscombe; no other bit is defined)", who, flags);
    return 0;
}
