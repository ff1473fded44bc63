// Arrays that stay on the device (wavelets_amd/resident.py): plain device blocks for the callers that have none of
// their own (wt_device_alloc / _free / _copy), and the copy between a caller's strided (nf, H, W) device array and
// frames of a batch plane (wt_batch_load_device / _store_device and the wt_batch64 pair) - what wt_batch_upload /
// wt_batch_download and wt_batch64_upload_elems do from and to host memory, without the two PCIe crossings.
//
// The unit reaches a batch through the C ABI alone (wt_batch_info, wt_batch_plane_ptr) plus the batch's context
// (wt_batch_ctx / wt_batch64_ctx, wt_host.h): it knows the layout of a plane - frames `frame_stride` elements apart,
// rows `pitch` elements apart - and nothing else of an engine.
//
// Streams.  The copies run on the context's stream, like every launch of the library.  A caller that produced the
// array on a stream of its own (or reads the result there) names it: stream_kind WT_STREAM_LEGACY (the legacy default
// stream), WT_STREAM_PER_THREAD (the per-thread default stream) or WT_STREAM_HANDLE (`stream` is a hipStream_t).  A load
// then makes the context's stream wait for what that stream holds so far, a store makes that stream wait for the copy:
// two events, no host synchronisation (resident_order, written once for the four entries).  WT_STREAM_NONE: the array
// is taken as ready, nothing is ordered.
#include <algorithm>

#include "wt_host.h"
#include "wt_resident_kernels.h"
#include "wt_unit_probe.h"

WT_UNIT_PROBE_DEFINE

// ------------------------------------------------------------------------------------------------ device blocks
extern "C" int wt_device_alloc(wt_ctx *c, size_t bytes, void **ptr)
{
    if (!c || !ptr) WT_FAIL("wt_device_alloc: null pointer");
    *ptr = nullptr;
    if (bytes == 0) return 0;                  // (an empty array: no block)
    WtGuard guard_(c);
    WT_HIP(hipMalloc(ptr, bytes));
    return 0;
}

extern "C" int wt_device_free(wt_ctx *c, void *ptr)
{
    if (!c) WT_FAIL("wt_device_free: null pointer");
    if (!ptr) return 0;
    WtGuard guard_(c);
    WT_HIP(hipFree(ptr));                      // (waits for the device: nothing queued still reads the block)
    return 0;
}

extern "C" int wt_device_copy(wt_ctx *c, void *dst, const void *src, size_t bytes, int kind)
{
    if (!c) WT_FAIL("wt_device_copy: null pointer");
    if (kind != WT_COPY_HOST_TO_DEVICE && kind != WT_COPY_DEVICE_TO_HOST && kind != WT_COPY_DEVICE_TO_DEVICE)
        WT_FAIL("wt_device_copy: kind %d (WT_COPY_HOST_TO_DEVICE, WT_COPY_DEVICE_TO_HOST or WT_COPY_DEVICE_TO_DEVICE)", kind);
    if (bytes == 0) return 0;
    if (!dst || !src) WT_FAIL("wt_device_copy: null pointer");
    WtGuard guard_(c);
    const void *host = kind == WT_COPY_HOST_TO_DEVICE ? src : (kind == WT_COPY_DEVICE_TO_HOST ? dst : nullptr);
    const bool pinned = host && try_pin(host, bytes);
    const hipMemcpyKind k = kind == WT_COPY_HOST_TO_DEVICE ? hipMemcpyHostToDevice
                            : (kind == WT_COPY_DEVICE_TO_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
    hipError_t e = hipMemcpyAsync(dst, src, bytes, k, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);       // the host block is free (or filled) when this returns
    if (e == hipSuccess) e = e2;
    if (pinned) (void)hipHostUnregister(const_cast<void *>(host));
    WT_HIP(e);
    return 0;
}

// ------------------------------------------------------------------------------------------------ stream hand-over
static int resident_stream(void *stream, int kind, const char *who, hipStream_t *st)
{
    switch (kind) {
        case WT_STREAM_NONE: *st = nullptr; return 0;
        case WT_STREAM_LEGACY: *st = nullptr; return 0;                  // (the null stream of this library's build: the legacy one)
        case WT_STREAM_PER_THREAD: *st = hipStreamPerThread; return 0;
        case WT_STREAM_HANDLE:
            if (!stream) WT_FAIL("%s: stream_kind WT_STREAM_HANDLE with a null stream", who);
            *st = (hipStream_t)stream;
            return 0;
        default: WT_FAIL("%s: stream_kind %d (WT_STREAM_NONE .. WT_STREAM_HANDLE)", who, kind);
    }
}

// `later` waits for everything `earlier` holds at this moment (the event is released once it has completed)
static int resident_order(hipStream_t earlier, hipStream_t later)
{
    if (earlier == later) return 0;
    hipEvent_t ev = nullptr;
    WT_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, earlier);
    if (e == hipSuccess) e = hipStreamWaitEvent(later, ev, 0);
    const hipError_t e2 = hipEventDestroy(ev);
    WT_HIP(e);
    WT_HIP(e2);
    return 0;
}

// ------------------------------------------------------------------------------------------------ load, store
static int resident_itemsize(int dtype)
{
    static const int isz[11] = {0, 1, 1, 2, 2, 4, 4, 8, 8, 4, 8};
    return dtype >= WT_INT8 && dtype <= WT_FLOAT64 ? isz[dtype] : 0;
}

template <typename E, typename T, bool STORE>
static void resident_launch(wt_ctx *c, void *array, T *plane, const WtResidentArgs &g, int nf, bool vec)
{
    const int G = vec ? 16 / (int)sizeof(T) : 1;
    const unsigned gx = (unsigned)(((int64_t)g.W + G - 1) / G + WT_RESIDENT_THREADS - 1) / WT_RESIDENT_THREADS;
    // about eight workgroups per compute unit in all, the rows of a frame strided over grid y
    const int64_t want = ((int64_t)c->num_cus * 8 + (int64_t)gx * nf - 1) / ((int64_t)gx * nf);
    const unsigned gy = (unsigned)std::min<int64_t>(g.H, std::max<int64_t>(1, want));
    const dim3 grid(gx, gy, (unsigned)nf), block(WT_RESIDENT_THREADS);
    ProfScope ps(c, STORE ? "wt_resident_copy_kernel<store>" : "wt_resident_copy_kernel<load>");
    if (vec) hipLaunchKernelGGL((wt_resident_copy_kernel<E, T, STORE, true>), grid, block, 0, c->stream, (char *)array, plane, g);
    else hipLaunchKernelGGL((wt_resident_copy_kernel<E, T, STORE, false>), grid, block, 0, c->stream, (char *)array, plane, g);
}

// the element types a plane of T takes exactly (what wt_upload_int hands a float plane and the reference's recast a
// double plane, among the types resident.eligible admits)
static bool resident_loads(int dtype, float) { return dtype == WT_UINT8 || dtype == WT_FLOAT32; }
static bool resident_loads(int dtype, double)
{
    return dtype == WT_UINT8 || dtype == WT_INT16 || dtype == WT_UINT16 || dtype == WT_INT32 || dtype == WT_FLOAT32 || dtype == WT_FLOAT64;
}

template <typename T>
static void resident_load_launch(wt_ctx *c, int dtype, void *array, T *plane, const WtResidentArgs &g, int nf, bool vec)
{
    if (dtype == WT_UINT8) return resident_launch<uint8_t, T, false>(c, array, plane, g, nf, vec);
    if constexpr (sizeof(T) == 8) {
        if (dtype == WT_INT16) return resident_launch<int16_t, T, false>(c, array, plane, g, nf, vec);
        if (dtype == WT_UINT16) return resident_launch<uint16_t, T, false>(c, array, plane, g, nf, vec);
        if (dtype == WT_INT32) return resident_launch<int32_t, T, false>(c, array, plane, g, nf, vec);
        if (dtype == WT_FLOAT32) return resident_launch<float, T, false>(c, array, plane, g, nf, vec);
    }
    resident_launch<T, T, false>(c, array, plane, g, nf, vec);          // (the plane's own type)
}

// One entry: every refusal is host logic and comes before any device work.  `info` / `plane_ptr`: the batch's own
// wt_batch_info / wt_batch_plane_ptr; dtype: the array's element type (a store: the plane's).
template <typename T, typename B>
static int resident_copy(B *b, wt_ctx *(*ctx_of_batch)(B *), int (*info)(B *, int64_t *), int (*plane_ptr)(B *, int, void **, int64_t *), int plane, int f0,
                         int nf, void *dev, int dtype, const int64_t *stride_bytes, void *stream, int stream_kind, bool store, const char *who)
{
    if (!b || !dev || !stride_bytes) WT_FAIL("%s: null pointer", who);
    int64_t v[7];
    WT_TRY(info(b, v));
    const int64_t n = v[0], H = v[1], W = v[2], P = v[3], fstride = v[4];
    if (f0 < 0 || nf < 1 || (int64_t)f0 + nf > n) WT_FAIL("%s: frames [%d, %lld) outside the batch of %lld", who, f0, (long long)f0 + nf, (long long)n);
    const int item = resident_itemsize(dtype);
    if (!item) WT_FAIL("%s: unknown element type %d", who, dtype);
    if (!resident_loads(dtype, T())) WT_FAIL("%s: element type %d is not one a %s plane takes exactly", who, dtype, sizeof(T) == 4 ? "float" : "double");
    for (int i = 0; i < 3; ++i)
        if (stride_bytes[i] <= 0 || stride_bytes[i] % item)
            WT_FAIL("%s: stride %lld bytes of axis %d (positive multiples of the %d bytes of an element)", who, (long long)stride_bytes[i], i, item);
    hipStream_t theirs = nullptr;
    WT_TRY(resident_stream(stream, stream_kind, who, &theirs));
    wt_ctx *c = ctx_of_batch(b);
    WtGuard guard_(c);
    WT_TRY(wt_side_join(c));
    void *q = nullptr;
    int64_t fs = 0;
    WT_TRY(plane_ptr(b, plane, &q, &fs));
    T *base = (T *)q + (int64_t)f0 * fstride;
    WtResidentArgs g;
    g.a_frame = stride_bytes[0];
    g.a_row = stride_bytes[1];
    g.a_col = stride_bytes[2];
    g.p_frame = fstride;
    g.W = (int)W;
    g.P = (int)P;
    g.H = (int)H;
    const bool vec = g.a_col == item && (((uintptr_t)dev | (uintptr_t)g.a_row | (uintptr_t)g.a_frame) & 15) == 0 &&
                     (((uintptr_t)base | (uintptr_t)(P * sizeof(T)) | (uintptr_t)(fstride * sizeof(T))) & 15) == 0;
    if (!store && stream_kind != WT_STREAM_NONE) WT_TRY(resident_order(theirs, c->stream));
    if (store) resident_launch<T, T, true>(c, dev, base, g, nf, vec);
    else resident_load_launch<T>(c, dtype, dev, base, g, nf, vec);
    WT_HIP(hipGetLastError());
    if (store && stream_kind != WT_STREAM_NONE) WT_TRY(resident_order(c->stream, theirs));
    return 0;
}

extern "C" int wt_batch_load_device(wt_batch *b, int plane, int f0, int nf, const void *dev, int dtype, const int64_t stride_bytes[3], void *stream,
                                    int stream_kind)
{
    return resident_copy<float>(b, wt_batch_ctx, wt_batch_info, wt_batch_plane_ptr, plane, f0, nf, const_cast<void *>(dev), dtype, stride_bytes, stream,
                                stream_kind, false, "wt_batch_load_device");
}

extern "C" int wt_batch_store_device(wt_batch *b, int plane, int f0, int nf, void *dev, const int64_t stride_bytes[3], void *stream, int stream_kind)
{
    return resident_copy<float>(b, wt_batch_ctx, wt_batch_info, wt_batch_plane_ptr, plane, f0, nf, dev, WT_FLOAT32, stride_bytes, stream, stream_kind, true,
                                "wt_batch_store_device");
}

extern "C" int wt_batch64_load_device(wt_batch64 *b, int plane, int f0, int nf, const void *dev, int dtype, const int64_t stride_bytes[3], void *stream,
                                      int stream_kind)
{
    return resident_copy<double>(b, wt_batch64_ctx, wt_batch64_info, wt_batch64_plane_ptr, plane, f0, nf, const_cast<void *>(dev), dtype, stride_bytes,
                                 stream, stream_kind, false, "wt_batch64_load_device");
}

extern "C" int wt_batch64_store_device(wt_batch64 *b, int plane, int f0, int nf, void *dev, const int64_t stride_bytes[3], void *stream, int stream_kind)
{
    return resident_copy<double>(b, wt_batch64_ctx, wt_batch64_info, wt_batch64_plane_ptr, plane, f0, nf, dev, WT_FLOAT64, stride_bytes, stream,
                                 stream_kind, true, "wt_batch64_store_device");
}
