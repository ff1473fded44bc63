// Kernels of the resident unit (wt_resident.hip): the copy between a caller's strided (nf, H, W) device array and
// frames of a batch plane (wt_batch: float planes, wt_batch64: double planes).  hipMemcpy2D does not serve here: it
// moves bytes, not elements (the load widens uint8 / int16 / uint16 / int32 as wt_upload_int and
// wt_batch64_widen_kernel do: one exact (T) conversion per element), it knows no inner stride, and it may refuse a range
// mapped over several physical chunks (include/watroo_hip.h, wt_plane_ptr).
//
// ONE kernel text: E the element type of the caller's array, T the plane's; STORE = plane -> array (E == T), else
// array -> plane.  Lanes run along x, rows are grid y (strided), the frame is grid z; every offset is 64-bit.
// VEC (chosen per launch by the host, never per lane): the inner stride is one element and every row of both sides
// starts on a 16-byte boundary - a lane moves one 16-byte group of the plane (4 floats, 2 doubles) and the matching
// 16 / sizeof(T) elements of the array as one access each; the last group of a row whose width is no multiple of the
// group goes element by element, so the plane's padding columns beyond W keep what they hold and the array is never
// touched beyond W.  Without VEC a lane moves one element.  One read and one write per element; no LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#define WT_RESIDENT_THREADS 256

struct WtResidentArgs {
    int64_t a_frame, a_row, a_col;      // the array: BYTES from frame to frame, row to row, element to element
    int64_t p_frame;                    // the plane: ELEMENTS from frame to frame
    int W, P, H;                        // width, plane pitch in elements, rows of a frame
};

template <typename X, int N>
struct alignas(sizeof(X) * N) WtResidentGroup {
    X v[N];
};

// N elements at column x0 of every row this lane serves: four rows' loads are issued before the first store, so a
// wave has four accesses in flight (register arrays under fully unrolled loops: no scratch)
template <typename E, typename T, bool STORE, int N>
__device__ __forceinline__ void wt_resident_rows(char *array, T *plane, const WtResidentArgs &g, int64_t x0, int64_t a_col)
{
    typedef WtResidentGroup<E, N> AG;
    typedef WtResidentGroup<T, N> PG;
    constexpr int U = 4;
    const int64_t gy = gridDim.y;
    char *acol = array + x0 * a_col;
    T *pcol = plane + x0;
    int64_t y = blockIdx.y;
    for (; y + (U - 1) * gy < g.H; y += U * gy) {
        if (STORE) {
            PG p[U];
#pragma unroll
            for (int u = 0; u < U; ++u) p[u] = *reinterpret_cast<const PG *>(pcol + (y + u * gy) * g.P);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                AG a;
#pragma unroll
                for (int k = 0; k < N; ++k) a.v[k] = (E)p[u].v[k];
                *reinterpret_cast<AG *>(acol + (y + u * gy) * g.a_row) = a;
            }
        } else {
            AG a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) a[u] = *reinterpret_cast<const AG *>(acol + (y + u * gy) * g.a_row);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                PG p;
#pragma unroll
                for (int k = 0; k < N; ++k) p.v[k] = (T)a[u].v[k];
                *reinterpret_cast<PG *>(pcol + (y + u * gy) * g.P) = p;
            }
        }
    }
    for (; y < g.H; y += gy) {
        AG *ap = reinterpret_cast<AG *>(acol + y * g.a_row);
        PG *pp = reinterpret_cast<PG *>(pcol + y * g.P);
        if (STORE) {
            const PG p = *pp;
            AG a;
#pragma unroll
            for (int k = 0; k < N; ++k) a.v[k] = (E)p.v[k];
            *ap = a;
        } else {
            const AG a = *ap;
            PG p;
#pragma unroll
            for (int k = 0; k < N; ++k) p.v[k] = (T)a.v[k];
            *pp = p;
        }
    }
}

template <typename E, typename T, bool STORE, bool VEC>
__global__ __launch_bounds__(WT_RESIDENT_THREADS) void wt_resident_copy_kernel(char *array, T *plane, WtResidentArgs g)
{
    static_assert(!STORE || sizeof(E) == sizeof(T), "a store hands the plane's own element type out");
    constexpr int G = VEC ? 16 / (int)sizeof(T) : 1;
    const int64_t x0 = ((int64_t)blockIdx.x * WT_RESIDENT_THREADS + threadIdx.x) * G;
    if (x0 >= g.W) return;
    const int64_t f = blockIdx.z;
    array += f * g.a_frame;
    plane += f * g.p_frame;
    if (VEC && x0 + G <= g.W) {
        wt_resident_rows<E, T, STORE, G>(array, plane, g, x0, (int64_t)sizeof(E));
    } else {                                  // (one element per lane, or the last, partial group of a row)
        for (int k = 0; k < G && x0 + k < g.W; ++k) wt_resident_rows<E, T, STORE, 1>(array, plane, g, x0 + k, g.a_col);
    }
}
