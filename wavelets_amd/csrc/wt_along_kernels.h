// Kernels of the axis unit (wt_along.hip): the 1-D transform along an axis of an array that is NOT its last one - the
// light curve of every pixel of a (T, H, W) movie, the spectrum of every pixel of a (lambda, Y, X) raster.  The array
// is viewed as (O, N, I): N samples of one signal lie I elements apart, and the I signals of one outer index are
// neighbours in memory.  A workgroup takes one outer index and a tile of TI neighbouring signals, loads all N samples
// of the tile into LDS as [n][ti] in contiguous runs of TI elements, filters along n with the lanes running along ti,
// and writes every plane once in the layout of the input: no transpose anywhere.
// The arithmetic is the signal unit's - wt_signal_smooth, wt_signal_point and the median helpers of
// wt_signal_common.h, which both units include - so every sample carries the bits of transform_signals /
// denoise_signals on the transposed stack.  gfx950 only.
#pragma once
#include "wt_signal_common.h"      // WT_SIGNALS_LDS_BYTES, wt_signal_smooth, wt_signal_point and the median helpers

// The tile: the two ping-pong buffers of N x TI elements share the signal unit's 64 KiB (WT_SIGNALS_LDS_BYTES).  A
// CHOSEN budget, not a measured optimum.  TI is the largest power of two that fits, at most WT_ALONG_MAX_TILE - and it
// is never adapted to a narrow I: a tile wider than I has idle lanes.  Runs shorter than WT_ALONG_MIN_RUN_BYTES are
// not taken (wt_along_ok), which admits N <= 512 in float32 (TI = 16) and in float64 (TI = 8).
#define WT_ALONG_THREADS 256
#define WT_ALONG_MAX_TILE 256
#define WT_ALONG_MIN_RUN_BYTES 64

struct WtAlongArgs {
    const void *in;        // (oc, N, ic)
    void *out;             // decompose: (level + 1, oc, N, ic); abs_median: (oc, ic); denoise: (oc, N, ic)
    const double *tab;     // denoise: (oc, ic, n_den) thresholds; double: (oc, ic, 2, n_den), then 1 / tau
    double wgt[WT_MAX_SUM_PLANES];       // denoise: the one row of weights
    int64_t plane;         // elements of one plane: oc * N * ic
    int N, ic, tiles;      // samples, inner positions of the chunk, tiles per outer index
    int TI, lg;            // the tile and its log2
    int level, n_den, soft;
    int n2, k5;            // abs_median: the next power of two of N; the family (1: five taps, 0: three)
};

// where a workgroup's tile starts: element (o, 0, i0) of an (oc, N, ic) block, and i0
__device__ __forceinline__ int64_t wt_along_tile(const WtAlongArgs &a, int *i0)
{
    const int64_t o = blockIdx.x / (unsigned)a.tiles;
    *i0 = (int)(blockIdx.x - o * a.tiles) << a.lg;
    return o * (int64_t)a.N * a.ic + *i0;
}

// the tile of the input into LDS as [n][ti]: element e = n * TI + ti is taken by thread e % 256, so a wave reads
// HBM runs of TI contiguous elements and writes consecutive LDS addresses.  Columns past the right edge of the chunk
// (a partial tile) hold zeros: they are computed and never stored.  ANS: every sample of the chunk goes through
// wt_anscombe_fwd (wt_signal_common.h) on its way into LDS (watroo/utils.py:93-94); the block in HBM stays as it is.
template <typename T, bool ANS>
__device__ __forceinline__ void wt_along_load(const WtAlongArgs &a, T *buf, int64_t base, int i0)
{
    const T *src = reinterpret_cast<const T *>(a.in) + base;
    const int total = a.N << a.lg;
    const int ti = threadIdx.x & (a.TI - 1);
    const bool ok = i0 + ti < a.ic;
    if constexpr (ANS) {
        for (int e = threadIdx.x; e < total; e += WT_ALONG_THREADS) buf[e] = ok ? wt_anscombe_fwd(src[(int64_t)(e >> a.lg) * a.ic + ti]) : (T)0;
    } else {
        for (int e = threadIdx.x; e < total; e += WT_ALONG_THREADS) buf[e] = ok ? src[(int64_t)(e >> a.lg) * a.ic + ti] : (T)0;
    }
}

// c_{s+1} at sample n of column ti from the buffer p of c_s, under the 'mirror' rule of the signal unit
template <typename T, int K>
__device__ __forceinline__ T wt_along_smooth(const T *p, int n, int ti, int N, int lg, int d)
{
    constexpr int hw = K / 2;
    T v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = p[(wt_refl_b(n + (j - hw) * d, N, d, 2) << lg) + ti];
    return wt_signal_smooth<K>(v);
}

// AtrousTransform.atrous_standard of every signal along the middle axis of an (oc, N, ic) block (watroo/wavelets.py:
// 408-444 over the 1-D branch of convolution(), :65-69).  Grid x = (outer index, tile of TI inner positions), 256
// threads.  Dynamic LDS: 2 * N * TI elements.
// HBM traffic: the block once, level + 1 planes once: sizeof(T) * (level + 2) bytes per sample, in runs of TI elements.
// LDS: element e = n * TI + ti belongs to thread e % 256 (TI divides 256, so a thread keeps its column): lane l of a
// wave reads address e0 + l + const * TI of the source buffer (away from the borders) and writes address e0 + l of the
// other one - consecutive lanes, consecutive addresses, no bank conflicts.
template <typename T, int K>
__global__ __launch_bounds__(WT_ALONG_THREADS) void wt_along_decompose_kernel(WtAlongArgs a)
{
    extern __shared__ __align__(16) unsigned char wt_along_lds[];
    const int total = a.N << a.lg;
    T *p = reinterpret_cast<T *>(wt_along_lds);
    T *q = p + total;
    int i0;
    const int64_t base = wt_along_tile(a, &i0);
    const int ti = threadIdx.x & (a.TI - 1);
    const bool ok = i0 + ti < a.ic;
    wt_along_load<T, false>(a, p, base, i0);
    __syncthreads();
    T *out = reinterpret_cast<T *>(a.out) + base + ti;
    for (int s = 0; s < a.level; ++s) {
        const int d = 1 << s;
        T *w = out + (int64_t)s * a.plane;
        for (int e = threadIdx.x; e < total; e += WT_ALONG_THREADS) {
            const int n = e >> a.lg;
            const T c = wt_along_smooth<T, K>(p, n, ti, a.N, a.lg, d);
            q[e] = c;
            if (ok) w[(int64_t)n * a.ic] = p[e] - c;            // w_s = c_s - c_{s+1}   watroo/wavelets.py:442
        }
        __syncthreads();
        T *t = p;
        p = q;
        q = t;
    }
    T *last = out + (int64_t)a.level * a.plane;
    if (ok)
        for (int e = threadIdx.x; e < total; e += WT_ALONG_THREADS) last[(int64_t)(e >> a.lg) * a.ic] = p[e];
}

// np.median(np.abs(w_0)) of every signal of the block (watroo/wavelets.py:126-127), exact, with the even / odd rule of
// wt_signals_abs_median_kernel: with the sorted magnitudes v, v[(N - 1) / 2] for an odd N and the mean of that and the
// next one, in T, for an even N.  The same tiling.  Only scale 0 is computed, in LDS, and no plane is written: the
// block is read once and one median per signal leaves.  The tile is loaded into the SECOND buffer; the bit patterns of
// |w_0| (which order like the values) go to the first one as [n][ti]; the rows N .. n2 - 1 of all-ones padding then
// overwrite the input, which is dead by then (n2 <= 2 N: the keys stay within the two buffers).  A bitonic network
// sorts every column over n2 rows; its (n2 / 2) * TI compare-exchanges of a stage are spread over the 256 threads with
// ti fastest: consecutive lanes, consecutive LDS addresses.  out: (oc, ic) medians.
// ANS: the medians of generalized_anscombe(block) - the noise level refers to the transformed data (watroo/utils.py:95-97).
template <typename T, bool ANS>
__global__ __launch_bounds__(WT_ALONG_THREADS) void wt_along_abs_median_kernel(WtAlongArgs a)
{
    typedef typename WtSignalKey<T>::U U;
    extern __shared__ __align__(16) unsigned char wt_along_lds[];
    const int total = a.N << a.lg;
    U *key = reinterpret_cast<U *>(wt_along_lds);
    T *src = reinterpret_cast<T *>(wt_along_lds) + total;
    int i0;
    const int64_t base = wt_along_tile(a, &i0);
    const int ti = threadIdx.x & (a.TI - 1);
    wt_along_load<T, ANS>(a, src, base, i0);
    __syncthreads();
    for (int e = threadIdx.x; e < total; e += WT_ALONG_THREADS) {
        const int n = e >> a.lg;
        const T c = a.k5 ? wt_along_smooth<T, 5>(src, n, ti, a.N, a.lg, 1) : wt_along_smooth<T, 3>(src, n, ti, a.N, a.lg, 1);
        key[e] = wt_signal_abs_key(src[e] - c);
    }
    __syncthreads();
    for (int e = total + threadIdx.x; e < (a.n2 << a.lg); e += WT_ALONG_THREADS) key[e] = ~(U)0;
    __syncthreads();
    const int pairs = (a.n2 >> 1) << a.lg;
    for (int k = 2; k <= a.n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int e = threadIdx.x; e < pairs; e += WT_ALONG_THREADS) {
                const int lo = WT_SIGNAL_PAIR_LO(e >> a.lg, j);            // the rows (lo, lo + j) of column ti
                const int alo = (lo << a.lg) + ti, ahi = ((lo + j) << a.lg) + ti;
                const U x = key[alo], y = key[ahi];
                const bool up = (lo & k) == 0;
                if ((x > y) == up) {
                    key[alo] = y;
                    key[ahi] = x;
                }
            }
            __syncthreads();
        }
    }
    if ((int)threadIdx.x < a.TI && i0 + ti < a.ic) {
        const int klo = (a.N - 1) / 2;
        const T med = wt_signal_median<T>(key, (klo << a.lg) + ti, ((klo + 1) << a.lg) + ti, a.N);
        const int64_t o = blockIdx.x / (unsigned)a.tiles;
        reinterpret_cast<T *>(a.out)[o * a.ic + i0 + ti] = med;
    }
}

// Coefficients.denoise over the first n_den planes + np.sum(planes, axis=0) of every signal of the block
// (watroo/wavelets.py:145-149, utils.py:98), fused with the transform: the tile is loaded and decomposed in LDS as in
// wt_along_decompose_kernel, every detail sample is thresholded and weighted as it appears (wt_signal_point) and added
// to its owner's register - in plane order, starting from plane 0, contraction off - the last smooth plane is added,
// and ONLY the sum is written.  A thread owns elements e = tid + 256 r of the tile through every scale (at most
// 8192 / 256 = 32 floats or 16 doubles: the LDS budget bounds the register array) and with them one column, so it
// reads its signal's thresholds once per scale.  HBM traffic: sizeof(T) read and sizeof(T) written per sample, plus
// the thresholds; no plane reaches HBM.  LDS: as wt_along_decompose_kernel.
// ANS: wt_anscombe_fwd at the load and wt_anscombe_inv on the sum before its one store (watroo/utils.py:93-94, 99-100):
// denoise(..., anscombe=True) of every signal at the same traffic, no pass of its own over the block or the sum.
template <typename T, int K, bool ANS>
__global__ __launch_bounds__(WT_ALONG_THREADS) void wt_along_denoise_kernel(WtAlongArgs a)
{
#pragma clang fp contract(off)
    constexpr int ITEMS = WT_SIGNALS_LDS_BYTES / 2 / (int)sizeof(T) / WT_ALONG_THREADS;
    constexpr int per = sizeof(T) == 8 ? 2 : 1;
    extern __shared__ __align__(16) unsigned char wt_along_lds[];
    const int total = a.N << a.lg;
    T *p = reinterpret_cast<T *>(wt_along_lds);
    T *q = p + total;
    int i0;
    const int64_t base = wt_along_tile(a, &i0);
    const int ti = threadIdx.x & (a.TI - 1);
    const bool ok = i0 + ti < a.ic;
    wt_along_load<T, ANS>(a, p, base, i0);
    __syncthreads();
    const int64_t o = blockIdx.x / (unsigned)a.tiles;
    const double *ft = a.tab + (o * a.ic + i0 + ti) * (int64_t)(per * a.n_den);
    T acc[ITEMS];
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) acc[r] = (T)0;
    for (int s = 0; s < a.level; ++s) {
        const int d = 1 << s;
        const bool den = s < a.n_den;
        const double tau = den && ok ? ft[s] : 0.0;
        const double inv_tau = den && ok && per == 2 ? ft[a.n_den + s] : 0.0;
        const double wgt = den ? a.wgt[s] : 1.0;
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            const int e = (int)threadIdx.x + r * WT_ALONG_THREADS;
            if (e < total) {
                const T c = wt_along_smooth<T, K>(p, e >> a.lg, ti, a.N, a.lg, d);
                q[e] = c;
                T w = p[e] - c;
                if (den) w = wt_signal_point(w, tau, inv_tau, wgt, a.soft);
                acc[r] = s == 0 ? w : acc[r] + w;
            }
        }
        __syncthreads();
        T *t = p;
        p = q;
        q = t;
    }
    T *dst = reinterpret_cast<T *>(a.out) + base + ti;
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const int e = (int)threadIdx.x + r * WT_ALONG_THREADS;
        if constexpr (ANS) {
            if (e < total && ok) dst[(int64_t)(e >> a.lg) * a.ic] = wt_anscombe_inv(acc[r] + p[e]);
        } else {
            if (e < total && ok) dst[(int64_t)(e >> a.lg) * a.ic] = acc[r] + p[e];
        }
    }
}
