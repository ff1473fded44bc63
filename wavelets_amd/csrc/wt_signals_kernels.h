// Kernels of the signal unit (wt_signals.hip): stacks of 1-D signals of one length, one workgroup per signal, the
// whole transform of a signal in LDS.  The reference transforms a signal with scipy's 'mirror' border
// (watroo/wavelets.py:65-69, 408-444); the per-signal call runs it as a 1 x N image, one launch per scale.  Here a
// signal is read from HBM once, its scales ping-pong between two LDS buffers, and every plane is written once.
// Every sample gets the bits of the per-signal call.  gfx950 only.
#pragma once
#include "wt_signal_common.h"      // the LDS budget, wt_signal_smooth, wt_signal_point and the median helpers: shared with wt_along_kernels.h

// AtrousTransform.atrous_standard of every signal (watroo/wavelets.py:408-444 over the 1-D branch of convolution(),
// :65-69).  Grid x = the signal, 256 threads.  in: signals Np elements apart (Np a multiple of the 16-byte group, the
// padding readable); planes: (signal, level + 1, Np).  Dynamic LDS: 2 * Np elements.
// HBM traffic: the signal once, level + 1 planes once: sizeof(T) * (level + 2) bytes per sample.
// LDS: at every dilation lane l of a wave reads element x0 + l + const of the source buffer (away from the borders)
// and writes element x0 + l of the other one - consecutive lanes, consecutive addresses, no bank conflicts.
template <typename T, int K>
__global__ __launch_bounds__(WT_SIGNALS_THREADS) void wt_signals_decompose_kernel(const T *in, T *planes, int N, int Np, int level)
{
    typedef typename WtVec<T>::V V;
    constexpr int PX = WtVec<T>::PX;
    constexpr int hw = K / 2;
    extern __shared__ __align__(16) unsigned char wt_signals_lds[];
    T *a = reinterpret_cast<T *>(wt_signals_lds);
    T *b = a + Np;
    const int64_t sig = blockIdx.x;
    const T *src = in + sig * Np;
    T *out = planes + sig * (int64_t)(level + 1) * Np;
    for (int i = threadIdx.x * PX; i < Np; i += WT_SIGNALS_THREADS * PX)
        *reinterpret_cast<V *>(a + i) = *reinterpret_cast<const V *>(src + i);
    __syncthreads();
    for (int s = 0; s < level; ++s) {
        const int d = 1 << s;
        T *w = out + (int64_t)s * Np;
        for (int x = threadIdx.x; x < N; x += WT_SIGNALS_THREADS) {
            T v[K];
#pragma unroll
            for (int j = 0; j < K; ++j) v[j] = a[wt_refl_b(x + (j - hw) * d, N, d, 2)];
            const T c = wt_signal_smooth<K>(v);
            b[x] = c;
            w[x] = a[x] - c;                             // w_s = c_s - c_{s+1}   watroo/wavelets.py:442
        }
        __syncthreads();
        T *t = a;
        a = b;
        b = t;
    }
    T *last = out + (int64_t)level * Np;
    for (int x = threadIdx.x; x < N; x += WT_SIGNALS_THREADS) last[x] = a[x];
}

// np.median(np.abs(w_0)) of every signal (watroo/wavelets.py:126-127), exact, the definition of wt_abs_median /
// wt64_abs_median: with the sorted magnitudes v, v[(N - 1) / 2] for an odd N and the mean of that and the next one,
// in T, for an even N.  Grid x = the signal.  The magnitudes' bit patterns (which order like the values) are sorted
// in LDS by a bitonic network over the next power of two, the tail filled with all-ones keys; no register arrays.
// plane: plane 0 of signal 0, `stride` elements from one signal's to the next.  Dynamic LDS: n2 keys.
template <typename T>
__global__ __launch_bounds__(WT_SIGNALS_THREADS) void wt_signals_abs_median_kernel(const T *plane, int64_t stride, int N, int n2, T *medians)
{
    typedef typename WtSignalKey<T>::U U;
    extern __shared__ __align__(16) unsigned char wt_signals_lds[];
    U *key = reinterpret_cast<U *>(wt_signals_lds);
    const T *w = plane + (int64_t)blockIdx.x * stride;
    for (int i = threadIdx.x; i < n2; i += WT_SIGNALS_THREADS) {
        U u = ~(U)0;
        if (i < N) u = wt_signal_abs_key(w[i]);
        key[i] = u;
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n2 >> 1); t += WT_SIGNALS_THREADS) {
                const int lo = WT_SIGNAL_PAIR_LO(t, j), hi = lo + j;
                const U x = key[lo], y = key[hi];
                const bool up = (lo & k) == 0;
                if ((x > y) == up) {
                    key[lo] = y;
                    key[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        const int klo = (N - 1) / 2;
        medians[blockIdx.x] = wt_signal_median<T>(key, klo, klo + 1, N);
    }
}

// Coefficients.denoise over the first n_den planes of every signal + np.sum(planes, axis=0) (watroo/wavelets.py:
// 145-149, utils.py:98), from the planes in HBM: the per-signal wt_denoise_sum / wt64_denoise_sum with one row of
// thresholds and one of weights per signal.  A lane owns one 16-byte group; g = groups per signal (Np / PX).
// Every thresholded sample is wt_signal_point's (wt_signal_common.h), the sum in plane order, contraction off.
// float: tab[signal * 2 * n_den + k] = tau (<= 0: the significance is one), [+ n_den + k] = the weight.
struct WtSignalsSumArgs {
    const void *planes;     // (signal, n, Np)
    void *dst;              // (signal, Np)
    const double *tab;
    int64_t groups;         // all signals' groups
    int g, Np, n, n_den, soft;
};
template <typename T>
__global__ __launch_bounds__(WT_SIGNALS_THREADS) void wt_signals_denoise_sum_kernel(WtSignalsSumArgs a);

template <>
__global__ __launch_bounds__(WT_SIGNALS_THREADS) void wt_signals_denoise_sum_kernel<float>(WtSignalsSumArgs a)
{
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.groups; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i / a.g;
        const int r = (int)(i - f * a.g);
        const double *ft = a.tab + f * 2 * a.n_den;
        const float *p = reinterpret_cast<const float *>(a.planes) + f * (int64_t)a.n * a.Np + 4 * r;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < a.n; ++k) {
            const float4 v = *reinterpret_cast<const float4 *>(p + (int64_t)k * a.Np);
            float c[4] = {v.x, v.y, v.z, v.w};
            if (k < a.n_den) {
                const double t = ft[k], wgt = ft[a.n_den + k];
#pragma unroll
                for (int j = 0; j < 4; ++j) c[j] = wt_signal_point(c[j], t, 0.0, wgt, a.soft);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = k == 0 ? c[j] : acc[j] + c[j];
        }
        reinterpret_cast<float4 *>(a.dst)[i] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}

// double: tab[signal * 3 * n_den + k] = tau, [+ n_den + k] = the host's 1 / tau, [+ 2 * n_den + k] = the weight.
// The expressions of the double wt_signal_point, written out for the two samples of a group under ONE test of tau:
// through two calls of the point the compiler emits two tests and another register allocation - the same values,
// another instruction stream - so this one kernel keeps its text ("One core for the two 1-D engines").
template <>
__global__ __launch_bounds__(WT_SIGNALS_THREADS) void wt_signals_denoise_sum_kernel<double>(WtSignalsSumArgs a)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.groups; i += (int64_t)gridDim.x * 256) {
        const int64_t f = i / a.g;
        const int r = (int)(i - f * a.g);
        const double *ft = a.tab + f * 3 * a.n_den;
        const double *p = reinterpret_cast<const double *>(a.planes) + f * (int64_t)a.n * a.Np + 2 * r;
        double2 acc = make_double2(0.0, 0.0);
        for (int k = 0; k < a.n; ++k) {
            double2 v = *reinterpret_cast<const double2 *>(p + (int64_t)k * a.Np);
            if (k < a.n_den) {
                const double tau = ft[k], inv_tau = ft[a.n_den + k], wgt = ft[2 * a.n_den + k];
                double2 sg = make_double2(1.0, 1.0);
                if (tau > 0.0) sg = make_double2(wt_sig64_inv(v.x, tau, inv_tau, a.soft), wt_sig64_inv(v.y, tau, inv_tau, a.soft));
                v = make_double2(v.x * (wgt * sg.x), v.y * (wgt * sg.y));
            }
            acc = k == 0 ? v : make_double2(acc.x + v.x, acc.y + v.y);
        }
        reinterpret_cast<double2 *>(a.dst)[i] = acc;
    }
}
