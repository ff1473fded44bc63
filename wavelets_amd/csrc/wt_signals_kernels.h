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
// ANS: every sample goes through wt_anscombe_fwd (wt_signal_common.h) on its way into LDS - the transform of
// generalized_anscombe(signal) (watroo/utils.py:93-95) at the traffic of the plain one; the input in HBM stays as it is.
template <typename T, int K, bool ANS>
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
    for (int i = threadIdx.x * PX; i < Np; i += WT_SIGNALS_THREADS * PX) {
        if constexpr (ANS) *reinterpret_cast<V *>(a + i) = wt_anscombe_fwd(*reinterpret_cast<const V *>(src + i));
        else *reinterpret_cast<V *>(a + i) = *reinterpret_cast<const V *>(src + i);
    }
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
// ANS: every sum goes through wt_anscombe_inv (wt_signal_common.h) before its one store - the inverse of
// watroo/utils.py:99-100 on np.sum(planes, axis=0), no pass of its own over the sum.
// double: tab[signal * 3 * n_den + k] = tau, [+ n_den + k] = the host's 1 / tau, [+ 2 * n_den + k] = the weight.
// The expressions of the double wt_signal_point, written out for the two samples of a group under ONE test of tau:
// through two calls of the point the compiler emits two tests and another register allocation - the same values,
// another instruction stream - so this one branch keeps its text ("One core for the two 1-D engines").
template <typename T, bool ANS>
__global__ __launch_bounds__(WT_SIGNALS_THREADS) void wt_signals_denoise_sum_kernel(WtSignalsSumArgs a)
{
    if constexpr (sizeof(T) == 4) {
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
            if constexpr (ANS) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = wt_anscombe_inv(acc[j]);
            }
            reinterpret_cast<float4 *>(a.dst)[i] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        }
    } else {
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
            if constexpr (ANS) acc = make_double2(wt_anscombe_inv(acc.x), wt_anscombe_inv(acc.y));
            reinterpret_cast<double2 *>(a.dst)[i] = acc;
        }
    }
}

// {sum, sum of squares} of every plane of every signal, in double (c.std() / np.mean(power) of watroo/utils.py:176-189;
// what wt_reduce / wt64_reduce give the per-signal call, in another fold order).  Grid x = signal * nplanes + plane
// (the planes of a stack lie back to back, Np elements each), 256 threads.
// THE ORDER IS FIXED, so the doubles are the same run to run: thread t folds its samples t, t + 256, t + 512, ... in
// index order, the 256 partial results go to LDS and a tree of fixed shape - partner t + 128, then t + 64, ... t + 1,
// a barrier between the steps - folds them; thread 0 writes moments[(signal * nplanes + plane) * 2 + {0, 1}].  No
// atomics.  Every partial result is a double PAIR {value, what the additions so far rounded away} (wt_two_sum; the
// square's own rounding error comes from one FMA), and the pair is folded into one double only at the very end: the
// factors of wow take sumsq / N - mean^2, which cancels - for a smooth plane on a pedestal to 1e-4 of its terms - so
// a rounding error of the sums is worth thousands of ulps of the result ("wow of 1-D signals").
__device__ __forceinline__ void wt_two_sum(double &hi, double &lo, double v, double vlo)
{
#pragma clang fp contract(off)
    const double s = hi + v;
    const double t = s - hi;
    const double e = (hi - (s - t)) + (v - t);
    hi = s;
    lo = lo + (e + vlo);
}
template <typename T>
__global__ __launch_bounds__(WT_SIGNALS_THREADS) void wt_signals_moments_kernel(const T *planes, int N, int Np, double *moments)
{
#pragma clang fp contract(off)
    __shared__ double red[4][WT_SIGNALS_THREADS];
    const T *p = planes + (int64_t)blockIdx.x * Np;
    double s = 0.0, sl = 0.0, q = 0.0, ql = 0.0;
    for (int x = threadIdx.x; x < N; x += WT_SIGNALS_THREADS) {
        const double v = (double)p[x];
        const double vv = v * v;
        wt_two_sum(s, sl, v, 0.0);
        wt_two_sum(q, ql, vv, fma(v, v, -vv));
    }
    red[0][threadIdx.x] = s;
    red[1][threadIdx.x] = sl;
    red[2][threadIdx.x] = q;
    red[3][threadIdx.x] = ql;
    __syncthreads();
    for (int off = WT_SIGNALS_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            wt_two_sum(s, sl, red[0][threadIdx.x + off], red[1][threadIdx.x + off]);
            wt_two_sum(q, ql, red[2][threadIdx.x + off], red[3][threadIdx.x + off]);
            red[0][threadIdx.x] = s;
            red[1][threadIdx.x] = sl;
            red[2][threadIdx.x] = q;
            red[3][threadIdx.x] = ql;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        moments[(int64_t)blockIdx.x * 2] = s + sl;
        moments[(int64_t)blockIdx.x * 2 + 1] = q + ql;
    }
}

// The per-scale loop of wow + np.sum(coefficients, axis=0) of every signal (watroo/utils.py:174-205 on a 1-D array,
// h = 0: no gamma sum), from the planes in HBM: per signal what wt_wow_scale / wt_wow_update per scale and
// wt_plane_sum give (wt64_smooth of the squares + wt64_wow_update + wt64_plane_sum in double), in ONE launch.
// Grid x = the signal, 256 threads.  A thread owns samples x = tid + 256 r through every scale (at most 8192 / 256 =
// 32 floats or 16 doubles: the LDS budget bounds the register array, as in wt_along_denoise_kernel) and keeps their
// running sum in registers - in plane order, starting from plane 0, contraction off.
// POWER (whitening): per detail scale s the thread squares its samples of plane s into an LDS buffer of Np elements;
// after ONE barrier the local power is conv_s(c^2) = wt_signal_smooth over the 'mirror' rule at dilation 2^s, read
// from that buffer.  Two buffers alternate with s: a wave that has passed the barrier of scale s + 1 writes the buffer
// of scale s + 2 = the buffer of scale s, which every wave has finished reading before it reached that barrier.
// Without POWER there is no LDS traffic and no barrier.  Every sample is then wt_wow_point's (wt_stencil.h): the
// significance, then factor * rsq(clip(power)) - the text of the per-frame and the batched 2-D kernels.  The last
// plane is multiplied by its factor and added.  tau: (signal, level) doubles, <= 0: significance one (the double
// point takes the quotient c / tau, as wt64_wow_kernel does: a staged 1 / tau would give other bits); factor:
// (signal, level + 1) doubles, rounded to T as the per-signal call rounds them.
// HBM traffic: sizeof(T) * (level + 1) read and sizeof(T) written per sample; with write_planes the planes are written
// back in place, sizeof(T) * (level + 1) more.  LDS: lane l of a wave writes element x0 + l and reads element
// x0 + l + const (away from the borders): consecutive lanes, consecutive addresses, no bank conflicts.
struct WtSignalsWowArgs {
    void *planes;            // (signal, level + 1, Np)
    void *sum;               // (signal, Np)
    const double *tau;       // (signal, level)
    const double *factor;    // (signal, level + 1)
    int N, Np, level, soft, write_planes;
};
template <typename T, int K, bool POWER>
__global__ __launch_bounds__(WT_SIGNALS_THREADS) void wt_signals_wow_kernel(WtSignalsWowArgs a)
{
#pragma clang fp contract(off)
    constexpr int ITEMS = WT_SIGNALS_LDS_BYTES / 2 / (int)sizeof(T) / WT_SIGNALS_THREADS;
    constexpr int hw = K / 2;
    extern __shared__ __align__(16) unsigned char wt_signals_lds[];
    T *sq0 = reinterpret_cast<T *>(wt_signals_lds);
    T *sq1 = sq0 + a.Np;
    const int64_t sig = blockIdx.x;
    T *pl = reinterpret_cast<T *>(a.planes) + sig * (int64_t)(a.level + 1) * a.Np;
    const double *taus = a.tau + sig * a.level;
    const double *fac = a.factor + sig * (a.level + 1);
    T acc[ITEMS];
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) acc[r] = (T)0;
    for (int s = 0; s < a.level; ++s) {
        const int d = 1 << s;
        const double tau = taus[s];
        const T tauf = (T)tau, factor = (T)fac[s];
        T *w = pl + (int64_t)s * a.Np;
        T *sq = (s & 1) ? sq1 : sq0;
        T c[ITEMS];
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            const int x = (int)threadIdx.x + r * WT_SIGNALS_THREADS;
            c[r] = (T)0;
            if (x < a.N) {
                c[r] = w[x];
                if constexpr (POWER) sq[x] = c[r] * c[r];
            }
        }
        if constexpr (POWER) __syncthreads();
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            const int x = (int)threadIdx.x + r * WT_SIGNALS_THREADS;
            if (x < a.N) {
                T pw = (T)0;
                if constexpr (POWER) {
                    T v[K];
#pragma unroll
                    for (int j = 0; j < K; ++j) v[j] = sq[wt_refl_b(x + (j - hw) * d, a.N, d, 2)];
                    pw = wt_signal_smooth<K>(v);
                }
                T g = (T)0;
                const T val = wt_wow_point(c[r], pw, POWER, (T)1, tau, tauf, a.soft, factor, g);
                acc[r] = s == 0 ? val : acc[r] + val;
                if (a.write_planes) w[x] = val;
            }
        }
    }
    T *last = pl + (int64_t)a.level * a.Np;
    T *dst = reinterpret_cast<T *>(a.sum) + sig * a.Np;
    const T factor = (T)fac[a.level];
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const int x = (int)threadIdx.x + r * WT_SIGNALS_THREADS;
        if (x < a.N) {
            T g = (T)0;
            const T val = wt_wow_point(last[x], (T)0, false, (T)1, 0.0, (T)0, a.soft, factor, g);
            dst[x] = acc[r] + val;
            if (a.write_planes) last[x] = val;
        }
    }
}
