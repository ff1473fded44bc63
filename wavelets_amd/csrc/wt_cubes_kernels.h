// One scale of the a-trous transform of a (Z, Y, X) cube in ONE launch: the x, y and z filters of the 3-D
// branch of convolution() (watroo/wavelets.py:46-64) and the detail subtraction (wavelets.py:442).  The cube is
// stored as everywhere in the library, a (Z*Y) x X image with pitch P.  One text for both element types (WtVec<T>):
// T = float - a lane owns a float4 group - or T = double - a double2 group; 16 bytes per access and the same
// registers and LDS either way.  The same march over the SQUARES of a detail plane, with the pointwise update of wow as
// its epilogue, is the whitening of one scale of wow on a cube (wt_cube_wow_kernel, below).  gfx950 only.
//
// A workgroup of 4 waves owns 64 PX columns (64 lanes x one group: 256 float / 128 double columns), TY = 8 rows of
// one polyphase row class y = q_y + d (r0 + i) and a chunk of one polyphase chain along z, z = q_z + d t.  Per chain
// step it
//   1. x-filters the TY + 2 hw rows y + (j - hw) d of slice z + hw d into LDS (wt_hrow_filter, the row filter of
//      every per-scale kernel; the rows go round the waves so that the wave that owns output row i is the one that
//      filters row i + hw and keeps its centre samples, c_s, in registers),
//   2. y-filters its two output rows from LDS,
//   3. pushes the result into a K-deep register ring whose z-filter is c_{s+1}(z), and stores c_{s+1}(z) and
//      w_s(z) = c_s(z) - c_{s+1}(z), c_s(z) being the centre sample that entered hw steps earlier.
// The LDS rows are double-buffered: one barrier per step.  Reflected rows and slices (wt_refl_b under the symmetric
// border) may lie in another residue class: they are simply filtered where they are needed; a chunk pays K - 1
// warm-up slices.  The ring and the centres are indexed through fully unrolled loops only (registers, no scratch).
//
// Bit contract: every K-tap sum is tap(0) v_0 followed by fma(tap(j), v_j, acc) for ascending j, x first, then y,
// then z - the arithmetic of wt_hrow_filter + WtVert (wt_stencil.h) on each slice followed by wt_zfilter_kernel
// and wt_binary(SUB) (wt_kernels_apps.h), so the planes equal those of wt_decompose3d bit for bit.  For double it is
// the arithmetic of wt64_rows_kernel / wt64_rows2_kernel and of wt64_axis_kernel on axis 1, then on axis 0 with the
// detail cen - acc (wt_kernels_f64.h: smooth64 with depth > 0), with the dyadic taps fused64_family recognises.
#pragma once
#include <hip/hip_runtime.h>

#include "wt_internal.h"
#include "wt_device.h"
#include "wt_stencil.h"

#define WT_CUBE_TY 8          // output rows of a workgroup (two per wave)

template <typename T>
struct CubeArgsT {
    const T *in;       // c_s
    T *out_c;          // c_{s+1}
    T *out_w;          // w_s
    int W, P;          // columns, row pitch (elements)
    int Y, Z;          // rows per slice, slices
    int d;             // dilation 2^s
    int ycls, zcls;    // row classes min(d, Y), z chains min(d, Z)
    int S;             // chain steps per chunk
    int nt;            // streaming stores (planes far larger than the caches)
};
typedef CubeArgsT<float> CubeArgs;

// grid: x = blocks of 64 PX columns, y = row class + ycls * row group, z = z chain + zcls * chunk
// The march of both kernels of this file.  HMODE is the mode of the row filter: MODE_SMOOTH, or MODE_SMOOTH_SQ - the
// rows are the SQUARES of the loaded samples, v * v rounded once in T as wt_binary(MUL) / wt64_binary(mul) store it,
// while the centre kept for the epilogue is the sample itself.  emit(off, x, lane_ok, cen, o) stores one lane's group
// of output row `off` (element offset of the row start): o = the z-filter result, cen = the centre sample that
// entered hw steps earlier.
template <typename T, int K, bool SMALL_D, int HMODE, typename Emit>
__device__ __forceinline__ void wt_cube_march(const CubeArgsT<T> &a, Emit emit)
{
    typedef typename WtVec<T>::V V;
    constexpr int PX = WtVec<T>::PX;
    constexpr int hw = K / 2;
    constexpr int TY = WT_CUBE_TY;
    constexpr int NR = TY + 2 * hw;          // x-filtered rows per step
    constexpr int RPW = (NR + 3) / 4;        // ... per wave
    __shared__ V xf[2][NR][64];

    const int lane = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.y);      // wave-uniform by construction
    const int d = a.d;
    const int x = (blockIdx.x * 64 + lane) * PX;
    const int qy = blockIdx.y % a.ycls, rg = blockIdx.y / a.ycls;
    const int qz = blockIdx.z % a.zcls, ck = blockIdx.z / a.zcls;
    const int ny = (a.Y - qy + d - 1) / d;   // rows of this class
    const int nz = (a.Z - qz + d - 1) / d;   // steps of this chain
    const int r0 = rg * TY;
    const int t0 = ck * a.S, t1 = min(t0 + a.S, nz);
    if (r0 >= ny || t0 >= t1) return;        // (the whole workgroup: no barrier is left waiting)
    const bool lane_ok = x < a.W;

    // rows this wave x-filters: rr = first + 4 m; output row i = wv + 4 mi has its centre in rr = i + hw
    const int first = (wv + hw) & 3;
    const int mshift = (wv + hw) >> 2;       // m of output row mi is mi + mshift
    int yrow[RPW];
#pragma unroll
    for (int m = 0; m < RPW; ++m)
        yrow[m] = wt_refl_b(qy + d * (r0 + first + 4 * m - hw), a.Y, d, 0);

    V ring[2][K], cen[2][hw + 1];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int j = 0; j < K; ++j) ring[mi][j] = wt_vzero<V>();
#pragma unroll
        for (int j = 0; j <= hw; ++j) cen[mi][j] = wt_vzero<V>();
    }

    const int nsteps = (t1 - t0) + K - 1;    // K - 1 warm-up slices, then one output slice per step
    for (int k = 0; k < nsteps; ++k) {
        const int buf = k & 1;
        const int zc = qz + d * (t0 + k - (K - 1));          // the slice this step completes (k >= K - 1)
        const int zs = wt_refl_b(zc + hw * d, a.Z, d, 0);    // the slice that enters
        const T *slice = a.in + (int64_t)zs * a.Y * a.P;
        V cnew[2];
        cnew[0] = cnew[1] = wt_vzero<V>();
#pragma unroll
        for (int m = 0; m < RPW; ++m) {
            const int rr = first + 4 * m;
            if (rr < NR) {
                V raw[K], h = wt_vzero<V>(), h2 = wt_vzero<V>(), c;
                wt_hrow_load<T, K, SMALL_D>(slice + (int64_t)yrow[m] * a.P, x, d, a.W, raw, 0);
                wt_hrow_filter<T, K, HMODE, SMALL_D>(raw, d, h, h2, c);
                xf[buf][rr][lane] = h;
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
                    if (m == mi + mshift) cnew[mi] = c;
            }
        }
        __syncthreads();
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            const int i = wv + 4 * mi;
            V v = f4_scale(wt_tap_s<K, T>(0), xf[buf][i][lane]);
#pragma unroll
            for (int j = 1; j < K; ++j) v = f4_fma(wt_tap_s<K, T>(j), xf[buf][i + j][lane], v);
#pragma unroll
            for (int j = 0; j < K - 1; ++j) ring[mi][j] = ring[mi][j + 1];
            ring[mi][K - 1] = v;
#pragma unroll
            for (int j = 0; j < hw; ++j) cen[mi][j] = cen[mi][j + 1];
            cen[mi][hw] = cnew[mi];
            if (k >= K - 1 && r0 + i < ny) {
                V o = f4_scale(wt_tap_s<K, T>(0), ring[mi][0]);
#pragma unroll
                for (int j = 1; j < K; ++j) o = f4_fma(wt_tap_s<K, T>(j), ring[mi][j], o);
                const int64_t off = ((int64_t)zc * a.Y + (qy + d * (r0 + i))) * a.P;
                emit(off, x, lane_ok, cen[mi][0], o);
            }
        }
    }
}

template <typename T, int K, bool SMALL_D>
__global__ __launch_bounds__(256) void wt_cube_scale_kernel(CubeArgsT<T> a)
{
    typedef typename WtVec<T>::V V;
    wt_cube_march<T, K, SMALL_D, MODE_SMOOTH>(a, [=](int64_t off, int x, bool lane_ok, V cen, V o) {
        wt_storev<T, V>(a.out_c + off, x, a.P, o, a.nt, lane_ok);
        wt_storev<T, V>(a.out_w + off, x, a.P, f4_sub(cen, o), a.nt, lane_ok);
    });
}

// One scale of the whitening loop of wow on a cube (watroo/utils.py:193-203 over the 3-D branch of convolution(),
// wavelets.py:46-64) in ONE launch: the same march over the squares of w_s gives the local power conv_s(w_s^2), and
// the epilogue is the shared pointwise update wt_wow_point (wt_stencil.h) of the centre sample w_s - significance,
// gamma sum, factor * rsq(clip(power)).  One plane is stored, c.out_c, which must not be the input: neighbouring
// workgroups still read the old values (the host writes a spare plane and swaps the plane pointers).  c.out_w is unused.
// Bit contract: the squares are those of wt_binary(MUL), the power is that of wt_smooth3d / smooth64(depth) (x, y, z;
// every K-tap sum in ascending tap order) and the update is wt_wow_point's, so the plane equals the one
// mul + smooth3d + wow_update leave.
// PLAIN: no per-voxel noise map and no gamma accumulator - the march has no conditional loads (MODE_WOW_PLAIN,
// wt_stencil.h).  Otherwise `noise` and `gamma` may each be null; the gamma plane is read, added to and written at the
// same voxel only.
template <typename T>
struct CubeWowArgsT {
    CubeArgsT<T> c;
    const T *noise;    // per-voxel noise map or nullptr
    T *gamma;          // gamma accumulator or nullptr
    double tau;        // significance threshold (<= 0: none)
    T factor;          // w * power_norm
    int soft;
};

template <typename T, int K, bool SMALL_D, bool PLAIN>
__global__ __launch_bounds__(256) void wt_cube_wow_kernel(CubeWowArgsT<T> a)
{
    typedef typename WtVec<T>::V V;
    constexpr int PX = WtVec<T>::PX;
    wt_cube_march<T, K, SMALL_D, MODE_SMOOTH_SQ>(a.c, [&](int64_t off, int x, bool lane_ok, V cen, V o) {
        T cc[PX], pw[PX], nn[PX], gg[PX], r[PX];
        wt_vunpack(cen, cc);
        wt_vunpack(o, pw);
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            nn[k] = (T)1;
            gg[k] = (T)0;
        }
        if constexpr (!PLAIN) {
            const bool full = x + PX - 1 < a.c.W;
            if (a.noise && lane_ok) {
#pragma unroll
                for (int k = 0; k < PX; ++k) if (full || x + k < a.c.W) nn[k] = a.noise[off + x + k];
            }
            if (a.gamma && lane_ok) {
#pragma unroll
                for (int k = 0; k < PX; ++k) if (full || x + k < a.c.W) gg[k] = a.gamma[off + x + k];
            }
        }
        const T tauf = (T)a.tau;
#pragma unroll
        for (int k = 0; k < PX; ++k) r[k] = wt_wow_point(cc[k], pw[k], true, nn[k], a.tau, tauf, a.soft, a.factor, gg[k]);
        wt_storev<T, V>(a.c.out_c + off, x, a.c.P, wt_vpack(r), a.c.nt, lane_ok);
        if constexpr (!PLAIN) {
            if (a.gamma) wt_storev<T, V>(a.gamma + off, x, a.c.P, wt_vpack(gg), a.c.nt, lane_ok);
        }
    });
}
