// Per-scale stencil kernels of the a-trous engine for gfx950: the chain march, the lattice kernel and the
// row kernel, written once for both element types (round 5).  A lane moves 16 bytes per access either
// way: T = float - a lane owns 4 adjacent pixels (float4) - or T = double - 2 pixels (double2); the
// register windows cost the same VGPRs, the float64 kernels are the float32 design at twice the bytes
// per pixel.  The reference computes float64 / integer inputs in float64 (watroo/wavelets.py:297,
// 319-320), so this is what every int16 / FITS frame runs on.
//
// Reference semantics restated by each kernel are cited as file:line under /root/reference.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "wt_internal.h"
#include "wt_device.h"
#include "wt_math64.h"

// Row pointer for GLOBAL row gy (any integer): reflect on the global image, then map into
// this strip's buffer (rows outside the strip live in the halo margins).
template <typename T>
__device__ __forceinline__ const T *wt_row(const T *base, const Geo &g, int gy)
{
    const int ry = wt_refl(gy, g.H);
    return base + (int64_t)(ry - g.row0) * g.P;
}

// border-mode aware forms used by the single-scale operators (d = dilation of the operator)
template <typename T>
__device__ __forceinline__ const T *wt_row_b(const T *base, const Geo &g, int gy, int d)
{
    const int ry = wt_refl_b(gy, g.H, d, g.border);
    return base + (int64_t)(ry - g.row0) * g.P;
}
// descriptor of one row (P elements of T) behind a wave-uniform pointer: range check = the row's pitch
template <typename T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wt_row_rsrc(const T *row, int P)
{
    const uint64_t ra = (uint64_t)row;
    const uint64_t ua = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(ra >> 32)) << 32) |
                        (uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)ra);
    return __builtin_amdgcn_make_buffer_rsrc((void *)ua, 0, P * (int)sizeof(T), 0x00020000);
}
// symmetric reflection of the bilateral kernels' two border rules (Geo::border 0 / 1; wt_refl_b without the
// 'mirror' rules the launch code refuses)
__device__ __forceinline__ int wt_refl_01(int i, int n, int d, int border)
{
    if ((unsigned)i < (unsigned)n) return i;
    if (border == 0) return wt_refl(i, n);
    int o = i % d;
    if (o < 0) o += d;
    return o + d * wt_refl((i - o) / d, (n - o + d - 1) / d);
}

__device__ __forceinline__ float4 wt_load4_b(const float *row, int xo, int W, int d, int border)
{
    if (xo >= 0 && xo + 3 < W) return *reinterpret_cast<const float4 *>(row + xo);
    return make_float4(row[wt_refl_b(xo, W, d, border)], row[wt_refl_b(xo + 1, W, d, border)],
                       row[wt_refl_b(xo + 2, W, d, border)], row[wt_refl_b(xo + 3, W, d, border)]);
}
// one lane's group of pixels starting at pixel xo (a multiple of the group size), reflected at the border
__device__ __forceinline__ float4 wt_loadv_b(const float *row, int xo, int W, int d, int border)
{
    return wt_load4_b(row, xo, W, d, border);
}
__device__ __forceinline__ double2 wt_loadv_b(const double *row, int xo, int W, int d, int border)
{
    if (xo >= 0 && xo + 1 < W) return *reinterpret_cast<const double2 *>(row + xo);
    return make_double2(row[wt_refl_b(xo, W, d, border)], row[wt_refl_b(xo + 1, W, d, border)]);
}

// 4 consecutive pixels starting at pixel xo (xo % 4 == 0) of a row, reflected at the image
// border.  Interior: one 16-byte load.
__device__ __forceinline__ float4 wt_load4(const float *row, int xo, int W)
{
    if (xo >= 0 && xo + 3 < W) return *reinterpret_cast<const float4 *>(row + xo);
    return make_float4(row[wt_refl(xo, W)], row[wt_refl(xo + 1, W)], row[wt_refl(xo + 2, W)],
                       row[wt_refl(xo + 3, W)]);
}

typedef unsigned int wt_su4 __attribute__((ext_vector_type(4)));
typedef float wt_sf4 __attribute__((ext_vector_type(4)));
typedef double wt_sd2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ wt_su4 wt_bits16(float4 v)
{
    const wt_sf4 t = {v.x, v.y, v.z, v.w};
    return __builtin_bit_cast(wt_su4, t);
}
__device__ __forceinline__ wt_su4 wt_bits16(double2 v)
{
    const wt_sd2 t = {v.x, v.y};
    return __builtin_bit_cast(wt_su4, t);
}
// 16-byte store of one lane's pixel group at pixel x of an image row (row = wave-uniform pointer to the
// row's first pixel, P = row pitch in elements) through a raw buffer descriptor: a lane that must not
// write (lane_ok false, or x beyond the row) gets an out-of-range offset and the hardware drops the
// store.  No exec-mask branch around the store, so the compiler's vmcnt bookkeeping stays exact:
// behind a branch it has to assume the store may not have been issued and every wait for the
// next row's loads also waits for this row's stores.  A group that straddles W writes into the
// row's pitch padding (allocated, never read as image data), like the fused passes.
// nt: streaming (nontemporal) store - the host sets it for planes far larger than the caches
// (wave-uniform), where write-once outputs only displace useful lines (wow 8192^2: -3 %)
template <typename T, typename V>
__device__ __forceinline__ void wt_storev(T *row, int x, int P, V v, int nt = 0, bool lane_ok = true)
{
    const uint64_t ra = (uint64_t)row;
    // (the builtin returns int: go through unsigned, or the low word sign-extends into the high one)
    const uint64_t ua = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(ra >> 32)) << 32) |
                        (uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)ra);
    __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)ua, 0, P * (int)sizeof(T), 0x00020000);
    const unsigned voff = (lane_ok && x >= 0) ? (unsigned)x * (unsigned)sizeof(T) : 0xfffffff0u;
    if (nt) __builtin_amdgcn_raw_buffer_store_b128(wt_bits16(v), r, voff, 0, 2);
    else __builtin_amdgcn_raw_buffer_store_b128(wt_bits16(v), r, voff, 0, 0);
}
__device__ __forceinline__ void wt_store4(float *row, int x, int P, float4 v, int nt = 0, bool lane_ok = true)
{
    wt_storev<float, float4>(row, x, P, v, nt, lane_ok);
}

__device__ __forceinline__ float wt_sig(float c, float tau, double taud, int soft)
{
    // Coefficients.significance - watroo/wavelets.py:137-141
    if (soft) return erff(fabsf(c / tau));
    return ((double)fabsf(c) > taud) ? 1.f : 0.f;
}
__device__ __forceinline__ double wt_sig(double c, double tau, double taud, int soft)
{
    return wt_sig64(c, tau, soft);
}

// sdev_loc from the two smoothed moments: vari = conv(I^2) - conv(I)^2 ; <= 0 -> 1e-20
// (watroo/wavelets.py:25-28), optional sqrt, then the two factors of wavelets.py:434-436.
// Shared by the variance chain kernel and the bilateral kernel so both give identical bits.
__device__ __forceinline__ float wt_var_point(float p, float m, float f1, float f2, int take_sqrt)
{
#pragma clang fp contract(off)
    float t = p - m * m;
    t = t <= 0.f ? 1e-20f : t;
    if (take_sqrt) t = sqrtf(t);
    return (t * f1) * f2;
}
// (the expression of wt64_var_kernel: identical bits to the two-plane form of the float64 engine)
__device__ __forceinline__ double wt_var_point(double p, double m, double f1, double f2, int take_sqrt)
{
#pragma clang fp contract(off)
    double t = p - m * m;
    t = t <= 0.0 ? 1e-20 : t;
    if (take_sqrt) t = sqrt(t);
    return (t * f1) * f2;
}

// wow per-scale update of one coefficient - watroo/utils.py:193-203:
//   c <- c * significance ; gamma += c ; c <- c * (factor / sqrt(clip(power)))
// Shared by wt_wow_kernel and the fused MODE_WOW chain kernel (identical bits).
__device__ __forceinline__ float wt_wow_point(float c, float power, bool has_power, float nn,
                                              double tau, float tauf, int soft, float factor,
                                              float &gamma_acc)
{
#pragma clang fp contract(off)
    float t = c;
    if (tau > 0.0) t = t * wt_sig(t, tauf * nn, tau * (double)nn, soft);
    gamma_acc = gamma_acc + t;
    float q = factor;
    if (has_power) {
        const float lp = power <= 0.f ? 1e-15f : power;   // utils.py:195
        // factor / sqrt(lp) (utils.py:196,203) as factor * rsq(lp): v_rsq_f32 is 1 ulp, well
        // inside the wow tolerance, and saves the IEEE sqrt + divide sequences (~40 VALU per
        // pixel, which is what made the fused wow kernel 1.5x slower than its filter alone)
        q = factor * __builtin_amdgcn_rsqf(lp);
    }
    return t * q;
}
// float64: the same update; factor / sqrt(lp) as factor * wt_rsq64(lp) (1 ulp; the float64 parity bound
// is 1e-12), the significance by wt_erf64
__device__ __forceinline__ double wt_wow_point(double c, double power, bool has_power, double nn,
                                               double tau, double tauf, int soft, double factor,
                                               double &gamma_acc)
{
#pragma clang fp contract(off)
    double t = c;
    if (tau > 0.0) t = t * wt_sig64(t, tau * nn, soft);
    gamma_acc = gamma_acc + t;
    double q = factor;
    if (has_power) {
        const double lp = power <= 0.0 ? 1e-15 : power;   // utils.py:195
        q = factor * wt_rsq64(lp);
    }
    return t * q;
}

// ---------------------------------------------------------------------------------------------
// K1  generic per-scale separable dilated convolution ("chain march")
//
//   c_{s+1} = h^(s) (*) c_s ,  w_s = c_s - c_{s+1}          watroo/wavelets.py:432,442
//   h^(s) = zero-stuffed outer product of the 1-D taps         watroo/wavelets.py:191-197
//
// A thread owns one group of adjacent columns (4 floats / 2 doubles) and one POLYPHASE ROW CHAIN
// y = q, q+d, q+2d, ...  (d = 2^s): along a chain the dilated vertical filter is an ordinary K-tap
// sliding window that lives in registers, so every input row is fetched once per chain (plus K-1 warm-up
// rows per chunk of S chain steps).  The horizontal taps are K coalesced 16-byte row loads at x + j*d
// (served by L1/L2 after the first touch; for d smaller than the group three aligned loads are recombined
// in registers).  Works for any dilation and any image size (multi-bounce reflection), which is what the
// large scales of wow() (d up to 1024) need; the fused kernels in wt_fused.h take over for the
// small dilations of the headline path.
// ---------------------------------------------------------------------------------------------
// MODE_WOW_PLAIN: the wow update WITHOUT a per-pixel noise map and without the gamma accumulator - the
// common case (scalar noise, h = 0).  A separate instantiation, not a run-time test: conditional loads in
// the row loop make the compiler's vmcnt bookkeeping inexact, every use of a (possibly) loaded value
// then waits for ALL outstanding memory operations - the prefetched rows and the row just stored
// included (13 % of the lattice kernel, 3 % of the row kernel at 8192^2).
// MODE_WOW_GAMMA: scalar noise WITH the gamma accumulator (wow(h > 0)): its row is read with one
// unconditional 16-byte load per lane (clamped column, like the input rows) instead of guarded scalars.
enum { MODE_SMOOTH = 0, MODE_SMOOTH_SQ = 1, MODE_DECOMP = 2, MODE_VAR = 3, MODE_WOW = 4, MODE_WOW_PLAIN = 5, MODE_WOW_GAMMA = 6 };
#define WT_IS_WOW(M) ((M) == MODE_WOW || (M) == MODE_WOW_PLAIN || (M) == MODE_WOW_GAMMA)

// component access of a lane's group
__device__ __forceinline__ void wt_vunpack(float4 v, float (&e)[4]) { e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w; }
__device__ __forceinline__ void wt_vunpack(double2 v, double (&e)[2]) { e[0] = v.x; e[1] = v.y; }
__device__ __forceinline__ float4 wt_vpack(const float (&e)[4]) { return make_float4(e[0], e[1], e[2], e[3]); }
__device__ __forceinline__ double2 wt_vpack(const double (&e)[2]) { return make_double2(e[0], e[1]); }
__device__ __forceinline__ double2 f4_mul(double2 a, double2 b) { return make_double2(a.x * b.x, a.y * b.y); }
__device__ __forceinline__ float wt_fma_s(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double wt_fma_s(double a, double b, double c) { return fma(a, b, c); }

// Raw operands of the horizontal K-tap filter of one row at the thread's PX pixels:
//   d >= PX: K groups at x + (j-hw) d      d < PX: 3 groups covering x-PX .. x+2PX-1
template <typename T, int K, bool SMALL_D>
__device__ __forceinline__ void wt_hrow_load(const T *row, int x, int d, int W, typename WtVec<T>::V (&raw)[K],
                                             int border = 0)
{
    constexpr int hw = K / 2;
    constexpr int PX = WtVec<T>::PX;
    if constexpr (!SMALL_D) {
#pragma unroll
        for (int j = 0; j < K; ++j) raw[j] = wt_loadv_b(row, x + (j - hw) * d, W, d, border);
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) raw[j] = wt_loadv_b(row, x - PX + PX * j, W, d, border);
    }
}

// Horizontal K-tap filter from the raw operands.
//   h   = sum_j k_j v(x + (j-hw) d)                  (v squared first for MODE_SMOOTH_SQ)
//   h2  = sum_j k_j v^2                              (MODE_VAR only)
//   cen = v(x)                                       (centre pixels, for the detail plane)
template <typename T, int K, int MODE, bool SMALL_D>
__device__ __forceinline__ void wt_hrow_filter(const typename WtVec<T>::V *raw, int d, typename WtVec<T>::V &h,
                                               typename WtVec<T>::V &h2, typename WtVec<T>::V &cen)
{
    typedef typename WtVec<T>::V V;
    constexpr int hw = K / 2;
    constexpr int PX = WtVec<T>::PX;
    if constexpr (!SMALL_D) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            V v = raw[j];
            if (j == hw) cen = v;
            V vv = f4_mul(v, v);
            if (MODE == MODE_SMOOTH_SQ || WT_IS_WOW(MODE)) v = vv;
            h = (j == 0) ? f4_scale(wt_tap_s<K, T>(0), v) : f4_fma(wt_tap_s<K, T>(j), v, h);
            if (MODE == MODE_VAR)
                h2 = (j == 0) ? f4_scale(wt_tap_s<K, T>(0), vv) : f4_fma(wt_tap_s<K, T>(j), vv, h2);
        }
    } else {
        // d < PX (float: 1 or 2; double: 1): pixels x-PX .. x+2PX-1 cover every tap (hw*d <= PX)
        const V L = raw[0], C = raw[1], R = raw[2];
        T e[3 * PX], e2[3 * PX];
        {
            T t0[PX], t1[PX], t2[PX];
            wt_vunpack(L, t0);
            wt_vunpack(C, t1);
            wt_vunpack(R, t2);
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                e[i] = t0[i];
                e[PX + i] = t1[i];
                e[2 * PX + i] = t2[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 3 * PX; ++i) {
            e2[i] = e[i] * e[i];
            if (MODE == MODE_SMOOTH_SQ || WT_IS_WOW(MODE)) e[i] = e2[i];
        }
        cen = C;
        T o[PX], o2[PX];
        // d is wave-uniform at run time: one scalar branch, bodies with static indices (selecting per
        // tap with `d == 1 ? e[..] : e[..]` doubled the VALU count of the d < 4 kernels: a v_cndmask
        // per operand)
        auto taps = [&](auto dtag) {
            constexpr int DD = decltype(dtag)::value;
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                T a = wt_tap_s<K, T>(0) * e[PX + k - DD * hw];
                T a2 = wt_tap_s<K, T>(0) * e2[PX + k - DD * hw];
#pragma unroll
                for (int j = 1; j < K; ++j) {
                    a = wt_fma_s(wt_tap_s<K, T>(j), e[PX + k + DD * (j - hw)], a);
                    a2 = wt_fma_s(wt_tap_s<K, T>(j), e2[PX + k + DD * (j - hw)], a2);
                }
                o[k] = a;
                o2[k] = a2;
            }
        };
        if constexpr (PX == 4) {
            if (d == 1) taps(std::integral_constant<int, 1>{});
            else taps(std::integral_constant<int, 2>{});
        } else {
            taps(std::integral_constant<int, 1>{});
        }
        h = wt_vpack(o);
        if (MODE == MODE_VAR) h2 = wt_vpack(o2);
    }
}

// XCD-aware block remap for the chain-march kernels.  Hardware deals consecutive workgroup ids
// round-robin over the 8 XCDs (each with a private 4 MiB L2).  The horizontal taps of a
// dilated filter re-read the SAME image rows at x +- d, x +- 2d, i.e. from the x-blocks next
// to this one; with the default order those neighbours sit on other XCDs and every XCD
// fetches the row segment again through the fabric.  Remapped, all x-blocks of one group of
// rows run on one XCD and the re-reads are L2 hits.  Pure speed: any placement is correct.
// Requires gridDim.y % 8 == 0 (the host rounds up; surplus blocks find no work and exit).
__device__ __forceinline__ void wt_xcd_remap(int &bx, int &by)
{
    const int gx = gridDim.x;
    const int b = blockIdx.y * gx + blockIdx.x;
    const int xcd = b & 7, j = b >> 3;
    bx = j % gx;
    by = (j / gx) * 8 + xcd;
}

template <typename T>
struct ChainArgsT {
    const T *in;  // local row 0 of the input plane
    T *out_c;     // smooth / variance output (local row 0)
    T *out_w;     // detail output or nullptr
    const T *aux; // bilateral: per-pixel variance plane
    Geo g;        // (P = row pitch in elements of T)
    int d;        // dilation 2^s
    int S;        // chain steps per thread
    int chunks;   // chunks per chain
    T f1, f2;     // MODE_VAR: factors applied to the clipped variance (wavelets.py:434-436)
    int take_sqrt;
    // MODE_WOW (fused wow per-scale update) / bilateral with in-kernel variance
    const T *noise;      // per-pixel noise map or nullptr
    T *gamma;            // gamma accumulator plane or nullptr
    double tau;          // significance threshold (<= 0: none)
    T factor;            // w * power_norm
    int soft, whiten, inline_var;
    int nt;              // streaming stores for the outputs (planes >> cache)
};
typedef ChainArgsT<float> ChainArgs;

// Vertical half shared by the chain-march kernel (taps fetched from global memory) and the
// row kernel (taps fetched from an LDS copy of the row): horizontal filter of each incoming row,
// K-row sliding window of the filtered rows, vertical filter, mode epilogue.  One code path so
// that both kernels produce identical bits.
template <typename T, int K, int MODE, bool SMALL_D>
struct WtVert {
    typedef typename WtVec<T>::V V;
    static constexpr int PX = WtVec<T>::PX;
    static constexpr int hw = K / 2;
    V hwin[K], h2win[K], cen[hw + 1];

    // warm-up rows r0-hw .. r0+hw-1 (j = 0 .. K-2)
    __device__ __forceinline__ void prime(int j, const V *raw, int d)
    {
        V ct;
        hwin[j] = wt_vzero<V>();
        h2win[j] = wt_vzero<V>();
        wt_hrow_filter<T, K, MODE, SMALL_D>(raw, d, hwin[j], h2win[j], ct);
        if (j >= hw) cen[j - hw] = ct;
    }

    // row r+hw enters; emits row r of the outputs at element offset `off` (row start), pixel x
    __device__ __forceinline__ void emit(const V *raw, const ChainArgsT<T> &a, int64_t off, int x,
                                         bool lane_ok)
    {
        const Geo &g = a.g;
        hwin[K - 1] = wt_vzero<V>();
        h2win[K - 1] = wt_vzero<V>();
        wt_hrow_filter<T, K, MODE, SMALL_D>(raw, a.d, hwin[K - 1], h2win[K - 1], cen[hw]);
        V o = f4_scale(wt_tap_s<K, T>(0), hwin[0]);
#pragma unroll
        for (int j = 1; j < K; ++j) o = f4_fma(wt_tap_s<K, T>(j), hwin[j], o);
        if (MODE == MODE_VAR) {
            V p = f4_scale(wt_tap_s<K, T>(0), h2win[0]);
#pragma unroll
            for (int j = 1; j < K; ++j) p = f4_fma(wt_tap_s<K, T>(j), h2win[j], p);
            T pp[PX], mm[PX], v[PX];
            wt_vunpack(p, pp);
            wt_vunpack(o, mm);
#pragma unroll
            for (int k = 0; k < PX; ++k) v[k] = wt_var_point(pp[k], mm[k], a.f1, a.f2, a.take_sqrt);
            wt_storev(a.out_c + off, x, g.P, wt_vpack(v), a.nt, lane_ok);
        } else if (WT_IS_WOW(MODE)) {
            // fused wow update: o = conv_s(c^2) (local power), cen[0] = c at this row; result
            // goes to a different plane (the host swaps plane pointers afterwards)
            T cc[PX], pw[PX], nn[PX], gg[PX], r4[PX];
            wt_vunpack(cen[0], cc);
            wt_vunpack(o, pw);
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                nn[k] = (T)1;
                gg[k] = (T)0;
            }
            if constexpr (MODE == MODE_WOW_GAMMA) {
                // (columns clamped into the row's pitch: lanes that store nothing read something harmless)
                const V g4 = *reinterpret_cast<const V *>(a.gamma + off + min(max(x, 0), g.P - PX));
                wt_vunpack(g4, gg);
            }
            if constexpr (MODE == MODE_WOW) {
                const bool full = x + PX - 1 < g.W;
                if (a.noise && lane_ok) {
#pragma unroll
                    for (int k = 0; k < PX; ++k) if (full || x + k < g.W) nn[k] = a.noise[off + x + k];
                }
                if (a.gamma && lane_ok) {
#pragma unroll
                    for (int k = 0; k < PX; ++k) if (full || x + k < g.W) gg[k] = a.gamma[off + x + k];
                }
            }
            const T tauf = (T)a.tau;
#pragma unroll
            for (int k = 0; k < PX; ++k)
                r4[k] = wt_wow_point(cc[k], pw[k], a.whiten != 0, nn[k], a.tau, tauf, a.soft, a.factor, gg[k]);
            wt_storev(a.out_c + off, x, g.P, wt_vpack(r4), a.nt, lane_ok);
            if constexpr (MODE == MODE_WOW) {
                if (a.gamma) wt_storev(a.gamma + off, x, g.P, wt_vpack(gg), a.nt, lane_ok);
            }
            if constexpr (MODE == MODE_WOW_GAMMA) wt_storev(a.gamma + off, x, g.P, wt_vpack(gg), a.nt, lane_ok);
        } else {
            wt_storev(a.out_c + off, x, g.P, o, a.nt, lane_ok);
            if (MODE == MODE_DECOMP && a.out_w)
                wt_storev(a.out_w + off, x, g.P, f4_sub(cen[0], o), a.nt, lane_ok);
        }
#pragma unroll
        for (int j = 0; j < K - 1; ++j) {
            hwin[j] = hwin[j + 1];
            h2win[j] = h2win[j + 1];
        }
#pragma unroll
        for (int j = 0; j < hw; ++j) cen[j] = cen[j + 1];
    }
};

// ---------------------------------------------------------------------------------------------
// Arguments of the row kernel (K1b, wt_stencil_march.h)
template <typename T>
struct RowArgsT {
    ChainArgsT<T> c;
    int Vx;   // valid (stored) pixels per x-strip, multiple of 32
    int HX;   // x halo in pixels, multiple of 32
};
typedef RowArgsT<float> RowArgs;

// A batch of frames (wt_batch): the arguments of frame 0, the distance between two frames' planes and the
// per-frame {tau, factor} pairs of the wow modes.  The batched kernels move every plane pointer (the noise map's too) by
// blockIdx.z * fstride and read their frame's pair once, at the start of the workgroup.
template <typename A>
struct WtFrameArgs {
    A k;                 // ChainArgsT<T> or RowArgsT<T> of frame 0
    int64_t fstride;     // elements from one frame's plane to the next
    const double *ftab;  // [frame][2] = {tau, factor} (wow modes; nullptr otherwise)
};

template <int MODE, typename T>
__device__ __forceinline__ ChainArgsT<T> wt_frame_move(ChainArgsT<T> a, int64_t fstride, const double *ftab)
{
    const int f = blockIdx.z;
    const int64_t o = (int64_t)f * fstride;
    a.in += o;
    a.out_c += o;
    if (a.out_w) a.out_w += o;
    if (a.gamma) a.gamma += o;
    if (a.noise) a.noise += o;
    if constexpr (WT_IS_WOW(MODE)) {
        a.tau = ftab[2 * f];
        a.factor = (T)ftab[2 * f + 1];
    }
    return a;
}
template <int MODE, typename T>
__device__ __forceinline__ ChainArgsT<T> wt_frame_args(const WtFrameArgs<ChainArgsT<T>> &fa)
{
    return wt_frame_move<MODE, T>(fa.k, fa.fstride, fa.ftab);
}
template <int MODE, typename T>
__device__ __forceinline__ RowArgsT<T> wt_frame_args(const WtFrameArgs<RowArgsT<T>> &fa)
{
    RowArgsT<T> r = fa.k;
    r.c = wt_frame_move<MODE, T>(fa.k.c, fa.fstride, fa.ftab);
    return r;
}

#define WT_SK_NAME(base) base##_kernel
#define WT_SK_PARAM(type, name) type name
#define WT_SK_FRAME(mode, name)
#include "wt_stencil_march.h"
#undef WT_SK_NAME
#undef WT_SK_PARAM
#undef WT_SK_FRAME
// (templates: instantiated only where a batched launch names them - wt_stencil32_batch.hip)
#define WT_SK_NAME(base) base##_batch_kernel
#define WT_SK_PARAM(type, name) WtFrameArgs<type> name##_frame0
#define WT_SK_FRAME(mode, name) const auto name = wt_frame_args<mode>(name##_frame0)
#include "wt_stencil_march.h"
#undef WT_SK_NAME
#undef WT_SK_PARAM
#undef WT_SK_FRAME
