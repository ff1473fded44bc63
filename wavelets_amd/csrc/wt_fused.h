// Fused multi-scale a-trous passes: NS consecutive scales per HBM round trip (NS = 2, 3; 4 for the
// 3-tap family, whose window for four scales is as large as the 5-tap family's for three).
//
//   pass(s0, NS):  read c_{s0} once  ->  write w_{s0} .. w_{s0+NS-1} and c_{s0+NS}
//                  (watroo/wavelets.py:429-442 for NS consecutive iterations of the loop)
//
// Algorithmic traffic 4*(NS+2) B/pixel instead of 12*NS for one kernel per scale.
//
// Geometry (D = 2^s0 is the base dilation of the pass):
//  * y: the image rows split into D POLYPHASE CHAINS  y = q, q+D, q+2D, ...; on a chain the
//    scales s0+a have dilation 2^a chain steps.  A workgroup marches down one chunk of one
//    chain, one row per step, so the vertical filters are sliding windows held in REGISTERS
//    (per lane: (K-1)*(2^NS-1) float4 = 28 for B3/NS=3), never re-read from memory.
//  * x: a workgroup of NW waves covers NW*256 contiguous pixels of the row (lane = 4 adjacent
//    pixels = one 16-byte coalesced access), including the cumulative halo
//    hw*(2^NS-1)*D pixels on each side (rounded up to 32 pixels so that every wave access
//    covers whole 128-byte lines) whose results are discarded.  The horizontal filter
//    needs the vertically-filtered row of the neighbouring lanes: it is staged through a
//    per-scale LDS row (one ds_write_b128 + K-1 ds_read_b128 per lane per scale) - for D >= 4
//    the dilated taps are whole-lane offsets, for D = 1 the taps of dilation 1 and 2 are
//    recombined from the two adjacent lanes' float4.  The NS scales of a step are software-
//    pipelined (scale a works on the row scale a-1 produced one step earlier): one barrier per
//    row, LDS rows double-buffered by step parity.
//  * borders: the chain simply continues through reflected rows / columns; symmetric
//    extension commutes with the symmetric filters, so every intermediate scale is the exact
//    symmetric extension too.  In a multi-GPU strip the rows beyond the strip come from the
//    halo margins (RCCL exchange of the pass input) instead.
//  * latency of the cascade: output row of scale a lags the input row by hw*(2^(a+1)-1)
//    chain steps (+ a for the pipeline skew), so a chunk of S rows reads S + 2*hw*(2^NS-1)
//    rows (warm-up).  The host picks the chunk count that minimises (dispatch rounds) x (rows
//    per workgroup) - normally one round with every resident slot filled.
//  * stores are branch-free: one fixed raw buffer descriptor per plane; a row outside the chunk
//    or a halo lane gets an out-of-range ("parked") offset and the hardware range check drops
//    the store.
//  * the march is instruction-issue bound as much as memory bound: ~218
//    instructions per step, every scalar instruction in the step was paid for.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "wt_internal.h"
#include "wt_device.h"
#include "wt_fused_decl.h"


// (WtVec<T>, the double2 forms of the float4 helpers, wt_tap_s, wt_vzero / wt_vrev / wt_vfence: wt_device.h)

template <typename T, int K, int SHIFT_PX, int NLANES>
__device__ __forceinline__ typename WtVec<T>::V wt_hfilter_lds(const typename WtVec<T>::V *vrow, int gl, typename WtVec<T>::V own)
{
    // horizontal K-tap filter with taps SHIFT_PX pixels apart; vrow = the WG's LDS row of
    // vertically filtered values (one 16-byte group per lane), gl = this lane's index in the row.
    typedef typename WtVec<T>::V V;
    constexpr int PX = WtVec<T>::PX;
    constexpr int hw = K / 2;
    if constexpr (SHIFT_PX % PX == 0) {
        constexpr int LO = SHIFT_PX / PX;
        V acc;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            V v;
            if (j == hw) v = own;
            else {
                int idx = gl + (j - hw) * LO;
                idx = idx < 0 ? 0 : (idx > NLANES - 1 ? NLANES - 1 : idx);
                v = vrow[idx];
            }
            acc = (j == 0) ? f4_scale(wt_tap_s<K, T>(0), v) : f4_fma(wt_tap_s<K, T>(j), v, acc);
        }
        return acc;
    } else if constexpr (PX == 2) {
        // double: the only sub-group shift is 1 pixel (D = 1, first scale): both neighbours' pairs
        static_assert(SHIFT_PX == 1, "float64: sub-group shift is 1 px");
        const V L = vrow[gl > 0 ? gl - 1 : 0];
        const V R = vrow[gl < NLANES - 1 ? gl + 1 : NLANES - 1];
        const T e[6] = {L.x, L.y, own.x, own.y, R.x, R.y};
        T o[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            T acc = wt_tap_s<K, T>(0) * e[2 + k - hw];
#pragma unroll
            for (int j = 1; j < K; ++j) acc = fma(wt_tap_s<K, T>(j), e[2 + k + (j - hw)], acc);
            o[k] = acc;
        }
        return make_double2(o[0], o[1]);
    } else {
        static_assert(SHIFT_PX == 1 || SHIFT_PX == 2, "sub-float4 shifts are 1 or 2 px");
        const float4 L = vrow[gl > 0 ? gl - 1 : 0];
        const float4 R = vrow[gl < NLANES - 1 ? gl + 1 : NLANES - 1];
        if constexpr (SHIFT_PX == 1) {
            // The 1-pixel taps pair (own.y, own.z).  Without this fence the vectoriser carries
            // that odd pairing back through the vertical filter into the window and the row
            // loads (a third copy of every row: one more load per row, waited on at once, 1.5x
            // the vertical arithmetic and 8 more VGPRs); with it the pair is formed here.
            asm volatile("" : "+v"(own.x), "+v"(own.y), "+v"(own.z), "+v"(own.w));
        }
        const float e[12] = {L.x, L.y, L.z, L.w, own.x, own.y, own.z, own.w, R.x, R.y, R.z, R.w};
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float acc = wt_tap<K>(0) * e[4 + k - hw * SHIFT_PX];
#pragma unroll
            for (int j = 1; j < K; ++j) acc = fmaf(wt_tap<K>(j), e[4 + k + (j - hw) * SHIFT_PX], acc);
            o[k] = acc;
        }
        return make_float4(o[0], o[1], o[2], o[3]);
    }
}

// Experiment (-DWT_FUSED_WAVEAUTO, D = 1 passes): WAVE-AUTONOMOUS horizontal taps.  Every wave
// covers its own 256 pixels including 4 halo lanes per side (the cumulative x halo of three scales
// at D = 1 is 14 px), neighbouring lanes' values come through DPP wave shifts, there is no LDS row
// and no barrier.  Same taps in the same order as wt_hfilter_lds: identical bits on the lanes
// that store.  DESIGN.md 3.1 has the measurement.
#ifdef WT_FUSED_WAVEAUTO
#define WT_FUSED_WA 1
#else
#define WT_FUSED_WA 0
#endif
__device__ __forceinline__ float wt_dpp_from_prev(float v)   // lane i <- lane i-1 (wave_shr:1)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wt_dpp_from_next(float v)   // lane i <- lane i+1 (wave_shl:1)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}
__device__ __forceinline__ float4 wt_dpp4_prev(float4 v)
{
    return make_float4(wt_dpp_from_prev(v.x), wt_dpp_from_prev(v.y), wt_dpp_from_prev(v.z), wt_dpp_from_prev(v.w));
}
__device__ __forceinline__ float4 wt_dpp4_next(float4 v)
{
    return make_float4(wt_dpp_from_next(v.x), wt_dpp_from_next(v.y), wt_dpp_from_next(v.z), wt_dpp_from_next(v.w));
}
template <int K, int SHIFT_PX>
__device__ __forceinline__ float4 wt_hfilter_dpp(float4 own)
{
    constexpr int hw = K / 2;
    static_assert(SHIFT_PX == 1 || SHIFT_PX == 2 || SHIFT_PX == 4, "D = 1 passes only");
    const float4 L = wt_dpp4_prev(own), R = wt_dpp4_next(own);
    if constexpr (SHIFT_PX == 4) {
        float4 nb[5] = {own, own, own, own, own};       // lanes -2 .. +2
        nb[1] = L; nb[3] = R;
        if constexpr (hw == 2) { nb[0] = wt_dpp4_prev(L); nb[4] = wt_dpp4_next(R); }
        float4 acc;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const float4 v = nb[2 + j - hw];
            acc = (j == 0) ? f4_scale(wt_tap<K>(0), v) : f4_fma(wt_tap<K>(j), v, acc);
        }
        return acc;
    } else {
        const float e[12] = {L.x, L.y, L.z, L.w, own.x, own.y, own.z, own.w, R.x, R.y, R.z, R.w};
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float acc = wt_tap<K>(0) * e[4 + k - hw * SHIFT_PX];
#pragma unroll
            for (int j = 1; j < K; ++j) acc = fmaf(wt_tap<K>(j), e[4 + k + (j - hw) * SHIFT_PX], acc);
            o[k] = acc;
        }
        return make_float4(o[0], o[1], o[2], o[3]);
    }
}

// vertical window of scale A: 2^A interleaved sub-chains, K-1 stored rows each
template <typename V, int K, int A>
struct VWin {
    V w[1 << A][K - 1];
};

typedef unsigned int wt_v4u __attribute__((ext_vector_type(4)));
typedef float wt_v4f __attribute__((ext_vector_type(4)));

// Branch-free predicated 16-byte stores through raw buffer descriptors: a row or lane that must
// not be written gets an out-of-range offset and the hardware range check drops the store.
// Control flow stays uniform, so the compiler's vmcnt bookkeeping is exact (loads stay in flight
// across the stores and barriers of several steps).
// AUX = cache-policy bits of the store (gfx950: 1 = sc0, 2 = nt, 16 = sc1).
//
// Store through a descriptor that stays FIXED for the whole march (base = the row the plane
// stores at step 0, length = the chunk's byte span): the row is selected by the byte offset
// k * step_bytes folded into voff (one v_add per step shared by all planes), a row or lane that
// must not be written gets the parked offset 2^31 >= length.  No per-store scalar work besides
// the row predicate: the march is instruction-issue bound.
#define WT_FUSED_PARKED 0x80000000u
template <int AUX>
__device__ __forceinline__ void wt_bstore4v(__amdgpu_buffer_rsrc_t r, unsigned voff, float4 v)
{
    wt_v4f t = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(wt_v4u, t), r, voff, 0, AUX);
}
typedef double wt_v2d __attribute__((ext_vector_type(2)));
template <int AUX>
__device__ __forceinline__ void wt_bstore4v(__amdgpu_buffer_rsrc_t r, unsigned voff, double2 v)
{
    wt_v2d t = {v.x, v.y};
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(wt_v4u, t), r, voff, 0, AUX);
}
__device__ __forceinline__ float4 wt_from_v4u(wt_v4u t, float4)
{
    const wt_v4f f = __builtin_bit_cast(wt_v4f, t);
    return make_float4(f.x, f.y, f.z, f.w);
}
__device__ __forceinline__ double2 wt_from_v4u(wt_v4u t, double2)
{
    const wt_v2d f = __builtin_bit_cast(wt_v2d, t);
    return make_double2(f.x, f.y);
}

// Ablation switches (FusedArgs::debug, env WT_FUSED_DEBUG) are compiled in only with
// -DWT_FUSED_ABLATION: their loop-invariant branches cost issue slots in every step.
#ifdef WT_FUSED_ABLATION
#define WT_FUSED_DBG(a) ((a).debug)
#else
#define WT_FUSED_DBG(a) 0
#endif

// The detail planes are write-once streams that nothing re-reads before the pass is over:
// nontemporal stores.  The smooth plane is the NEXT pass's input and keeps the default policy
// (up to 4096^2 it is still in the Infinity Cache when the next pass starts: 0.125 -> 0.097 ms
// for the D = 8 pass).  Measured on several MI355X hosts at 8192^2: +-1.5 % on most, but 25 %
// faster on a host where plain stores ran the passes at 0.46 ms instead of 0.33 ms, i.e. the
// streaming stores also remove most of the host-to-host spread.
#ifndef WT_FUSED_W_AUX
#define WT_FUSED_W_AUX 2
#endif
#ifndef WT_FUSED_P_AUX
#define WT_FUSED_P_AUX 0   // running sum between two passes (re-read by the next pass)
#endif
#ifndef WT_FUSED_C_AUX
#define WT_FUSED_C_AUX 0
#endif
#ifndef WT_FUSED_R_AUX
#define WT_FUSED_R_AUX WT_FUSED_W_AUX   // the finished reconstruction (last pass of a carried sum)
#endif

// Vertical half of one scale of one step: push `cur` (a row of c_{s0+A}) into the window and
// return the vertically filtered row (centred hw*2^A steps back); `cen` = matching row of
// c_{s0+A} (for the detail plane).
template <typename T, int K, int A>
__device__ __forceinline__ typename WtVec<T>::V wt_fused_vstage(VWin<typename WtVec<T>::V, K, A> &win, const int kk,
                                                                const typename WtVec<T>::V cur, typename WtVec<T>::V &cen)
{
    typedef typename WtVec<T>::V V;
    constexpr int hw = K / 2;
    constexpr int KM = K - 1;
    const int rho = kk % (1 << A);
    const int p = (kk >> A) % KM;
    V *w = win.w[rho];
    V v = f4_scale(wt_tap_s<K, T>(0), w[p]);
#pragma unroll
    for (int j = 1; j < KM; ++j) v = f4_fma(wt_tap_s<K, T>(j), w[(p + j) % KM], v);
    v = f4_fma(wt_tap_s<K, T>(KM), cur, v);
    cen = w[(p + hw) % KM];
    w[p] = cur;
    return v;
}

// The NS scales are SOFTWARE-PIPELINED across steps: in step j scale a works on the row scale
// a-1 produced in step j-1, so the NS vertical filters, the NS LDS row writes, ONE barrier and
// the NS horizontal filters of a step are mutually independent (one s_barrier per row instead
// of NS, 4*NS LDS reads in flight together).  LDS rows are double-buffered by step parity.
#ifndef WT_FUSED_WPS4_K3
#define WT_FUSED_WPS4_K3 3   // 3-tap family: 148 VGPRs, three 4-wave workgroups per CU (0.345 -> 0.32 ms)
#endif
#ifndef WT_FUSED_WPS4
#define WT_FUSED_WPS4 2   // waves per SIMD requested for the 4-wave workgroup variant
#endif
// workgroups of 4 waves per CU (= waves per SIMD): 3 for the plain 3-tap passes of up to three scales,
// 1 for the four-scale accumulate variants (98 KB of LDS), else 2
#define WT_FUSED_WG4_PER_CU(K, NS, ACC) \
    ((K) == 3 && (NS) < 4 && ((ACC) == 0 || (ACC) == 3) ? WT_FUSED_WPS4_K3 : ((NS) == 4 && ((ACC) == 1 || (ACC) == 2) ? 1 : WT_FUSED_WPS4))
#define WT_FUSED_KERNEL_NAME wt_fused_kernel
#define WT_FUSED_KERNEL_BATCH 0
#include "wt_fused_march.h"
#undef WT_FUSED_KERNEL_NAME
#undef WT_FUSED_KERNEL_BATCH
// (the batched kernels are instantiated only in the batch units, -DWT_TU_BATCH=1: the image units compile exactly
//  the code they had before batches existed)
#ifndef WT_TU_BATCH
#define WT_TU_BATCH 0
#endif
#if WT_TU_BATCH
#define WT_FUSED_KERNEL_NAME wt_fused_batch_kernel
#define WT_FUSED_KERNEL_BATCH 1
#include "wt_fused_march.h"
#undef WT_FUSED_KERNEL_NAME
#undef WT_FUSED_KERNEL_BATCH
#endif

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// S = element type (float: wt_plan, double: wt_plan64 - both carry `ctx` and the geometry `g`)
template <typename T, int K, int NS, int D, int NW, int PD, int ACC, typename PLAN>
static int wt_fused_launch_t(PLAN *p, const FusedArgsT<T> &base, const char *name, const FusedRows &rows)
{
    constexpr int PX = WtVec<T>::PX;
    constexpr int ALIGN_PX = 128 / (int)sizeof(T);           // strips start on 128-byte lines

    constexpr int hw = K / 2;
    constexpr int LAT = hw * ((1 << NS) - 1) + (NS - 1);
    constexpr int HX = (hw * ((1 << NS) - 1) * D + ALIGN_PX - 1) / ALIGN_PX * ALIGN_PX;
    constexpr int NL = NW * 64;
    constexpr int VXMAX = (WT_FUSED_WA && D == 1 && PX == 4) ? NW * 56 * 4     // 56 storing lanes per wave
                                                             : NL * PX - 2 * HX; // widest valid strip per WG
    constexpr int UMAX = (K - 1) << (NS - 1);
    static_assert(VXMAX >= 2 * ALIGN_PX, "workgroup too narrow for this halo");
    const Geo &g = p->g;
    FusedArgsT<T> a = base;
    const int W4 = (g.W + PX - 1) / PX * PX;
    const int nx = (W4 + VXMAX / ALIGN_PX * ALIGN_PX - 1) / (VXMAX / ALIGN_PX * ALIGN_PX);
    a.Vx = std::min(VXMAX / ALIGN_PX * ALIGN_PX, ((W4 + nx - 1) / nx + ALIGN_PX - 1) / ALIGN_PX * ALIGN_PX);   // balanced, 128-B aligned
    if ((int64_t)a.Vx * nx < W4) WT_FAIL("fused pass: strip sizing failed");
    const int phases = std::min(D, g.nrows);
    int nranges = rows.n ? rows.n : 1, span_rows = 0;
    for (int i = 0; i < 2; ++i) {
        a.rlo[i] = rows.n ? (i < rows.n ? rows.lo[i] : 0) : 0;
        a.rhi[i] = rows.n ? (i < rows.n ? rows.hi[i] : 0) : (i == 0 ? g.nrows : 0);
        if (a.rlo[i] < 0 || a.rhi[i] > g.nrows || a.rlo[i] > a.rhi[i]) WT_FAIL("fused pass: bad row range [%d,%d)", a.rlo[i], a.rhi[i]);
        span_rows = std::max(span_rows, a.rhi[i] - a.rlo[i]);
    }
    if (span_rows == 0) return 0;
    const int n_max = (span_rows + D - 1) / D;           // longest chain of a range
    // Chunking: the resident capacity is `slots` workgroups (256 CUs x workgroups per CU) and a
    // workgroup's cost is its S stored rows plus the 2*LAT warm-up rows.  Pick the chunk count
    // that minimises (dispatch rounds) x (rows per workgroup): usually ONE round with every
    // slot filled; when the x-strips x phases alone under-fill the chip (tall narrow-ish strips:
    // 160 workgroups for 256 CUs at 32768 columns) a few shorter chunks in two rounds win.
    // (the single-scale passes are light - 92 VGPRs, 16 KB of LDS - two 8-wave workgroups per CU)
    const int wg_per_cu = NW == 4 ? WT_FUSED_WG4_PER_CU(K, NS, ACC) : (NS == 1 ? 2 : std::max(1, 8 / NW));
    static const int rounds_env = getenv("WT_FUSED_ROUNDS") ? std::max(1, atoi(getenv("WT_FUSED_ROUNDS"))) : 0;
    // (a batch: the frames' workgroups share the chip - 64 frames of 512^2 fill it with long chunks)
    const int frames = std::max(1, rows.frames);
    const int64_t nbase = (int64_t)nx * phases * nranges * frames;
    int chunks = 1, S = n_max;
    double best = 1e300;
    auto search = [&](int slots) {
        chunks = 1; S = n_max; best = 1e300;
        for (int c = 1; c <= 4096 && c <= n_max; ++c) {
            const int Sc = (n_max + c - 1) / c;
            const int cc = (n_max + Sc - 1) / Sc;                    // chunks actually needed
            const int64_t rounds = (nbase * cc + slots - 1) / slots;
            // the kernel addresses the rows of a chunk with 31-bit byte offsets
            if ((int64_t)(Sc + 2 * LAT + 2 * UMAX + 1) * D * g.P * (int64_t)sizeof(T) >= ((int64_t)1 << 31)) continue;
            // more than one round: keep the warm-up <= ~50 % of a chunk.  A grid that fits in one
            // round anyway (small images: the chip is not full) is latency-bound by the steps of
            // ONE workgroup, so shorter chunks win even if most of their steps are warm-up.
            if (c > 1 && Sc < std::min(n_max, rounds > 1 ? 2 * LAT : 4)) break;
            if (rounds_env && rounds > rounds_env) break;
            const double cost = (double)rounds * (Sc + 2 * LAT + 8);
            if (cost < best) { best = cost; chunks = cc; S = Sc; }
        }
    };
    const int cus = p->ctx->num_cus;
    search(std::max(64, (cus - rows.reserve) * wg_per_cu));
    // Large images, D = 1: ONE workgroup per CU with chunks twice as long.  The pass is bound by
    // its memory pattern, not by latency (section 3.1 of DESIGN.md), so the second workgroup per CU
    // buys nothing, while half as many chunks halve the warm-up share and the number of isolated
    // write fronts: 8192^2 0.297 -> 0.277 ms, 6144^2 -8 %, 12288^2 -8 %, 16384^2 -5 %
    // (profiles/r02_f_chunks.txt).  At 4096^2 (chunks of 81 rows) it is 3 % slower: the planes sit in
    // the Infinity Cache there and latency matters again - hence the threshold on the chunk length.
    static const int wpc1_env = getenv("WT_FUSED_WPC1") ? atoi(getenv("WT_FUSED_WPC1")) : -1;   // -1 auto, 0 off, 1 force
    if (D == 1 && NW == 4 && wg_per_cu > 1 && wpc1_env != 0) {
        const int c2 = chunks, S2 = S;
        const double b2 = best;
        // (an interior launch beside a halo exchange, rows.reserve > 0: with one 4-wave workgroup
        // per CU half of every CU's register file and LDS stays free for the RCCL kernels, so no CU
        // is set aside - setting 16 aside costs a whole chunk per strip, 7-10 % of the pass at
        // 32768 columns: 36 strips x 7 chunks = 252 workgroups fit 256 CUs, 6 chunks do not fill 240)
        search(std::max(64, cus));
        if (best == 1e300 || (wpc1_env < 0 && S < 128)) { chunks = c2; S = S2; best = b2; }
    }
    if (best == 1e300) WT_FAIL("fused pass: no chunking keeps a chunk's byte span below 2 GiB");
    static const int chunks_env = getenv("WT_FUSED_CHUNKS") ? atoi(getenv("WT_FUSED_CHUNKS")) : 0;   // experiments (D = 1 passes)
    if (D == 1 && chunks_env > 0 && chunks_env <= n_max) {
        S = (n_max + chunks_env - 1) / chunks_env;
        chunks = (n_max + S - 1) / S;
    }
    a.S = S;
    a.chunks = chunks;
    static const int dbg = getenv("WT_FUSED_DEBUG") ? atoi(getenv("WT_FUSED_DEBUG")) : 0;
    a.debug = dbg;
    const int64_t gy = (int64_t)D * chunks;
    if (gy > 65535) WT_FAIL("fused pass: grid too large");
    a.fstride = frames > 1 ? rows.fstride : 0;
    if (frames > 65535) WT_FAIL("fused pass: %d frames exceed the grid (the host splits larger batches)", frames);
    if (frames > 1 && nranges != 1) WT_FAIL("fused pass: a batch of frames takes whole passes");
    dim3 grid(nx, (unsigned)gy, (unsigned)(frames > 1 ? frames : nranges)), block(NL);
    // (the two parts of a split pass are timed under their own names: bench.py reports per-pass
    //  exchange / interior / edge times of the multi-GPU schedule)
    const std::string pname = std::string(name) + (rows.part == 1 ? "/interior" : rows.part == 2 ? "/edge" : "");
    ProfScope ps(p->ctx, pname.c_str());
    // fast addressing: a group outside the image is a group inside it read backwards (any width since round 6: the one
    // group that straddles the right border is a swizzle of its own four pixels) and no index reflects twice.  (The
    // riding histogram counts whole groups: it keeps the generic addressing for widths the groups do not divide.)
    const bool fast = g_opt_fused_fast && (g.W % PX == 0 || ACC != 3) && g.W >= HX && g.W >= 2 * PX &&
                      g.H >= D * (hw * ((1 << NS) - 1) + 1);
#if WT_TU_BATCH
    // (a batch unit launches the batched kernels only: the image kernels live in the image units)
    // (float32 batches: wt_batch, float64 batches: wt_batch64 - plain and accumulate passes of either)
    if constexpr (ACC != 3) {
        if (fast) hipLaunchKernelGGL((wt_fused_batch_kernel<T, K, NS, D, NW, PD, ACC, true>), grid, block, 0, p->ctx->stream, a);
        else hipLaunchKernelGGL((wt_fused_batch_kernel<T, K, NS, D, NW, PD, ACC, false>), grid, block, 0, p->ctx->stream, a);
    } else {
        WT_FAIL("fused pass: no batched form of this pass (plain / accumulate passes only)");
    }
#else
    if (frames > 1) WT_FAIL("fused pass: batches run in the batch units (wt_fused_tu_f{32,64}_k*_batch_acc*)");
    if (fast) hipLaunchKernelGGL((wt_fused_kernel<T, K, NS, D, NW, PD, ACC, true>), grid, block, 0, p->ctx->stream, a);
    else hipLaunchKernelGGL((wt_fused_kernel<T, K, NS, D, NW, PD, ACC, false>), grid, block, 0, p->ctx->stream, a);
#endif
    WT_HIP(hipGetLastError());
    return 0;
}

// Tuned on MI355X (8192^2, B3): the D = 1 pass prefers 4-wave workgroups (2 resident per CU),
// the D = 8 and D = 64 passes 8-wave workgroups (x halo 256 of 2048 px instead of 256 of 1024);
// 4 rows of prefetch.  acc: 0 = plain pass, 1 = also carry the plane sum (p_in -> p_out),
// 2 = last pass of a sum (adds the smooth plane, streaming store).
template <int K, int ACC>
static int wt_fused_dispatch_acc(wt_plan *p, const FusedArgs &a, int s0, int ns, const FusedRows &rows)
{
    typedef float T;
    static const char *names[4][7] = {
        {"wt_fused<d1x3>", "wt_fused<d1x2>", "wt_fused<d8x3>", "wt_fused<d8x2>", "wt_fused<d64x2>", "wt_fused<d1x4>", "wt_fused<d16x4>"},
        {"wt_fused_acc<d1x3>", "wt_fused_acc<d1x2>", "wt_fused_acc<d8x3>", "wt_fused_acc<d8x2>", "wt_fused_acc<d64x2>", "wt_fused_acc<d1x4>",
         "wt_fused_acc<d16x4>"},
        {"wt_fused_sum<d1x3>", "wt_fused_sum<d1x2>", "wt_fused_sum<d8x3>", "wt_fused_sum<d8x2>", "wt_fused_sum<d64x2>", "wt_fused_sum<d1x4>",
         "wt_fused_sum<d16x4>"},
        {"wt_fused_hist<d1x3>", "wt_fused_hist<d1x2>", "", "", "", "wt_fused_hist<d1x4>", ""}};
    // 3-tap family: FOUR scales per pass (register window 2 * 15 float4): L = 8 is two passes,
    // (0,4) at D = 1 and (4,4) at D = 16 (x halo 240 px: 8-wave workgroups; the accumulate variants
    // take 7 waves, their delay rings of 3 + 5 + 9 rows would not fit the LDS with 8)
    if constexpr (K == 3) {
        if (s0 == 0 && ns == 4) return wt_fused_launch_t<T, K, 4, 1, 4, 4, ACC>(p, a, names[ACC][5], rows);
        if constexpr (ACC != 3) {
            if (s0 == 4 && ns == 4)
                return wt_fused_launch_t<T, K, 4, 16, (ACC == 0 ? 8 : 7), (ACC == 0 ? 4 : 2), ACC>(p, a, names[ACC][6], rows);   // (accumulate: 2 rows ahead, 256 VGPRs)
        }
    }
    if (s0 == 0 && ns == 3) return wt_fused_launch_t<T, K, 3, 1, 4, 4, ACC>(p, a, names[ACC][0], rows);
    if (s0 == 0 && ns == 2) return wt_fused_launch_t<T, K, 2, 1, 4, 4, ACC>(p, a, names[ACC][1], rows);
    if constexpr (ACC != 3) {
        if (s0 == 3 && ns == 3) return wt_fused_launch_t<T, K, 3, 8, 8, 4, ACC>(p, a, names[ACC][2], rows);
        if (s0 == 3 && ns == 2) return wt_fused_launch_t<T, K, 2, 8, 8, 4, ACC>(p, a, names[ACC][3], rows);
        // D = 64 (scales 6-7): taps are 16 / 32 lanes apart
        if (s0 == 6 && ns == 2) return wt_fused_launch_t<T, K, 2, 64, 8, 4, ACC>(p, a, names[ACC][4], rows);
    }
    // Single-scale passes that END a schedule ((3,1) of 4 scales, (6,1) of 7): with them every pass
    // of such a schedule can carry the plane sum (wt_decompose_sum, the interleaved denoise).  The
    // plain variant exists so that wt_decompose writes the same bits as wt_decompose_sum (the fused
    // passes filter rows first, the per-scale kernels columns first: last-bit differences).
    if constexpr (ACC != 3) {
        static const char *names1[3][2] = {{"wt_fused<d8x1>", "wt_fused<d64x1>"}, {"wt_fused_acc<d8x1>", "wt_fused_acc<d64x1>"},
                                           {"wt_fused_sum<d8x1>", "wt_fused_sum<d64x1>"}};
        if (s0 == 3 && ns == 1) return wt_fused_launch_t<T, K, 1, 8, 8, (K == 5 ? 4 : 2), ACC>(p, a, names1[ACC][0], rows);
        if (s0 == 6 && ns == 1) return wt_fused_launch_t<T, K, 1, 64, 8, (K == 5 ? 4 : 2), ACC>(p, a, names1[ACC][1], rows);
    }
    WT_FAIL("fused pass (first scale %d, %d scales) is not built", s0, ns);
}

// the float64 passes (wt_plan64; called from wt_f64.h through wt_fused_tu.hip)
template <int K, int ACC>
static int wt_fused64_dispatch_acc(wt_plan64 *p, const FusedArgsT<double> &a, int s0, int ns, const FusedRows &rows)
{
    typedef double T;
    static const char *pre[4] = {"wt64_fused", "wt64_fused_acc", "wt64_fused_sum", "wt64_fused_hist"};
    static char names[4][16][32];
    auto nm = [&](int slot, const char *tag) -> const char * {
        if (!names[ACC][slot][0]) snprintf(names[ACC][slot], sizeof names[ACC][slot], "%s<%s>", pre[ACC], tag);
        return names[ACC][slot];
    };
    // Workgroup shapes as the float passes: 4 waves at D = 1 (512 pixels per row step), 8 waves for
    // the dilated passes (1024 pixels, x halo 112 / 48 / 192 px per side) - the four-scale accumulate
    // variants included: a double2 lane owns 2 pixels, so the 240-pixel halo leaves 272 storing lanes
    // and the delay rings (17 rows x 273 x 16 B) fit beside the row buffers (140 KB of LDS), where the
    // float variant (392 storing lanes) has to drop to 7 waves.  8 instead of 7 waves: 0.86 -> 0.75 ms
    // for the (4,4) pass that carries the sum at 8192^2.
    if constexpr (K == 3) {
        if (s0 == 0 && ns == 4) return wt_fused_launch_t<T, K, 4, 1, 4, 4, ACC>(p, a, nm(7, "d1x4"), rows);
        if constexpr (ACC != 3) {
            if (s0 == 4 && ns == 4) return wt_fused_launch_t<T, K, 4, 16, 8, (ACC == 0 ? 4 : 2), ACC>(p, a, nm(8, "d16x4"), rows);
        }
    }
    if (s0 == 0 && ns == 3) return wt_fused_launch_t<T, K, 3, 1, 4, 4, ACC>(p, a, nm(0, "d1x3"), rows);
    if (s0 == 0 && ns == 2) return wt_fused_launch_t<T, K, 2, 1, 4, 4, ACC>(p, a, nm(1, "d1x2"), rows);
    if constexpr (ACC != 3) {      // (the histogram variant exists for the first pass only)
        if (s0 == 3 && ns == 3) return wt_fused_launch_t<T, K, 3, 8, 8, 4, ACC>(p, a, nm(2, "d8x3"), rows);
        if (s0 == 3 && ns == 2) return wt_fused_launch_t<T, K, 2, 8, 8, 4, ACC>(p, a, nm(3, "d8x2"), rows);
        if (s0 == 6 && ns == 2) return wt_fused_launch_t<T, K, 2, 64, 8, 4, ACC>(p, a, nm(4, "d64x2"), rows);
        if (s0 == 3 && ns == 1) return wt_fused_launch_t<T, K, 1, 8, 8, (K == 5 ? 4 : 2), ACC>(p, a, nm(5, "d8x1"), rows);
        if (s0 == 6 && ns == 1) return wt_fused_launch_t<T, K, 1, 64, 8, (K == 5 ? 4 : 2), ACC>(p, a, nm(6, "d64x1"), rows);
    }
    WT_FAIL("float64 fused pass (first scale %d, %d scales) is not built", s0, ns);
}

