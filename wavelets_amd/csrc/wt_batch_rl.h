// The Richardson-Lucy half of the two batch engines (watroo/utils.py:222-290), written once over the element type:
// wt_batch and wt_batch64 derive from WtBatchRl<T>, the core plus richardson_lucy's planes and the two PSF operands.
// Here: the plane lookup and the release of those buffers, and the host side of psf_ok, set_psf, filter2d, binary
// and mrs_update - the argument checks in each engine's order and words (`who`: the entry point's name), the planes,
// the table.  Kernels and launch lines stay in the engine's file and come in as callables; so does whatever one
// engine does differently (wt_batch64.hip: the planes belong to the batch from its first PSF on, the op numbering).
// The element size decides which PSFs one launch takes: the LDS tile of wt_rl_point.h holds sizeof(T) per sample.
// Host only; included by the two engine files and by nothing else.
#pragma once
#include "wt_batch_core.h"
#include "wt_rl_point.h"

template <typename T>
struct WtBatchRl : WtBatchCore<T> {
    explicit WtBatchRl(const char *prefix) : WtBatchCore<T>(prefix) {}
    // WT_PLANE_SCRATCH(6 .. 10) = data, psi, phi, residual, correlation; WT_PLANE_SCRATCH(16 + s) = the support plane
    // of scale s (utils.richardson_lucy's plane ids); d_psf: the forward / backward PSF of set_psf
    T *rl[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<T *> mrs;           // max_level entries, once the planes belong to the batch
    T *d_psf[2] = {nullptr, nullptr};
    size_t psf_cap[2] = {0, 0};
    int psf_kh[2] = {0, 0}, psf_kw[2] = {0, 0};
};

// richardson_lucy's planes by id (WtBatchCore::extra_plane)
template <typename T>
static T **batch_rl_plane(WtBatchCore<T> *core, int id)
{
    WtBatchRl<T> *b = static_cast<WtBatchRl<T> *>(core);
    if (id <= WT_PLANE_SCRATCH(6) && id >= WT_PLANE_SCRATCH(10)) return &b->rl[WT_PLANE_SCRATCH(6) - id];
    if (id <= WT_PLANE_SCRATCH(16) && id > WT_PLANE_SCRATCH(16) - (int)b->mrs.size()) return &b->mrs[WT_PLANE_SCRATCH(16) - id];
    return nullptr;
}

// from here on richardson_lucy's planes are planes of the batch (no-op when they are already)
template <typename T>
static void batch_rl_own_planes(WtBatchRl<T> *b)
{
    if (b->extra_plane) return;
    b->mrs.assign(std::min(b->max_level, WT_NUM_SCRATCH - 16), nullptr);
    b->extra_plane = batch_rl_plane<T>;
    b->extra_planes = ", 6..10, 16.." + std::to_string(15 + (int)b->mrs.size());
}

template <typename T>
static void batch_rl_release(WtBatchRl<T> *b, int *bad)
{
    auto f = [&](void *q) { if (q && hipFree(q) != hipSuccess) *bad = 1; };
    for (T *q : b->rl) f(q);
    for (T *q : b->mrs) f(q);
    f(b->d_psf[0]);
    f(b->d_psf[1]);
}

// host logic: *ok = 1 when set_psf takes a kh x kw PSF - filter2d applies it in ONE launch
template <typename T>
static int batch_psf_ok(int kh, int kw, int *ok, const char *who)
{
    if (!ok) WT_FAIL("%s: null pointer", who);
    *ok = wt_f2d_single_launch(kh, kw, sizeof(T)) ? 1 : 0;
    return 0;
}

// One of the two PSF operands of a richardson_lucy call (slot 0: forward, watroo/utils.py:257; slot 1: backward,
// utils.py:286) -> device memory of the batch, once per call: the iterations then correlate without a stream drain
// and without a PSF copy (the per-frame filter2d does both on every call - its kernel comes from caller-owned memory).
template <typename T>
static int batch_set_psf(WtBatchRl<T> *b, int slot, const T *kernel, int kh, int kw, const char *who)
{
    if (!b || !kernel) WT_FAIL("%s: null pointer", who);
    WtGuard guard_(b->ctx);
    if (slot < 0 || slot > 1) WT_FAIL("%s: slot %d (0: forward, 1: backward)", who, slot);
    if (!wt_f2d_single_launch(kh, kw, sizeof(T)))
        WT_FAIL("%s: a %d x %d PSF is not applied in one launch (at most %d taps, rows of at most %d, an LDS tile of at most %d KB)", who, kh, kw,
                WT_F2D_MAX_TAPS, WT_F2D_MAX_KW, WT_F2D_MAX_LDS / 1024);
    const size_t ntaps = (size_t)kh * kw;
    // a launch on the stream may still read the slot, and `kernel` is the caller's: drain, then copy synchronously
    WT_HIP(hipStreamSynchronize(b->ctx->stream));
    if (ntaps > b->psf_cap[slot]) {
        (void)hipFree(b->d_psf[slot]);
        b->d_psf[slot] = nullptr;
        b->psf_cap[slot] = 0;
        b->psf_kh[slot] = b->psf_kw[slot] = 0;
        WT_HIP(hipMalloc((void **)&b->d_psf[slot], ntaps * sizeof(T)));
        b->psf_cap[slot] = ntaps;
    }
    WT_HIP(hipMemcpy(b->d_psf[slot], kernel, ntaps * sizeof(T), hipMemcpyHostToDevice));
    b->psf_kh[slot] = kh;
    b->psf_kw[slot] = kw;
    return 0;
}

// filter2d per frame (watroo/utils.py:257,286; periodic: the circular products of utils.py:245-254,284) with the PSF
// of `slot`: one launch for all active frames.  kernel_for(periodic) gives the engine's __global__ shell around
// wt_f2d_batch_tile for that border; `prof` is its profiling name.
template <typename T, typename KernelFor>
static int batch_filter2d(WtBatchRl<T> *b, int nf, int src, int dst, int slot, int ay, int ax, int border, const char *who, const char *prof,
                          KernelFor kernel_for)
{
    WT_TRY(batch_check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    if (slot < 0 || slot > 1 || !b->d_psf[slot] || !b->psf_kh[slot]) WT_FAIL("%s: PSF slot %d is not set (%s_set_psf)", who, slot, b->name);
    const int kh = b->psf_kh[slot], kw = b->psf_kw[slot];
    if (!wt_f2d_single_launch(kh, kw, sizeof(T))) WT_FAIL("%s: a %d x %d PSF is not applied in one launch", who, kh, kw);
    if (ay < 0 || ay >= kh || ax < 0 || ax >= kw) WT_FAIL("%s: anchor (%d, %d) outside the %d x %d kernel", who, ay, ax, kh, kw);
    if (src == dst) WT_FAIL("%s: src and dst must differ", who);
    if (border != WT_BORDER_SYMMETRIC && border != WT_BORDER_PERIODIC) WT_FAIL("%s: border %d unsupported (symmetric or periodic)", who, border);
    const Geo &g = b->g;
    dim3 grid((g.W + WT_F2D_TW - 1) / WT_F2D_TW, (g.H + WT_F2D_TH - 1) / WT_F2D_TH, nf), block(64, 4);
    if (grid.y > 65535u) WT_FAIL("%s: frames of %d rows are too tall (%u row tiles, at most 65535)", who, g.H, grid.y);
    if (grid.z > 65535u) WT_FAIL("%s: %d frames in one launch (at most 65535)", who, nf);
    T *in = nullptr, *o = nullptr;
    WT_TRY(batch_plane(b, src, &in));
    WT_TRY(batch_plane(b, dst, &o));
    const size_t lds = wt_f2d_lds_bytes(kh, kw, sizeof(T));
    auto kernel = kernel_for(border == WT_BORDER_PERIODIC);
    ProfScope ps(b->ctx, prof);
    if (lds > 64 * 1024) WT_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, block, lds, b->ctx->stream, (const T *)in, o, g, b->fstride, (const T *)b->d_psf[slot], kh, kw, ay, ax);
    WT_HIP(hipGetLastError());
    return 0;
}

// the binary ops over the active frames (watroo/utils.py:259,280-281,288), op in wt_batch_binary's numbering
// (WT_OP_*): launch(a, b, dst) runs the engine's kernel over the frames as one flat range
template <typename T, typename Launch>
static int batch_binary(WtBatchRl<T> *b, int nf, int op, int a, int b2, int dst, const char *who, Launch launch)
{
    WT_TRY(batch_check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    if (op < 0 || op > WT_OP_ADD_DIV) WT_FAIL("%s: unknown op %d", who, op);
    T *pa = nullptr, *pb = nullptr, *pd = nullptr;
    WT_TRY(batch_plane(b, a, &pa));
    WT_TRY(batch_plane(b, b2, &pb));
    WT_TRY(batch_plane(b, dst, &pd));
    launch((const T *)pa, (const T *)pb, pd);
    WT_HIP(hipGetLastError());
    return 0;
}

// the support update per frame (watroo/utils.py:263-276) with the frame's tau[f], scalar noise only:
// launch(c, mrs, table) runs the engine's kernel with the frame as grid y, {tau[f], 0} the frame's row of the table
template <typename T, typename Launch>
static int batch_mrs_update(WtBatchRl<T> *b, int nf, int plane, int mrs_plane, const double *tau, const char *who, Launch launch)
{
    WT_TRY(batch_check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    if (!tau) WT_FAIL("%s: null tau", who);
    if (plane == mrs_plane) WT_FAIL("%s: plane and mrs_plane must differ", who);
    T *c = nullptr, *m = nullptr;
    WT_TRY(batch_plane(b, plane, &c));
    WT_TRY(batch_plane(b, mrs_plane, &m));
    std::vector<double> pairs((size_t)nf * 2, 0.0);
    for (int f = 0; f < nf; ++f) pairs[2 * f] = tau[f];
    const double *dt = nullptr;
    WT_TRY(batch_table(b, nf, pairs.data(), &dt));
    launch(c, m, dt);
    WT_HIP(hipGetLastError());
    return 0;
}
