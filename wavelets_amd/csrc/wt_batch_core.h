// Host core of the two batch engines, written once over the element type: wt_batch (wt_batch.hip, float) and
// wt_batch64 (wt_batch64.hip, double) derive from WtBatchCore<T>.  It holds what both have - the common planes and
// their lazy allocation, the frame checks, the table ring of per-frame parameter pairs, the host <-> plane copy, the
// schedule run and the bilateral loop, the shared argument checks, the arguments and the table of the threshold sums,
// fill and replicate, the reduce buffers, the release of every common buffer.  Kernels, launch lines and the median
// select stay in the engine's file; where a shared function needs one of them the engine hands it in as a callable.
// Every message carries the engine's prefix (`name`) or the entry point's name (`who`), so the texts are the ones
// each engine had of its own.  The Richardson-Lucy half is wt_batch_rl.h, on top of this header.
// Host code, but for the two loops of fill and replicate over 16-byte groups (batch_fill_groups,
// batch_replicate_groups), which each engine wraps in its kernel; included by the two engine files (through
// wt_batch_rl.h) and by nothing else.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "wt_host.h"
#include "wt_fused_decl.h"
#include "wt_stencil_launch.h"

template <typename T>
struct WtBatchCore {
    const char *name;               // "wt_batch" / "wt_batch64": the prefix of the messages
    wt_ctx *ctx = nullptr;
    int family = WT_B3SPLINE;
    int n = 0, max_level = 0;
    int64_t fstride = 0;            // elements from one frame to the next (H * P)
    Geo g;                          // ONE frame's geometry (P in elements)
    std::vector<T *> coef;          // planes 0 .. max_level
    T *input = nullptr, *out = nullptr, *scr[2] = {nullptr, nullptr};
    // wow: WT_PLANE_SCRATCH(3) = the output plane of wow_scale (swapped with the coefficient plane, as the per-frame
    // wow_scale does), WT_PLANE_SCRATCH(4) = the gamma accumulator (utils.wow's plane ids)
    T *spare = nullptr, *gamma = nullptr;
    T *noise = nullptr;             // WT_PLANE_SCRATCH(5): the per-pixel noise maps of the frames (Coefficients' noise plane id)
    // planes only one engine has: their slot for an id (or null), and how the "not a plane" message lists them
    T **(*extra_plane)(WtBatchCore *, int id) = nullptr;
    std::string extra_planes;
    double *d_tau = nullptr;        // the per-frame threshold (and weight) rows of denoise_sum / enhance_sum
    double *h_tau = nullptr;        // pinned staging of the table
    // per-frame parameter pairs of one launch ({tau, factor}, {gmin, gmax}): a ring of table slots [n][2], pinned
    // staging + device copy; a slot is refilled only after the copy that last read it has completed (its event)
    static constexpr int kTabSlots = 16;
    double *d_ptab = nullptr, *h_ptab = nullptr;
    hipEvent_t ptab_ev[kTabSlots] = {};
    int ptab_next = 0;
    // reduce: [n][red_blocks][4] partials + [n][4] results on the device, [n][4] pinned
    double *d_red = nullptr, *h_red = nullptr;
    int red_blocks = 0;

    explicit WtBatchCore(const char *prefix) : name(prefix) {}
};

// ------------------------------------------------------------------------------------------------ planes, frames
// a plane of the batch by id, allocated on first use
template <typename T>
static int batch_plane(WtBatchCore<T> *b, int id, T **out)
{
    T **slot = nullptr;
    if (id >= 0 && id <= b->max_level) slot = &b->coef[id];
    else if (id == WT_PLANE_INPUT) slot = &b->input;
    else if (id == WT_PLANE_OUT) slot = &b->out;
    else if (id == WT_PLANE_SCRATCH(0)) slot = &b->scr[0];
    else if (id == WT_PLANE_SCRATCH(1)) slot = &b->scr[1];
    else if (id == WT_PLANE_SCRATCH(3)) slot = &b->spare;
    else if (id == WT_PLANE_SCRATCH(4)) slot = &b->gamma;
    else if (id == WT_PLANE_SCRATCH(5)) slot = &b->noise;
    else if (b->extra_plane) slot = b->extra_plane(b, id);
    if (!slot)
        WT_FAIL("%s: plane %d is not a plane of a batch (0..%d, input, out, scratch 0/1/3/4/5%s)", b->name, id, b->max_level,
                b->extra_planes.c_str());
    if (!*slot) WT_HIP(hipMalloc((void **)slot, (size_t)b->n * (size_t)b->fstride * sizeof(T)));
    b->ctx->overlap_plan = nullptr;      // a batch's launches are main-stream work: no plan keeps the side route (wt_ctx)
    *out = *slot;
    return 0;
}

template <typename T>
static int batch_check_frames(const WtBatchCore<T> *b, int nf, const char *who)
{
    if (!b) WT_FAIL("%s: null batch", who);
    if (nf < 1 || nf > b->n) WT_FAIL("%s: %d active frames (batch of %d)", who, nf, b->n);
    return 0;
}

template <typename T>
static int batch_check_range(const WtBatchCore<T> *b, int f0, int nf, const char *who)
{
    if (f0 < 0 || nf < 1 || f0 + nf > b->n) WT_FAIL("%s: frames [%d, %d) outside the batch of %d", who, f0, f0 + nf, b->n);
    return 0;
}

// the frames of a batched stencil launch on the batch's stream: ONE frame's geometry (what a plan of that shape hands
// the per-frame launcher, so the kernel choice and the streaming-store flag are its own)
template <typename T>
static StencilCtx batch_stencil_ctx(const WtBatchCore<T> *b)
{
    return StencilCtx{b->ctx, b->ctx->stream, b->g, b->family};
}

template <typename T>
static WtFrames batch_frames(const WtBatchCore<T> *b, int nf, const double *ftab = nullptr)
{
    WtFrames fr;
    fr.n = nf;
    fr.fstride = b->fstride;
    fr.ftab = ftab;
    return fr;
}

// the batched per-scale stencil of each element type under its profiling name (MODE_DECOMP, or a wow mode)
static inline int batch_stencil_launch(const StencilCtx &sc, int mode, const ChainArgsT<float> &a, int s, const WtFrames &fr)
{
    return wt32_stencil_batch_launch(sc, mode, a, s, mode == MODE_DECOMP ? "wt_chain_batch_kernel<decomp>" : "wt_chain_batch_kernel<wow>", fr);
}
static inline int batch_stencil_launch(const StencilCtx &sc, int mode, const ChainArgsT<double> &a, int s, const WtFrames &fr)
{
    return wt64_stencil_batch_launch(sc, mode, a, s, mode == MODE_DECOMP ? "wt64_chain_batch_kernel<decomp>" : "wt64_chain_batch_kernel<wow>", fr);
}

// ------------------------------------------------------------------------------------------------ create, release
// the arguments both create calls refuse, in their order; clears *out
template <typename B>
static int batch_check_create(wt_ctx *ctx, B **out, int n, int H, int W, int family, int max_level, const char *who)
{
    if (!ctx || !out) WT_FAIL("%s: null pointer", who);
    *out = nullptr;
    if (n < 1 || n > 65535) WT_FAIL("%s: %d frames (1..65535 per batch)", who, n);
    if (H < 1 || W < 1) WT_FAIL("%s: frame %d x %d", who, H, W);
    if (family != WT_B3SPLINE && family != WT_TRIANGLE) WT_FAIL("%s: family %d (built-in families only)", who, family);
    if (max_level < 0 || max_level > 30) WT_FAIL("%s: max_level %d", who, max_level);
    return 0;
}

// the shape of a new batch: frames of H x W at a pitch of P elements
template <typename T>
static void batch_init(WtBatchCore<T> *b, wt_ctx *ctx, int n, int H, int W, int P, int family, int max_level)
{
    b->ctx = ctx;
    b->family = family;
    b->n = n;
    b->max_level = max_level;
    b->g = Geo{W, P, H, 0, H, 0, 0};
    b->fstride = (int64_t)H * P;
    b->coef.assign(max_level + 1, nullptr);
}

// every buffer of the core back to the runtime (the failure path of create, destroy); *bad = 1 when one would not go
template <typename T>
static void batch_release(WtBatchCore<T> *b, int *bad)
{
    auto f = [&](void *q) { if (q && hipFree(q) != hipSuccess) *bad = 1; };
    auto hf = [&](void *q) { if (q && hipHostFree(q) != hipSuccess) *bad = 1; };
    for (T *q : b->coef) f(q);
    f(b->input);
    f(b->out);
    f(b->scr[0]);
    f(b->scr[1]);
    f(b->spare);
    f(b->gamma);
    f(b->noise);
    f(b->d_tau);
    f(b->d_ptab);
    f(b->d_red);
    hf(b->h_tau);
    hf(b->h_ptab);
    hf(b->h_red);
    for (hipEvent_t e : b->ptab_ev)
        if (e && hipEventDestroy(e) != hipSuccess) *bad = 1;
}

template <typename T>
static int batch_info(WtBatchCore<T> *b, int64_t *info, const char *who)
{
    if (!b || !info) WT_FAIL("%s: null pointer", who);
    const int64_t v[7] = {b->n, b->g.H, b->g.W, b->g.P, b->fstride, b->max_level, b->family};
    memcpy(info, v, sizeof v);
    return 0;
}

template <typename T>
static int batch_plane_ptr(WtBatchCore<T> *b, int plane, void **ptr, int64_t *frame_stride, const char *who)
{
    if (!b || !ptr || !frame_stride) WT_FAIL("%s: null pointer", who);
    WtGuard guard_(b->ctx);
    T *q = nullptr;
    WT_TRY(batch_plane(b, plane, &q));
    *ptr = q;
    *frame_stride = b->fstride;
    return 0;
}

// ------------------------------------------------------------------------------------------------ transfers
// frames [f0, f0 + nf) of a plane <-> host frames `hstride` elements apart (rows of W elements back to back within a frame)
template <typename T>
static int batch_copy(WtBatchCore<T> *b, int plane, int f0, int nf, T *host, int64_t hstride, bool up, const char *who)
{
    if (!b || !host) WT_FAIL("%s: null pointer", who);
    WT_TRY(batch_check_range(b, f0, nf, who));
    const Geo &g = b->g;
    const int64_t fpx = (int64_t)g.H * g.W;
    if (hstride == 0) hstride = fpx;
    if (hstride < fpx) WT_FAIL("%s: host frame stride %lld below the %lld pixels of a frame", who, (long long)hstride, (long long)fpx);
    WtGuard guard_(b->ctx);
    WT_TRY(wt_side_join(b->ctx));
    T *q = nullptr;
    WT_TRY(batch_plane(b, plane, &q));
    T *dev = q + (int64_t)f0 * b->fstride;
    const size_t span = ((size_t)(nf - 1) * (size_t)hstride + (size_t)fpx) * sizeof(T);
    const bool pinned = try_pin(host, span);     // (no-op for page-locked blocks: _lib.host_empty)
    hipError_t e = hipSuccess;
    // contiguous frames are one tall image of nf * H rows; else one 2-D copy per frame
    const int pieces = hstride == fpx ? 1 : nf;
    const size_t rows = (size_t)g.H * (size_t)(hstride == fpx ? nf : 1);
    const size_t dpitch = (size_t)g.P * sizeof(T), hpitch = (size_t)g.W * sizeof(T);
    for (int i = 0; i < pieces && e == hipSuccess; ++i) {
        T *d = dev + (int64_t)i * b->fstride, *h = host + (int64_t)i * hstride;
        e = up ? hipMemcpy2DAsync(d, dpitch, h, hpitch, hpitch, rows, hipMemcpyHostToDevice, b->ctx->stream)
               : hipMemcpy2DAsync(h, hpitch, d, dpitch, hpitch, rows, hipMemcpyDeviceToHost, b->ctx->stream);
    }
    hipError_t e2 = hipStreamSynchronize(b->ctx->stream);
    if (e == hipSuccess) e = e2;
    if (pinned) (void)hipHostUnregister(host);
    WT_HIP(e);
    return 0;
}

// level 0 of a transform: the active frames of `src` -> plane 0
template <typename T>
static int batch_copy_to_plane0(WtBatchCore<T> *b, int nf, const T *src)
{
    T *d = nullptr;
    WT_TRY(batch_plane(b, 0, &d));
    WT_HIP(hipMemcpyAsync(d, src, (size_t)nf * (size_t)b->fstride * sizeof(T), hipMemcpyDeviceToDevice, b->ctx->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------ the table ring
// per-frame parameter pairs (pairs[2 * f], pairs[2 * f + 1]) -> a device table slot, stream-ordered (*dev)
template <typename T>
static int batch_table(WtBatchCore<T> *b, int nf, const double *pairs, const double **dev)
{
    wt_ctx *c = b->ctx;
    constexpr int slots = WtBatchCore<T>::kTabSlots;
    if (!b->d_ptab) {
        WT_HIP(hipMalloc((void **)&b->d_ptab, (size_t)slots * b->n * 2 * sizeof(double)));
        WT_HIP(hipHostMalloc((void **)&b->h_ptab, (size_t)slots * b->n * 2 * sizeof(double), 0));
    }
    const int slot = b->ptab_next;
    b->ptab_next = (slot + 1) % slots;
    if (b->ptab_ev[slot]) WT_HIP(hipEventSynchronize(b->ptab_ev[slot]));    // (the copy of kTabSlots calls ago)
    else WT_HIP(hipEventCreateWithFlags(&b->ptab_ev[slot], hipEventDisableTiming));
    double *h = b->h_ptab + (size_t)slot * b->n * 2, *d = b->d_ptab + (size_t)slot * b->n * 2;
    memcpy(h, pairs, (size_t)nf * 2 * sizeof(double));
    WT_HIP(hipMemcpyAsync(d, h, (size_t)nf * 2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    WT_HIP(hipEventRecord(b->ptab_ev[slot], c->stream));
    *dev = d;
    return 0;
}

// {lo[f], hi[f]} of the active frames as doubles -> a table slot ({tau, factor} of wow, {gmin, gmax} of the gamma blend)
template <typename T, typename A, typename B>
static int batch_pairs(WtBatchCore<T> *b, int nf, const A *lo, const B *hi, const double **dev)
{
    std::vector<double> pairs((size_t)nf * 2);
    for (int f = 0; f < nf; ++f) {
        pairs[2 * f] = (double)lo[f];
        pairs[2 * f + 1] = (double)hi[f];
    }
    return batch_table(b, nf, pairs.data(), dev);
}

// ------------------------------------------------------------------------------------------------ the transform
// one single-scale pass of the transform on the batched MODE_DECOMP stencil (the per-frame drivers' per-scale branch)
template <typename T>
static int batch_stencil_pass(WtBatchCore<T> *b, int nf, int cur, int nxt, int s0)
{
    if (s0 < 0 || s0 > 24 || s0 > b->max_level) WT_FAIL("%s_decompose: scale %d outside the batch (max_level %d)", b->name, s0, b->max_level);
    if (cur == nxt || cur == s0 || nxt == s0) WT_FAIL("%s_decompose: input/output planes alias the detail plane of the pass", b->name);
    T *in = nullptr, *oc = nullptr, *ow = nullptr;
    WT_TRY(batch_plane(b, cur, &in));
    WT_TRY(batch_plane(b, nxt, &oc));
    WT_TRY(batch_plane(b, s0, &ow));
    ChainArgsT<T> a{};
    a.in = in; a.out_c = oc; a.out_w = ow;
    a.f1 = 1; a.f2 = 1;
    return batch_stencil_launch(batch_stencil_ctx(b), MODE_DECOMP, a, s0, batch_frames(b, nf));
}

// The arguments of one fused pass and its planes, allocated in this order: cur, nxt, the ns detail planes, then - for
// acc != 0, once it is known to alias none of them - the sum plane (*ps; null for a plain pass).
template <typename T>
static int batch_pass_planes(WtBatchCore<T> *b, int cur, int nxt, int s0, int ns, int acc, int sum_plane, bool first, T **in, T **oc,
                             T *ow[WT_FUSED_MAX_SCALES], T **ps)
{
    if (ns < 1 || ns > WT_FUSED_MAX_SCALES || s0 < 0 || s0 + ns - 1 > b->max_level)
        WT_FAIL("%s_decompose_pass: scales [%d,%d) outside the batch (max_level %d)", b->name, s0, s0 + ns, b->max_level);
    if (cur == nxt || (cur >= s0 && cur < s0 + ns) || (nxt >= s0 && nxt < s0 + ns))
        WT_FAIL("%s_decompose_pass: input/output planes alias the detail planes of the pass", b->name);
    if (!wt_fused_has_pass(s0, ns, b->family)) WT_FAIL("%s_decompose_pass: no fused kernel for first scale %d x %d scales", b->name, s0, ns);
    if (acc && first != (s0 == 0))
        WT_FAIL("%s_decompose_pass_sum: first must be set for the pass that starts at scale 0 and only for it (got first=%d, s0=%d)", b->name,
                (int)first, s0);
    WT_TRY(batch_plane(b, cur, in));
    WT_TRY(batch_plane(b, nxt, oc));
    for (int k = 0; k < ns; ++k) WT_TRY(batch_plane(b, s0 + k, &ow[k]));
    if (acc) {
        if (sum_plane == cur || sum_plane == nxt || (sum_plane >= s0 && sum_plane < s0 + ns))
            WT_FAIL("%s_decompose_pass_sum: the sum plane aliases a plane of the pass", b->name);
        WT_TRY(batch_plane(b, sum_plane, ps));
    }
    return 0;
}

// The passes of a transform of `level` scales from `src`, ping-pong over scratch planes 0/1; with_sum: every pass
// carries the plane sum into `dst`.  The engine supplies its schedule - schedule(level, with_sum, tr, &np, who) gives
// the passes or refuses - and its fused pass - fused_pass(nf, cur, nxt, s0, ns, acc, sum_plane, first); a pass without
// a fused kernel (single-scale, in a schedule without a sum) takes the batched stencil.
template <typename T, typename Schedule, typename FusedPass>
static int batch_schedule_run(WtBatchCore<T> *b, int nf, int src, int level, bool with_sum, int dst, const char *who, Schedule schedule,
                              FusedPass fused_pass)
{
    if (src >= 0 && src <= level) WT_FAIL("%s: src plane %d is one of the output planes", who, src);
    if (src == WT_PLANE_SCRATCH(0) || src == WT_PLANE_SCRATCH(1)) WT_FAIL("%s: scratch planes 0/1 are used internally", who);
    if (with_sum && ((dst >= 0 && dst <= level) || dst == src || dst == WT_PLANE_SCRATCH(0) || dst == WT_PLANE_SCRATCH(1)))
        WT_FAIL("%s: dst plane %d is an input / output / internal plane of the transform", who, dst);
    int32_t tr[3 * 32];
    int np = 0;
    WT_TRY(schedule(level, with_sum, tr, &np, who));
    int cur = src;
    for (int i = 0; i < np; ++i) {
        const int s0 = tr[3 * i], ns = tr[3 * i + 1];
        const bool last = s0 + ns == level;
        const int nxt = last ? level : WT_PLANE_SCRATCH(i & 1);
        if (!wt_fused_has_pass(s0, ns, b->family)) WT_TRY(batch_stencil_pass(b, nf, cur, nxt, s0));
        else WT_TRY(fused_pass(nf, cur, nxt, s0, ns, with_sum ? (last ? 2 : 1) : 0, dst, i == 0));
        cur = nxt;
    }
    return 0;
}

// The bilateral transform for the active frames (watroo/wavelets.py:433-442): scale s reads the current smooth, writes
// c_{s+1} to a scratch plane (the two ping-pong; plane `level` on the last scale) and w_s to plane s, the variance
// formed in the march with f1 = sigma_b[s]^2, f2 = s + 1 under bilateral_scaling.  One launch per scale for all
// frames: launch(a, s, frames).  refuse(): the engine's own objection to marching at all (after the level-0 copy).
template <typename T, typename Refuse, typename Launch>
static int batch_decompose_bilateral(WtBatchCore<T> *b, int nf, int src, int level, const double *sigma_b, int bilateral_scaling, const char *who,
                                     Refuse refuse, Launch launch)
{
    if (!sigma_b) WT_FAIL("%s: null pointer", who);
    if (level < 0 || level > b->max_level) WT_FAIL("%s: level %d exceeds the batch's max_level %d", who, level, b->max_level);
    if (src >= 0 && src <= level) WT_FAIL("%s: src plane %d is one of the output planes", who, src);
    if (src == WT_PLANE_SCRATCH(0) || src == WT_PLANE_SCRATCH(1)) WT_FAIL("%s: scratch planes 0/1 are used internally", who);
    if (level > 25) WT_FAIL("%s: scale %d out of range", who, level - 1);
    T *in = nullptr;
    WT_TRY(batch_plane(b, src, &in));
    if (level == 0) return batch_copy_to_plane0(b, nf, in);
    WT_TRY(refuse());
    const WtFrames fr = batch_frames(b, nf);
    for (int s = 0; s < level; ++s) {
        const int nxt = (s == level - 1) ? level : WT_PLANE_SCRATCH(s & 1);
        T *oc = nullptr, *ow = nullptr;
        WT_TRY(batch_plane(b, nxt, &oc));
        WT_TRY(batch_plane(b, s, &ow));
        ChainArgsT<T> a{};
        a.in = in; a.out_c = oc; a.out_w = ow;
        // variance = sdev_loc(c_s)^2-form * sigma_b[s]**2 (* (s+1))   watroo/wavelets.py:434-436
        a.f1 = (T)(sigma_b[s] * sigma_b[s]);
        a.f2 = bilateral_scaling ? (T)(s + 1) : (T)1;
        WT_TRY(launch(a, s, fr));
        in = oc;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ threshold sums
// what denoise_sum, denoise_sum_map and enhance_sum refuse alike; min_den: the fewest thresholded planes (0, or 1)
template <typename T>
static int batch_check_sum(const WtBatchCore<T> *b, int count, int dst, int n_den, int min_den, const double *tau, const double *wgt, const char *who)
{
    if (count < 1 || count > WT_MAX_SUM_PLANES || count - 1 > b->max_level)
        WT_FAIL("%s: count %d out of range [1,%d]", who, count, std::min(WT_MAX_SUM_PLANES, b->max_level + 1));
    if (n_den < min_den || n_den > count) WT_FAIL("%s: n_den %d outside [%d,%d]", who, n_den, min_den, count);
    if (n_den > 0 && (!tau || !wgt)) WT_FAIL("%s: null tau/wgt", who);
    if (dst >= 0 && dst < count) WT_FAIL("%s: dst plane %d is one of the summed planes", who, dst);
    return 0;
}

// the head of a threshold sum's kernel arguments (Args: the engine's struct - p[], n, n_den, soft, write_back) with
// planes 0 .. count - 1, then the destination plane
template <typename T, typename Args>
static int batch_sum_args(WtBatchCore<T> *b, int count, int dst, int n_den, int soft, int write_back, Args *a, T **o)
{
    a->n = count; a->n_den = n_den; a->soft = soft; a->write_back = write_back;
    for (int i = 0; i < count; ++i) WT_TRY(batch_plane(b, i, &a->p[i]));
    return batch_plane(b, dst, o);
}

// The per-frame rows of a threshold sum -> d_tau: fill_row(f, r) writes the `row` doubles of frame f (what a row
// holds is the engine's; nf <= n and row <= the doubles per frame the engine allocated).  The table goes up
// stream-ordered from pinned staging, and the previous call's kernel may still read d_tau: drain first.
template <typename T, typename FillRow>
static int batch_sum_table(WtBatchCore<T> *b, int nf, int row, FillRow fill_row)
{
    WT_HIP(hipStreamSynchronize(b->ctx->stream));
    for (int f = 0; f < nf; ++f) fill_row(f, b->h_tau + (size_t)f * row);
    WT_HIP(hipMemcpyAsync(b->d_tau, b->h_tau, (size_t)nf * row * sizeof(double), hipMemcpyHostToDevice, b->ctx->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------ fill, replicate
// x blocks per frame of the batched pointwise kernels (grid y = the frame) over `groups` 16-byte groups per frame:
// about 2048 blocks in all
static inline unsigned batch_frame_blocks(int64_t groups, int nf)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((groups + 255) / 256, (2048 + nf - 1) / nf));
}

// V = float4 / double2: `n` 16-byte groups <- value, by blocks of `block` threads on any grid
template <typename V>
__device__ __forceinline__ void batch_fill_groups(V *d, int64_t n, V value, unsigned block)
{
    for (int64_t i = (int64_t)blockIdx.x * block + threadIdx.x; i < n; i += (int64_t)gridDim.x * block) d[i] = value;
}

// frame 0 of a plane -> frames 1 .. gridDim.y, `fg` groups apart (a noise map shared by the frames of a chunk crosses PCIe once)
template <typename V>
__device__ __forceinline__ void batch_replicate_groups(V *d, int64_t fg, unsigned block)
{
    const V *src = d;
    V *dst = d + (int64_t)(blockIdx.y + 1) * fg;
    for (int64_t i = (int64_t)blockIdx.x * block + threadIdx.x; i < fg; i += (int64_t)gridDim.x * block) dst[i] = src[i];
}

// plane <- value over the active frames, pitch padding included: launch(d) runs the engine's fill kernel
template <typename T, typename Launch>
static int batch_fill(WtBatchCore<T> *b, int nf, int plane, const char *who, Launch launch)
{
    WT_TRY(batch_check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    T *d = nullptr;
    WT_TRY(batch_plane(b, plane, &d));
    launch(d);
    WT_HIP(hipGetLastError());
    return 0;
}

// frame 0 of the plane -> the other active frames: launch(d) runs the engine's replicate kernel on a grid of
// (batch_frame_blocks, nf - 1)
template <typename T, typename Launch>
static int batch_replicate(WtBatchCore<T> *b, int nf, int plane, const char *who, Launch launch)
{
    WT_TRY(batch_check_frames(b, nf, who));
    WtGuard guard_(b->ctx);
    T *d = nullptr;
    WT_TRY(batch_plane(b, plane, &d));
    if (nf == 1) return 0;
    launch(d);
    WT_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ wow
// the planes of a pointwise wow update: the updated plane, the gamma accumulator and the noise maps (either may be
// WT_PLANE_NONE: null), then the frames' {tau, factor} table
template <typename T, typename F>
static int batch_wow_update_args(WtBatchCore<T> *b, int nf, int plane, const double *tau, const F *factor, int gamma_plane, int noise_plane,
                                 const char *who, T **c, T **gm, T **nz, const double **dt)
{
    if (gamma_plane == plane) WT_FAIL("%s: the gamma plane is the updated plane", who);
    if (noise_plane != WT_PLANE_NONE && (noise_plane == plane || noise_plane == gamma_plane)) WT_FAIL("%s: the noise plane aliases a plane of the update", who);
    WT_TRY(batch_plane(b, plane, c));
    if (gamma_plane != WT_PLANE_NONE) WT_TRY(batch_plane(b, gamma_plane, gm));
    if (noise_plane != WT_PLANE_NONE) WT_TRY(batch_plane(b, noise_plane, nz));
    if (!tau || !factor) WT_FAIL("%s: null tau / factor", who);
    return batch_pairs(b, nf, tau, factor, dt);
}

template <typename T>
static int batch_check_wow_scale(const WtBatchCore<T> *b, int plane, int s, const char *who)
{
    if (plane < 0 || plane > b->max_level) WT_FAIL("%s: plane %d is not a coefficient plane", who, plane);
    if (s < 0 || s > 24) WT_FAIL("%s: scale %d out of range", who, s);
    return 0;
}

// The fused wow update of scale s (local power, significance, gamma sum, whitening) for the active frames, after
// batch_check_wow_scale: ONE launch of the batched stencil into WT_PLANE_SCRATCH(3), then the swap of the two planes.
// (the per-frame wow_scale's arguments and its choice of instantiation; tau and factor come from the frame's row of the table)
template <typename T, typename F>
static int batch_wow_scale_run(WtBatchCore<T> *b, int nf, int plane, int s, const double *tau, int soft, const F *factor, int gamma_plane,
                               int noise_plane, const char *who)
{
    if (gamma_plane == plane || gamma_plane == WT_PLANE_SCRATCH(3)) WT_FAIL("%s: the gamma plane aliases a plane of the update", who);
    if (noise_plane != WT_PLANE_NONE && (noise_plane == plane || noise_plane == WT_PLANE_SCRATCH(3) || noise_plane == gamma_plane))
        WT_FAIL("%s: the noise plane aliases a plane of the update", who);
    T *c = nullptr, *t = nullptr, *gm = nullptr, *nz = nullptr;
    WT_TRY(batch_plane(b, plane, &c));
    WT_TRY(batch_plane(b, WT_PLANE_SCRATCH(3), &t));
    if (gamma_plane != WT_PLANE_NONE) WT_TRY(batch_plane(b, gamma_plane, &gm));
    if (noise_plane != WT_PLANE_NONE) WT_TRY(batch_plane(b, noise_plane, &nz));
    if (!tau || !factor) WT_FAIL("%s: null tau / factor", who);
    const double *dt = nullptr;
    WT_TRY(batch_pairs(b, nf, tau, factor, &dt));
    ChainArgsT<T> a{};
    a.in = c; a.out_c = t;
    a.noise = nz; a.gamma = gm; a.soft = soft; a.whiten = 1;
    WT_TRY(batch_stencil_launch(batch_stencil_ctx(b), nz ? MODE_WOW : (gm ? MODE_WOW_GAMMA : MODE_WOW_PLAIN), a, s, batch_frames(b, nf, dt)));
    std::swap(b->coef[plane], b->spare);          // (wow_scale: "in place" at pointer level)
    return 0;
}

// ------------------------------------------------------------------------------------------------ reduce, plane_sum
// the partials and results of reduce for `blocks` blocks per frame; drain: the stream is drained before a regrowth
template <typename T>
static int batch_reduce_buffers(WtBatchCore<T> *b, int blocks, bool drain)
{
    if (b->d_red && b->red_blocks == blocks) return 0;
    if (drain) WT_HIP(hipStreamSynchronize(b->ctx->stream));
    (void)hipFree(b->d_red);
    (void)hipHostFree(b->h_red);
    b->d_red = nullptr;
    b->h_red = nullptr;
    WT_HIP(hipMalloc((void **)&b->d_red, (size_t)b->n * ((size_t)blocks + 1) * 4 * sizeof(double)));
    WT_HIP(hipHostMalloc((void **)&b->h_red, (size_t)b->n * 4 * sizeof(double), 0));
    b->red_blocks = blocks;
    return 0;
}
template <typename T>
static double *batch_reduce_results(WtBatchCore<T> *b)
{
    return b->d_red + (size_t)b->n * b->red_blocks * 4;
}

// after the engine's two launches: {sum, sumsq, min, max} of the active frames -> out
template <typename T>
static int batch_reduce_fetch(WtBatchCore<T> *b, int nf, double *out)
{
    wt_ctx *c = b->ctx;
    WT_HIP(hipGetLastError());
    WT_HIP(hipMemcpyAsync(b->h_red, batch_reduce_results(b), (size_t)nf * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    WT_HIP(hipStreamSynchronize(c->stream));               // the one host round trip for all nf frames
    memcpy(out, b->h_red, (size_t)nf * 4 * sizeof(double));
    return 0;
}

// planes [first, first + count) and dst of a plane sum (max_count: what one launch of the engine's kernel folds)
template <typename T>
static int batch_plane_sum_planes(WtBatchCore<T> *b, int first, int count, int dst, int max_count, const char *who, const T **planes, T **o)
{
    if (count < 1 || count > max_count) WT_FAIL("%s: count %d out of range [1,%d]", who, count, max_count);
    if (first < 0 || first + count - 1 > b->max_level) WT_FAIL("%s: planes [%d,%d) outside [0,%d]", who, first, first + count, b->max_level);
    if (dst >= first && dst < first + count) WT_FAIL("%s: dst plane %d is one of the summed planes", who, dst);
    for (int i = 0; i < count; ++i) {
        T *q = nullptr;
        WT_TRY(batch_plane(b, first + i, &q));
        planes[i] = q;
    }
    return batch_plane(b, dst, o);
}
