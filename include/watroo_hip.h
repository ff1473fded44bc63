/* watroo_hip.h - C ABI of libwatroo_hip.so, the MI355X (gfx950) a-trous wavelet engine.
 *
 * The reference (frederic-auchere/wavelets, "watroo" 0.0.4) is pure Python and has no
 * FFI/plugin interface of its own: its boundary to native code is the handful of calls it
 * makes into OpenCV / numexpr / scipy / numpy.  Each entry point below replaces one of those
 * call sites (cited as file:line relative to /root/reference) for 2-D float32 images, plus
 * the plan/buffer plumbing a device-resident engine needs.  Host Python
 * (wavelets_amd/_lib.py) binds these with ctypes; INTEGRATION.md shows the stub a watroo
 * maintainer would add.
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on failure; wt_last_error() returns a
 *    thread-local message (argument errors, HIP errors, RCCL errors).
 *  - plain pointers and sizes only; host pointers are borrowed for the duration of a call.
 *  - one HIP stream per context; calls on a context are serialised on that stream and are
 *    asynchronous unless they return a host value (upload/download/median/reduce sync).
 *  - images are row-major float32.  A plan describes ONE row strip [row0,row0+nrows) of a
 *    global H x W image (the whole image when nranks == 1).  Planes live in HBM with a row
 *    pitch of round_up(W,4) floats and `halo` margin rows above and below the strip that are
 *    filled by the RCCL halo exchange (nranks > 1) - borders of the GLOBAL image are always
 *    handled by symmetric reflection (cv2.BORDER_REFLECT == np.pad 'symmetric').
 *  - plane ids: 0..max_level are the coefficient planes (plane s = detail w_s, plane
 *    `level` = final smooth); WT_PLANE_INPUT holds the image handed to the transform;
 *    WT_PLANE_OUT the reconstruction; WT_PLANE_SCRATCH(i), i in [0,WT_NUM_SCRATCH), are
 *    general purpose (allocated on first use).
 */
#ifndef WATROO_HIP_H
#define WATROO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WT_ABI_VERSION 8

typedef struct wt_ctx wt_ctx;   /* device + stream (+ RCCL communicator) */
typedef struct wt_plan wt_plan; /* geometry + device planes of one image strip */

enum { WT_TRIANGLE = 0, WT_B3SPLINE = 1 };      /* watroo/wavelets.py:232-287 */

#define WT_PLANE_INPUT (-1)
#define WT_PLANE_OUT (-2)
#define WT_NUM_SCRATCH 32
#define WT_PLANE_SCRATCH(i) (-3 - (i))
#define WT_PLANE_NONE (-1000)

/* ---- library / device ------------------------------------------------------------- */
int wt_abi_version(void);
const char *wt_last_error(void);
int wt_device_count(int *count);
/* process-wide tuning / A-B switches (every setting produces the same bits).
 * "row_kernel" (default 1): single-scale operators use the LDS row kernel where the dilation
 *   allows, 0 forces the chain-march kernel;  "lattice_kernel" (1): lattice kernel for d >= 64;
 *   "bilateral_paired" (1): the float32 bilateral march fetches an operand pair with one 8-byte load (0: two 4-byte loads:
 *                  the generic path of polyphase borders; same bits).
 * "overlap" (1): multi-GPU strips run the halo exchange of the next pass beside the interior
 *   rows of the current one (second stream), 0 = every exchange between the passes;
 *   "overlap_reserve" (16): compute units the interior launch leaves to the RCCL kernels.
 * "fused_fast" (1): fused passes use the single-bounce / whole-group addressing where the image
 *   allows (halo <= image; any width since round 6); 0 forces the generic (multi-bounce, gather) addressing.
 * "scatter" (4; env WT_SCATTER): planes >= 8 MiB of single-GPU plans created from now on are
 *   mapped over shuffled 2-MiB physical chunks created in groups worth this many planes
 *   (DESIGN.md section 2); 0 = one hipMalloc per plane (see wt_plane_ptr).
 * "split_dry" (0): measurement aid - launch the passes of a strip plan split into edge and
 *   interior rows as "overlap" does, without exchanging (FLAG_NO_EXCHANGE runs).
 * "stencil64" (1): float64 images with a built-in family run the tuned per-scale kernels (chain / lattice /
 *   row kernels for double, the float64 bilateral march); 0 = the generic float64 kernels (identical bits for
 *   the filters, 1e-12 for the bilateral operator).  "fused64", "f64_pairs", "select64_list", "hist_window",
 *   "tri4", "host_pipeline", "scatter_strips": further A/B switches of the same kind.
 * "wow_overlap" (1): behind wt_decompose_bilateral / wt64_decompose_bilateral the per-scale wow updates and
 *   the MAD median run on a side stream beside the bilateral scales still queued; 0 = serial order (same bits).
 * "axis_filter" (1): wt_axis_filter / wt64_axis_filter use the tiled kernels; 0 = the tap-list operator
 *   (same bits).
 * (the 2-MiB chunks of "scatter" are 8 MiB since ABI version 7; env WT_SCATTER_CHUNK_KB) */
int wt_set_option(const char *name, int value);

/* ---- context ---------------------------------------------------------------------- */
int wt_ctx_create(int device, wt_ctx **out);
int wt_ctx_destroy(wt_ctx *ctx);
int wt_ctx_sync(wt_ctx *ctx);
/* hipMemGetInfo of the context's device: out[0] = free bytes, out[1] = total bytes (leak checks
 * around plan create / destroy cycles; sizing of strips for 288 GB of HBM). */
int wt_device_memory(wt_ctx *ctx, int64_t out[2]);
/* hipEvent stopwatch on the context's stream (the stream every kernel is launched on). */
int wt_timer_start(wt_ctx *ctx);
int wt_timer_stop(wt_ctx *ctx, float *elapsed_ms);
/* Per-kernel HIP-event profile: when enabled every kernel launch is bracketed by events.
 * wt_profile_entry copies the i-th kernel name (<= 63 chars) and its call count and total
 * device milliseconds.  Used by bench.py for the live roofline figure. */
int wt_profile_enable(wt_ctx *ctx, int on);
int wt_profile_reset(wt_ctx *ctx);
int wt_profile_count(wt_ctx *ctx, int *n);
int wt_profile_entry(wt_ctx *ctx, int i, char *name64, int64_t *calls, double *total_ms);

/* The translation units the library's device code is built as ("core", "transform", "fused_f32_k5_acc0", ...):
 * count and names, in the order a context's warm-up threads know them (wt_ctx_create loads the runtime's copy
 * machinery and the host-side units in the background, a plan's creation the fused passes of its family;
 * wt_ctx_sync waits for both; WATROO_HIP_NO_WARMUP=1 disables).  Build / test bookkeeping - the reference,
 * interpreted Python, has nothing to load (watroo/wavelets.py:1-11). */
int wt_unit_count(void);
const char *wt_unit_name(int i);

/* ---- multi-GPU (one process per GPU; RCCL over xGMI) --------------------------------- */
/* 128-byte ncclUniqueId; rank 0 creates it, the launcher broadcasts it out of band. */
int wt_comm_unique_id(void *id128);
int wt_ctx_comm_init(wt_ctx *ctx, int rank, int nranks, const void *id128);
/* rank / size as the RCCL communicator itself reports them (ncclCommUserRank / ncclCommCount);
 * 0 / 1 without a communicator.  bench.py prints the size as "rccl_ranks". */
int wt_ctx_comm_info(wt_ctx *ctx, int *rank, int *nranks);
/* ncclGetVersion of the loaded RCCL (0: unknown), and one line describing the context's GPU ("device=<hip
 * ordinal> pci=<bus id> cus=<n> name=<...>", NUL-terminated, truncated to cap): what bench.py lists per rank
 * in the multi-GPU line (the reference has no counterpart: it runs on one host, watroo/utils.py:83-219). */
int wt_comm_version(int *version);
int wt_ctx_device_info(wt_ctx *ctx, char *buf, int cap);
/* test hook: nranks==1 periodic self exchange through RCCL send/recv (plumbing check). */
int wt_comm_selftest(wt_ctx *ctx, int64_t nfloats, int *ok);

/* ---- plan --------------------------------------------------------------------------- */
/* Whole image on one GPU. */
int wt_plan_create(wt_ctx *ctx, int64_t H, int64_t W, int family, int max_level,
                   wt_plan **out);
/* Row strip [row0,row0+nrows) of a global H x W image.  halo_rows = margin rows to allocate
 * above/below (>= the largest halo any requested op needs; 0 lets the library size it from
 * max_level).  rank/nranks give the strip's position: neighbours are rank-1 / rank+1. */
int wt_plan_create_strip(wt_ctx *ctx, int64_t H, int64_t W, int family, int max_level,
                         int64_t row0, int64_t nrows, int64_t halo_rows, int rank,
                         int nranks, wt_plan **out);
/* wt_plan_create with the placement of THIS plan's planes given instead of taken from the process-wide "scatter"
 * option: scatter = 0 keeps every plane on plain hipMalloc, n > 0 maps planes >= 8 MiB over shuffled physical chunks
 * created in groups worth n planes.  What the Python API's plan pool uses for its numpy-to-numpy calls
 * (watroo/utils.py:83-102 crosses PCIe both ways: the mapping costs more than it earns there; no counterpart in the
 * reference). */
int wt_plan_create_placed(wt_ctx *ctx, int64_t H, int64_t W, int family, int max_level, int scatter,
                          wt_plan **out);
int wt_plan_destroy(wt_plan *plan);
/* geometry query: out[0..7] = H, W, pitch, row0, nrows, halo, max_level, family */
int wt_plan_info(wt_plan *plan, int64_t out[8]);
/* Device memory held by the plan right now: out[0] = all bytes (hipMalloc'ed planes, the bounce
 * plane of host transfers, mapped chunks, idle chunks), out[1] = bytes of planes mapped over
 * scattered 2-MiB chunks, out[2] = bytes of idle chunks (created in groups, not yet mapped:
 * wt_plan_trim gives them back), out[3] = 1 when this context has stopped scattering planes
 * because the virtual-memory API failed on it (wt_ctx_scatter_status names the failing call; the
 * fused passes run ~20 % slower on physically contiguous planes).  Leaves
 * wt_last_error alone. */
int wt_plan_memory(wt_plan *plan, int64_t out[4]);
/* *disabled = 1 when the context has fallen back to plain hipMalloc per plane; `reason` (up to
 * `cap` bytes, may be NULL) then names the HIP call that failed when it happened.  The fallback
 * is also announced once on stderr.  (No reference counterpart: device-memory management.) */
int wt_ctx_scatter_status(wt_ctx *ctx, int *disabled, char *reason, int cap);
/* Release the plan's idle physical chunks (a plan keeps up to three planes' worth after its last
 * plane was allocated).  The Python plan pool calls this when a plan is handed back. */
int wt_plan_trim(wt_plan *plan);
/* Decomposition schedule (host logic, needs no GPU): for `level` scales of `family`, writes
 * up to `cap` passes as triples {first_scale, n_scales, halo_rows_of_input}.  The same
 * schedule drives the kernels and the halo exchange; tests use it for the gloo CPU model. */
int wt_schedule(int family, int level, int fused, int32_t *triples, int cap, int *n_passes);
/* Border rule of the single-scale operators on this plan: 0 (default) symmetric reflection =
 * cv2.BORDER_REFLECT; 1 = symmetric reflection inside each polyphase component of the
 * operator's dilation - the rule atrous_recursive applies to its sub-arrays
 * (watroo/wavelets.py:354-390); 2 = scipy 'mirror' (reflection without edge duplication), the
 * border of the 1-D branch (watroo/wavelets.py:66-69; a 1-D signal is a 1 x N image); 3 = 'mirror'
 * inside each polyphase component (atrous_recursive on a 1-D signal).
 * Modes 1-3: per-scale kernels only (the bilateral and 3-D operators accept 0 and 1), single GPU. */
int wt_plan_set_border(wt_plan *plan, int border);
/* User-defined scaling function (a subclass of AbstractScalingFunction with its own
 * coefficients_1d, watroo/wavelets.py:152-229): `ntaps` odd 1-D taps (<= 15) replace the plan's
 * built-in family for wt_decompose / wt_decompose_pass (one scale) / wt_atrous_scale /
 * wt_smooth / wt_local_variance / wt_bilateral_conv / wt_decompose_bilateral and the 3-D
 * operators, which then run generic kernels (no fused passes; scratch planes 12, 13 and 15 are
 * used internally); the fused wow update fails.  ntaps = 0 restores the family.  Single GPU.
 * Orientation: taps are applied like cv2.filter2D applies its kernel (correlation, tap j at
 * offset (j - ntaps/2) * 2^s; watroo/wavelets.py:39-45).  The range-weighted operator is a true
 * convolution in the reference (kernel index i at offset (ntaps/2 - i) * 2^s, :87-91) and
 * applies the same taps accordingly.  A caller that stored the taps reversed - to get scipy's
 * convolution for a 1-D signal (:65-69) - passes flag bit3 to the bilateral entry points. */
int wt_plan_set_taps(wt_plan *plan, const float *taps, int ntaps);
/* dst plane <- window of a (larger) source plan's plane starting at (y0, x0); device copy.
 * (atrous_recursive pads by hw*2^(level-1) and crops at the end, watroo/wavelets.py:394-406) */
int wt_crop_plane(wt_plan *src, int src_plane, wt_plan *dst, int dst_plane, int64_t y0,
                  int64_t x0);
/* the reverse: dst[y0:y0+src.nrows, x0:x0+src.W] = src (both windows in LOCAL rows; same
 * device).  With wt_crop_plane this scatters / gathers row strips of a resident image without
 * a host round trip (tools/check_large.py builds and checks a 32768^2 image this way). */
int wt_paste_plane(wt_plan *src, int src_plane, wt_plan *dst, int dst_plane, int64_t y0,
                   int64_t x0);
/* general form: dst[dy:dy+rows, dx:dx+cols] = src[sy:sy+rows, sx:sx+cols] (local rows, same
 * device) - the crop of a padded CUBE back to its (Z, Y, X) block is one window per z slice
 * (atrous_recursive on 3-D data, watroo/wavelets.py:394-406). */
int wt_copy_window(wt_plan *src, int src_plane, wt_plan *dst, int dst_plane, int64_t sy,
                   int64_t sx, int64_t dy, int64_t dx, int64_t rows, int64_t cols);
/* Device pointer of a plane's local row 0 (zero-copy interop / virtual-strip tests).
 * RESTRICTION: on a single-GPU plan a plane of 8 MiB or more is one contiguous VIRTUAL range
 * mapped over many 2-MiB physical allocations (hipMemMap).  Kernels read and write it like any
 * pointer; hipMemcpy / hipMemcpy2D, IPC handles and RCCL transports may refuse a range that
 * spans several mappings (the library's own transfers bounce through a hipMalloc'ed plane for
 * that reason).  Consumers that need plain hipMalloc memory create their plans after
 * wt_set_option("scatter", 0) (or with WT_SCATTER=0 in the environment); strip plans
 * (nranks > 1) are always plain hipMalloc. */
int wt_plane_ptr(wt_plan *plan, int plane, void **dev_ptr);

/* ---- host <-> device ---------------------------------------------------------------- */
/* Page-locked host memory for results handed back to the caller.  A fresh pageable array costs
 * a first-touch page fault per 4 KiB during the download (8192^2: 17-31 ms instead of 4.7 ms at
 * 57 GB/s); the Python host side keeps a pool of these blocks behind the ndarrays it returns
 * (wavelets_amd/_lib.py host_empty) - the reference returns fresh numpy arrays at
 * watroo/utils.py:98,205,219 and watroo/wavelets.py:426. */
int wt_host_alloc(wt_ctx *ctx, size_t bytes, void **host_ptr);
int wt_host_free(void *host_ptr);
/* host image = this strip's rows, `host_stride` floats between rows (>= W). */
int wt_upload(wt_plan *plan, int plane, const float *host, int64_t host_stride);
/* plane <- (float) of an image of another element type, widened (byte-swapped) on the device: what the
 * reference does not recast to float64 (watroo/wavelets.py:297) - uint8 pictures, raw big-endian FITS
 * integers - is served in float32 here, without a host astype.  Type codes: WT_INT8 .. WT_FLOAT64,
 * | WT_BYTESWAPPED (defined with wt64_upload_int below). */
int wt_upload_int(wt_plan *plan, int plane, const void *host, int64_t host_pitch_bytes, int dtype);
int wt_download(wt_plan *plan, int plane, float *host, int64_t host_stride);
int wt_copy_plane(wt_plan *plan, int src, int dst);
int wt_fill_plane(wt_plan *plan, int plane, float value);
/* In-process stand-in for the RCCL halo exchange between two plans on the SAME device
 * ("virtual strips", tests/test_gpu_strips.py): `upper` owns the rows just above `lower`;
 * upper's last `rows` rows go to lower's top margin and lower's first `rows` rows to upper's
 * bottom margin - exactly the rows and margins the RCCL exchange moves. */
int wt_halo_exchange_local(wt_plan *upper, wt_plan *lower, int plane, int64_t rows);
/* RCCL halo exchange of `rows` margin rows of `plane` with the strip neighbours. */
int wt_halo_exchange(wt_plan *plan, int plane, int64_t rows);

/* ---- the hot path --------------------------------------------------------------------- */
/* AtrousTransform.atrous_standard, bilateral=None  (watroo/wavelets.py:408-444):
 * planes[0..level-1] <- detail, planes[level] <- smooth, from plane `src` (left intact).
 * flags: bit0 = allow fused multi-scale passes (default path), bit1 = skip halo exchange
 * (caller did it / virtual strips), bit2 (bilateral only) = materialise the variance plane
 * with a separate kernel instead of forming it inside the bilateral kernel, bit3 (bilateral with
 * user-defined taps only) = the plan's taps are stored reversed (see wt_plan_set_taps), bit4
 * (wt_decompose / wt_decompose_pass whose first pass is a fused pass from scale 0) = that pass
 * also histograms the first radix level of |w_0| as it produces the plane
 * (np.median(np.abs(data[0])), watroo/wavelets.py:127): a wt_abs_median(plan, 0, .) that follows
 * before anything else touches plane 0 reads the plane twice instead of three times.  Same
 * result; costs nothing measurable. */
int wt_decompose(wt_plan *plan, int src, int level, int flags);
/* one pass of the schedule (wt_schedule): scales [s0,s0+ns) from plane `cur` (c_{s0}) into
 * detail planes s0..s0+ns-1 and plane `nxt` (c_{s0+ns}); exchanges the pass halo first.
 * flags bit4: as for wt_decompose. */
int wt_decompose_pass(wt_plan *plan, int cur, int nxt, int s0, int ns, int flags);
/* wt_decompose followed by wt_plane_sum(0, level+1, dst) - the transform and its synthesis
 * np.sum(coefficients, axis=0) (watroo/wavelets.py:408-444 then watroo/utils.py:98,205) - in the
 * SAME passes: all level+1 planes are written as usual and the plane-order sum rides along
 * (each pass reads the running sum and writes it back), so the planes are not re-read:
 * 4*(L+2) + 8*passes - 4 B/pixel of traffic instead of 8*(L+2).  Bit-identical to the two-call
 * form.  Schedules with single-scale passes other than the one that ends 4 or 7 scales (9 scales
 * and more, user-defined taps, non-symmetric borders) run as the two calls. */
int wt_decompose_sum(wt_plan *plan, int src, int level, int dst, int flags);
/* Host-to-host form of wt_decompose_sum: host_in (H x W floats, row stride in_stride) -> planes
 * 0..level and the reconstruction in plane dst on the device AND in host_out.  Equivalent to
 * wt_upload(WT_PLANE_INPUT) + wt_decompose_sum + wt_download(dst), with identical bits, but the
 * three legs are PIPELINED over blocks of rows (block_rows, 0 = H/16): the passes run on a block as
 * soon as its rows and the pass's halo rows have arrived, finished rows of the reconstruction go
 * down while later blocks are still coming up (PCIe is full duplex): about one transfer leg
 * instead of two (8192^2: 10.2 -> ~6 ms).  Single-GPU plans with a fully fused schedule;
 * anything else (and wt_set_option("host_pipeline", 0)) runs the three legs in turn.  Host
 * buffers are used as they are (pageable or page-locked; the runtime locks pages per copy).
 * Reference flow: watroo/utils.py:83-102 (numpy in, numpy out). */
int wt_decompose_sum_host(wt_plan *plan, const float *host_in, int64_t in_stride, int level,
                          int dst, float *host_out, int64_t out_stride, int block_rows);
/* utils.denoise(data, weights, noise=<given>) host to host (watroo/utils.py:83-102): as
 * wt_decompose_sum_host with Coefficients.denoise placed between the passes - the first k_passes
 * passes of the fused schedule (wt_schedule) run plain, wt_denoise_sum over their n_den planes
 * (thresholds tau[k], weights wgt[k]; tau <= 0: weight only) starts the plane sum on the rows they
 * have finished, the remaining passes carry it, finished rows of dst go down while later blocks of
 * the image are still coming up.  The planes are left unthresholded (denoise() does not return
 * them).  Bit-identical to the serial sequence.  Requires 0 < k_passes < number of passes, n_den =
 * the scales of those passes, an all-fused schedule and an image worth pipelining (else an error:
 * run the serial sequence). */
int wt_denoise_sum_host(wt_plan *plan, const float *host_in, int64_t in_stride, int level,
                        int k_passes, int n_den, const double *tau, const double *wgt, int soft,
                        int dst, float *host_out, int64_t out_stride, int block_rows);
/* *ok = 1 when wt_decompose_sum(plan, ., level, ., bit0) runs as accumulate passes (else it is the
 * two-call form).  The host uses it to interleave Coefficients.denoise with the passes:
 * wt_decompose_pass for the passes that produce the thresholded planes, wt_abs_median,
 * wt_denoise_sum over those planes into the sum plane, wt_decompose_pass_sum (first = 0) for the
 * rest - the same bits as transform, denoise, sum (watroo/utils.py:95-98) with the planes read
 * once less. */
int wt_plan_fused_ok(wt_plan *plan, int level, int *ok);
/* one pass of that (fused passes only): `first` = the sum starts with this pass's first detail
 * plane, `last` = the smooth plane `nxt` is added and the sum is complete. */
int wt_decompose_pass_sum(wt_plan *plan, int cur, int nxt, int s0, int ns, int flags,
                          int sum_plane, int first, int last);
/* one scale of the above on explicit planes (per-scale operator; virtual-strip tests):
 * dst_c <- h_s (*) src ; dst_w <- src - dst_c (dst_w may be WT_PLANE_NONE). */
int wt_atrous_scale(wt_plan *plan, int src, int dst_c, int dst_w, int s, int flags);
/* convolution(arr, scaling_function, s)  (watroo/wavelets.py:35-45; cv2.filter2D with the
 * zero-stuffed kernel of :191-197, BORDER_REFLECT).  square_input: smooth src*src
 * (utils.py:177,194). */
int wt_smooth(wt_plan *plan, int src, int dst, int s, int square_input, int flags);
/* sdev_loc(image, sf, s, variance)  (watroo/wavelets.py:24-32), times f1 then f2
 * (the sigma_bilateral**2 and (s+1) factors of :434-436). */
int wt_local_variance(wt_plan *plan, int src, int dst, int s, float f1, float f2,
                      int take_sqrt, int flags);
/* atrous_convolution(image, kernel, bilateral_variance, s, 'symmetric')
 * (watroo/wavelets.py:74-105; numexpr expression :97).  flags: bit1, bit3 as for wt_decompose. */
int wt_bilateral_conv(wt_plan *plan, int src, int var, int dst, int s, int flags);
/* atrous_standard with bilateral (watroo/wavelets.py:421-442): sigma_b[level] */
int wt_decompose_bilateral(wt_plan *plan, int src, int level, const double *sigma_b,
                           int bilateral_scaling, int flags);
/* np.sum(coefficients, axis=0) (watroo/utils.py:98,205): dst <- sum planes[first..first+n) */
int wt_plane_sum(wt_plan *plan, int first, int count, int dst);
/* The same sum in two parts, for wow() behind a bilateral transform (watroo/utils.py:174-205: the planes of the
 * first scales are final long before the transform's last scales have run).  wt_plane_sum_early: dst <- planes
 * [0, count), queued on the side stream behind the per-scale updates already there (*done = 1), or nothing at all
 * when the plan is not in that overlapped state (*done = 0: sum in one piece with wt_plane_sum).
 * wt_plane_sum_resume: dst <- dst + planes [first, first + count).  Additions in plane order: the bits of
 * wt_plane_sum(plan, 0, first + count, dst).  dst: WT_PLANE_OUT or a scratch plane. */
int wt_plane_sum_early(wt_plan *plan, int count, int dst, int *done);
int wt_plane_sum_resume(wt_plan *plan, int first, int count, int dst);
/* np.median(np.abs(data[0])) (watroo/wavelets.py:127): exact radix select, fp32 result */
int wt_abs_median(wt_plan *plan, int plane, float *median);
/* Coefficients.significance (watroo/wavelets.py:129-143): dst <- erf(|c|/tau) (soft) or
 * |c| > tau (hard, 1.0/0.0).  tau = sigma*noise*sigma_e[scale]; with noise_plane !=
 * WT_PLANE_NONE tau is multiplied per pixel by that plane (ndarray noise map, :133). */
int wt_significance(wt_plan *plan, int plane, int dst, double tau, int soft, int noise_plane);
/* Coefficients.denoise body (watroo/wavelets.py:149): plane *= wgt * significance */
int wt_denoise(wt_plan *plan, int plane, double tau, double wgt, int soft, int noise_plane);
/* Coefficients.denoise (watroo/wavelets.py:145-149) of the first n_den planes fused with the
 * plane sum (watroo/utils.py:98): dst <- sum_k plane[first+k] * (wgt[k]*significance_k) for
 * k < n_den, plain planes after.  tau[k] <= 0: significance one.  write_back != 0 also stores
 * the thresholded planes (exactly denoise-then-sum); 0 leaves the planes untouched
 * (utils.denoise discards them).  Bit-identical to wt_denoise + wt_plane_sum. */
int wt_denoise_sum(wt_plan *plan, int first, int count, int dst, int n_den, const double *tau,
                   const double *wgt, int soft, int noise_plane, int write_back);
/* wow per-scale update (watroo/utils.py:193-203) fused:
 *   c <- c * significance(tau)            (skipped when tau <= 0)
 *   gamma_plane += c                      (skipped when gamma_plane == WT_PLANE_NONE)
 *   c <- c * (factor / sqrt(clip(P)))     P = power_plane (conv of c^2), clip <=0 -> 1e-15;
 *                                         power_plane == WT_PLANE_NONE: c <- c * factor */
int wt_wow_update(wt_plan *plan, int plane, int power_plane, double tau, int soft,
                  int noise_plane, float factor, int gamma_plane);
/* The whitening form of the above (power = conv_s(c^2), watroo/utils.py:193-196) in ONE kernel:
 * the local power is formed in registers, never written; the updated plane replaces plane
 * `plane` by a pointer swap with WT_PLANE_SCRATCH(3).  Bit-identical to
 * wt_smooth(square_input=1) + wt_wow_update. */
int wt_wow_scale(wt_plan *plan, int plane, int s, double tau, int soft, int noise_plane,
                 float factor, int gamma_plane, int flags);
/* global reductions for wow (watroo/utils.py:180-187,209-211): out = {sum, sumsq, min, max} */
int wt_reduce(wt_plan *plan, int plane, double out[4]);
/* plane <- standard normal deviates, Philox4x32-10 keyed by seed, counter (x>>2, y, trial, 0)
 * (the frame np.random.normal(size=...).astype(np.float32) draws in watroo/wavelets.py:225) */
int wt_fill_normal(wt_plan *plan, int plane, uint64_t seed, uint32_t trial);
/* gamma blend (watroo/utils.py:212-217):
 *   g <- clip((g-gmin)/(gmax-gmin),0,1)**(1/gamma); recon <- (1-h)*recon + h*g */
int wt_gamma_blend(wt_plan *plan, int recon, int gamma_plane, float gmin, float gmax,
                   float inv_gamma, float h);
/* ---- 3-D cubes (watroo/wavelets.py:46-64) ---------------------------- */
/* A (Z, Y, X) cube lives on a plan as a (Z*Y) x X image (depth = Z).  convolution() 3-D branch:
 * per-slice 2-D filter, then the same K-tap dilated filter along axis 0 (BORDER_REFLECT). */
int wt_smooth3d(wt_plan *plan, int src, int dst, int s, int depth);
/* atrous_standard on the cube: planes[0..level-1] <- detail, planes[level] <- smooth. */
int wt_decompose3d(wt_plan *plan, int src, int level, int depth);
/* The float32 cube engine: the planes of wt_decompose3d, bit for bit, with ONE launch per scale (x, y and z
 * filters and the detail subtraction fused; a scale whose z chains are too short runs on the sequence of
 * wt_decompose3d).  Same plane contract: planes[0..level], `src` intact, WT_PLANE_SCRATCH(0/1) as ping-pong.
 * Built-in scaling functions, one rank and the symmetric border only: anything else is refused before any
 * device work. */
int wt_decompose_cube(wt_plan *plan, int src, int level, int depth);
/* One scale of the whitening loop of wow on a (Z, Y, X) cube, depth = Z (watroo/utils.py:193-203 over the 3-D branch of
 * convolution(), watroo/wavelets.py:46-64): the local power conv_s(plane^2) of the 3-D filter and the update of
 * wt_wow_update in ONE launch - the squares are taken on load, the power never leaves the registers - where
 * wt_binary(mul) + wt_smooth3d + wt_wow_update take depth + 3.  The updated plane replaces `plane` (0 .. max_level) by
 * a pointer swap with WT_PLANE_SCRATCH(3), as in wt_wow_scale.  Bit-identical to that sequence, which still serves a
 * scale the rule of wt_decompose_cube or the grid limit refuses (through WT_PLANE_SCRATCH(6), (7) and (15)).
 * noise_plane / gamma_plane: as wt_wow_update; they must not alias the plane or those scratch planes.  Refusals as
 * wt_decompose_cube.  Additive entry: wt_abi_version() stays 8. */
int wt_wow_cube_scale(wt_plan *plan, int plane, int s, int depth, double tau, int soft, int noise_plane,
                      float factor, int gamma_plane);
/* bilateral transform of cubes, one scale at a time (watroo/wavelets.py:433-440 on 3-D input):
 * wt_local_variance3d = sdev_loc(cube, variance=True) * f1 * f2 (3-D smoothing of I and I^2,
 * scratch planes 13-15); wt_bilateral3d_conv = atrous_convolution with the K^3 kernel and that
 * variance (watroo/wavelets.py:74-105).  The detail plane is wt_binary(SUB). */
int wt_local_variance3d(wt_plan *plan, int src, int dst, int s, int depth, float f1, float f2);
int wt_bilateral3d_conv(wt_plan *plan, int src, int var, int dst, int s, int depth);

/* ---- Richardson-Lucy support (watroo/utils.py:222-290) -------------- */
/* cv2.filter2D(src, -1, kernel, dst, (-1,-1), 0, BORDER_REFLECT) with a small arbitrary kernel
 * (watroo/utils.py:257,286): correlation, anchor = kernel centre.  `kernel` is a host pointer
 * to kh*kw floats.  Up to 4096 taps run as one LDS-tiled launch; larger PSFs (the reference has
 * no size limit; up to 2^22 taps here) are applied in bands of rows / columns that accumulate
 * (O(kh*kw) per pixel: the direct form, not an FFT). */
int wt_filter2d(wt_plan *plan, int src, int dst, const float *kernel, int kh, int kw, int flags);
/* General form: explicit anchor (ay, ax) and border WT_BORDER_SYMMETRIC or WT_BORDER_PERIODIC.
 * The periodic border with anchor k/2 (correlation) or k-1-k/2 (flipped kernel = convolution)
 * is the circular product the reference forms with rfft2/irfft2 when fft=True
 * (watroo/utils.py:245-254, 284); whole-image plans only. */
#define WT_BORDER_SYMMETRIC 0
#define WT_BORDER_PERIODIC 3
int wt_filter2d_ex(wt_plan *plan, int src, int dst, const float *kernel, int kh, int kw, int ay,
                   int ax, int border, int flags);
/* elementwise dst = a OP b: 0 a-b, 1 a+b, 2 a*b, 3 a/b, 4 (a+b)/b  (watroo/utils.py:259,280-281,288) */
int wt_binary(wt_plan *plan, int op, int a, int b, int dst);
/* Generic tap-list operator: atrous_convolution(image, kernel, bilateral_variance, s, mode) for
 * ANY kernel and np.pad mode (watroo/wavelets.py:74-105) - what the tuned operators above do not
 * take (non-separable kernels, even / large tap counts, borders other than 'symmetric').
 *   var == WT_PLANE_NONE:  dst = [center_weight * I] + sum_t weights[t] * I_t      (tap order kept)
 *   else (range weights):  dst = ([cw * I] + sum_t e_t I_t) / ([cw] + sum_t e_t),
 *                          e_t = weights[t] * exp(-(I - I_t)^2 / var / 2)            (ref:97)
 * I_t = the sample at offsets[3t .. 3t+2] = (dz, dy, dx); the border rule pad_mode (WT_PAD_*:
 * np.pad's 'symmetric', 'reflect', 'edge', 'wrap', 'constant' with fill_value) applies per axis.
 * depth = 0: an image (1 x N: a signal), Z > 0: a (Z, Y, X) cube stored as a (Z*Y) x X image.
 * One sample per thread, taps read from a device list (<= 65536): a correctness path, not a
 * tuned one.  The Python layer builds the list in the reference's tap order. */
#define WT_PAD_SYMMETRIC 0
#define WT_PAD_REFLECT 1
#define WT_PAD_EDGE 2
#define WT_PAD_WRAP 3
#define WT_PAD_CONSTANT 4
int wt_taps_conv(wt_plan *plan, int src, int var, int dst, const int32_t *offsets,
                 const float *weights, int ntaps, float center_weight, int has_center,
                 int depth, int pad_mode, float fill_value);
/* The same with the two border rules of the RECURSIVE algorithm (watroo/wavelets.py:330-406: every
 * polyphase sub-array of stride `dilation` is filtered on its own with the base operator, i.e. an
 * out-of-range index is extended inside its own residue class modulo `dilation`): symmetric
 * (cv2.BORDER_REFLECT per sub-array, images and cubes) or scipy's 'mirror' (signals).  `dilation`
 * is ignored by the np.pad modes above. */
#define WT_PAD_POLY_SYMMETRIC 5
#define WT_PAD_POLY_MIRROR 6
int wt_taps_conv_ex(wt_plan *plan, int src, int var, int dst, const int32_t *offsets,
                    const float *weights, int ntaps, float center_weight, int has_center,
                    int depth, int pad_mode, float fill_value, int dilation);
/* One axis of the separable kernel of a scaling function (watroo/wavelets.py:170-187: kernel = outer product of
 * coefficients_1d; conv_s = convolution() with the zero-stuffed kernel, :35-69, :191-197): dst[i] = sum_j
 * weights[j] * src[pad(i + offsets[j])] along axis 2 (x), 1 (y, inside every slice) or 0 (z, across the depth
 * slices of a cube); pad_mode / fill_value / dilation as wt_taps_conv_ex.  Up to 33 taps run on tiled kernels
 * (LDS row segments along x, an LDS ring of rows down the polyphase chains along y / z); anything else on the
 * tap-list operator, with identical bits. */
int wt_axis_filter(wt_plan *plan, int src, int dst, int axis, const int32_t *offsets,
                   const float *weights, int ntaps, int depth, int pad_mode, float fill_value,
                   int dilation);
/* sdev_loc's last step (watroo/wavelets.py:27-32) from the two smoothed moments: dst = (meansq -
 * mean^2, values <= 0 -> 1e-20, optionally sqrt) * f1 * f2 - for callers that form conv(I) and
 * conv(I^2) themselves (scaling functions the tuned wt_local_variance does not take) */
int wt_variance_from_moments(wt_plan *plan, int mean, int meansq, int dst, float f1, float f2,
                             int take_sqrt);
/* Circular products of richardson_lucy(fft=True) (watroo/utils.py:245-254, 284) through a
 * hand-written FFT, for whole-image plans whose height and width are products of 2s, 3s and 5s
 * (2 .. 8192; powers of two: radix 2, other lengths: mixed radix 2 / 3 / 5):
 *   wt_fft_spectrum(plan, src)        kernel spectrum of the plan <- rfft2-equivalent of plane src
 *                                     (the PSF as the caller placed it periodically, :246-250)
 *   wt_fft_apply(plan, src, dst, conj) dst = irfft2(rfft2(src) * K)  (conj: * conj(K), :254 / :284)
 * wt_fft_supported: host logic, *ok = 1 when an H x W image qualifies.  Other sizes (and small PSFs,
 * where it is faster) keep the direct periodic form of wt_filter2d_ex. */
int wt_fft_supported(int64_t H, int64_t W, int *ok);
int wt_fft_spectrum(wt_plan *plan, int src);
int wt_fft_apply(wt_plan *plan, int src, int dst, int conj);
/* multiresolution-support update of a residual plane (watroo/utils.py:263-276):
 * sig = significance(plane, tau); hard: mrs = persistent ? max(mrs,sig) : sig, plane *= mrs;
 * soft: mrs = persistent ? mrs*sig : sig, plane *= mrs**inv_pow */
int wt_mrs_update(wt_plan *plan, int plane, int mrs_plane, double tau, int soft, int noise_plane,
                  int persistent, float inv_pow);
/* generalized_anscombe (watroo/wavelets.py:14-21) */
int wt_anscombe(wt_plan *plan, int src, int dst, float alpha, float g, float sigma,
                int inverse);

/* ---- float64 engine ------------------------------------------------------------------------
 * The reference computes float64 inputs in float64 and promotes int / big-endian inputs to
 * float64 (watroo/wavelets.py:297,319-320).  A wt_plan64 holds double planes (same plane ids as a
 * wt_plan: 0..max_level, WT_PLANE_INPUT, WT_PLANE_OUT, 32 scratch planes; wt64_decompose uses
 * scratch 0 and 1) and runs the decomposition (standard and, through border modes 1 / 3, recursive;
 * plain or bilateral), the Coefficients operators and wow's per-scale loop in double arithmetic
 * on generic kernels with the given 1-D taps (cv2.filter2D's correlation order).  Single GPU, whole images.  `depth`: 0 = an H x W image (a
 * 1 x N image is a signal: no column pass; its 'mirror' border is border mode 2), Z > 0 = a
 * (Z, Y, X) cube stored as a (Z*Y) x X image (watroo/wavelets.py:46-63). */
typedef struct wt_plan64 wt_plan64;
int wt64_plan_create(wt_ctx *ctx, int64_t H, int64_t W, int max_level, const double *taps,
                     int ntaps, wt_plan64 **plan);
int wt64_plan_destroy(wt_plan64 *plan);
int wt64_plan_set_border(wt_plan64 *plan, int border);
int wt64_upload(wt_plan64 *plan, int plane, const double *host, int64_t host_pitch);
/* plane <- (double) of an image of another element type, widened on the device: the reference recasts
 * integer and big-endian input to float64 on the host before anything else (watroo/wavelets.py:297,
 * 319-320: int16 .. int64, '>f4', '>f8' - what a FITS file holds).  host: nrows rows of W elements of type
 * `dtype`, host_pitch_bytes apart; dtype | WT_BYTESWAPPED: the elements are in the other byte order.
 * Integers are exact up to 2^53 and round to nearest even beyond (numpy's astype). */
#define WT_INT8 1
#define WT_UINT8 2
#define WT_INT16 3
#define WT_UINT16 4
#define WT_INT32 5
#define WT_UINT32 6
#define WT_INT64 7
#define WT_UINT64 8
#define WT_FLOAT32 9
#define WT_FLOAT64 10
#define WT_BYTESWAPPED 16
int wt64_upload_int(wt_plan64 *plan, int plane, const void *host, int64_t host_pitch_bytes, int dtype);
int wt64_download(wt_plan64 *plan, int plane, double *host, int64_t host_pitch);
/* AtrousTransform.atrous_standard (watroo/wavelets.py:408-444).  Images (depth 0) under the
 * symmetric border with the taps of a built-in family run the FUSED multi-scale passes of the
 * float32 engine instantiated for double (two pixels per lane; wavelets_amd/csrc/wt_fused.h),
 * any width and height (H >= 2; scales beyond the fused passes: one generic kernel each);
 * signals, cubes, user-defined taps and non-default borders run one generic kernel per scale.
 * wt_set_option("fused64", 0) forces the generic kernels (A/B; results agree to rounding: the
 * fused passes filter columns first, the generic kernels rows first). */
int wt64_decompose(wt_plan64 *plan, int src, int level, int depth);
/* the same with flags: bit4 (16) = where the first pass is a fused one it also histograms the first
 * radix level of |w_0| (as flag bit4 of wt_decompose): a wt64_abs_median(plan, 0) that follows -
 * Coefficients.get_noise, watroo/wavelets.py:126-127 - then reads the plane once less */
int wt64_decompose_ex(wt_plan64 *plan, int src, int level, int depth, int flags);
/* The float64 cube engine (watroo/wavelets.py:432,442 over the 3-D branch of convolution(), :46-64, on the float64 and
 * recast inputs of :297,319-320): the planes of wt64_decompose(plan, src, level, depth) on a (Z, Y, X) cube, depth = Z
 * >= 1, bit for bit, with ONE launch per scale (x, y and z filters and the detail subtraction fused, no private
 * temporary; a scale whose grid does not fit runs the sequence of wt64_decompose).  Same plane contract:
 * planes[0..level], `src` intact, WT_PLANE_SCRATCH(0/1) as ping-pong.  The taps of a built-in family and the symmetric
 * border only: anything else is refused before any device work.  Additive entry: wt_abi_version() stays 8. */
int wt64_decompose_cube(wt_plan64 *plan, int src, int level, int depth);
/* wt_wow_cube_scale on a float64 plan (watroo/utils.py:193-203 over watroo/wavelets.py:46-64, float64 and recast
 * cubes): one launch where wt64_binary(mul) + wt64_smooth(depth) + wt64_wow_update take five through cube-sized
 * temporaries; the updated plane replaces `plane` by a pointer swap with the plan's first private temporary, as in
 * wt64_wow_scale.  Bit-identical to that sequence, which serves a scale the rule of wt64_decompose_cube or the grid
 * limit refuses (through WT_PLANE_SCRATCH(6) and (7)).  Additive entry: wt_abi_version() stays 8. */
int wt64_wow_cube_scale(wt_plan64 *plan, int plane, int s, int depth, double tau, int soft, int noise_plane,
                        double factor, int gamma_plane);
/* Pass-level entry points of the fused float64 schedule (wt_schedule; as wt_decompose_pass /
 * wt_decompose_pass_sum / wt_plan_fused_ok): they let the caller place Coefficients.denoise between
 * the passes (watroo/utils.py:95-98: transform, denoise, sum) */
int wt64_plan_fused_ok(wt_plan64 *plan, int level, int *ok);
int wt64_decompose_pass(wt_plan64 *plan, int cur, int nxt, int s0, int ns, int flags);
int wt64_decompose_pass_sum(wt_plan64 *plan, int cur, int nxt, int s0, int ns, int sum_plane,
                            int first, int last);
/* wt_decompose_sum in float64: planes 0..level and np.sum(planes, axis=0) (plane order) -> dst,
 * the sum carried through the fused passes where they apply (*fused = 1), else transform +
 * wt64_plane_sum (*fused = 0; fused may be NULL). */
int wt64_decompose_sum(wt_plan64 *plan, int src, int level, int dst, int *fused);
/* convolution(arr, scaling_function, s) (watroo/wavelets.py:35-69); square_input: of src*src */
int wt64_smooth(wt_plan64 *plan, int src, int dst, int s, int square_input, int depth);
/* sdev_loc (watroo/wavelets.py:24-32) times f1 then f2 */
int wt64_local_variance(wt_plan64 *plan, int src, int dst, int s, double f1, double f2,
                        int take_sqrt, int depth);
/* atrous_convolution(image, kernel, bilateral_variance, s) (watroo/wavelets.py:74-105);
 * taps_reversed as flag bit3 of wt_bilateral_conv */
int wt64_bilateral_conv(wt_plan64 *plan, int src, int var, int dst, int s, int depth,
                        int taps_reversed);
/* AtrousTransform(bilateral=...)(image, level) in float64 (watroo/wavelets.py:408-444, bilateral branch
 * :433-440): as wt_decompose_bilateral - planes 0..level from plane src (not 0..level, not scratch 0 / 1),
 * variance = sdev_loc(c_s) * sigma_b[s]**2 (* (s + 1) under bilateral_scaling).  Built-in taps: one marching
 * kernel per scale (variance formed in its register window, both output planes written). */
int wt64_decompose_bilateral(wt_plan64 *plan, int src, int level, const double *sigma_b,
                             int bilateral_scaling);
/* wt_axis_filter in float64 */
int wt64_axis_filter(wt_plan64 *plan, int src, int dst, int axis, const int32_t *offsets,
                     const double *weights, int ntaps, int depth, int pad_mode, double fill_value,
                     int dilation);
/* wt_taps_conv / wt_taps_conv_ex / wt_variance_from_moments in float64 */
int wt64_taps_conv(wt_plan64 *plan, int src, int var, int dst, const int32_t *offsets,
                   const double *weights, int ntaps, double center_weight, int has_center,
                   int depth, int pad_mode, double fill_value);
int wt64_taps_conv_ex(wt_plan64 *plan, int src, int var, int dst, const int32_t *offsets,
                      const double *weights, int ntaps, double center_weight, int has_center,
                      int depth, int pad_mode, double fill_value, int dilation);
int wt64_variance_from_moments(wt_plan64 *plan, int mean, int meansq, int dst, double f1, double f2,
                               int take_sqrt);
/* device copy of a window between planes of two plans (crop of atrous_recursive, :405-406) */
int wt64_copy_window(wt_plan64 *src, int src_plane, wt_plan64 *dst, int dst_plane, int64_t sy,
                     int64_t sx, int64_t dy, int64_t dx, int64_t rows, int64_t cols);
/* np.median(np.abs(plane)) (watroo/wavelets.py:127): exact select on the 63-bit keys - two radix
 * levels (the first may ride on the transform, wt64_decompose_ex), then the keys of the selected bin
 * are gathered and one workgroup finishes on that list; radix passes to the end where the bin does
 * not fit the list (ties) */
int wt64_abs_median(wt_plan64 *plan, int plane, double *median);
/* mode 0: dst = Coefficients.significance (watroo/wavelets.py:129-143); mode 1: dst = src * (wgt *
 * significance) (Coefficients.denoise with dst = src, :145-149).  tau <= 0: significance one;
 * noise_plane: per-pixel noise map multiplying tau, or WT_PLANE_NONE */
int wt64_significance(wt_plan64 *plan, int src, int dst, double tau, double wgt, int soft,
                      int noise_plane, int mode);
/* np.sum(planes[first..first+count), axis=0) in plane order (watroo/utils.py:98) */
int wt64_plane_sum(wt_plan64 *plan, int first, int count, int dst);
/* wt_plane_sum_early / wt_plane_sum_resume on a float64 plan (watroo/utils.py:174-205 with float64 data) */
int wt64_plane_sum_early(wt_plan64 *plan, int count, int dst, int *done);
int wt64_plane_sum_resume(wt_plan64 *plan, int first, int count, int dst);
/* wt_denoise_sum in float64: Coefficients.denoise over the first n_den planes (tau[k] <= 0: weight
 * only) fused with the plane sum of planes [first, first + count) -> dst (watroo/wavelets.py:145-149,
 * utils.py:98); write_back stores the thresholded planes */
int wt64_denoise_sum(wt_plan64 *plan, int first, int count, int dst, int n_den, const double *tau,
                     const double *wgt, int soft, int noise_plane, int write_back);
/* dst = a OP b: 0 add, 1 sub, 2 mul, 3 div, 4 (a+b)/b */
int wt64_binary(wt_plan64 *plan, int op, int a, int b, int dst);
/* the operators of utils.wow without bilateral filtering (watroo/utils.py:157-217) in float64:
 * per-scale update (as wt_wow_update), gamma blend, fill, {sum, sumsq, min, max} */
int wt64_wow_update(wt_plan64 *plan, int plane, int power_plane, double tau, int soft,
                    int noise_plane, double factor, int gamma_plane);
/* one scale of the wow loop on a float64 image (watroo/utils.py:193-203): local power conv_s(c^2) and the
 * update in a row pass + a column pass with the update as its epilogue, in place (no power plane);
 * identical bits to wt64_smooth(square) + wt64_wow_update. */
int wt64_wow_scale(wt_plan64 *plan, int plane, int s, double tau, int soft, int noise_plane, double factor,
                   int gamma_plane);
int wt64_gamma_blend(wt_plan64 *plan, int recon, int gamma_plane, double gmin, double gmax,
                     double inv_gamma, double h);
int wt64_fill_plane(wt_plan64 *plan, int plane, double value);
int wt64_reduce(wt_plan64 *plan, int plane, double out[4]);
/* Richardson-Lucy support in float64 (watroo/utils.py:222-290), as wt_filter2d_ex / wt_mrs_update;
 * `kernel` is a host pointer to kh*kw doubles */
int wt64_filter2d(wt_plan64 *plan, int src, int dst, const double *kernel, int kh, int kw, int ay,
                  int ax, int border);
int wt64_mrs_update(wt_plan64 *plan, int plane, int mrs_plane, double tau, int soft,
                    int noise_plane, int persistent, double inv_pow);
/* wt_fft_spectrum / wt_fft_apply in float64 */
int wt64_fft_spectrum(wt_plan64 *plan, int src);
int wt64_fft_apply(wt_plan64 *plan, int src, int dst, int conj);
/* generalized_anscombe (watroo/wavelets.py:14-21) */
int wt64_anscombe(wt_plan64 *plan, int src, int dst, double alpha, double g, double sigma,
                  int inverse);

/* ---- batches of same-shape frames (float32) ------------------------------------------------
 * A wt_batch holds the planes of N frames of one H x W shape back to back (frame f at f * frame_stride
 * floats, rows of the pitch a wt_plan of that width has): every fused pass of the schedule runs over the
 * active frames in ONE launch (the frame is a grid dimension), pointwise steps run once over the stack.
 * A frame's result is bit-identical to the per-frame call on a wt_plan.  Passes that carry a sum run only
 * on all-fused schedules (wt_plan_fused_ok); built-in families only.  Every operation takes the number of
 * ACTIVE frames nf (frames 0 .. nf-1; the last chunk of a stack may be shorter than the batch).
 * Planes: 0..max_level, WT_PLANE_INPUT, WT_PLANE_OUT, WT_PLANE_SCRATCH(0/1) (scratch used internally) and the
 * planes of wow and of richardson_lucy (WT_PLANE_SCRATCH(3/4), (6 .. 10), (16 ..), below).  wt_batch_decompose runs a single-scale pass that has no fused
 * kernel on the batched per-scale stencil (levels >= 9); the other passes are fused. */
typedef struct wt_batch wt_batch;
int wt_batch_create(wt_ctx *ctx, int n, int H, int W, int family, int max_level, wt_batch **batch);
int wt_batch_destroy(wt_batch *batch);
/* info[7] = {n, H, W, pitch, frame_stride, max_level, family} */
int wt_batch_info(wt_batch *batch, int64_t *info);
/* frames [f0, f0+nf) of a plane <- / -> host frames of H x W contiguous floats, host_frame_stride floats apart
 * (0 = H * W: a C-contiguous (nf, H, W) block, np.stack of the frames) */
int wt_batch_upload(wt_batch *batch, int plane, int f0, int nf, const float *host, int64_t host_frame_stride);
int wt_batch_download(wt_batch *batch, int plane, int f0, int nf, float *host, int64_t host_frame_stride);
/* device pointer of frame 0 of a plane (allocated on first use) and the frame stride in floats */
int wt_batch_plane_ptr(wt_batch *batch, int plane, void **ptr, int64_t *frame_stride);
/* wt_decompose per frame (watroo/wavelets.py:408-444 via AtrousTransform.__call__, ref:307-328); flags bit0 */
int wt_batch_decompose(wt_batch *batch, int nf, int src, int level, int flags);
/* wt_decompose_bilateral per frame (watroo/wavelets.py:433-442: the range-weighted branch of atrous, variance of
 * :434-436 formed in the march): scale s reads the current smooth plane, writes c_{s+1} to a scratch plane (planes
 * WT_PLANE_SCRATCH(0/1) ping-pong; plane `level` on the last scale) and w_s to plane s.  One launch per scale for all
 * active frames.  sigma_b: `level` entries.  flags: reserved (the two-kernel form and the side-stream overlap of
 * wt_decompose_bilateral are not carried over). */
int wt_batch_decompose_bilateral(wt_batch *batch, int nf, int src, int level, const double *sigma_b,
                                 int bilateral_scaling, int flags);
/* wt_decompose_sum per frame: planes + np.sum(planes, axis=0) (watroo/utils.py:98) in the same passes */
int wt_batch_decompose_sum(wt_batch *batch, int nf, int src, int level, int dst, int flags);
/* wt_decompose_pass / wt_decompose_pass_sum per frame (utils.denoise, watroo/utils.py:95-98, interleaved) */
int wt_batch_decompose_pass(wt_batch *batch, int nf, int cur, int nxt, int s0, int ns, int flags);
int wt_batch_decompose_pass_sum(wt_batch *batch, int nf, int cur, int nxt, int s0, int ns, int flags,
                                int sum_plane, int first, int last);
/* np.median(np.abs(data[0])) of every active frame (watroo/wavelets.py:127): medians[nf], exact, one
 * host round trip; a frame that holds NaN is an error naming the frame */
int wt_batch_abs_median(wt_batch *batch, int nf, int plane, float *medians);
/* wt_denoise_sum per frame (Coefficients.denoise + np.sum, watroo/wavelets.py:145-149, utils.py:97-98):
 * planes 0..count-1, the first n_den thresholded at tau[frame * n_den + k] (<= 0: significance one),
 * weights wgt[k] shared by the frames; scalar noise only */
int wt_batch_denoise_sum(wt_batch *batch, int nf, int count, int dst, int n_den, const double *tau,
                         const double *wgt, int soft, int write_back);
/* wt_batch_denoise_sum with one weight row per frame too (utils.enhance per channel, watroo/utils.py:60-78: the
 * channels of a colour image are frames with their own sigmas AND weights): tau and wgt hold nf * n_den entries, the
 * row of frame f at f * n_den; 1 <= n_den <= count; scalar noise only */
int wt_batch_enhance_sum(wt_batch *batch, int nf, int count, int dst, int n_den, const double *tau,
                         const double *wgt, int soft, int write_back);
/* wt_batch_denoise_sum with a per-pixel noise map per frame (Coefficients.significance on an ndarray noise,
 * watroo/wavelets.py:133-141; wt_denoise_sum with its noise_plane): the threshold of pixel i is
 * tau[frame * n_den + k] * noise_plane[i].  noise_plane is a plane of the batch (WT_PLANE_SCRATCH(5)) holding one map
 * per active frame, finite in the pitch padding too; a frame with a scalar noise level holds ones */
int wt_batch_denoise_sum_map(wt_batch *batch, int nf, int count, int dst, int n_den, const double *tau,
                             const double *wgt, int soft, int write_back, int noise_plane);
/* frame 0 of the plane -> frames 1 .. nf-1 on the device (one noise map shared by the frames of a stack, the
 * `noise` of watroo/utils.py:96 given once: it crosses PCIe once per chunk) */
int wt_batch_replicate(wt_batch *batch, int nf, int plane);
/* generalized_anscombe over the active frames (watroo/utils.py:93-94, 99-100; as wt_anscombe) */
int wt_batch_anscombe(wt_batch *batch, int nf, int src, int dst, float alpha, float g, float sigma,
                      int inverse);
/* ---- wow over a batch (watroo/utils.py:105-219, utils.wow per frame).  Extra planes: WT_PLANE_SCRATCH(3), the
 * output plane of wt_batch_wow_scale, and WT_PLANE_SCRATCH(4), wow's gamma accumulator.  Per-frame parameters are
 * arrays of nf entries; every frame gets the bits of the per-frame call on a wt_plan.  WT_PLANE_SCRATCH(5): the
 * per-pixel noise maps of the *_map entries. */
/* plane <- value over the active frames (gamma_scaled = zeros, watroo/utils.py:157-158; as wt_fill_plane) */
int wt_batch_fill(wt_batch *batch, int nf, int plane, float value);
/* frame f of the plane <- wt_fill_normal(seed, first_trial + f) of a wt_plan of the frame's shape, frames 0 .. nf-1
 * (the frames of compute_noise_weights' trials, watroo/wavelets.py:223-225) */
int wt_batch_fill_normal(wt_batch *batch, int nf, int plane, uint64_t seed, uint32_t first_trial);
/* wt_wow_update per frame without a power plane or noise map (watroo/utils.py:185-191 with local_power = 1, 199-203):
 * wow's last plane, whitening=False and h >= 1; tau[f] <= 0: significance one; gamma_plane may be WT_PLANE_NONE */
int wt_batch_wow_update(wt_batch *batch, int nf, int plane, const double *tau, int soft, const float *factor,
                        int gamma_plane);
/* wt_wow_scale per frame, scalar noise (watroo/utils.py:192-203): local power conv_s(c^2), significance, gamma sum
 * and whitening of plane `plane` at scale s in one batched stencil launch; the result goes to WT_PLANE_SCRATCH(3)
 * and the two planes' buffers are swapped */
int wt_batch_wow_scale(wt_batch *batch, int nf, int plane, int s, const double *tau, int soft, const float *factor,
                       int gamma_plane);
/* wt_batch_wow_update with a per-pixel noise map per frame (watroo/utils.py:199 on an ndarray noise,
 * wavelets.py:133-141; wt_wow_update with its noise_plane): noise_plane as in wt_batch_denoise_sum_map */
int wt_batch_wow_update_map(wt_batch *batch, int nf, int plane, const double *tau, int soft, const float *factor,
                            int gamma_plane, int noise_plane);
/* wt_batch_wow_scale with a per-pixel noise map per frame (watroo/utils.py:192-203 on an ndarray noise,
 * wavelets.py:133-141; wt_wow_scale with its noise_plane: the stencil's instantiation with the map and, when
 * gamma_plane is given, the gamma accumulator): noise_plane as in wt_batch_denoise_sum_map */
int wt_batch_wow_scale_map(wt_batch *batch, int nf, int plane, int s, const double *tau, int soft,
                           const float *factor, int gamma_plane, int noise_plane);
/* wt_reduce per frame ({sum, sumsq, min, max}, fp64, the per-frame call's doubles; np.std / np.mean(c**2) of
 * watroo/utils.py:178-189, gamma_scaled.min / max of utils.py:208-211): out[4 * nf], one host round trip */
int wt_batch_reduce(wt_batch *batch, int nf, int plane, double *out);
/* wt_gamma_blend per frame (watroo/utils.py:212-217) with the frame's gmin[f] / gmax[f] */
int wt_batch_gamma_blend(wt_batch *batch, int nf, int recon, int gamma_plane, const float *gmin, const float *gmax,
                         float inv_gamma, float h);
/* wt_plane_sum per frame: dst = planes [first, first + count) summed in plane order (np.sum(coefficients, axis=0),
 * watroo/utils.py:205) */
int wt_batch_plane_sum(wt_batch *batch, int nf, int first, int count, int dst);
/* ---- richardson_lucy over a batch (watroo/utils.py:222-290, utils.richardson_lucy per frame).  Extra planes, the
 * per-frame call's ids, allocated on first use: WT_PLANE_SCRATCH(6 .. 10) - data, psi, phi, residual, correlation - and
 * WT_PLANE_SCRATCH(16 + s), s < max_level, the support plane of scale s.  Every frame gets the bits of the per-frame
 * call on a wt_plan. */
/* One PSF operand of the call -> device memory of the batch: slot 0 the forward operand (the flipped PSF of
 * watroo/utils.py:257), slot 1 the backward one (utils.py:286).  `kernel`: kh * kw host floats, copied before the
 * call returns.  PSFs wt_filter2d_ex applies in one launch without bands only: kh * kw <= 4096, kw <= 512 and
 * (64 + kw - 1) * (16 + kh - 1) * 4 <= 96 KB. */
int wt_batch_set_psf(wt_batch *batch, int slot, const float *kernel, int kh, int kw);
/* host logic: *ok = 1 when wt_batch_set_psf takes a kh x kw PSF (the rule above; no GPU needed) */
int wt_batch_psf_ok(int kh, int kw, int *ok);
/* wt_filter2d_ex per frame with the PSF of `slot` (cv2.filter2D of watroo/utils.py:257,286 with WT_BORDER_SYMMETRIC;
 * the circular products of utils.py:245-254,284 with WT_BORDER_PERIODIC), anchor (ay, ax) inside the kernel, src != dst:
 * one launch for all active frames, no stream drain, no PSF copy */
int wt_batch_filter2d(wt_batch *batch, int nf, int src, int dst, int slot, int ay, int ax, int border);
/* wt_binary over the active frames: dst = a OP b (watroo/utils.py:259,280-281,288) */
int wt_batch_binary(wt_batch *batch, int nf, int op, int a, int b, int dst);
/* wt_mrs_update per frame (watroo/utils.py:263-276) with the frame's tau[f] (<= 0: significance one); scalar noise
 * only - the noise of richardson_lucy is the data's MAD estimate (utils.py:262) */
int wt_batch_mrs_update(wt_batch *batch, int nf, int plane, int mrs_plane, const double *tau, int soft,
                        int persistent, float inv_pow);
/* The circular products of richardson_lucy(fft=True) for PSFs the per-frame call hands to wt_fft_apply
 * (watroo/utils.py:245-254, 284), over a batch: the FFT kernels of wt_fft_spectrum / wt_fft_apply with the frame as a
 * grid dimension and ONE kernel spectrum for all frames.  Work buffers (two complex arrays of n * H * W, one H * W
 * spectrum, two twiddle tables) are allocated by the first wt_batch_fft_spectrum and freed with the batch. */
/* host logic: *ok = 1 when batches of H x W frames take these products (wt_fft_supported's rule; no GPU needed) */
int wt_batch_fft_ok(int64_t H, int64_t W, int *ok);
/* the kernel spectrum of the batch <- the forward transform of FRAME 0 of plane src, where the caller uploaded the PSF
 * placed periodically (fft_psf of watroo/utils.py:246-251); once per call of the stack function, every chunk reuses it */
int wt_batch_fft_spectrum(wt_batch *batch, int src);
/* wt_fft_apply per frame: dst = irfft2(rfft2(src) * K) (watroo/utils.py:254) or, conj, * conj(K) (utils.py:284) for
 * frames 0 .. nf-1, src != dst, after wt_batch_fft_spectrum: six launches whatever nf is, no stream drain, no host
 * round trip */
int wt_batch_fft_apply(wt_batch *batch, int nf, int src, int dst, int conj);

/* ---- batches of same-shape frames (float64) ------------------------------------------------
 * A wt_batch64 is the wt_batch of the float64 engine: the stacks the reference computes in float64 (float64
 * frames, and the int16 .. int64 / big-endian frames it recasts, watroo/wavelets.py:297, 319-320).  Planes hold the
 * N frames back to back at the pitch of a wt_plan64 of that width (frame f at f * frame_stride doubles).  Every
 * frame runs the per-frame float64 schedule, kernel choice and geometry with the frame as grid z, so a frame's
 * result is bit-identical to the per-frame call on a wt_plan64.  Images (H >= 2) with a built-in family only;
 * the transforms with a plane sum need an all-fused float64 schedule (wt_batch64_fused_ok), the plain transform
 * also takes the schedules of wt_batch64_wow_ok.  Planes: 0..max_level, WT_PLANE_INPUT, WT_PLANE_OUT,
 * WT_PLANE_SCRATCH(0/1) (used internally), WT_PLANE_SCRATCH(3/4/5) (wow, noise maps).  Operations take the number of ACTIVE
 * frames nf (frames 0 .. nf-1). */
typedef struct wt_batch64 wt_batch64;
/* host logic: *ok = 1 when H x W frames of `family` have an all-fused float64 schedule of `level` scales
 * (wt64_plan_fused_ok of a wt_plan64 of that shape) */
int wt_batch64_fused_ok(int family, int64_t H, int64_t W, int level, int *ok);
int wt_batch64_create(wt_ctx *ctx, int n, int H, int W, int family, int max_level, wt_batch64 **batch);
int wt_batch64_destroy(wt_batch64 *batch);
/* info[7] = {n, H, W, pitch, frame_stride, max_level, family} */
int wt_batch64_info(wt_batch64 *batch, int64_t *info);
/* frames [f0, f0+nf) of a plane <- / -> host frames of H x W contiguous doubles, host_frame_stride doubles apart
 * (0 = H * W: a C-contiguous (nf, H, W) block) - as wt64_upload / wt64_download */
int wt_batch64_upload(wt_batch64 *batch, int plane, int f0, int nf, const double *host, int64_t host_frame_stride);
int wt_batch64_download(wt_batch64 *batch, int plane, int f0, int nf, double *host, int64_t host_frame_stride);
/* wt64_upload_int for frames [f0, f0+nf): a C-contiguous (nf, H, W) block of element type `dtype` (WT_INT8 ..
 * WT_FLOAT64, | WT_BYTESWAPPED) crosses PCIe as it is and is widened on the device (the reference's recast to
 * float64, watroo/wavelets.py:297, 319-320) */
int wt_batch64_upload_elems(wt_batch64 *batch, int plane, int f0, int nf, const void *host, int dtype);
/* device pointer of frame 0 of a plane (allocated on first use) and the frame stride in doubles */
int wt_batch64_plane_ptr(wt_batch64 *batch, int plane, void **ptr, int64_t *frame_stride);
/* wt64_decompose per frame (watroo/wavelets.py:408-444 via AtrousTransform.__call__, ref:307-328); flags bit0 */
int wt_batch64_decompose(wt_batch64 *batch, int nf, int src, int level, int flags);
/* host logic: *ok = 1 when an H x W frame of `family` takes the float64 bilateral march per frame
 * (wt64_decompose_bilateral, watroo/wavelets.py:433-442, with built-in taps: option "stencil64" on, an image of
 * H >= 2 rows that wt_batch64_create accepts) and 1 <= level <= 25 - the frames wt_batch64_decompose_bilateral
 * reproduces bit for bit; with the option off the per-frame call runs three generic kernels per scale */
int wt_batch64_bilateral_ok(int family, int64_t H, int64_t W, int level, int *ok);
/* wt64_decompose_bilateral per frame (watroo/wavelets.py:433-442: the range-weighted branch of atrous on float64 /
 * recast input, :297, 319-320; variance of :434-436 formed in the march): scale s reads the current smooth plane,
 * writes c_{s+1} to a scratch plane (planes WT_PLANE_SCRATCH(0/1) ping-pong; plane `level` on the last scale) and
 * w_s to plane s.  One launch per scale for all active frames.  sigma_b: `level` entries.  flags: reserved */
int wt_batch64_decompose_bilateral(wt_batch64 *batch, int nf, int src, int level, const double *sigma_b,
                                   int bilateral_scaling, int flags);
/* wt64_decompose_sum per frame: planes + np.sum(planes, axis=0) (watroo/utils.py:98) in the same passes */
int wt_batch64_decompose_sum(wt_batch64 *batch, int nf, int src, int level, int dst, int flags);
/* wt64_decompose_pass / wt64_decompose_pass_sum per frame (utils.denoise, watroo/utils.py:95-98, interleaved) */
int wt_batch64_decompose_pass(wt_batch64 *batch, int nf, int cur, int nxt, int s0, int ns, int flags);
int wt_batch64_decompose_pass_sum(wt_batch64 *batch, int nf, int cur, int nxt, int s0, int ns, int flags,
                                  int sum_plane, int first, int last);
/* np.median(np.abs(data[0])) of every active frame (watroo/wavelets.py:127): medians[nf], exact (the values
 * wt64_abs_median gives), one host round trip */
int wt_batch64_abs_median(wt_batch64 *batch, int nf, int plane, double *medians);
/* wt64_denoise_sum per frame (Coefficients.denoise + np.sum, watroo/wavelets.py:145-149, utils.py:97-98): planes
 * 0..count-1, the first n_den thresholded at tau[frame * n_den + k] (<= 0: significance one), weights wgt[k]
 * shared by the frames; scalar noise only */
int wt_batch64_denoise_sum(wt_batch64 *batch, int nf, int count, int dst, int n_den, const double *tau,
                           const double *wgt, int soft, int write_back);
/* wt_batch64_denoise_sum with one weight row per frame too (utils.enhance per channel, watroo/utils.py:60-78): tau
 * and wgt hold nf * n_den entries, the row of frame f at f * n_den; 1 <= n_den <= count; scalar noise only */
int wt_batch64_enhance_sum(wt_batch64 *batch, int nf, int count, int dst, int n_den, const double *tau,
                           const double *wgt, int soft, int write_back);
/* wt_batch64_denoise_sum with a per-pixel noise map per frame (Coefficients.significance on an ndarray noise,
 * watroo/wavelets.py:133-141; wt64_denoise_sum with its noise_plane): noise_plane is a plane of the batch
 * (WT_PLANE_SCRATCH(5)) of float64 maps, finite in the pitch padding too.  has_map[nf] (NULL: every frame): a frame
 * with has_map[f] == 0 has a scalar noise level and is thresholded as wt_batch64_denoise_sum thresholds it (the
 * reciprocal form of the map-free kernel), whatever its slot of the plane holds */
int wt_batch64_denoise_sum_map(wt_batch64 *batch, int nf, int count, int dst, int n_den, const double *tau,
                               const double *wgt, int soft, int write_back, int noise_plane, const int *has_map);
/* plane <- value over the active frames, pitch padding included (as wt_batch_fill): ones in the noise plane before
 * the maps go up, so that a frame with a scalar level of watroo/wavelets.py:133-135 and every padding lane read 1 */
int wt_batch64_fill(wt_batch64 *batch, int nf, int plane, double value);
/* frame 0 of the plane -> frames 1 .. nf-1 on the device (as wt_batch_replicate; watroo/utils.py:96) */
int wt_batch64_replicate(wt_batch64 *batch, int nf, int plane);
/* generalized_anscombe over the active frames (watroo/utils.py:93-94, 99-100; as wt64_anscombe) */
int wt_batch64_anscombe(wt_batch64 *batch, int nf, int src, int dst, double alpha, double g, double sigma,
                        int inverse);
/* ---- wow over a float64 batch (watroo/utils.py:105-219, utils.wow per frame on a wt_plan64): the float64 twins of
 * the wt_batch_wow_* entries, `double` where those have `float`.  Extra planes: WT_PLANE_SCRATCH(3), the output plane
 * of wt_batch64_wow_scale, WT_PLANE_SCRATCH(4), wow's gamma accumulator, WT_PLANE_SCRATCH(5), the per-pixel noise
 * maps of the *_map entries.  Per-frame parameters are arrays of nf entries; every frame gets the bits of the
 * per-frame call.  wt_batch64_decompose serves wow's transform: levels 1..24 where wt_batch64_wow_ok, the single-scale
 * passes without a fused kernel on the batched per-scale stencil (watroo/wavelets.py:408-444). */
/* host logic: *ok = 1 when wow over H x W frames of `family` with `level` scales (1..24) runs on the batch: an image
 * (H >= 2) with rows wt_batch64_create accepts, a float64 schedule (watroo/wavelets.py:408-444) of fused passes and
 * single-scale passes, and option "stencil64" on - with it off wt64_decompose and wt64_wow_scale take the generic
 * kernels per frame, whose bits differ.  wt_batch64_fused_ok keeps its narrower meaning */
int wt_batch64_wow_ok(int family, int64_t H, int64_t W, int level, int *ok);
/* wt64_wow_update per frame without a power plane or noise map (watroo/utils.py:185-191 with local_power = 1,
 * 199-203): wow's last plane, whitening=False and h >= 1; tau[f] <= 0: significance one; gamma_plane may be
 * WT_PLANE_NONE */
int wt_batch64_wow_update(wt_batch64 *batch, int nf, int plane, const double *tau, int soft, const double *factor,
                          int gamma_plane);
/* wt64_wow_scale per frame, scalar noise (watroo/utils.py:192-203): local power conv_s(c^2), significance, gamma sum
 * and whitening of plane `plane` at scale s in one batched stencil launch; the result goes to WT_PLANE_SCRATCH(3)
 * and the two planes' buffers are swapped */
int wt_batch64_wow_scale(wt_batch64 *batch, int nf, int plane, int s, const double *tau, int soft,
                         const double *factor, int gamma_plane);
/* wt_batch64_wow_update with a per-pixel noise map per frame (watroo/utils.py:199 on an ndarray noise,
 * wavelets.py:133-141; wt64_wow_update with its noise_plane): noise_plane as in wt_batch64_denoise_sum_map, ones in
 * the slot of a frame with a scalar level */
int wt_batch64_wow_update_map(wt_batch64 *batch, int nf, int plane, const double *tau, int soft,
                              const double *factor, int gamma_plane, int noise_plane);
/* wt_batch64_wow_scale with a per-pixel noise map per frame (watroo/utils.py:192-203 on an ndarray noise,
 * wavelets.py:133-141; wt64_wow_scale with its noise_plane) */
int wt_batch64_wow_scale_map(wt_batch64 *batch, int nf, int plane, int s, const double *tau, int soft,
                             const double *factor, int gamma_plane, int noise_plane);
/* wt64_reduce per frame ({sum, sumsq, min, max}, the per-frame call's doubles; np.std / np.mean(c**2) of
 * watroo/utils.py:178-189, gamma_scaled.min / max of utils.py:208-211): out[4 * nf], one host round trip */
int wt_batch64_reduce(wt_batch64 *batch, int nf, int plane, double *out);
/* wt64_gamma_blend per frame (watroo/utils.py:212-217) with the frame's gmin[f] / gmax[f] */
int wt_batch64_gamma_blend(wt_batch64 *batch, int nf, int recon, int gamma_plane, const double *gmin,
                           const double *gmax, double inv_gamma, double h);
/* wt64_plane_sum per frame: dst = planes [first, first + count) summed in plane order (np.sum(coefficients, axis=0),
 * watroo/utils.py:205); count <= 32 */
int wt_batch64_plane_sum(wt_batch64 *batch, int nf, int first, int count, int dst);
/* ---- richardson_lucy over a float64 batch (watroo/utils.py:222-290, utils.richardson_lucy per frame on a wt_plan64):
 * the float64 twins of the wt_batch_set_psf / _filter2d / _binary / _mrs_update entries.  Extra planes, the per-frame
 * call's ids, allocated on first use: WT_PLANE_SCRATCH(6 .. 10) - data, psi, phi, residual, correlation - and
 * WT_PLANE_SCRATCH(16 + s), s < max_level, the support plane of scale s; they are planes of a batch from its first
 * wt_batch64_set_psf on.  Every frame gets the bits of the per-frame call. */
/* host logic: *ok = 1 when wt_batch64_set_psf takes a kh x kw PSF (cv2.filter2D of watroo/utils.py:257,286 in one launch
 * of the tiled kernel): kh * kw <= 4096, kw <= 512 and (64 + kw - 1) * (16 + kh - 1) * 8 <= 96 KB; no GPU needed */
int wt_batch64_psf_ok(int kh, int kw, int *ok);
/* One PSF operand of the call -> device memory of the batch: slot 0 the forward operand (the flipped PSF of
 * watroo/utils.py:257), slot 1 the backward one (utils.py:286).  `kernel`: kh * kw host doubles, copied before the
 * call returns.  PSFs of wt_batch64_psf_ok only. */
int wt_batch64_set_psf(wt_batch64 *batch, int slot, const double *kernel, int kh, int kw);
/* wt64_filter2d per frame with the PSF of `slot` (cv2.filter2D of watroo/utils.py:257,286 with WT_BORDER_SYMMETRIC;
 * the circular products of utils.py:245-254,284 with WT_BORDER_PERIODIC), anchor (ay, ax) inside the kernel,
 * src != dst: one launch for all active frames (64 x 16 output tiles, the input window staged in LDS as doubles), no
 * stream drain, no PSF copy */
int wt_batch64_filter2d(wt_batch64 *batch, int nf, int src, int dst, int slot, int ay, int ax, int border);
/* wt64_binary over the active frames: dst = a OP b (watroo/utils.py:259,280-281,288); op as in wt_batch_binary
 * (0 sub, 1 add, 2 mul, 3 div, 4 (a + b) / b) */
int wt_batch64_binary(wt_batch64 *batch, int nf, int op, int a, int b, int dst);
/* wt64_mrs_update per frame (watroo/utils.py:263-276) with the frame's tau[f] (<= 0: significance one); scalar noise
 * only - the noise of richardson_lucy is the data's MAD estimate (utils.py:262) */
int wt_batch64_mrs_update(wt_batch64 *batch, int nf, int plane, int mrs_plane, const double *tau, int soft,
                          int persistent, double inv_pow);

/* ---- stacks of 1-D signals of one length (wt_signals) ------------------------------------------------------------
 * M signals of N samples, float or double: one workgroup per signal, the scales of a signal in LDS, every plane
 * written once.  The reference transforms a signal in the 1-D branch of convolution() (watroo/wavelets.py:65-69,
 * scipy's 'mirror' border) under atrous_standard (:408-444); every signal gets the bits of the per-signal call
 * (wt_decompose / wt64_decompose on a 1 x N plan under wt_plan_set_border(2)).  Operations take the number of active
 * signals `count` (signals 0 .. count-1); transfers address signals [first, first + count). */
typedef struct wt_signals wt_signals;
/* host logic, no GPU needed: 1 when signals of n_samples samples of `itemsize` bytes (4: float, 8: double) of
 * `family` over `level` scales (watroo/wavelets.py:426-444) run on a wt_signals, else 0: a built-in family, 1 .. 24
 * scales, and the two LDS buffers of a signal within 64 KiB - n_samples <= 8192 floats, <= 4096 doubles */
int wt_signals_ok(int family, int64_t n_samples, int level, int itemsize);
/* device memory for n_signals signals of n_samples samples (wt_signals_ok) and transforms of up to max_level scales:
 * the signals, max_level + 1 planes and one sum per signal (watroo/wavelets.py:426-427) */
int wt_signals_create(wt_ctx *ctx, int n_signals, int n_samples, int family, int max_level, int itemsize,
                      wt_signals **out);
int wt_signals_destroy(wt_signals *signals);
/* info[6] = {n_signals, n_samples, pitch in elements, family, max_level, itemsize} */
int wt_signals_info(wt_signals *signals, int64_t *info);
/* signals [first, first + count) <- `count` rows of n_samples contiguous elements (the arr of watroo/wavelets.py:307);
 * the block is free when the call returns */
int wt_signals_upload(wt_signals *signals, int first, int count, const void *host);
/* AtrousTransform.atrous_standard of signals 0 .. count-1 over `level` scales (watroo/wavelets.py:408-444 over
 * :65-69): one launch; HBM traffic sizeof(element) * (level + 2) bytes per sample */
int wt_signals_decompose(wt_signals *signals, int count, int level);
/* wt_signals_decompose with `flags`: bit 0 = Anscombe - every sample goes through generalized_anscombe(x) =
 * 2 sqrt(max(x + 3/8, 0)) (watroo/wavelets.py:14-21 with alpha = 1, g = 0, sigma = 0; watroo/utils.py:93-94) as it is
 * loaded, the bits of wt_anscombe / wt64_anscombe; the signals in device memory stay as they are.  The same launch, the
 * same traffic.  Any other bit is refused; flags = 0 is wt_signals_decompose.  A mode of the call, never of the stack */
int wt_signals_decompose_ex(wt_signals *signals, int count, int level, int flags);
/* np.median(np.abs(w_0)) of signals 0 .. count-1 (Coefficients.get_noise, watroo/wavelets.py:126-127), exact and
 * with the even / odd rule of wt_abs_median: medians[count] of the stack's element type, one host round trip */
int wt_signals_abs_median(wt_signals *signals, int count, void *medians);
/* Coefficients.denoise + np.sum(coefficients, axis=0) of signals 0 .. count-1 (watroo/wavelets.py:145-149,
 * utils.py:97-98; wt_denoise_sum / wt64_denoise_sum per signal, planes left as they are): tau[count * n_den] and
 * wgt[count * n_den], one row per signal; tau <= 0: significance one.  At most 16 planes (level <= 15) */
int wt_signals_denoise_sum(wt_signals *signals, int count, int n_den, const double *tau, const double *wgt,
                           int soft);
/* wt_signals_denoise_sum with `flags`: bit 0 = Anscombe - every sum goes through the inverse (x / 2)^2 - 3/8
 * (watroo/wavelets.py:16-17; watroo/utils.py:99-100) before its one store, the bits of wt_anscombe / wt64_anscombe
 * with inverse = 1.  tau refers to the transformed data (utils.py:95-97).  Any other bit is refused; flags = 0 is
 * wt_signals_denoise_sum */
int wt_signals_denoise_sum_ex(wt_signals *signals, int count, int n_den, const double *tau, const double *wgt,
                              int soft, int flags);
/* {sum, sum of squares} of every plane 0 .. level of signals 0 .. count-1 of the last wt_signals_decompose, in double
 * (c.std() and np.mean(power) of watroo/utils.py:176-189 as wt_reduce / wt64_reduce give them per signal):
 * moments[count * (level + 1) * 2], one host round trip.  The fold order is fixed: the same bits run to run */
int wt_signals_moments(wt_signals *signals, int count, double *moments);
/* the per-scale loop of wow and np.sum(coefficients, axis=0) of signals 0 .. count-1 (watroo/utils.py:174-205 on a
 * 1-D array, without gamma sum; wt_wow_scale / wt_wow_update / wt_plane_sum and their wt64_ forms per signal) in one
 * launch: tau[count * n_scales] (tau <= 0: significance one) and factor[count * (n_scales + 1)] (w * power_norm, the
 * last plane's divided by its local power), one row per signal; `whitening`: the detail planes are divided by the
 * square root of their local power conv_s(c^2), clipped at 1e-15 (utils.py:193-196).  n_scales: the level of the last
 * wt_signals_decompose.  The sum goes where wt_signals_download_sum finds it; with `write_planes` the whitened
 * planes replace the planes in place (wt_signals_download_planes) */
int wt_signals_wow_sum(wt_signals *signals, int count, int n_scales, const double *tau, const double *factor,
                       int whitening, int soft, int write_planes);
/* the planes of signals [first, first + count) of the last wt_signals_decompose -> host (count, level + 1, n_samples)
 * (Coefficients.data per signal, watroo/wavelets.py:426-444) */
int wt_signals_download_planes(wt_signals *signals, int first, int count, void *host);
/* the sums of wt_signals_denoise_sum / wt_signals_wow_sum of signals [first, first + count) -> host (count, n_samples)
 * (utils.py:98, :205) */
int wt_signals_download_sum(wt_signals *signals, int first, int count, void *host);

/* ---- the 1-D transform along an axis that is not the last one (wt_along) -------------------------------------------
 * An array viewed as (O, N, I), float or double: N samples of a signal lie I elements apart (every pixel's light curve
 * of a (T, H, W) movie: O = 1, N = T, I = H * W).  A workgroup takes a tile of TI neighbouring signals with their
 * scales in LDS and writes every plane once in the layout of the input; no transpose.  Every signal gets the bits of
 * wt_signals on the transposed stack, hence of the reference's 1-D branch (watroo/wavelets.py:65-69 under :408-444).
 * The stack holds one chunk (n_outer, N, n_inner) at a time (wt_along_upload); a plane of a chunk is laid out as the
 * chunk.  Host blocks are addressed as rows of n_inner elements, `pitch` elements apart (pitch = I). */
typedef struct wt_along wt_along;
/* host logic, no GPU needed: 1 when signals of n_samples samples n_inner elements apart of `itemsize` bytes (4: float,
 * 8: double) of `family` over `level` scales (watroo/wavelets.py:426-444) run on a wt_along, else 0: a built-in family,
 * 1 .. 24 scales, n_inner >= 2, and a tile of at least 64 bytes per run whose two LDS buffers fit 64 KiB -
 * n_samples <= 512 in either type (a chosen budget, not a measured optimum) */
int wt_along_ok(int family, int64_t n_samples, int64_t n_inner, int level, int itemsize);
/* device memory for chunks of up to n_signals signals (n_outer * n_inner) of n_samples samples: with_planes != 0 for
 * transforms of up to max_level scales (the block and max_level + 1 planes, watroo/wavelets.py:426-427), 0 for the
 * fused thresholded sum (the block, the sum and the threshold table, utils.py:97-98) */
int wt_along_create(wt_ctx *ctx, int64_t n_signals, int n_samples, int family, int max_level, int itemsize,
                    int with_planes, wt_along **out);
int wt_along_destroy(wt_along *along);
/* info[8] = {n_signals, n_samples, tile TI, family, max_level, itemsize, with_planes, scales of the last transform} */
int wt_along_info(wt_along *along, int64_t *info);
/* the chunk (n_outer, n_samples, n_inner) <- n_outer * n_samples host rows of n_inner elements, `pitch` elements apart
 * (the arr of watroo/wavelets.py:307, in place); the block is free when the call returns */
int wt_along_upload(wt_along *along, int n_outer, int n_inner, const void *host, int64_t pitch);
/* AtrousTransform.atrous_standard of every signal of the chunk over `level` scales (watroo/wavelets.py:408-444 over
 * :65-69): one launch; HBM traffic sizeof(element) * (level + 2) bytes per sample */
int wt_along_decompose(wt_along *along, int level);
/* np.median(np.abs(w_0)) of every signal of the chunk (Coefficients.get_noise, watroo/wavelets.py:126-127), exact,
 * the even / odd rule of wt_signals_abs_median: scale 0 in LDS only, no plane written; medians[n_outer * n_inner] of
 * the stack's element type, one host round trip */
int wt_along_abs_median(wt_along *along, void *medians);
/* wt_along_abs_median with `flags`: bit 0 = Anscombe - the medians of generalized_anscombe(chunk) (watroo/wavelets.py:
 * 14-21; the noise level of watroo/utils.py:95-97 refers to the transformed data), the forward transform applied as the
 * chunk is loaded.  Any other bit is refused; flags = 0 is wt_along_abs_median */
int wt_along_abs_median_ex(wt_along *along, void *medians, int flags);
/* Coefficients.denoise + np.sum(coefficients, axis=0) of every signal of the chunk (watroo/wavelets.py:145-149,
 * utils.py:97-98) fused with the transform over `level` scales: only the sum is written.  tau[n_outer * n_inner *
 * n_den], one row per signal (tau <= 0: significance one), wgt[n_den] shared; n_den <= level <= 15 */
int wt_along_denoise(wt_along *along, int level, int n_den, const double *tau, const double *wgt, int soft);
/* wt_along_denoise with `flags`: bit 0 = Anscombe - generalized_anscombe as the chunk is loaded and its inverse on the
 * sum before the one store (watroo/wavelets.py:14-21; watroo/utils.py:93-94, 99-100): denoise(..., anscombe=True) of
 * every signal in the same launch at the same traffic.  Any other bit is refused; flags = 0 is wt_along_denoise */
int wt_along_denoise_ex(wt_along *along, int level, int n_den, const double *tau, const double *wgt, int soft,
                        int flags);
/* the planes of the last wt_along_decompose -> host: plane s at host + s * plane_stride elements, each as the rows of
 * wt_along_upload (Coefficients.data per signal, watroo/wavelets.py:426-444) */
int wt_along_download_planes(wt_along *along, void *host, int64_t pitch, int64_t plane_stride);
/* the sum of wt_along_denoise -> host rows as wt_along_upload (utils.py:98) */
int wt_along_download_sum(wt_along *along, void *host, int64_t pitch);

/* ---- arrays that stay on the device (wavelets_amd/resident.py, wt_resident.hip) ----------------------------------
 * Frames that already lie in device memory - the output of a model, of a calibration kernel, of a previous call - go
 * into a batch and come out of it without crossing PCIe.  Additive entries: wt_abi_version() stays 8. */
#define WT_COPY_HOST_TO_DEVICE 1
#define WT_COPY_DEVICE_TO_HOST 2
#define WT_COPY_DEVICE_TO_DEVICE 3
/* how `stream` of the load / store entries is read: nothing to order (the array is ready), the legacy default stream,
 * the per-thread default stream, or `stream` is a hipStream_t */
#define WT_STREAM_NONE 0
#define WT_STREAM_LEGACY 1
#define WT_STREAM_PER_THREAD 2
#define WT_STREAM_HANDLE 3
/* a plain block of `bytes` bytes of device memory on the context's GPU (0 bytes: *ptr = NULL).  Replaces the page-locked
 * host block of wt_host_alloc as the home of a result: the block behind a resident.DeviceArray */
int wt_device_alloc(wt_ctx *ctx, size_t bytes, void **ptr);
/* ... and back (NULL: nothing).  Replaces wt_host_free; waits for the device, so nothing queued still uses the block */
int wt_device_free(wt_ctx *ctx, void *ptr);
/* `bytes` contiguous bytes dst <- src, kind WT_COPY_*; complete when it returns.  Replaces the host side of wt_upload /
 * wt_download for a block that belongs to no plan (DeviceArray.from_numpy, DeviceArray.numpy) */
int wt_device_copy(wt_ctx *ctx, void *dst, const void *src, size_t bytes, int kind);
/* frames [f0, f0+nf) of a plane <- the (nf, H, W) DEVICE array at `dev` of element type `dtype` (WT_UINT8 or
 * WT_FLOAT32), stride_bytes[3] = bytes from frame to frame, row to row, element to element (positive multiples of the
 * element size; any pitch, any inner stride), each element converted as wt_upload_int converts it.  Replaces
 * wt_batch_upload for frames that are on the device already: one kernel, one read and one write per element, the
 * plane's padding columns untouched.  With a stream_kind other than WT_STREAM_NONE the context's stream first waits
 * for what that stream holds; no host synchronisation either way */
int wt_batch_load_device(wt_batch *batch, int plane, int f0, int nf, const void *dev, int dtype,
                         const int64_t stride_bytes[3], void *stream, int stream_kind);
/* frames [f0, f0+nf) of a plane -> the (nf, H, W) float DEVICE array at `dev`, strides as above.  Replaces
 * wt_batch_download for a result that stays on the device.  With a stream_kind other than WT_STREAM_NONE that stream
 * then waits for the copy; no host synchronisation either way */
int wt_batch_store_device(wt_batch *batch, int plane, int f0, int nf, void *dev, const int64_t stride_bytes[3],
                          void *stream, int stream_kind);
/* wt_batch_load_device for the float64 batch: `dtype` WT_UINT8, WT_INT16, WT_UINT16, WT_INT32, WT_FLOAT32 or
 * WT_FLOAT64, widened as wt_batch64_upload_elems widens (the reference's recast to float64).  Replaces
 * wt_batch64_upload and wt_batch64_upload_elems, the device staging block of the latter included */
int wt_batch64_load_device(wt_batch64 *batch, int plane, int f0, int nf, const void *dev, int dtype,
                           const int64_t stride_bytes[3], void *stream, int stream_kind);
/* wt_batch_store_device for the float64 batch: a (nf, H, W) double DEVICE array.  Replaces wt_batch64_download */
int wt_batch64_store_device(wt_batch64 *batch, int plane, int f0, int nf, void *dev, const int64_t stride_bytes[3],
                            void *stream, int stream_kind);

#ifdef __cplusplus
}
#endif
#endif /* WATROO_HIP_H */
