// The kernel of the fused passes (see wt_fused.h), included twice by wt_fused.h: as wt_fused_kernel (one image;
// blockIdx.z = the row range) and as wt_fused_batch_kernel (a batch of frames, wt_batch: blockIdx.z = the frame,
// whose planes lie frame * fstride elements after frame 0's; whole passes).  Two kernels from one text, so that
// the image kernel compiles to exactly the code it had before batches existed.
//   WT_FUSED_KERNEL_NAME, WT_FUSED_KERNEL_BATCH (0 / 1): set by the includer
template <typename T, int K, int NS, int D, int NW, int PDREQ, int ACC, bool FAST>
__global__ __launch_bounds__(NW * 64, (NW == 4 ? WT_FUSED_WG4_PER_CU(K, NS, ACC) : 2)) void WT_FUSED_KERNEL_NAME(FusedArgsT<T> a)
{
    typedef typename WtVec<T>::V V;                      // a lane's 16 bytes: float4 or double2
    constexpr int PX = WtVec<T>::PX;                     // pixels per lane
    constexpr int ALIGN_PX = 128 / (int)sizeof(T);       // pixels per 128-byte line
    // ACC: 0 = plain pass; 1 / 2 = the pass carries the plane sum (2: last pass, adds the smooth
    // plane); 3 = plain pass that also histograms |w_{s0}| (first level of wt_abs_median's select:
    // Coefficients.get_noise reads plane 0 once less)
    constexpr bool SUM = ACC == 1 || ACC == 2;
    constexpr bool HIST = ACC == 3;
    static_assert(!HIST || D == 1, "the histogram variant exists for the first pass only");
    static_assert(NS <= 3 || K == 3, "four scales per pass: 3-tap family only");
    constexpr int hw = K / 2;
    constexpr int KM = K - 1;
    constexpr int LAT_IN = hw * ((1 << NS) - 1);         // rows of input beyond a stored row
    constexpr int LAT = LAT_IN + (NS - 1);               // + pipeline skew between the scales
    // x halo rounded up to 32 pixels (128 B): with strip starts that are multiples of 32 pixels
    // every wave's 1-KiB row access is cache-line aligned (8 lines, not 9 with two half lines)
    constexpr int HX = (hw * ((1 << NS) - 1) * D + ALIGN_PX - 1) / ALIGN_PX * ALIGN_PX;
    constexpr int U = KM << (NS - 1);                    // register-rotation period
    constexpr int PD = (U % PDREQ == 0) ? PDREQ : 4;     // rows prefetched ahead
    constexpr int NL = NW * 64;                          // lanes (16-byte columns) per WG
    static_assert(U % PD == 0 && U % 2 == 0, "prefetch depth / LDS parity must divide the unroll period");

    __shared__ V vbuf[2][NS][NL];
    // output row of scale a at step t: t - a - hw*(2^(a+1)-1)
    constexpr int LAG0 = hw, LAG1 = 1 + 3 * hw, LAG2 = 2 + 7 * hw, LAG3 = 3 + 15 * hw;
    constexpr int LAGC = NS == 1 ? LAG0 : (NS == 2 ? LAG1 : (NS == 3 ? LAG2 : LAG3));
    // peeled prologue steps (see `step` below): the cascade's fill time rounded up to whole unrolled
    // bodies, at most two of them (code size); none for the single-scale passes
    // Built where the extra code does not cost registers the kernel does not have: the float D = 1
    // passes of up to three scales (B3 d1x3: 220 -> 240 VGPRs, no scratch).  The D = 8 three-scale
    // passes sit at 256 VGPRs already and the four-scale / double variants spill with it (16 - 220
    // spilled registers; still 21 with a single peeled trip, and gating only the horizontal filters
    // and stores changes nothing), so they keep the plain march.
#ifdef WT_FUSED_NO_PROLOGUE
    constexpr int PRO = 0;
#else
    constexpr bool PRO_FITS = D == 1 && NS >= 2 && NS <= 3 && sizeof(T) == 4;
    constexpr int PRO = !PRO_FITS ? 0 : (((LAT_IN + LAGC + U - 1) / U) < 2 ? ((LAT_IN + LAGC + U - 1) / U) : 2) * U;
#endif
    // ACC: the running sum of a row waits in per-lane LDS rings until the next scale's detail
    // row of the SAME image row comes out of the cascade (G1, then G2 steps later); only lanes
    // that own stored pixels take part (NV of them), nothing crosses lanes: no barrier.
    constexpr int G1 = NS > 1 ? LAG1 - LAG0 : 0, G2 = NS > 2 ? LAG2 - LAG1 : 0, G3 = NS > 3 ? LAG3 - LAG2 : 0;
    constexpr int NV = NL - 2 * HX / PX;
    __shared__ V ring[SUM && NS > 1 ? (G1 + G2 + G3) * (NV + 1) : 1];   // + one spare slot per row for the halo lanes

    __shared__ uint32_t lh[HIST ? WT_HIST_BINS : 1];
    // windowed bins: shift 10 (float) / 41 (double) and the window's first key; plain: shift 20 / 52, base 0 - one code path
    int hist_shift = 20, hist_lo = 0;
    if constexpr (HIST) {                                // (before the early exits: all waves pass the barrier)
        for (int i = threadIdx.x; i < WT_HIST_BINS; i += NL) lh[i] = 0;
        if (a.hist_base) {
            hist_shift = PX == 4 ? 10 : 41;
            hist_lo = (int)__builtin_amdgcn_readfirstlane(*a.hist_base);
        } else if (PX == 2) {
            hist_shift = 52;                             // double, plain: the exponent field
        }
        __syncthreads();
    }
    // Keys below / above the window (bins 0 and WT_HIST_BINS - 1 of the clamped index) are ~90 % of a windowed
    // histogram's samples - the window spans +-12 % around the predicted median - and as LDS atomics they all hit the
    // same two words: 64 lanes serialise on one address.  They are counted in two registers per lane instead and
    // added to their bins once, at the end of the chunk (round 6); only the in-window keys take the atomic.
    int hist_out = 0, hist_below = 0;                    // samples outside the window / below it (this lane)
    auto hist_count = [&](int rel) {                     // rel = key - first key of the window
        if ((unsigned)(rel - 1) < (unsigned)(WT_HIST_BINS - 2)) atomicAdd(&lh[rel], 1u);
        else ++hist_out;
        hist_below += rel <= 0;
    };

    const Geo g = a.g;
#if WT_FUSED_KERNEL_BATCH
    // a frame of a batch: the frame-0 planes moved by fstride elements (scalar setup; whole passes: range 0)
    const int64_t foff = (int64_t)blockIdx.z * a.fstride;
#define WT_FP(x) ((x) + foff)
#define WT_ZR 0
#else
#define WT_FP(x) (x)
#define WT_ZR blockIdx.z
#endif
    const int gl = threadIdx.x;                          // lane index within the WG row
    const int X0 = blockIdx.x * a.Vx;                    // first valid pixel of this x-strip
    constexpr bool WA = WT_FUSED_WA && D == 1 && NS <= 3 && PX == 4;   // wave-autonomous horizontal taps (experiment)
    const int wa_ln = gl & 63, wa_vw = a.Vx / NW;        // lane in the wave; stored pixels per wave
    const int x = WA ? X0 + (gl >> 6) * wa_vw - 16 + 4 * wa_ln
                     : X0 - HX + PX * gl;                // this lane's first pixel (may be < 0)
    const int item = blockIdx.y;
    const int q = item % D;                              // chain phase
    const int chunk = item / D;
    if (q >= g.nrows) return;                            // whole WG exits together
    // chain elements r of this phase with rlo <= q + D*r < rhi
    const int lo = a.rlo[WT_ZR], hi = a.rhi[WT_ZR];
    const int ra = lo > q ? (lo - q + D - 1) / D : 0;
    const int rb = hi > q ? (hi - q + D - 1) / D : 0;
    const int r0 = ra + chunk * a.S;
    const int r1 = min(r0 + a.S, rb);
    if (r0 >= r1) return;

    // lanes that own stored pixels; a float4 that straddles W writes into the row's pitch
    // padding (allocated, never read as image data)
    const bool lane_store = WA ? (wa_ln >= 4 && 4 * (wa_ln - 4) < wa_vw && x < g.W)
                               : (x >= X0) && (x < X0 + a.Vx) && (x < g.W);
    const unsigned voff = lane_store ? (unsigned)x * (unsigned)sizeof(T) : WT_FUSED_PARKED;
    const int row_bytes = g.P * (int)sizeof(T);
    // Every lane issues ONE aligned in-bounds dwordx4 per row.
    // FAST (host: W % 4 == 0, W >= HX, H >= D * (LAT_IN + 1) - every image the benchmarks name):
    //   the reflection of an aligned 4-pixel group that lies outside the image is an aligned group
    //   read backwards, so a border lane loads that group like any other lane and reverses the
    //   four values when the row is CONSUMED (wave-uniform branch around four v_cndmask: no load
    //   sits behind a branch, every workgroup runs the same instruction stream), and a row index
    //   reflects at most once (two s_max / s_min instead of a modulo behind a branch).
    // generic: lanes whose 4 pixels are not all inside the image (reflected halo at the image
    //   border, ragged right edge) patch the value with a reflected gather under a wave-uniform
    //   branch (border waves only); rows reflect any number of times.
    const bool lane_interior = (x >= 0) && (x + PX - 1 < g.W);
    const bool wave_has_edge = !__all(lane_interior);
    // FAST with W % PX != 0 (round 6): ONE group per row straddles the right border.  Its reflected pixels lie inside
    // the same four pixels - (g0, g1, g1, g0) for W % 4 == 2, (g0, g1, g2, g2) for 3, and for 1 the four pixels that
    // END at the border read as (g3, g3, g2, g1); doubles: (g0, g0) - so it is one load and a swizzle like the
    // reversed groups, which then start at 2W - PX - x: 8-byte aligned for odd W (a 16-byte load needs 4).
    const int wrem = g.W % PX;                           // (wave-uniform)
    const bool lane_str = FAST && x < g.W && x + PX > g.W;
    const bool lane_rev = FAST && !lane_interior && !lane_str;
    const int xg = x < 0 ? -PX - x : (x >= g.W ? 2 * g.W - PX - x : (lane_str && PX == 4 && wrem == 1 ? g.W - PX : x));   // FAST: the group this lane loads
    const int xc = FAST ? min(max(xg, 0), g.P - PX) : min(max(x, 0), g.P - PX);
    const int xi0 = wt_refl(x, g.W), xi1 = wt_refl(x + 1, g.W), xi2 = wt_refl(x + (PX > 2 ? 2 : 0), g.W),
              xi3 = wt_refl(x + (PX > 2 ? 3 : 0), g.W);
    const int gy0 = g.row0 + q;                          // global row of chain element 0

    const int dbg = WT_FUSED_DBG(a);
    const int t_last = r1 - 1 + LAT_IN;                  // last input row any stored output needs
    const unsigned xoff = (unsigned)xc * (unsigned)sizeof(T);   // byte offset of this lane's aligned load
    const int H2m1 = 2 * g.H - 1;
    auto load_row = [&](int t) -> V {
        // steps past t_last only flush the pipeline / unroll padding: keep the address in range.
        // Uniform row pointer + 32-bit lane offset: one global_load_dwordx4 with an SGPR base.
        if constexpr (FAST) {
            const int gy = gy0 + D * ((dbg & 2) ? r0 : min(t, t_last));
            const int up = max(gy, ~gy);                 // -1 - gy above the image
            const int ry = min(up, H2m1 - up);           // 2H - 1 - gy below it
            const T *row = WT_FP(a.in) + (int64_t)(ry - g.row0) * g.P;
            return *reinterpret_cast<const V *>(reinterpret_cast<const char *>(row) + xoff);
        } else {
            const T *row = WT_FP(a.in) + (int64_t)(wt_refl(gy0 + D * ((dbg & 2) ? r0 : min(t, t_last)), g.H) - g.row0) * g.P;   // (= wt_row)
            V v = *reinterpret_cast<const V *>(reinterpret_cast<const char *>(row) + xoff);
            if (wave_has_edge) {
                if constexpr (PX == 4) {
                    if (!lane_interior) v = make_float4(row[xi0], row[xi1], row[xi2], row[xi3]);
                } else {
                    if (!lane_interior) v = make_double2(row[xi0], row[xi1]);
                }
            }
            return v;
        }
    };
    // Output rows advance by one chain step (D image rows) per iteration.  Every plane has ONE
    // descriptor for the whole march, based at the row it stores at step 0 (row t0 - LAG of the
    // chain; before the chunk, never written) and as long as the chunk's byte span (< 2 GiB,
    // host); step k adds k * step_bytes to the lane offset.  A row outside [r0, r1) parks the
    // offset instead of branching, so control flow stays uniform.
    const unsigned span = (unsigned)(r1 - r0);
    const unsigned step_bytes = (unsigned)D * (unsigned)row_bytes;
    auto row_addr0 = [&](T *base, int ro) -> uint64_t {
        return (uint64_t)base + (uint64_t)((int64_t)(q + (int64_t)D * ro) * (int64_t)row_bytes);
    };

    constexpr int A1 = NS > 1 ? 1 : 0, A2 = NS > 2 ? 2 : 0, A3 = NS > 3 ? 3 : 0;
    VWin<V, K, 0> w0;
    VWin<V, K, A1> w1;
    VWin<V, K, A2> w2;
    VWin<V, K, A3> w3;
    const V zero = wt_vzero<V>();
#pragma unroll
    for (int j = 0; j < KM; ++j) {
        w0.w[0][j] = zero;
#pragma unroll
        for (int r = 0; r < (1 << A1); ++r) w1.w[r][j] = zero;
#pragma unroll
        for (int r = 0; r < (1 << A2); ++r) w2.w[r][j] = zero;
        if constexpr (NS > 3) {
#pragma unroll
            for (int r = 0; r < (1 << A3); ++r) w3.w[r][j] = zero;
        }
    }

    const int t0 = r0 - LAT_IN;                          // first input chain index
    const int nsteps = ((r1 - r0) + LAT + LAT_IN + U - 1) / U * U;
    V pf[PD];
#pragma unroll
    for (int i = 0; i < PD; ++i) pf[i] = load_row(t0 + i);
    V c1 = zero, c2 = zero, c3 = zero;                   // rows handed from scale a to a+1
    // Stores: every plane has ONE descriptor for the whole march - base = row r0 of the chain (the
    // chunk's first stored row), length = the chunk's byte span.  At step k a plane stores row
    // k - (LAT_IN + LAG) of the chunk, i.e. the lane offset is x*4 + (k - LAT_IN - LAG) * step_bytes:
    // before the chunk that is negative (wraps to ~4 GiB), after it >= the length - the hardware
    // range check IS the row predicate, no scalar work per store.  Halo lanes park at 2^31 (the host
    // keeps a chunk's span incl. warm-up below 2^31, so a parked lane never wraps into range).
    const unsigned chunk_len = (span - 1u) * step_bytes + (unsigned)row_bytes;
    auto plane_rsrc = [&](T *base, int) -> __amdgpu_buffer_rsrc_t {
        // Length and flag words pass through an empty asm so that every descriptor owns its four
        // SGPRs: shared words would be copied into place before every store (2 s_mov each).
        unsigned len = chunk_len, flags = 0x00020000;
        asm volatile("" : "+s"(len), "+s"(flags));
        return __builtin_amdgcn_make_buffer_rsrc((void *)row_addr0(base, r0), 0, len, flags);
    };
    // byte offset of a plane's row at step 0 (negative, as unsigned): -(LAT_IN + LAG) * step_bytes
    auto lag_off = [&](int lag) -> unsigned { return 0u - (unsigned)(LAT_IN + lag) * step_bytes; };
    const unsigned o0 = lag_off(LAG0), o1 = lag_off(LAG1), o2 = lag_off(LAG2), o3 = NS > 3 ? lag_off(LAG3) : 0u, oc = lag_off(LAGC);
    const __amdgpu_buffer_rsrc_t rw0 = plane_rsrc(WT_FP(a.out_w[0]), LAG0);
    const __amdgpu_buffer_rsrc_t rw1 = plane_rsrc(WT_FP(a.out_w[A1]), LAG1);
    const __amdgpu_buffer_rsrc_t rw2 = plane_rsrc(WT_FP(a.out_w[A2]), LAG2);
    // (only a four-scale pass builds the fourth descriptor: plane_rsrc pins four SGPRs)
    const __amdgpu_buffer_rsrc_t rw3 = NS > 3 ? plane_rsrc(WT_FP(a.out_w3), LAG3) : rw2;
    const __amdgpu_buffer_rsrc_t rc = plane_rsrc(WT_FP(a.out_c), LAGC);
    // ---- ACC state.  The first pass of a sum (D = 1, s0 = 0) has no incoming partial sum, every
    // later pass has one: decided at compile time (the host checks first == (s0 == 0)).
    constexpr bool PIN = SUM && D != 1;
    const __amdgpu_buffer_rsrc_t rp = plane_rsrc(SUM ? WT_FP(a.p_out) : WT_FP(a.out_c), LAGC);
    unsigned koff = 0;                                   // k * step_bytes
    // incoming partial sum: the same fixed-descriptor addressing as the stores (row r0 of the chain,
    // the chunk's byte span) - a row before or after the chunk reads as 0 without touching memory
    // (its sum is never stored), so there is no clamp and no scalar address arithmetic per step
    const __amdgpu_buffer_rsrc_t rpin = plane_rsrc(PIN ? const_cast<T *>(WT_FP(a.p_in)) : WT_FP(a.out_c), 0);
    // (halo lanes are parked like their stores: they read nothing)
    auto load_acc = [&](int k_ahead) -> V {              // p_in row of chain element t0 + k - LAG0, k = current step + k_ahead
        const wt_v4u t = __builtin_amdgcn_raw_buffer_load_b128(rpin, voff + koff + o0 + (unsigned)k_ahead * step_bytes, 0, 0);
        return wt_from_v4u(t, V());
    };
    V pa[PIN ? PD : 1];
    if constexpr (PIN) {
        // (with a prologue the first p_in row that matters is loaded by its step LAT_IN + LAG0 - PD)
#pragma unroll
        for (int i = 0; i < PD; ++i) pa[i] = PRO > 0 ? zero : load_acc(i);   // koff = 0 here
    }
    const int li = lane_store ? (x - X0) / PX : NV;      // slot in the ring rows; NV = the spare slot
    int i1 = 0, i2 = 0, i3 = 0;                          // ring positions (wave-uniform)

    // One chain step.
    // PROLOGUE (round 3).  The cascade fills over the first LAT_IN + LAG_last steps of a chunk: scale
    // a's horizontal filter produces a row that some stored row depends on only from step H_a on,
    // its vertical window needs real input only from step V_a on, and plane a stores from step
    // ST_a on:
    //     R_a  = hw * (2^NS - 2^(a+1))      rows of c_{a+1} beyond the chunk that later scales reach
    //     H_a  = LAG_a + LAT_IN - R_a       B3, NS = 3:  4, 13, 30
    //     V_a  = H_a - 2 * hw * 2^a                      0,  5, 14
    //     ST_a = LAT_IN + LAG_a                          16, 21, 30
    // The steady-state step does all of it at every step (3 * 30 scale-steps where 47 + 43 are
    // needed), which nobody notices while the pass waits for memory, but a grid of short chunks
    // (4096^2: 40 stored rows per chunk behind 30 warm-up steps) is bound by instruction issue.
    // The first PRO steps therefore run as peeled copies of the step in which everything that is
    // not needed yet is compiled out (k is a constant there): no vertical / horizontal filter, no
    // LDS row, no parked store, no ring traffic, no p_in load before its time.  The last PD peeled
    // steps keep the full store pattern, so that the loop is entered with the steady state's
    // vector-memory queue (what the parked stores of the vmcnt padding provided before).
    // Bit-identical: every value a stored row depends on is computed by the same instructions.
    auto step = [&](const int kb, const int kk, auto pro_tag) {
        constexpr bool PROL = decltype(pro_tag)::value;       // a peeled prologue step (kb + kk is a constant)
        const int k = kb + kk;
        const int t = t0 + k;
        constexpr int R0 = hw * ((1 << NS) - 2), R1 = hw * ((1 << NS) - 4), R2 = hw * ((1 << NS) - 8);
        constexpr int H0 = LAG0 + LAT_IN - R0, H1 = LAG1 + LAT_IN - R1, H2 = LAG2 + LAT_IN - R2, H3 = LAG3 + LAT_IN;
        constexpr int V1 = H1 - 4 * hw, V2 = H2 - 8 * hw, V3 = H3 - 16 * hw;
        constexpr int ST0 = LAT_IN + LAG0, ST1 = LAT_IN + LAG1, ST2 = LAT_IN + LAG2, ST3 = LAT_IN + LAG3;
        const bool full = !PROL || k >= PRO - PD;             // steady-state store pattern
        const bool eh0 = !PROL || k >= H0, eh1 = !PROL || k >= H1, eh2 = !PROL || k >= H2, eh3 = !PROL || k >= H3;
        const bool ev1 = !PROL || k >= V1, ev2 = !PROL || k >= V2, ev3 = !PROL || k >= V3;
        const bool es0 = full || k >= ST0, es1 = full || k >= ST1, es2 = full || k >= ST2, es3 = full || k >= ST3;
        const bool esc = full || k >= LAT_IN + LAGC;          // smooth plane / carried sum
        // step k stores row t0 + k - LAG of a plane: inside the chunk iff k - (LAT_IN + LAG) < span
        const unsigned vk = voff + koff + ((dbg & 1) ? WT_FUSED_PARKED : 0u);
        auto at = [&](int lag) -> unsigned {             // lane offset of this step's row of a plane
            if constexpr (NS > 3) return vk + (lag == LAG0 ? o0 : lag == LAG1 ? o1 : lag == LAG2 ? o2 : o3);
            else return vk + (lag == LAG0 ? o0 : lag == LAG1 ? o1 : lag == LAG2 ? o2 : oc);
        };
        V cur = pf[kk % PD];
        pf[kk % PD] = load_row(t + PD);
        if constexpr (FAST) {
            // The fence pins the reversal to THIS step: without it the (w, z) swap is scheduled
            // right behind the load it reads (same basic block), and the wave waits for every row
            // in the step that issued it - no prefetch left.
            wt_vfence(cur);
            if (wave_has_edge) {
                if (lane_rev) cur = wt_vrev(cur);
                if (wrem != 0) {
                    if (lane_str) cur = wt_vstraddle(cur, wrem);
                }
            }
        }
        V (*buf)[NL] = vbuf[kk & 1];
#ifdef WT_FUSED_ABLATION
        if (dbg & 4) {   // ablation: same loads / stores / addresses, no filtering at all
            wt_bstore4v<WT_FUSED_W_AUX>(rw0, at(LAG0), cur);
            if constexpr (NS > 1) wt_bstore4v<WT_FUSED_W_AUX>(rw1, at(LAG1), cur);
            if constexpr (NS > 2) wt_bstore4v<WT_FUSED_W_AUX>(rw2, at(LAG2), cur);
            if constexpr (NS > 3) wt_bstore4v<WT_FUSED_W_AUX>(rw3, at(LAG3), cur);
            wt_bstore4v<WT_FUSED_C_AUX>(rc, at(LAGC), cur);
            if constexpr (SUM) {
                V pv = cur;
                if constexpr (PIN) {
                    pv = pa[kk % PD];
                    pa[kk % PD] = load_acc(PD);
                }
                wt_bstore4v<(ACC == 2 ? WT_FUSED_R_AUX : WT_FUSED_P_AUX)>(rp, at(LAGC), pv);
            }
            koff += step_bytes;
            return;
        }
#endif
        V pin_cur = zero;
        if constexpr (PIN) {
            pin_cur = pa[kk % PD];
            if (!PROL || k + PD >= ST0) pa[kk % PD] = load_acc(PD);   // (rows before the chunk read as 0 anyway)
        }
        // ACC: the ring slots that come due in this step were written G1 / G2 steps ago - read
        // them before the barrier so the LDS latency hides behind the vertical filters.  Lanes
        // without stored pixels share the spare slot NV of each ring row (their sums are never
        // stored), which keeps the ring traffic free of exec-mask branches.
        V old1 = zero, old2 = zero, old3 = zero;
        if constexpr (SUM && NS > 1) {
            if (es1) old1 = ring[i1 * (NV + 1) + li];
            if constexpr (NS > 2) {
                if (es2) old2 = ring[(G1 + i2) * (NV + 1) + li];
            }
            if constexpr (NS > 3) {
                if (es3) old3 = ring[(G1 + G2 + i3) * (NV + 1) + li];
            }
        }
        V cen0, cen1, cen2, cen3, v0, v1, v2, v3;
        v0 = wt_fused_vstage<T, K, 0>(w0, kk, cur, cen0);
        if constexpr (!WA) {
            if (eh0) buf[0][gl] = v0;
        }
        if constexpr (NS > 1) {
            v1 = zero;
            if (ev1) v1 = wt_fused_vstage<T, K, A1>(w1, kk, c1, cen1);
            if constexpr (!WA) {
                if (eh1) buf[A1][gl] = v1;
            }
        }
        if constexpr (NS > 2) {
            v2 = zero;
            if (ev2) v2 = wt_fused_vstage<T, K, A2>(w2, kk, c2, cen2);
            if constexpr (!WA) {
                if (eh2) buf[A2][gl] = v2;
            }
        }
        if constexpr (NS > 3) {
            v3 = zero;
            if (ev3) v3 = wt_fused_vstage<T, K, A3>(w3, kk, c3, cen3);
            if (eh3) buf[A3][gl] = v3;
        }
        if constexpr (!WA) {
            if (eh0) __syncthreads();                         // (no scale reads the LDS rows before step H0)
        }
        V n0 = zero, d0 = zero;
        if (eh0) {
            if constexpr (WA) n0 = wt_hfilter_dpp<K, (D <= 4 ? D : 4)>(v0);
            else n0 = wt_hfilter_lds<T, K, D, NL>(buf[0], gl, v0);
            d0 = f4_sub(cen0, n0);
        }
        if (es0) wt_bstore4v<WT_FUSED_W_AUX>(rw0, at(LAG0), d0);
        if constexpr (HIST) {
            // the same predicate as the store of this row: chunk row k - (LAT_IN + LAG0) in [0, span)
            // (wave-uniform) and a lane that owns stored pixels
            if ((!PROL || k >= ST0) && (unsigned)(k - (LAT_IN + LAG0)) < span && lane_store) {
                if constexpr (PX == 4) {
                    const uint32_t b[4] = {__float_as_uint(d0.x), __float_as_uint(d0.y), __float_as_uint(d0.z),
                                           __float_as_uint(d0.w)};
#pragma unroll
                    for (int j = 0; j < 4; ++j)       // (one v_bfe_u32 for the magnitude's top bits: the march is issue-bound)
                        if (FAST || x + j < g.W) hist_count((int)__builtin_amdgcn_ubfe(b[j], (uint32_t)hist_shift, 31u - (uint32_t)hist_shift) - hist_lo);
                } else {
                    // double: the top 11 bits of the 63-bit magnitude are the exponent field (first level
                    // of wt64_abs_median's select)
                    const unsigned long long b[2] = {(unsigned long long)__double_as_longlong(d0.x),
                                                     (unsigned long long)__double_as_longlong(d0.y)};
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        if (FAST || x + j < g.W) hist_count((int)((b[j] & 0x7fffffffffffffffull) >> hist_shift) - hist_lo);
                }
            }
        }
        if constexpr (NS == 1) {
            if (esc) wt_bstore4v<WT_FUSED_C_AUX>(rc, at(LAGC), n0);
        }
        V d1 = zero, d2 = zero, d3 = zero, n1 = zero, n2 = zero, n3 = zero;
        if constexpr (NS > 1) {
            if (eh1) {
                if constexpr (WA) n1 = wt_hfilter_dpp<K, ((D << A1) <= 4 ? (D << A1) : 4)>(v1);
                else n1 = wt_hfilter_lds<T, K, (D << A1), NL>(buf[A1], gl, v1);
                d1 = f4_sub(cen1, n1);
            }
            if (es1) wt_bstore4v<WT_FUSED_W_AUX>(rw1, at(LAG1), d1);
            if constexpr (NS == 2) {
                if (esc) wt_bstore4v<WT_FUSED_C_AUX>(rc, at(LAGC), n1);
            }
            if constexpr (NS > 2) {
                if (eh2) {
                    if constexpr (WA) n2 = wt_hfilter_dpp<K, ((D << A2) <= 4 ? (D << A2) : 4)>(v2);
                    else n2 = wt_hfilter_lds<T, K, (D << A2), NL>(buf[A2], gl, v2);
                    d2 = f4_sub(cen2, n2);
                }
                if (es2) wt_bstore4v<WT_FUSED_W_AUX>(rw2, at(LAG2), d2);
                if constexpr (NS == 3) {
                    if (esc) wt_bstore4v<WT_FUSED_C_AUX>(rc, at(LAGC), n2);
                }
                if constexpr (NS > 3) {
                    if (eh3) {
                        n3 = wt_hfilter_lds<T, K, (D << A3), NL>(buf[A3], gl, v3);
                        d3 = f4_sub(cen3, n3);
                    }
                    if (es3) wt_bstore4v<WT_FUSED_W_AUX>(rw3, at(LAG3), d3);
                    if (esc) wt_bstore4v<WT_FUSED_C_AUX>(rc, at(LAGC), n3);
                    c3 = n2;
                }
            }
            c2 = n1;
        }
        if constexpr (SUM) {
            // plane-order sum of image row rho: ((p_in + w_s0) + w_s0+1) + w_s0+2 (+ c): the
            // partial sum of a row is parked in the ring until the next scale's detail row of the
            // same image row appears (G1, then G2 steps later)
            V s = PIN ? f4_add(pin_cur, d0) : d0;                       // row t - LAG0
            if constexpr (NS > 1) {
                V s1 = f4_add(old1, d1);                                  // row t - LAG1
                V s2 = s1;
                if constexpr (NS > 2) s2 = f4_add(old2, d2);              // row t - LAG2
                // (a ring slot written at step k is read when the next scale's detail row of the same
                //  image row comes out: needed from the step at which that row is a stored one)
                if (es0) ring[i1 * (NV + 1) + li] = s;
                if constexpr (NS > 2) {
                    if (es1) ring[(G1 + i2) * (NV + 1) + li] = s1;
                }
                if constexpr (NS > 3) {
                    if (es2) ring[(G1 + G2 + i3) * (NV + 1) + li] = s2;
                    s = f4_add(old3, d3);                                 // row t - LAG3
                } else {
                    s = s2;
                }
                i1 = (i1 + 1 == G1) ? 0 : i1 + 1;
                if constexpr (NS > 2) i2 = (i2 + 1 == G2) ? 0 : i2 + 1;
                if constexpr (NS > 3) i3 = (i3 + 1 == G3) ? 0 : i3 + 1;
            }
            if constexpr (ACC == 2) s = f4_add(s, NS == 1 ? n0 : (NS == 2 ? n1 : (NS == 3 ? n2 : n3)));
            // the finished reconstruction is a write-once stream; an intermediate sum is re-read
            // by the next pass
            if (esc) wt_bstore4v<(ACC == 2 ? WT_FUSED_R_AUX : WT_FUSED_P_AUX)>(rp, at(LAGC), s);
        }
        c1 = n0;
        koff += step_bytes;
#ifndef WT_FUSED_NO_SCHEDBAR
        // Keep the scheduler from interleaving consecutive steps: with the branch-free FAST loads
        // the unrolled body is one basic block, and free motion across steps costs 30 more VGPRs
        // (spills) and turns every wait into vmcnt(0).
        if constexpr (FAST) __builtin_amdgcn_sched_barrier(0);
#endif
    };

    // The register rotation fixes the unroll factor at U steps, not the trip count: leave the
    // body at the last step that stores anything (a loop EXIT, not a skipped step - nothing
    // rejoins inside the loop, so the vmcnt bookkeeping of the steps stays exact).  S = 147 at
    // 8192^2 would otherwise march 192 steps instead of 177.
#ifndef WT_FUSED_NO_EARLY_EXIT
    const int nexact = (r1 - r0) + LAT + LAT_IN;
#else
    const int nexact = nsteps;
#endif
    int kb0 = 0;
    if constexpr (PRO > 0) {
        // the peeled prologue: PRO / U copies of the unrolled body with constant step numbers
        // (compile-time recursion: the step number must be a constant in every copy; as a `#pragma
        // unroll` loop around the early exit the body is NOT unrolled - the register window would
        // land in scratch memory)
        auto prologue = [&](auto self, auto ic) -> bool {
            constexpr int KK = decltype(ic)::value;
            if constexpr (KK < PRO) {
                if (KK >= nexact) return true;               // a chunk shorter than the prologue
                step(KK / U * U, KK % U, std::true_type{});
                return self(self, std::integral_constant<int, KK + 1>{});
            } else {
                return false;
            }
        };
        if (prologue(prologue, std::integral_constant<int, 0>{})) goto done;
        kb0 = PRO;
    } else {
        // (no prologue: NS = 1, or -DWT_FUSED_NO_PROLOGUE)
        // The compiler sizes every `s_waitcnt vmcnt(N)` of the loop from the FEWEST vector-memory
        // operations that can lie between a prefetch and its use on any path into that point - and on
        // the path from here the PD prefetches would be back to back, while in the steady state a
        // step's stores sit between them.  Without the padding below the first PD steps of every trip
        // through the unrolled body wait with vmcnt(2..15), i.e. for the STORES of the previous steps
        // to be acknowledged (once per U steps the wave drains its store queue).  Issue as many parked
        // stores (out-of-range offset: dropped by the range check, no memory traffic) as the steady
        // state has behind the prefetches, so that every wait in the loop becomes vmcnt(~PD*ops/step).
#ifndef WT_FUSED_NO_VMPAD
        constexpr int ST = NS + 1 + (SUM ? 1 : 0);          // stores per step
#pragma unroll
        for (int i = 0; i < PD * ST; ++i) wt_bstore4v<0>(rc, WT_FUSED_PARKED + 16u * i, zero);   // distinct: not merged
#endif
    }
    for (int kb = kb0; kb < nsteps; kb += U) {
#pragma unroll
        for (int kk = 0; kk < U; ++kk) {
            if (kb + kk >= nexact) goto done;
            step(kb, kk, std::false_type{});
        }
    }
done:;
    if constexpr (HIST) {
        if (hist_below) atomicAdd(&lh[0], (uint32_t)hist_below);
        if (hist_out - hist_below) atomicAdd(&lh[WT_HIST_BINS - 1], (uint32_t)(hist_out - hist_below));
        __syncthreads();
        for (int i = threadIdx.x; i < WT_HIST_BINS; i += NL)
            if (lh[i]) atomicAdd(&a.hist[i], lh[i]);
    }
}
#undef WT_FP
#undef WT_ZR
