// The per-scale stencil kernels (chain march, lattice, row kernel; see wt_stencil.h), included twice by
// wt_stencil.h: as wt_chain_kernel / wt_lattice_kernel / wt_row_kernel (one image) and as wt_chain_batch_kernel /
// wt_lattice_batch_kernel / wt_row_batch_kernel (a batch of frames, wt_batch: blockIdx.z = the frame, whose planes
// lie frame * fstride elements after frame 0's, its tau and factor in a small device table).  Two kernels from one
// text, so that the image kernels compile to exactly the code they had before batches existed (wt_fused_march.h
// does the same for the fused passes); the batched ones are instantiated only in wt_stencil32_batch.hip.
//   WT_SK_NAME(base), WT_SK_PARAM(type, name), WT_SK_FRAME(mode, name): set by the includer

template <typename T, int K, int MODE, bool SMALL_D>
__global__ __launch_bounds__(256) void WT_SK_NAME(wt_chain)(WT_SK_PARAM(ChainArgsT<T>, a))
{
    WT_SK_FRAME(MODE, a);
    typedef typename WtVec<T>::V V;
    constexpr int PX = WtVec<T>::PX;
    constexpr int hw = K / 2;
    const Geo g = a.g;
    int bx, by;
    wt_xcd_remap(bx, by);
    const int x = (bx * 64 + threadIdx.x) * PX;
    if (x >= g.W) return;
    // one wave = one threadIdx.y: make the item (and with it the chain phase, the chunk, the row
    // pointers and the loop counters) scalar - the compiler cannot prove threadIdx.y wave-uniform
    const int item = __builtin_amdgcn_readfirstlane(by * blockDim.y + threadIdx.y);
    const int d = a.d;
    const int q = item % d;   // chain phase (local row offset)
    const int c = item / d;   // chunk along the chain
    if (c >= a.chunks || q >= g.nrows) return;
    const int n_q = (g.nrows - q + d - 1) / d;  // chain length
    const int r0 = c * a.S;
    const int r1 = min(r0 + a.S, n_q);
    if (r0 >= r1) return;

    WtVert<T, K, MODE, SMALL_D> vert;
    const int gy0 = g.row0 + q;  // global row of chain element 0
    V raw[K], nxt[K];
#pragma unroll
    for (int j = 0; j < K - 1; ++j) {
        wt_hrow_load<T, K, SMALL_D>(wt_row_b(a.in, g, gy0 + d * (r0 - hw + j), d), x, d, g.W, raw, g.border);
        vert.prime(j, raw, d);
    }
    // software prefetch: the operands of the NEXT chain row are in flight while this row is
    // filtered (the kernel is latency-bound at 3-4 waves/SIMD otherwise)
    wt_hrow_load<T, K, SMALL_D>(wt_row_b(a.in, g, gy0 + d * (r0 + hw), d), x, d, g.W, nxt, g.border);
    for (int r = r0; r < r1; ++r) {
#pragma unroll
        for (int j = 0; j < K; ++j) raw[j] = nxt[j];
        wt_hrow_load<T, K, SMALL_D>(wt_row_b(a.in, g, gy0 + d * min(r + 1, r1 - 1) + d * hw, d), x, d, g.W, nxt, g.border);
        vert.emit(raw, a, (int64_t)(q + d * r) * g.P, x, true);
    }
}

// ---------------------------------------------------------------------------------------------
// K1c  "lattice" kernel: the chain march for LARGE dilations (d >= 256, wow() scales 8-10, where
// the x halo no longer fits a workgroup and the chain kernel pays K tap loads per row).  A thread
// owns C columns of the POLYPHASE LATTICE in x as well - pixel groups x0, x0+d, ..., x0+(C-1)d of its
// chain - so neighbouring lattice columns share taps in registers: C+K-1 row loads feed C
// horizontal filters (2 loads per output for C = 4 instead of 5).  Lanes run over the phase
// (consecutive pixels), so every load is still a coalesced 16 B per lane; reflection is per tap
// address as in the chain kernel, so any width / border mode works.  Arithmetic is WtVert per
// lattice column: bit-identical to the chain and row kernels.
// ---------------------------------------------------------------------------------------------
template <typename T, int K, int MODE, int C>
__global__ __launch_bounds__(256, 2) void WT_SK_NAME(wt_lattice)(WT_SK_PARAM(ChainArgsT<T>, a))
{
    WT_SK_FRAME(MODE, a);
    typedef typename WtVec<T>::V V;
    constexpr int PX = WtVec<T>::PX;
    constexpr int hw = K / 2;
    constexpr int NR = C + K - 1;                // row operands per step
    const Geo g = a.g;
    int bx, by;
    wt_xcd_remap(bx, by);
    const int d = a.d;
    const int p4 = d >> (PX == 4 ? 2 : 1);       // group phases per lattice column (d % PX == 0)
    const int t = bx * 64 + threadIdx.x;
    const int gi = t / p4, ph = t - gi * p4;
    const int x0 = PX * ph + d * C * gi;         // first lattice column of this thread
    if (x0 >= g.W) return;
    // one wave = one threadIdx.y: make the item (and with it the chain phase, the chunk, the row
    // pointers and the loop counters) scalar - the compiler cannot prove threadIdx.y wave-uniform
    const int item = __builtin_amdgcn_readfirstlane(by * blockDim.y + threadIdx.y);
    const int q = item % d;
    const int c = item / d;
    if (c >= a.chunks || q >= g.nrows) return;
    const int n_q = (g.nrows - q + d - 1) / d;
    const int r0 = c * a.S;
    const int r1 = min(r0 + a.S, n_q);
    if (r0 >= r1) return;

    // The operand columns do not depend on the row: with W % PX == 0 (host-checked) an aligned
    // group of PX pixels is either inside the image or entirely outside, and the symmetric
    // reflection of an outside group is an aligned group read backwards (even number of
    // bounces: forwards).  One offset and one flag per operand, no branches in the row loop.
    int off[NR];
    unsigned rev = 0;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int xo = x0 + (j - hw) * d;
        const int a0 = wt_refl(xo, g.W), a3 = wt_refl(xo + PX - 1, g.W);
        off[j] = min(a0, a3);
        if (a3 < a0) rev |= 1u << j;
    }
    WtVert<T, K, MODE, false> vert[C];
    const int gy0 = g.row0 + q;
    V lat[NR], nxt[NR];
    auto load_lat = [&](int r, V (&dst)[NR]) {
        const T *row = wt_row(a.in, g, gy0 + d * r);
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const V v = *reinterpret_cast<const V *>(row + off[j]);
            dst[j] = (rev >> j) & 1u ? wt_vrev(v) : v;
        }
    };
#pragma unroll
    for (int j = 0; j < K - 1; ++j) {
        load_lat(r0 - hw + j, lat);
#pragma unroll
        for (int cc = 0; cc < C; ++cc) vert[cc].prime(j, lat + cc, d);
    }
    load_lat(r0 + hw, nxt);
    for (int r = r0; r < r1; ++r) {
#pragma unroll
        for (int j = 0; j < NR; ++j) lat[j] = nxt[j];
        load_lat(min(r + 1, r1 - 1) + hw, nxt);
        const int64_t o = (int64_t)(q + d * r) * g.P;
#pragma unroll
        for (int cc = 0; cc < C; ++cc) vert[cc].emit(lat + cc, a, o, x0 + cc * d, x0 + cc * d < g.W);
    }
}

// ---------------------------------------------------------------------------------------------
// K1b  "row" kernel: the same single-scale operators for the dilations whose horizontal halo
// fits a workgroup (hw*d <= 1/8 of its width).  A workgroup of NW waves marches down one chunk
// of one polyphase chain like the fused pass: ONE coalesced 16-byte load per lane per row, the
// row is shared through LDS (double-buffered, one barrier per PAIR of rows) and the K dilated taps are
// LDS reads at lane offsets +-d/PX, +-2d/PX (or the two adjacent lanes for d < PX) - instead of K
// global loads per row.  Arithmetic is WtVert, i.e. bit-identical to the chain kernel.
// ---------------------------------------------------------------------------------------------
template <typename T, int K, int MODE, bool SMALL_D, int NW>
__global__ __launch_bounds__(NW * 64) void WT_SK_NAME(wt_row)(WT_SK_PARAM(RowArgsT<T>, ra))
{
    WT_SK_FRAME(MODE, ra);
    typedef typename WtVec<T>::V V;
    constexpr int PX = WtVec<T>::PX;
    constexpr int hw = K / 2;
    constexpr int NL = NW * 64;
    __shared__ V rowbuf[2][2][NL];                       // [pair parity][row of the pair][lane]
    const ChainArgsT<T> &a = ra.c;
    const Geo g = a.g;
    const int d = a.d;
    const int gl = threadIdx.x;
    const int X0 = blockIdx.x * ra.Vx;
    const int x = X0 - ra.HX + PX * gl;
    const int item = blockIdx.y;
    const int q = item % d;
    const int c = item / d;
    if (c >= a.chunks || q >= g.nrows) return;           // whole workgroup exits together
    const int n_q = (g.nrows - q + d - 1) / d;
    const int r0 = c * a.S;
    const int r1 = min(r0 + a.S, n_q);
    if (r0 >= r1) return;

    const bool lane_ok = (x >= X0) && (x < X0 + ra.Vx) && (x < g.W);
    const bool lane_interior = (x >= 0) && (x + PX - 1 < g.W);
    const bool wave_has_edge = !__all(lane_interior);
    const int xc = min(max(x, 0), g.P - PX);
    const int xi0 = wt_refl_b(x, g.W, d, g.border), xi1 = wt_refl_b(x + 1, g.W, d, g.border);
    int xi2 = 0, xi3 = 0;
    if constexpr (PX == 4) {
        xi2 = wt_refl_b(x + 2, g.W, d, g.border);
        xi3 = wt_refl_b(x + 3, g.W, d, g.border);
    }
    const int gy0 = g.row0 + q;
    const int t_last = r1 - 1 + hw;
    auto load_row = [&](int t) -> V {
        const T *row = wt_row_b(a.in, g, gy0 + d * min(t, t_last), d);
        V v = *reinterpret_cast<const V *>(row + xc);
        if (wave_has_edge) {
            if (!lane_interior) {
                if constexpr (PX == 4) v = make_float4(row[xi0], row[xi1], row[xi2], row[xi3]);
                else v = make_double2(row[xi0], row[xi1]);
            }
        }
        return v;
    };
    // taps of this lane out of the shared row (out-of-range lanes clamp: halo lanes only)
    const int lo = d / PX;                               // lane offset of one dilation step
    auto gather = [&](const V *rowv, V own, V (&raw)[K]) {
        if constexpr (SMALL_D) {
            raw[0] = rowv[max(gl - 1, 0)];
            raw[1] = own;
            raw[2] = rowv[min(gl + 1, NL - 1)];
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j)
                raw[j] = (j == hw) ? own : rowv[min(max(gl + (j - hw) * lo, 0), NL - 1)];
        }
    };

    WtVert<T, K, MODE, SMALL_D> vert;
    V raw[K];
    // Four rows in flight, in NAMED registers used in turn (the loop is unrolled by that many): a
    // rotating array (pf0 = pf1; pf1 = load) makes the compiler copy the load it has just issued at
    // the end of every iteration, i.e. wait for it at once - no prefetch left.
    // TWO ROWS PER BARRIER (round 3): the kernel sat at s_waitcnt / s_barrier for 72 % of its wave
    // cycles with one barrier per row (SQ_WAIT_ANY, profiles/r02_e) - four waves re-synchronising
    // every ~130 VALU instructions.  A step now shares a PAIR of rows through LDS (two row buffers
    // per parity) behind one barrier and filters both; same arithmetic per row, identical bits.
    V pfa = load_row(r0 - hw), pfb = load_row(r0 - hw + 1);
    V pfc = load_row(r0 - hw + 2), pfd = load_row(r0 - hw + 3);
    // steps t = r0-hw .. r1-1+hw ; the pair index selects the LDS buffers
    const int nsteps = (r1 - r0) + 2 * hw;
    auto share = [&](const int k, const V cur0, const V cur1, const V *&rv0, const V *&rv1) {
        V *w0 = rowbuf[(k >> 1) & 1][0], *w1 = rowbuf[(k >> 1) & 1][1];
        w0[gl] = cur0;
        w1[gl] = cur1;
        __syncthreads();
        rv0 = w0;
        rv1 = w1;
    };
    auto emit_row = [&](const int k, const V *rowv, const V cur) {
        gather(rowv, cur, raw);
        vert.emit(raw, a, (int64_t)(q + d * (r0 - 2 * hw + k)) * g.P, x, lane_ok);   // row t - hw, t = r0 - hw + k
    };
    auto pair_emit = [&](const int k, const V cur0, const V cur1) {
        const V *rv0, *rv1;
        share(k, cur0, cur1, rv0, rv1);
        emit_row(k, rv0, cur0);
        if (k + 1 < nsteps) emit_row(k + 1, rv1, cur1);      // workgroup-uniform
    };
    // warm-up rows k = 0 .. K-2 fill the window: (K-1)/2 pairs with STATIC window indices (a switch on
    // the run-time step number made the compiler index the window dynamically: scratch memory)
    {
        const V c0 = pfa, c1 = pfb;
        pfa = load_row(r0 - hw + 4);
        pfb = load_row(r0 - hw + 5);
        const V *rv0, *rv1;
        share(0, c0, c1, rv0, rv1);
        gather(rv0, c0, raw);
        vert.prime(0, raw, d);
        gather(rv1, c1, raw);
        vert.prime(1, raw, d);
    }
    {
        const V c0 = pfc, c1 = pfd;
        pfc = load_row(r0 - hw + 6);
        pfd = load_row(r0 - hw + 7);
        if constexpr (K > 3) {
            const V *rv0, *rv1;
            share(2, c0, c1, rv0, rv1);
            gather(rv0, c0, raw);
            vert.prime(2, raw, d);
            gather(rv1, c1, raw);
            vert.prime(3, raw, d);
        } else {
            pair_emit(2, c0, c1);                            // (nsteps >= 3: row 2 exists)
        }
    }
    for (int k = 4; k < nsteps; k += 4) {
        {
            const V c0 = pfa, c1 = pfb;
            pfa = load_row(r0 - hw + k + 4);
            pfb = load_row(r0 - hw + k + 5);
            pair_emit(k, c0, c1);
        }
        if (k + 2 < nsteps) {                                // workgroup-uniform
            const V c0 = pfc, c1 = pfd;
            pfc = load_row(r0 - hw + k + 6);
            pfd = load_row(r0 - hw + k + 7);
            pair_emit(k + 2, c0, c1);
        }
    }
}
