// The first stage of the {sum, sumsq, min, max} reduction (wt_reduce.h), included twice: as wt_reduce_kernel by
// wt_kernels_apps.h (one plane) and as wt_batch_reduce_kernel by wt_batch.hip (frame blockIdx.y of a batch, whose
// plane lies blockIdx.y * fstride floats after frame 0's; its partials in row blockIdx.y of gridDim.x blocks).  Two
// kernels from one text: the image kernel compiles to exactly the code it had before batches existed.
//   WT_REDUCE_KERNEL_NAME, WT_REDUCE_KERNEL_BATCH (0 / 1): set by the includer
// K7  {sum, sumsq, min, max}: fp64 sums, deterministic two-stage reduction (per-block partials
// over whole rows, then one block folds them in a fixed order).  Rows are walked with 2-D
// indices (no 64-bit modulo per element); min/max are taken in fp32, which is exact.
// Round 4: four 16-byte loads in flight per thread feeding four independent accumulator sets (folded
// in a fixed order at the end), nontemporal loads, 8 blocks per CU - the one-load loop with its
// dependent fp64 chains kept 16 KB in flight per CU and streamed at 0.52 of the HBM rate.
__global__ __launch_bounds__(256) void WT_REDUCE_KERNEL_NAME(const float *p, int nrows, int P4, int W,
#if WT_REDUCE_KERNEL_BATCH
                                                              int64_t fstride,
#endif
                                                              double *partials)
{
#if WT_REDUCE_KERNEL_BATCH
    p += (int64_t)blockIdx.y * fstride;
    partials += (int64_t)blockIdx.y * gridDim.x * 4;
#endif
    constexpr int U = 4;
    double sa[U] = {0.0, 0.0, 0.0, 0.0}, sb[U] = {0.0, 0.0, 0.0, 0.0};
    float mn = INFINITY, mx = -INFINITY;
    const int X4 = (W + 3) >> 2;
    // work items are (row, chunk of 256 * U float4) pairs dealt round-robin to the blocks (a fixed
    // assignment: deterministic sums); the loads of the NEXT item are issued before the current one is
    // folded - 8 loads of 16 B in flight per thread, as in the select passes
    const int nchunk = (X4 + 256 * U - 1) / (256 * U);
    const int64_t nitems = (int64_t)nrows * nchunk;
    auto load = [&](int64_t item, float4 (&v)[U]) {
        const int r = (int)(item / nchunk), c = (int)(item - (int64_t)r * nchunk);
        const float *row = p + (int64_t)r * P4 * 4;
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = wt_ldnt4(row + 4 * min(c * 256 * U + 256 * u + (int)threadIdx.x, X4 - 1));
    };
    auto fold = [&](int64_t item, const float4 (&v)[U]) {
        const int c = (int)(item % nchunk);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int xx = c * 256 * U + 256 * u + (int)threadIdx.x;
            const int nv = xx < X4 ? min(4, W - xx * 4) : 0;
            const float b[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) {
                    const double t = (double)b[k];
                    sa[u] += t;
                    sb[u] = fma(t, t, sb[u]);
                    mn = fminf(mn, b[k]);
                    mx = fmaxf(mx, b[k]);
                }
        }
    };
    float4 va[U], vb[U];
    int64_t item = blockIdx.x;
    if (item < nitems) load(item, va);
    while (item < nitems) {
        const int64_t i1 = item + gridDim.x, i2 = i1 + gridDim.x;
        if (i1 < nitems) load(i1, vb);
        fold(item, va);
        if (i1 >= nitems) break;
        if (i2 < nitems) load(i2, va);
        fold(i1, vb);
        item = i2;
    }
    double s = (sa[0] + sa[1]) + (sa[2] + sa[3]), s2 = (sb[0] + sb[1]) + (sb[2] + sb[3]);
    __shared__ double red[4][2];
    __shared__ float redf[4][2];
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off);
        s2 += __shfl_down(s2, off);
        mn = fminf(mn, __shfl_down(mn, off));
        mx = fmaxf(mx, __shfl_down(mx, off));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave][0] = s; red[wave][1] = s2; redf[wave][0] = mn; redf[wave][1] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            s += red[w][0]; s2 += red[w][1];
            mn = fminf(mn, redf[w][0]); mx = fmaxf(mx, redf[w][1]);
        }
        double *o = partials + (int64_t)blockIdx.x * 4;
        o[0] = s; o[1] = s2; o[2] = (double)mn; o[3] = (double)mx;
    }
}
