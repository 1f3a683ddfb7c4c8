// Outer product of gradients: B[i][j] = sum_n s_ni s_nj of the per-track scores s[N][n] the forward-mode gradient kernels leave in
// device memory (XtBucketDesc::scores_out).  Tracks are independent, so B estimates the Fisher information of the fitted parameters and
// its inverse their covariance (BHHH); the host never sees the N x n matrix unless it asks for it.
//
// Two stages, both in a fixed order (no floating-point atomics: the result depends on N and n only, not on the device or the run):
//   1. one workgroup per tile of XT_OPG_TILE rows.  The tile passes through LDS in chunks of XT_OPG_CHUNK rows; the n (n + 1) / 2 pairs
//      i <= j of the upper triangle are dealt over the threads, and where there are fewer pairs than threads every pair is served by
//      several threads that take the rows r = slice, slice + nslice, ... of a chunk ("slices").  The slices of a pair are then summed in
//      slice order: partials[tile][pair].
//   2. one workgroup per pair sums the tiles (the pattern of xt_grad_reduce) and writes B[col[i]][col[j]] and its mirror image - the
//      score matrix is in the launch order of the directions, col[] gives the caller's index of every column.
#pragma once
#include <stdint.h>

#define XT_OPG_MAXDIR 32
#define XT_OPG_TILE 1024   // rows per first-stage workgroup (= EXTRACK_OPG_TILE of the public header)
#define XT_OPG_CHUNK 128   // rows in LDS at a time: 128 x 32 doubles = 32 KiB
#define XT_OPG_THREADS 256
#define XT_OPG_ITEMS 3     // (pair, slice) items per thread: ceil(528 / 256)

struct XtOpgCols {
    int32_t idx[XT_OPG_MAXDIR];
};

__host__ __device__ inline int xt_opg_pairs(int n) { return n * (n + 1) / 2; }
// pair index p (row-major over the upper triangle) -> (i, j), i <= j
__host__ __device__ inline void xt_opg_pair(int n, int p, int& i, int& j)
{
    i = 0;
    while (p >= n - i) {
        p -= n - i;
        ++i;
    }
    j = i + p;
}

__global__ void __launch_bounds__(XT_OPG_THREADS) xt_opg_partial_kernel(const double* __restrict__ scores, int64_t N, int n, double* __restrict__ partials)
{
    __shared__ double sh[XT_OPG_CHUNK * XT_OPG_MAXDIR];
    const int tid = threadIdx.x;
    const int npairs = xt_opg_pairs(n);
    const int nslice = npairs < XT_OPG_THREADS ? XT_OPG_THREADS / npairs : 1;
    const int nitems = npairs * nslice;  // <= XT_OPG_ITEMS * XT_OPG_THREADS
    int pi[XT_OPG_ITEMS], pj[XT_OPG_ITEMS], ps[XT_OPG_ITEMS];
    double acc[XT_OPG_ITEMS];
#pragma unroll
    for (int k = 0; k < XT_OPG_ITEMS; ++k) {
        const int item = tid + k * XT_OPG_THREADS;
        acc[k] = 0.0;
        pi[k] = pj[k] = 0;
        ps[k] = XT_OPG_CHUNK;  // no row of a chunk: an idle item
        if (item < nitems) {
            xt_opg_pair(n, item % npairs, pi[k], pj[k]);
            ps[k] = item / npairs;
        }
    }
    const int64_t row0 = (int64_t)blockIdx.x * XT_OPG_TILE;
    const int64_t rows = N - row0 < XT_OPG_TILE ? N - row0 : XT_OPG_TILE;
    for (int64_t c0 = 0; c0 < rows; c0 += XT_OPG_CHUNK) {
        const int nr = (int)(rows - c0 < XT_OPG_CHUNK ? rows - c0 : XT_OPG_CHUNK);
        const double* src = scores + (row0 + c0) * n;  // nr rows of n doubles, contiguous
        for (int i = tid; i < nr * n; i += XT_OPG_THREADS) sh[i] = src[i];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < XT_OPG_ITEMS; ++k)
            for (int r = ps[k]; r < nr; r += nslice) acc[k] = fma(sh[r * n + pi[k]], sh[r * n + pj[k]], acc[k]);
        __syncthreads();
    }
    // slices of a pair -> one number, in slice order
    double* red = sh;  // [nitems] <= 768 doubles
#pragma unroll
    for (int k = 0; k < XT_OPG_ITEMS; ++k) {
        const int item = tid + k * XT_OPG_THREADS;
        if (item < nitems) red[item] = acc[k];
    }
    __syncthreads();
    for (int p = tid; p < npairs; p += XT_OPG_THREADS) {
        double s = 0.0;
        for (int sl = 0; sl < nslice; ++sl) s += red[sl * npairs + p];
        partials[(int64_t)blockIdx.x * npairs + p] = s;
    }
}

__global__ void __launch_bounds__(256) xt_opg_reduce_kernel(const double* __restrict__ partials, int ntiles, int n, double* __restrict__ B, XtOpgCols cols)
{
    __shared__ double sh[256];
    const int npairs = xt_opg_pairs(n);
    const int p = blockIdx.x;
    double s = 0.0;
    for (int t = threadIdx.x; t < ntiles; t += 256) s += partials[(int64_t)t * npairs + p];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int i, j;
        xt_opg_pair(n, p, i, j);
        const int ci = cols.idx[i], cj = cols.idx[j];
        B[ci * n + cj] = sh[0];
        B[cj * n + ci] = sh[0];
    }
}

inline int64_t xt_opg_tiles(int64_t N) { return (N + XT_OPG_TILE - 1) / XT_OPG_TILE; }
// scores [N][n] (device) -> B [n][n] (device); partials: xt_opg_tiles(N) * xt_opg_pairs(n) doubles of scratch
inline void xt_opg_launch(hipStream_t st, const double* scores, int64_t N, int n, double* partials, double* B, const XtOpgCols& cols)
{
    const int ntiles = (int)xt_opg_tiles(N);
    hipLaunchKernelGGL(xt_opg_partial_kernel, dim3(ntiles), dim3(XT_OPG_THREADS), 0, st, scores, N, n, partials);
    hipLaunchKernelGGL(xt_opg_reduce_kernel, dim3(xt_opg_pairs(n)), dim3(256), 0, st, partials, ntiles, n, B, cols);
}
