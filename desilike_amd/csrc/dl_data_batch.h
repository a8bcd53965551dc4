// dl_data_batch.h -- log-posteriors of a batch of points against a BATCH of data vectors (include/desilike_amd.h: dl_data_set, dl_eval_logposterior_data).
//
// The data enter the whitened residual d~ = W~ . power + L^T (bias - flatdata) through its additive term only: with y_b = W~ . power_b (the split-K slabs of the
// window GEMM, or the rows of the feature GEMM: what the theory side leaves in the residual workspace BEFORE any bias) and bias_m = L^T (bias - flatdata_m),
//     chi2(b, m) = sum_j (y_bj + bias_mj)^2,
// one theory evaluation and one GEMM per point, whatever the number of data vectors.  The sum is formed by DIRECT DIFFERENCES: expanded into |y|^2 + 2 y . bias + |bias|^2
// its terms are 1e5 - 1e6 where chi2 is 1e2, and the cancellation would cost four to five of the sixteen digits.
//
// Order of the arithmetic (a function of n and of the number of slabs only: not of the tile, the batch, the number of data vectors or the kernel):
//   y_bj   = the slabs of column j summed as dl_finalize_kernel does (groups of eight slabs as balanced trees, group after group), starting from zero;
//   d_j    = y_bj + bias_mj;
//   p_q    = fma(d_j, d_j, p_q) over the columns j = q, q + 8, q + 16 .. < n in increasing order, q = 0 .. 7 (DL_DB_NP independent chains);
//   chi2   = ((p_0 + p_1) + (p_2 + p_3)) + ((p_4 + p_5) + (p_6 + p_7));
//   logprior = the terms of dl_prior_logpdf added parameter after parameter.
// Both kernels are built from the functions below, so that cross[b, m] and paired[b] with index m are the same bits; tests/csrc/emulate_data_batch.cpp compiles the
// same functions with g++ and runs them on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dl_fullshape.h"

#define DL_DB_NP 8       // partial sums of one pair
#define DL_DB_TB 32      // points of a tile of the cross kernel
#define DL_DB_TM 32      // data vectors of a tile
#define DL_DB_JC 64      // columns staged at a time by the cross kernel (a multiple of DL_DB_NP)
#define DL_DB_PC 512     // columns staged at a time by a wavefront of the paired kernel (a multiple of DL_DB_NP)
#define DL_DB_MAX_M 65536

// column j of the residual row before the bias: `col` points at the entry of slab 0.  T: double, or the 16-byte pair of columns (j, j + 1) of dl_data_resid_kernel
// (the same tree on each component; slab_stride in units of T)
template <typename T>
DL_HD T dl_db_slab_sum_t(const T* col, int n_slabs, int64_t slab_stride) {
    T v = (T)0.;
    int sl = 0;
    for (; sl + 8 <= n_slabs; sl += 8) {
        T t[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = col[(size_t)(sl + q) * slab_stride];
        v += ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
    }
    T t[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) t[q] = sl + q < n_slabs ? col[(size_t)(sl + q) * slab_stride] : (T)0.;
    v += ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
    return v;
}

DL_HD double dl_db_slab_sum(const double* col, int n_slabs, int64_t slab_stride) { return dl_db_slab_sum_t<double>(col, n_slabs, slab_stride); }

// entry j of the whitened residual row of a (point, data vector) pair from y_bj (dl_db_slab_sum) and bias_mj: the d_j whose squares dl_db_step sums
template <typename T>
DL_HD T dl_db_resid(T y, T bias) { return y + bias; }

// one column of one pair: partial sum p of the chain the column belongs to (j % DL_DB_NP)
DL_HD void dl_db_step(double& p, double y, double bias) {
    const double d = dl_db_resid(y, bias);
    p = fma(d, d, p);
}

// Live entry (j < n) of the residual row of a point against data vector m (dl_data_resid_kernel; the analytic derivative paths with a data batch,
// dl_eval_fisher_analytic_data and dl_eval_logposterior_grad_data): `col` points at the entry of the point in slab 0, `bias` at the entry of the data vector's row of
// the table, or is NULL for a point whose CHECKED index (dl_data_index_kernel) is -1: NaN, and the table is not read.  T as in dl_db_slab_sum_t.
template <typename T>
DL_HD T dl_db_resid_entry(const T* col, int n_slabs, int64_t slab_stride, const T* bias) {
    if (!bias) return (T)__builtin_nan("");
    return dl_db_resid(dl_db_slab_sum_t<T>(col, n_slabs, slab_stride), *bias);
}

// Columns (j, j + 1), j even, of that row as one 16-byte value: the work of one thread of dl_data_resid_kernel.  `row`: the point's row of slab 0; `brow`: the data
// vector's row of the table, NULL for a checked index of -1.  Columns >= n are exact zeros: the pair at or beyond n reads nothing, the pair that straddles n (n odd)
// reads both of its columns -- column n < N_pad lies inside the rows -- and zeroes the second.  T2: two doubles .x, .y with + (the device's vector; a struct on the CPU).
template <typename T2>
DL_HD T2 dl_db_resid_pair(const double* row, int n_slabs, int64_t slab_stride, const double* brow, int j, int n) {
    T2 v = (T2)0.;
    if (j < n) {
        v = dl_db_resid_entry<T2>(reinterpret_cast<const T2*>(row + j), n_slabs, slab_stride >> 1, brow ? reinterpret_cast<const T2*>(brow + j) : nullptr);
        if (j + 1 >= n) v.y = 0.;
    }
    return v;
}

// The whole row, column after column: what dl_data_resid_kernel distributes over its lanes, two columns each (tests/csrc/emulate_data_resid.cpp runs this on the
// CPU).  `row`: the point's row of slab 0; m: its checked index; columns [n, N_pad) are exact zeros (the Gram kernel and the second GEMM of the gradient read them).
DL_HD void dl_db_resid_row(const double* row, int n_slabs, int64_t slab_stride, const double* bias_tab, int64_t ldb, int m, int n, int N_pad, double* out) {
    for (int j = 0; j < N_pad; ++j)
        out[j] = j < n ? dl_db_resid_entry<double>(row + j, n_slabs, slab_stride, m < 0 ? nullptr : bias_tab + (size_t)m * ldb + j) : 0.;
}

DL_HD double dl_db_tree(const double* p) { return ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7])); }

// chi2 of one pair from the residual row before the bias y [n] and the whitened bias of the data vector [n]: the statement the kernels distribute over lanes
DL_HD double dl_db_pair_chi2(const double* y, const double* bias, int n) {
    double p[DL_DB_NP];
    for (int q = 0; q < DL_DB_NP; ++q) p[q] = 0.;
    for (int j0 = 0; j0 < n; j0 += DL_DB_NP)
        for (int q = 0; q < DL_DB_NP && j0 + q < n; ++q) dl_db_step(p[q], y[j0 + q], bias[j0 + q]);
    return dl_db_tree(p);
}

#if defined(__HIPCC__) && !defined(DL_DB_NO_KERNELS)   // (DL_DB_NO_KERNELS: the functions above alone, for dl_data_batch_marg.h in dl_kernels.hip)
#include "dl_kernels.h"
#include "dl_prior.h"

// log-prior and NaN flag of one point by ONE lane
__device__ __forceinline__ double dl_db_logprior(const double* __restrict__ theta_row, const double* __restrict__ priors, int n_params, int& nan_in) {
    double lp = 0.;
    nan_in = 0;
    for (int p = 0; p < n_params; ++p) {
        const double x = theta_row[p];
        if (x != x) nan_in = 1;
        lp += dl_prior_logpdf(priors + 5 * p, x);
    }
    return lp;
}

// log-posterior of a pair with the conventions of dl_eval_logposterior (post_mode of dl_finalize_kernel)
__device__ __forceinline__ double dl_db_logposterior(double chi2, double lp, int nan_in, int& st) {
    const double inf = __builtin_huge_val();
    const double ll = -0.5 * chi2;
    st = DL_ST_OK;
    if (nan_in) st = DL_ST_NAN_INPUT;
    else if (lp == -inf) st = DL_ST_OUT_OF_PRIOR;
    else if (!(ll == ll) || ll == inf || ll == -inf) st = DL_ST_NONFINITE;
    return st == DL_ST_OK ? ll + lp : -inf;
}

typedef double dl_db_double2 __attribute__((ext_vector_type(2)));

// Cross: out[b, m] for a tile of DL_DB_TB points x DL_DB_TM data vectors per workgroup; thread (tb, tm) owns the 2 x 2 pairs (2 tb + {0, 1}, 2 tm + {0, 1}).  The y rows
// (slabs summed once per point and tile) and the bias rows are staged transposed in LDS, DL_DB_JC columns at a time: one 16-byte read of each per column and thread
// feeds four pairs.  Columns beyond n and rows beyond B / M are staged as zeros (d = 0 leaves a partial sum as it is); nothing outside [0, B) x [0, M) is read or
// written.  Priors and the point's flags: once per point of the tile, by one thread.  status (may be null) is written by the tiles of data vector 0: NaN input,
// out of prior, or a likelihood that is not finite against data vector 0 (the data are finite: dl_data_set checks them, so this is a property of the point).
__global__ __launch_bounds__(256) void dl_data_cross_kernel(const double* __restrict__ dtilde, int64_t ld, int n, int n_slabs, int64_t slab_stride,
                                                            const double* __restrict__ bias_tab, int64_t ldb, int M, const double* __restrict__ theta, int n_params,
                                                            const double* __restrict__ priors, int64_t B, double* __restrict__ out, int32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) double yT[DL_DB_JC][DL_DB_TB + 2];   // (+2 doubles: 16-byte aligned rows that do not all start on one bank)
    __shared__ __attribute__((aligned(16))) double bT[DL_DB_JC][DL_DB_TM + 2];
    __shared__ double lp_s[DL_DB_TB];
    __shared__ int nan_s[DL_DB_TB];
    const int tid = threadIdx.x, tm = tid & 15, tb = tid >> 4;
    const int64_t b0 = (int64_t)blockIdx.x * DL_DB_TB;
    const int m0 = (int)blockIdx.y * DL_DB_TM;
    if (tid < DL_DB_TB) {
        int nan_in = 0;
        double lp = 0.;
        if (b0 + tid < B) lp = dl_db_logprior(theta + (size_t)(b0 + tid) * n_params, priors, n_params, nan_in);
        lp_s[tid] = lp;
        nan_s[tid] = nan_in;
    }
    double p[2][2][DL_DB_NP];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int q = 0; q < DL_DB_NP; ++q) p[i][k][q] = 0.;
    for (int base = 0; base < n; base += DL_DB_JC) {
        // stage: element e = tid + 256 s -> column e % 64 (consecutive lanes read consecutive columns of one row), row e / 64
#pragma unroll
        for (int s = 0; s < DL_DB_TB * DL_DB_JC / 256; ++s) {
            const int e = tid + 256 * s, c = e & (DL_DB_JC - 1), r = e / DL_DB_JC, j = base + c;
            const int64_t b = b0 + r;
            yT[c][r] = (b < B && j < n) ? dl_db_slab_sum(dtilde + (size_t)b * ld + j, n_slabs, slab_stride) : 0.;
        }
#pragma unroll
        for (int s = 0; s < DL_DB_TM * DL_DB_JC / 256; ++s) {
            const int e = tid + 256 * s, c = e & (DL_DB_JC - 1), r = e / DL_DB_JC, j = base + c;
            const int m = m0 + r;
            bT[c][r] = (m < M && j < n) ? bias_tab[(size_t)m * ldb + j] : 0.;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < DL_DB_JC; ++c) {
            const dl_db_double2 y2 = *reinterpret_cast<const dl_db_double2*>(&yT[c][2 * tb]);
            const dl_db_double2 b2 = *reinterpret_cast<const dl_db_double2*>(&bT[c][2 * tm]);
            dl_db_step(p[0][0][c % DL_DB_NP], y2.x, b2.x);
            dl_db_step(p[0][1][c % DL_DB_NP], y2.x, b2.y);
            dl_db_step(p[1][0][c % DL_DB_NP], y2.y, b2.x);
            dl_db_step(p[1][1][c % DL_DB_NP], y2.y, b2.y);
        }
        __syncthreads();   // (the chunk has been read: the next one may overwrite it; with n = 0 the barrier after the priors below is the only one)
    }
    if (n <= 0) __syncthreads();   // lp_s / nan_s of the other threads
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int64_t b = b0 + 2 * tb + i;
            const int m = m0 + 2 * tm + k;
            if (b >= B || m >= M) continue;
            int st;
            const double v = dl_db_logposterior(dl_db_tree(p[i][k]), lp_s[2 * tb + i], nan_s[2 * tb + i], st);
            out[(size_t)b * M + m] = v;
            if (status && m == 0) status[b] = st;
        }
}

// Paired: out[b] against data vector index[b]; one wavefront per point (dl_finalize_kernel with the bias row chosen by the index).  The lanes sum the slabs of
// DL_DB_PC columns into the wavefront's LDS row, lanes 0 .. 7 then run the eight chains of dl_db_pair_chi2 over it: the order of the cross kernel.
// An index outside [0, M): NaN and DL_STATUS_NAN_INPUT; the table is not read for that row.
__global__ __launch_bounds__(256) void dl_data_paired_kernel(const double* __restrict__ dtilde, int64_t ld, int n, int n_slabs, int64_t slab_stride,
                                                             const double* __restrict__ bias_tab, int64_t ldb, int M, const int32_t* __restrict__ index,
                                                             const double* __restrict__ theta, int n_params, const double* __restrict__ priors, int64_t B,
                                                             double* __restrict__ out, int32_t* __restrict__ status) {
    __shared__ double ybuf[4][DL_DB_PC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= B) return;   // (whole wavefronts leave: no workgroup barrier below)
    const int m = index[b];
    const bool bad = m < 0 || m >= M;
    const double* brow = bias_tab + (size_t)(bad ? 0 : m) * ldb;
    const double* row = dtilde + (size_t)b * ld;
    double* yw = ybuf[wave];
    double pq = 0.;
    for (int base = 0; base < n; base += DL_DB_PC) {
        const int width = n - base < DL_DB_PC ? n - base : DL_DB_PC;
        for (int c = lane; c < width; c += 64) yw[c] = dl_db_slab_sum(row + base + c, n_slabs, slab_stride);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane < DL_DB_NP && !bad)
            for (int c = lane; c < width; c += DL_DB_NP) dl_db_step(pq, yw[c], brow[base + c]);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();   // the chunk has been read: the next one may overwrite it
    }
    double p[DL_DB_NP];
#pragma unroll
    for (int q = 0; q < DL_DB_NP; ++q) p[q] = __shfl(pq, q, 64);
    if (lane == 0) {
        int nan_in, st;
        const double lp = dl_db_logprior(theta + (size_t)b * n_params, priors, n_params, nan_in);
        double v = dl_db_logposterior(dl_db_tree(p), lp, nan_in, st);
        if (bad) { v = __builtin_nan(""); st = DL_ST_NAN_INPUT; }
        out[b] = v;
        if (status) status[b] = st;
    }
}

// index [B] -> checked [B]: the index where it lies in [0, M), else -1 (the Fisher kernel then puts NaN in its residual row instead of reading the table)
__global__ void dl_data_index_kernel(const int32_t* __restrict__ index, int64_t B, int M, int32_t* __restrict__ checked) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int m = index[b];
    checked[b] = (m >= 0 && m < M) ? m : -1;
}

// Residual rows of (point, data vector) pairs: resid[b][j] = dl_db_resid_row of point b against data vector checked[b], for the kernels that take d~ as a given row
// (dl_fisher_kernel<TILES, GIVEN = true>, the second GEMM of the analytic gradient).  One thread per 16 bytes of the output: thread t of the launch owns columns
// (2 c, 2 c + 1) of row b with b = t / (N_pad / 2), c = t % (N_pad / 2) -- consecutive lanes read consecutive 16 bytes of every slab and of the bias row and write
// consecutive 16 bytes; a wavefront covers one row of N_pad = 128, so B = 1 is one wavefront of a workgroup whose other three leave at once.  N_pad is even and the
// rows (ld, slab_stride, ldb, ldr: even, bases from hipMalloc) are 16-byte aligned.  No LDS: every input byte is used once.  Nothing outside [0, B) x [0, N_pad) is
// read from the slabs or written; columns >= n are written as zeros without a read, the pair that straddles n reads both of its columns (inside the row) and zeroes
// the second; the table is read for rows with checked[b] >= 0 only.
__global__ __launch_bounds__(256) void dl_data_resid_kernel(const double* __restrict__ dtilde, int64_t ld, int n, int n_slabs, int64_t slab_stride,
                                                            const double* __restrict__ bias_tab, int64_t ldb, const int32_t* __restrict__ checked, int64_t B, int N_pad,
                                                            double* __restrict__ resid, int64_t ldr) {
    const int half = N_pad >> 1;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t b = t / half;
    if (b >= B) return;
    const int j = 2 * (int)(t - b * half);
    const int m = checked[b];
    *reinterpret_cast<dl_db_double2*>(resid + (size_t)b * ldr + j) =
        dl_db_resid_pair<dl_db_double2>(dtilde + (size_t)b * ld, n_slabs, slab_stride, m < 0 ? nullptr : bias_tab + (size_t)m * ldb, j, n);
}

static void dl_launch_data_resid(const double* dtilde, int64_t ld, int n, int n_slabs, int64_t slab_stride, const double* bias_tab, int64_t ldb, const int32_t* checked,
                                 int64_t B, int N_pad, double* resid, int64_t ldr, hipStream_t stream) {
    const int64_t threads = B * (N_pad / 2);
    DL_LAUNCH(dl_data_resid_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, dtilde, ld, n, n_slabs, slab_stride, bias_tab, ldb, checked, B, N_pad,
              resid, ldr);
}

// out: [B, M] (index == nullptr: cross) or [B] (paired)
static void dl_launch_data_finalize(const double* dtilde, int64_t ld, int n, int n_slabs, int64_t slab_stride, const double* bias_tab, int64_t ldb, int M, const int32_t* index,
                                    const double* theta, int n_params, const double* priors, int64_t B, double* out, int32_t* status, hipStream_t stream) {
    if (index)
        DL_LAUNCH(dl_data_paired_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, dtilde, ld, n, n_slabs, slab_stride, bias_tab, ldb, M, index, theta, n_params,
                  priors, B, out, status);
    else
        DL_LAUNCH(dl_data_cross_kernel, dim3((unsigned)((B + DL_DB_TB - 1) / DL_DB_TB), (unsigned)((M + DL_DB_TM - 1) / DL_DB_TM)), dim3(256), 0, stream, dtilde, ld, n,
                  n_slabs, slab_stride, bias_tab, ldb, M, theta, n_params, priors, B, out, status);
}

static void dl_launch_data_index(const int32_t* index, int64_t B, int M, int32_t* checked, hipStream_t stream) {
    DL_LAUNCH(dl_data_index_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, index, B, M, checked);
}
#endif
