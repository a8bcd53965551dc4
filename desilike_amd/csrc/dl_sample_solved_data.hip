// dl_sample_solved_data.hip -- the draw kernel of dl_sample_solved_data (dl_sample_solved_data.h states the arithmetic and the random draws) and its launcher.
#include <type_traits>

#include "dl_kernels.h"
#define DL_DB_NO_KERNELS   // (dl_data_batch.h: its reduction functions alone)
#include "dl_sample_solved_data.h"

// ONE WAVEFRONT PER POINT, four points per workgroup, modelled on dl_dbm_paired_kernel.
//   Row phase: that kernel's, in its order -- d = y + bias_m through the wavefront's LDS row, lanes 0 .. 7 the eight chains of G00, lane 8 + s the chain of gd_s, the
//   partials gathered by __shfl -- so that x0 + dx has the bits dl_eval_solved_data returns for the row.
//   Then EVERY lane runs dl_dbm_pair_finish on the same inputs (uniform: the wave index is made a scalar, so the record is read through the scalar cache), and the
//   draws are spread over the lanes: lane l owns draws l, l + 64, ..; a point with size <= 64 costs one trip.
//   The factor C | 1 / C_ii is staged once into the wavefront's LDS and read from there by all lanes at the same address (broadcast): no per-lane triangle in registers.
// Wavefront b writes [b, b + 1) x size of the three outputs and status[b], nothing else.  An index outside [0, M): the table is not read for that row.
template <int NSP>
__global__ __launch_bounds__(256) void dl_dbm_draw_kernel(const double* __restrict__ rows_ws, int64_t ld, int n, int rows_per_point, const double* __restrict__ rec_ws,
                                                          DlMargDev mg, DlDbmConst kc, const double* __restrict__ bias_tab, int64_t ldb, int M,
                                                          const int32_t* __restrict__ index, int64_t B, int64_t index0, int size, uint32_t k0, uint32_t k1,
                                                          double* __restrict__ solved_out, double* __restrict__ loglike_out, double* __restrict__ logprior_out,
                                                          int32_t* __restrict__ status) {
    __shared__ double dbuf[4][64 * DL_MARG_NJ];   // (n <= 512: the limit of solved contexts)
    __shared__ double fbuf[4][DL_SSD_FAC];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= B) return;   // (whole wavefronts leave: no workgroup barrier below)
    const int ns = mg.n_s;
    const int m = index[b];
    const bool bad = m < 0 || m >= M;
    const double* brow = bias_tab + (size_t)(bad ? 0 : m) * ldb;
    const double* yrow = rows_ws + (size_t)b * rows_per_point * ld;
    const double* rec = rec_ws + (size_t)b * DL_DBM_REC;
    double* dw = dbuf[wave];
    double* fw = fbuf[wave];
    double pq = 0., gs = 0.;
    if (!bad) {
        for (int c = lane; c < n; c += 64) dw[c] = yrow[c];
    }
    for (int e = lane; e < DL_SSD_FAC; e += 64) fw[e] = rec[DL_DBM_C + e];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (!bad) {
        if (lane < DL_DB_NP) {
            for (int c = lane; c < n; c += DL_DB_NP) dl_db_step(pq, dw[c], brow[c]);
        } else if (lane < DL_DB_NP + ns) {
            const double* trow = dl_dbm_trow(mg, lane - DL_DB_NP, rows_ws, b, rows_per_point, ld);
            for (int c = 0; c < n; ++c) {
                const double d = dw[c] + brow[c];
                gs = fma(trow[c], d, gs);
            }
        }
    }
    double p[DL_DB_NP], g[NSP];
#pragma unroll
    for (int q = 0; q < DL_DB_NP; ++q) p[q] = __shfl(pq, q, 64);
#pragma unroll
    for (int s = 0; s < NSP; ++s) g[s] = __shfl(gs, DL_DB_NP + s, 64);
    double ll, lps, dx[NSP];
    dl_dbm_pair_finish<NSP>(dl_db_tree(p), g, rec, kc, ll, lps, dx);
    const int st = dl_ssd_status(rec, ll, bad);
    if (status && lane == 0) status[b] = st;
    const double hld = rec[DL_DBM_HLD], lpp = rec[DL_DBM_LP] + lps;
    double* xo = solved_out + (size_t)b * size * ns;
    double* lo = loglike_out + (size_t)b * size;
    double* po = logprior_out + (size_t)b * size;
    for (int d = lane; d < size; d += 64) {
        double x[NSP], loglike, logprior;
        if (st == 0) dl_ssd_draw<NSP>(fw, hld, kc, ns, dx, ll, lpp, index0 + b, (uint32_t)d, k0, k1, x, loglike, logprior);
        else {
            loglike = logprior = __builtin_nan("");
#pragma unroll
            for (int s = 0; s < NSP; ++s) x[s] = __builtin_nan("");
        }
#pragma unroll
        for (int s = 0; s < NSP; ++s)
            if (s < ns) xo[(size_t)d * ns + s] = x[s];
        lo[d] = loglike;
        po[d] = logprior;
    }
}

template <int NSP>
static void dl_ssd_launch(const DlMargDev& mg, const DlDbmConst& kc, const double* rows_ws, int64_t ld, int n, int rows_per_point, const double* rec_ws, const double* bias_tab,
                          int64_t ldb, int M, const int32_t* index, int64_t B, int64_t index0, int size, uint64_t seed, double* solved_out, double* loglike_out,
                          double* logprior_out, int32_t* status, hipStream_t stream) {
    DL_LAUNCH(dl_dbm_draw_kernel<NSP>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, rows_ws, ld, n, rows_per_point, rec_ws, mg, kc, bias_tab, ldb, M, index, B, index0, size,
              (uint32_t)seed, (uint32_t)(seed >> 32), solved_out, loglike_out, logprior_out, status);
}

void dl_launch_data_marg_draw(const DlMargDev& mg, const double* rows_ws, int64_t ld, int n, int rows_per_point, const double* rec_ws, const double* bias_tab, int64_t ldb, int M,
                              const int32_t* index, int64_t B, int64_t index0, int size, uint64_t seed, double* solved_out, double* loglike_out, double* logprior_out,
                              int32_t* status, hipStream_t stream) {
    if (B <= 0 || size <= 0) return;
    const int ns = mg.n_s;
    DlDbmConst kc;
    for (int s = 0; s < DL_MAX_SOLVED; ++s) { kc.x0[s] = s < ns ? mg.x0[s] : 0.; kc.loc[s] = s < ns ? mg.loc[s] : 0.; kc.prec[s] = s < ns ? mg.prec[s] : 0.; }
    auto launch = [&](auto tag) {
        dl_ssd_launch<decltype(tag)::value>(mg, kc, rows_ws, ld, n, rows_per_point, rec_ws, bias_tab, ldb, M, index, B, index0, size, seed, solved_out, loglike_out, logprior_out,
                                            status, stream);
    };
    switch (dl_dbm_nsp(ns)) {   // the nine sizes of dl_launch_data_marg
        case 1: launch(std::integral_constant<int, 1>()); break;
        case 2: launch(std::integral_constant<int, 2>()); break;
        case 3: launch(std::integral_constant<int, 3>()); break;
        case 4: launch(std::integral_constant<int, 4>()); break;
        case 5: launch(std::integral_constant<int, 5>()); break;
        case 6: launch(std::integral_constant<int, 6>()); break;
        case 8: launch(std::integral_constant<int, 8>()); break;
        case 12: launch(std::integral_constant<int, 12>()); break;
        default: launch(std::integral_constant<int, 16>()); break;
    }
}
