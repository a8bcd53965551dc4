// dl_sample_solved_data.h -- posterior draws of the analytically solved parameters of a point given ONE data vector of a data batch (include/desilike_amd.h:
// dl_sample_solved_data): the consumer of the per-point record and of the per-pair arithmetic of dl_data_batch_marg.h that dl_sample_solved.h is for a context's own
// data vector.
//
// Per pair (b, m), from dl_dbm_pair_finish (dx, ll, lps) and the record of the point (C with A = H + diag(prec) = C C^T, 1 / C_ii, 1/2 logdet A[marg, marg], lp):
//   x^ = x0 + dx: the solution of the pair -- the bits dl_eval_solved_data returns;
//   draw d:  z = n_s standard Gaussians,  v = C^-T z  (covariance A^-1),  x = x^ + v,
//            loglike  = ll + (-1/2 (|z|^2 - sum_s prec_s v_s^2) + 1/2 logdet A[marg, marg])
//            logprior = (lp + lps) - 1/2 sum_s prec_s v_s^2
// the definitions and the split of dl_sample_solved_lane (dl_sample_solved.h:5-12): ll of dl_dbm_pair_finish carries -1/2 logdet, the correction gives it back, and
// loglike + logprior is the log-posterior at (theta, x) against data vector m with nothing marginalised.
// NSP >= n_s is the compiled size of dl_data_batch_marg.h.  Sums and draws run over s < n_s: the padded components of z are never drawn (a unit factor would add z_s^2
// to |z|^2) and enter every chain as exact zeros, so that every NSP >= n_s gives the bits of NSP = n_s.  Every product that feeds a sum is an explicit fma.
// Random draws: those of dl_sample_solved.h (dl_solved_gauss_pair, (n_s + 1) / 2 Box-Muller pairs): a draw is a pure function of (seed, global point index, draw,
// component) -- not of the data index, the number of data vectors, the batch, `size` or how a chain is cut into calls.
// Status (dl_dbm_logposterior's rules): index outside [0, M) or NaN input 3, outside the prior 1, a pivot that was not positive or a non-finite ll 2; NaN outputs then.
// Written for the device and for the host (tests/csrc/emulate_sample_solved_data.cpp compiles this file with g++).
#pragma once
#include <math.h>
#include <stdint.h>

#include "dl_data_batch_marg.h"
#include "dl_sample_solved.h"

#define DL_SSD_FAC (DL_DBM_HLD - DL_DBM_C)   // doubles of the record that hold the factor: C [16][16] | 1 / C_ii [16], contiguous

// status of the pair; 0: the draws are defined.  The values of DL_STATUS_* (include/desilike_amd.h)
DL_HD int dl_ssd_status(const double* rec, double ll, bool bad_index) {
    const double inf = HUGE_VAL;
    const int flags = (int)rec[DL_DBM_FLAGS];
    if (bad_index || (flags & 1)) return 3;   // DL_STATUS_NAN_INPUT
    if (rec[DL_DBM_LP] == -inf) return 1;     // DL_STATUS_OUT_OF_PRIOR
    if ((flags & 2) || !(ll == ll) || ll == inf || ll == -inf) return 2;   // DL_STATUS_NONFINITE
    return 0;
}

// Draw `draw` of the pair.  fac: C [16][16] | 1 / C_ii [16] (the record from DL_DBM_C on, or its copy in LDS); hld: 1/2 logdet A[marg, marg]; dx, ll: dl_dbm_pair_finish;
// lpp = lp + lps; index: global index of the point.  Outputs x [NSP] (components s < n_s are the draw, the others x0_s = 0), loglike, logprior.
template <int NSP>
DL_HD void dl_ssd_draw(const double* fac, double hld, const DlDbmConst& k, int n_s, const double* dx, double ll, double lpp, int64_t index, uint32_t draw, uint32_t k0,
                       uint32_t k1, double* x, double& loglike, double& logprior) {
    const double* C = fac;
    const double* inv = fac + (DL_DBM_INV - DL_DBM_C);
    double v[NSP + 1];
#pragma unroll
    for (int p = 0; p < (NSP + 1) / 2; ++p) {
        double z0 = 0., z1 = 0.;
        if (2 * p < n_s) dl_solved_gauss_pair(index, draw, p, k0, k1, z0, z1);
        v[2 * p] = z0;
        v[2 * p + 1] = z1;
    }
    double zz = 0.;
#pragma unroll
    for (int s = 0; s < NSP; ++s) {
        if (s >= n_s) v[s] = 0.;   // (the second half of the last pair when n_s is odd; padding)
        zz = fma(v[s], v[s], zz);
    }
#pragma unroll
    for (int i = NSP - 1; i >= 0; --i) {   // v = C^-T z, in place
        double sum = v[i];
#pragma unroll
        for (int j = i + 1; j < NSP; ++j) sum = fma(-C[j * 16 + i], v[j], sum);
        v[i] = sum * inv[i];
    }
    double pv = 0.;
#pragma unroll
    for (int s = 0; s < NSP; ++s) {
        pv = fma(k.prec[s] * v[s], v[s], pv);
        x[s] = (k.x0[s] + dx[s]) + v[s];
    }
    loglike = ll + fma(-0.5, zz - pv, hld);
    logprior = fma(-0.5, pv, lpp);
}

#if defined(__HIPCC__)
struct DlMargDev;
// the draws of B points whose rows and records dl_launch_data_marg_points left in rows_ws / rec_ws, point b against data vector index[b]; index0: global index of the
// first point; outputs solved_out [B, size, n_s], loglike_out [B, size], logprior_out [B, size], status [B] (may be null)
void dl_launch_data_marg_draw(const DlMargDev& mg, const double* rows_ws, int64_t ld, int n, int rows_per_point, const double* rec_ws, const double* bias_tab, int64_t ldb, int M,
                              const int32_t* index, int64_t B, int64_t index0, int size, uint64_t seed, double* solved_out, double* loglike_out, double* logprior_out,
                              int32_t* status, hipStream_t stream);
#endif
