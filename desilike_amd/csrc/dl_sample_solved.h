// dl_sample_solved.h -- posterior draws of the analytically solved (marginalised / best-fit) linear parameters of ONE point by ONE lane (reference:
// Chain.sample_solved, desilike/samples/chain.py:229-263 with _get_solved_covariance 46-76), from the outputs of dl_eval_batch_derived: the solution x^ [NS] and
// the likelihood Hessian H_L = -Tt Tt^T [NS, NS] (notation of dl_marg_solve.h).
//   A = -H_L + diag(prec) = C C^T (SPD, C lower triangular): the posterior precision of the solved parameters at this point.
//   draw d:  z = NS standard Gaussians,  v = C^-T z  (covariance A^-1: the distribution of chain.py:241-248),  x = x^ + v,
//            dloglike  = 1/2 v H_L v + 1/2 logdet A[marg, marg]     (chain.py:251-261; the determinant over the '.marg' parameters only)
//            dlogprior = -1/2 sum_s prec_s v_s^2
//   loglike + dloglike + logprior + dlogprior is then the un-marginalised log-posterior at (theta, x): the marginalised values are those at x^ (the gradient of
//   the sum vanishes there) minus 1/2 logdet.  As in the reference the SUM is exact; with a Gaussian prior the split between the two differs from the separate
//   likelihood and prior at x by the prior's gradient at x^ times v (opposite signs in the two).
// 1/2 v H_L v is evaluated as -1/2 (|z|^2 - sum_s prec_s v_s^2): v H_L v = -v (A - diag(prec)) v and C^T v = z, so H_L is read once, for the factorisation, and
// only ONE triangle lives in registers (136 doubles at NS = 16).  The factorisation is in place.  Partially marginalised sets (0 < n_marg < NS) take the
// determinant from a first factorisation in which the rows / columns of the parameters that are only solved are unit vectors (the construction of
// dl_marg_solve_lane), then read H_L again for C.
// NS is a compile-time size: the triangle lives in registers, nothing is indexed at run time, no LDS, no cross-lane traffic.
//
// Random draws: Philox4x32-10 keyed by the 64-bit seed, counter (global point index lo, global point index hi, draw index, DL_SOLVED_STREAM | pair << 8); the
// Box-Muller pair gives components 2 pair and 2 pair + 1 (the convention of dl_nuts.h:32; streams in use elsewhere: dl_ens_fold.h 0-4, dl_mh.h 16-21, dl_nuts.h
// 32-34, dl_mclmc.h 48-49, dl_smc.h 50-52, dl_nested.h 64-66).  A draw is a pure function of (seed, global point index, draw index, component): it does not
// depend on the batch, on how a chain is cut into calls or on the number of draws asked for.
//
// Status: a point whose status from the evaluation is not 0, or with a pivot of A that is not positive and finite, gets NaN draws and NaN corrected values; the
// pivot failure is reported as DL_STATUS_NONFINITE (2), an evaluation status is passed on unchanged.
// Written for the device and for the host (tests/csrc/emulate_sample_solved.cpp compiles this file with g++).
#pragma once
#include <math.h>
#include <stdint.h>

#include "dl_fullshape.h"
#include "dl_philox.h"

#define DL_SOLVED_STREAM 80u

// 1 / sqrt(d), d > 0 normal.  Device: v_rsq_f64 and two Newton steps (dl_marg_solve.h); host: the plain quotient
DL_HD double dl_solved_rsqrt(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
    double y = __builtin_amdgcn_rsq(d);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double h = 0.5 * y, e = fma(-d * y, h, 0.5);
        y = fma(y, e, y);
    }
    return y;
#else
    return 1. / sqrt(d);
#endif
}

// d = mant x 2^ex, mant in [1/2, 1)
DL_HD double dl_solved_frexp(double d, int& ex) {
#if defined(__HIP_DEVICE_COMPILE__)
    ex = __builtin_amdgcn_frexp_exp(d);
    return __builtin_amdgcn_frexp_mant(d);
#else
    return frexp(d, &ex);
#endif
}

// In-place Cholesky factorisation of A = -H_L + diag(prec) of one point (hessian: H_L [NS, NS], symmetric, its lower triangle is read): C[i][j], j < i, and
// inv[j] = 1 / C[j][j] on return; logdet = log det of the factorised matrix.  PARTIAL: rows / columns of parameters with is_marg == 0 are unit vectors (logdet is
// then log det A[marg, marg]).  Returns false if a pivot is not positive and finite (the pivot is replaced by 1: everything stays finite, nothing of it is used).
template <int NS, bool PARTIAL, class Marg>
DL_HD bool dl_solved_cholesky(const double* __restrict__ hessian, const Marg& mg, double (&C)[NS][NS], double (&inv)[NS], double& logdet) {
    const double inf = HUGE_VAL;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double a = -hessian[i * NS + j] + (i == j ? mg.prec[i] : 0.);
            if (PARTIAL) C[i][j] = (mg.is_marg[i] != 0 && mg.is_marg[j] != 0) ? a : (i == j ? 1. : 0.);
            else C[i][j] = a;
        }
    }
    bool ok = true;
    // log det = log of the product of the pivots: mantissas and exponents apart (the product of NS <= 16 mantissas in [1/2, 1) cannot underflow), ONE logarithm
    double mant_all = 1.;
    int exp_all = 0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        double d = C[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= C[j][k] * C[j][k];
        if (!(d > 0.) || d == inf) { ok = false; d = 1.; }
        int ex;
        mant_all *= dl_solved_frexp(d, ex);
        exp_all += ex;
        inv[j] = dl_solved_rsqrt(d);
#pragma unroll
        for (int i = j + 1; i < NS; ++i) {
            double sum = C[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) sum -= C[i][k] * C[j][k];
            C[i][j] = sum * inv[j];
        }
    }
    logdet = log(mant_all) + (double)exp_all * 0.693147180559945309417;
    return ok;
}

// standard Gaussians 2 pair, 2 pair + 1 of draw `draw` of global point `index`
DL_HD void dl_solved_gauss_pair(int64_t index, uint32_t draw, int pair, uint32_t k0, uint32_t k1, double& z0, double& z1) {
    const DlPhilox r = dl_philox4x32((uint32_t)index, (uint32_t)((uint64_t)index >> 32), draw, DL_SOLVED_STREAM | ((uint32_t)pair << 8), k0, k1);
    const double rad = sqrt(-2. * log1p(-dl_uniform53(r.x[0], r.x[1]))), ang = 6.283185307179586 * dl_uniform53(r.x[2], r.x[3]);
    z0 = rad * cos(ang);
    z1 = rad * sin(ang);
}

// The `size` draws of one point.  Marg: DlMargDev (dl_kernels.h) or any struct with its prec[], is_marg[] and n_marg.  hessian [NS, NS], xhat [NS], loglike /
// logprior / status_in: what the evaluation returned for the point; index: global index of the point in the chain.  Outputs of this point: solved_out [size, NS],
// loglike_out [size], logprior_out [size].  Returns the status of the point.
template <int NS, class Marg>
DL_HD int dl_sample_solved_lane(const double* __restrict__ hessian, const double* __restrict__ xhat, const Marg& mg, double loglike, double logprior, int status_in,
                                int64_t index, int size, uint32_t k0, uint32_t k1, double* __restrict__ solved_out, double* __restrict__ loglike_out,
                                double* __restrict__ logprior_out) {
    double C[NS][NS], inv[NS], logdet = 0., logdet_marg = 0.;
    bool ok = status_in == 0;
    if (ok) {
        if (mg.n_marg > 0 && mg.n_marg < NS) ok = dl_solved_cholesky<NS, true>(hessian, mg, C, inv, logdet_marg);
        ok = dl_solved_cholesky<NS, false>(hessian, mg, C, inv, logdet) && ok;
        if (mg.n_marg == NS) logdet_marg = logdet;
    }
    if (!ok) {
        const double nan = __builtin_nan("");
        for (int d = 0; d < size; ++d) {
#pragma unroll
            for (int s = 0; s < NS; ++s) solved_out[(int64_t)d * NS + s] = nan;
            loglike_out[d] = nan;
            logprior_out[d] = nan;
        }
        return status_in != 0 ? status_in : 2;   // DL_STATUS_NONFINITE
    }
    for (int d = 0; d < size; ++d) {
        double v[NS + 1], zz = 0.;
#pragma unroll
        for (int p = 0; p < (NS + 1) / 2; ++p) dl_solved_gauss_pair(index, (uint32_t)d, p, k0, k1, v[2 * p], v[2 * p + 1]);
#pragma unroll
        for (int s = 0; s < NS; ++s) zz += v[s] * v[s];
#pragma unroll
        for (int i = NS - 1; i >= 0; --i) {   // v = C^-T z, in place
            double sum = v[i];
#pragma unroll
            for (int k = i + 1; k < NS; ++k) sum -= C[k][i] * v[k];
            v[i] = sum * inv[i];
        }
        double pv = 0.;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            pv += mg.prec[s] * v[s] * v[s];
            solved_out[(int64_t)d * NS + s] = xhat[s] + v[s];   // (x^ from the cache at every draw: NS fewer doubles held across the loop)
        }
        loglike_out[d] = loglike + (-0.5 * (zz - pv) + 0.5 * logdet_marg);
        logprior_out[d] = logprior - 0.5 * pv;
    }
    return 0;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
struct DlMargDev;
// draws of B points (one lane per point) from the outputs of the evaluation: hessian [B, n_s, n_s], solved [B, n_s], loglike [B], logprior [B], status_in [B];
// index0: global index of the first point; outputs solved_out [B, size, n_s], loglike_out [B, size], logprior_out [B, size], status_out [B] (may be null)
void dl_launch_sample_solved(const DlMargDev& mg, const double* hessian, const double* solved, const double* loglike, const double* logprior, const int32_t* status_in,
                             int64_t B, int64_t index0, int size, uint64_t seed, double* solved_out, double* loglike_out, double* logprior_out, int32_t* status_out,
                             hipStream_t stream);
#endif
