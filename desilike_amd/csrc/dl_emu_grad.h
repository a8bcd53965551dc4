// dl_emu_grad.h -- analytic gradient of the log-posterior of an emulated (velocileptors-table) full-shape likelihood with analytically solved parameters: the
// value_and_grad the reference's HMC / NUTS samplers take from jax (desilike/samplers/hmc.py:194, samplers/nuts.py:205) for BASELINE configs[2].
//
// Notation (one point, whitened data space, columns j < N_pad; dl_feature_gemm.h:1-9):
//   U_m[j] = sum_h G[(m, j)][h] basis_h(theta)                            the folded operator applied to the basis of the table engine, m < 19 monomials
//   dt[j]  = sum_m c_0m U_m[j] + bias[j]                                  residual at the solved parameters' x0 (c_0 = the 19 bias monomials, row 0 of the record)
//   Tt_s[j] = sum_m c_sm U_m[j] + tconst_s[j]                             derivative row of solved parameter s (c_s = record row 1 + var_slot[s]: d mono / d lambda_s)
//   A = Tt Tt^T + diag(prec),  dx = A^-1 (-Tt dt - (x0 - loc) prec),  r* = dt + Tt^T dx                                     (dl_marg_solve.h)
//   J = -1/2 |r*|^2 - 1/2 sum_s prec_s (x0 + dx - loc)_s^2 - 1/2 logdet A[marg, marg] + logprior(theta)   (likelihoods/base.py:314-413, the log-posterior)
// dx minimises the first two terms over the solved parameters (all of them, '.best' or '.marg'), so by the envelope theorem their theta-derivative is taken at fixed dx:
//   d/dtheta (-1/2 |r*|^2 - ...) = -r* . (d dt + sum_s dx_s d Tt_s).
// The determinant of the '.marg' block Am differentiates to -1/2 tr(Am^-1 dAm) = -sum_{s, t in marg} (Am^-1)_st Tt_t . d Tt_s.  With Wc = -Am^-1 on the marg block and
// zero elsewhere, every theta-dependence enters through the rows:
//   dJ = sum_j [ y_0[j] d dt[j] + sum_s y_s[j] d Tt_s[j] ],   y_0 = -r*,   y_s = -r* dx_s + sum_t Wc_st Tt_t.
// dt and Tt_s are bilinear in (c, U).  With rho(r) the record row of y_r (rho(0) = 0, rho(s) = 1 + var_slot[s]):
//   dJ/d c_rho(r),m = U_m . y_r = Q[rho(r)][m]                            (19 (1 + n_var) dot products per point)
//   dJ/d U_m[j] = V[m][j] = sum_r c_rho(r),m y_r[j]                       (the adjoint of the folded operator's output)
//   dJ/d basis_h = g_h = sum_{m, j} G[(m, j)][h] V[m][j]                  (ONE GEMM over all points: K = 19 N_pad, through the transposed operator)
// Q goes through the velocileptors 'pars' to the eleven bias / counter inputs and to sigma8, fsigma8 (dl_eg_mono_vjp below: reverse mode of dl_velocileptors_prelude,
// _row0 and _drow); g_h goes back through the hidden layers of the table MLP (delta <- (W delta) * act'(z)), the sigma8 / fsigma8 adjoints through their MLPs
// (output = v yscale + ylo), and the three input gradients through the x-scaler (v - lo) / (hi - lo) to the theta columns of x_in.  relu: act'(0) = 0 (jax's convention).
//
// Scope (dl_eval_logposterior_grad returns 2 otherwise): ONE emulated observable on the feature path, table engine and the sigma8 / fsigma8 engines MLPs or constants,
// up to DL_EG_MAX_SOLVED solved parameters, uniform / norm priors, no transform.  Taylor engines, the stacked layout (dl_emu_stacked_split.h) and several observables are not covered.
//
// The per-point arithmetic (dl_eg_mono_vjp, dl_eg_marg_adjoint) is host-buildable (tests/csrc/emulate_emu_grad.cpp); the kernels follow under __HIPCC__.
#pragma once
#include "dl_fullshape.h"

#define DL_EG_MAX_SOLVED 8   // solved parameters the gradient kernels are instantiated for (more: dl_eval_logposterior_grad returns 2)
#define DL_EG_NIN 13   // inputs of the monomials: the eleven velocileptors 'pars' inputs, sigma8, fsigma8

// Q [(1 + n_var)][DL_N_MONO] (row 0: monomials, row 1 + slot: derivative row of variable slot `slot`) -> g [DL_EG_NIN] = sum_r,m Q[r][m] d mono_r[m] / d input
DL_HD void dl_eg_mono_vjp(const DlObsDev& o, const double* v, double sigma8, double fsigma8, const double* Q, double* g) {
    DlVeloPre p;
    dl_velocileptors_prelude(o, v, sigma8, fsigma8, p);
    const bool rept = (o.mono_mode == 2 || o.mono_mode == 4);
    for (int k = 0; k < DL_EG_NIN; ++k) g[k] = 0.;
    const double b1 = p.pars[0], b2 = p.pars[1], bs = p.pars[2], b3 = p.pars[3];
    const double* q0 = Q;
    double gP[DL_N_VPARS];
    const double gb1 = q0[1] + 2. * b1 * q0[2] + b2 * q0[4] + bs * q0[7] + b3 * q0[11];
    const double gb2 = q0[3] + b1 * q0[4] + 2. * b2 * q0[5] + bs * q0[8];
    const double gbs = q0[6] + b1 * q0[7] + b2 * q0[8] + 2. * bs * q0[9];
    const double gb3 = q0[10] + b1 * q0[11];
    for (int c = 4; c < 8; ++c) gP[c] = q0[12 + (c - 4)];
    for (int c = 8; c < 11; ++c) gP[c] = q0[16 + (c - 8)] / o.nd;
    if (rept) { gP[0] = gb1 - (2. / 7.) * gbs + gb3; gP[2] = gbs; gP[3] = 3. * gb3; }   // co-evolution, full_shape.py:1481-1485
    else { gP[0] = gb1; gP[2] = gbs; gP[3] = gb3; }
    gP[1] = gb2;
    if (!p.physical) {
        for (int c = 0; c < DL_N_VPARS; ++c) g[c] = gP[c];   // (derivative rows are constants)
        return;
    }
    const double s = sigma8, one = p.one_b1L, f = p.f;
    double g_one = gP[0] + (rept ? (8. / 21.) * gP[1] : 0.), g_f = 0., g_s = 0.;
    // derivative rows of the solved alpha* (dl_velocileptors_drow): entries one^2, f one, f^2
    for (int c = 4; c <= 6; ++c) {
        const int slot = o.vp_slot[c];
        if (slot < 0) continue;
        const double* qs = Q + (size_t)(1 + slot) * DL_N_MONO;
        if (c == 4) { g_one += 2. * one * qs[12] + f * qs[13]; g_f += one * qs[13]; }
        else { const int m = c == 5 ? 13 : 14; g_one += f * qs[m]; g_f += one * qs[m] + 2. * f * qs[m + 1]; }
    }
    // pars 4 .. 10
    g_one += 2. * one * v[4] * gP[4];                  g[4] += one * one * gP[4];
    g_f += one * (v[4] + v[5]) * gP[5];                g_one += f * (v[4] + v[5]) * gP[5];  g[4] += f * one * gP[5];  g[5] += f * one * gP[5];
    g_f += (2. * f * v[5] + one * v[6]) * gP[6];       g_one += f * v[6] * gP[6];           g[5] += f * f * gP[6];    g[6] += f * one * gP[6];
    g_f += 2. * f * v[6] * gP[7];                      g[6] += f * f * gP[7];
    for (int i = 0; i < 3; ++i) g[8 + i] += p.sn_scale[i] * gP[8 + i];
    // b2L = v1 / s^2, bsL = v2 / s^2, b3L = v3 / s^3, one = v0 / s, f = fsigma8 / s
    const double is = 1. / s, is2 = is * is, is3 = is2 * is;
    g[1] += gP[1] * is2;  g_s += -2. * v[1] * is3 * gP[1];
    g[2] += gP[2] * is2;  g_s += -2. * v[2] * is3 * gP[2];
    g[3] += gP[3] * is3;  g_s += -3. * v[3] * is3 * is * gP[3];
    g[0] += g_one * is;   g_s += -v[0] * is2 * g_one;
    g[12] += g_f * is;    g_s += -fsigma8 * is2 * g_f;
    g[11] += g_s;
}

// Marginalisation adjoint of one point from its Gram matrix G [(1 + NS)][ldg] (full symmetric: entry (0, 0) = |dt|^2, (0, 1 + s) = dt . Tt_s, (1 + s, 1 + t) = Tt_s . Tt_t):
// dx [NS] (the solution, as dl_marg_solve_lane forms it) and Wc [NS][NS] = -(A[marg, marg])^-1 on the marg block, 0 on rows / columns of '.best' parameters.
// Returns false if a pivot is not positive.  NS is a compile-time size (as in dl_marg_solve_lane): every array lives in registers on the device.
template <int NS>
DL_HD bool dl_eg_marg_adjoint(const double* G, int ldg, const double* x0, const double* loc, const double* prec, const int32_t* is_marg, double* dx, double* Wc) {
    double C[NS][NS], y[NS], xs[NS];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NS; ++j) {   // Cholesky of A = Tt Tt^T + diag(prec)
        double d = G[(size_t)(1 + j) * ldg + 1 + j] + prec[j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= C[j][k] * C[j][k];
        if (!(d > 0.) || d == HUGE_VAL) { ok = false; d = 1.; }
        C[j][j] = sqrt(d);
#pragma unroll
        for (int i = j + 1; i < NS; ++i) {
            double sum = G[(size_t)(1 + i) * ldg + 1 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) sum -= C[i][k] * C[j][k];
            C[i][j] = sum / C[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double sum = -G[(size_t)(1 + i) * ldg] - (x0[i] - loc[i]) * prec[i];
#pragma unroll
        for (int k = 0; k < i; ++k) sum -= C[i][k] * y[k];
        y[i] = sum / C[i][i];
    }
#pragma unroll
    for (int i = NS - 1; i >= 0; --i) {
        double sum = y[i];
#pragma unroll
        for (int k = i + 1; k < NS; ++k) sum -= C[k][i] * xs[k];
        xs[i] = sum / C[i][i];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) dx[i] = xs[i];
    // Am: the marg block of A, unit rows / columns for the '.best' parameters (its inverse is (A[marg, marg])^-1 there and the identity elsewhere)
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const bool mj = is_marg[j] != 0;
        double d = mj ? G[(size_t)(1 + j) * ldg + 1 + j] + prec[j] : 1.;
#pragma unroll
        for (int k = 0; k < j; ++k) d -= C[j][k] * C[j][k];
        if (!(d > 0.) || d == HUGE_VAL) { ok = false; d = 1.; }
        C[j][j] = sqrt(d);
#pragma unroll
        for (int i = j + 1; i < NS; ++i) {
            double sum = (mj && is_marg[i] != 0) ? G[(size_t)(1 + i) * ldg + 1 + j] : 0.;
#pragma unroll
            for (int k = 0; k < j; ++k) sum -= C[i][k] * C[j][k];
            C[i][j] = sum / C[j][j];
        }
    }
#pragma unroll
    for (int t = 0; t < NS; ++t) {   // column t of Am^-1
        double z[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            double sum = i == t ? 1. : 0.;
#pragma unroll
            for (int k = 0; k < i; ++k) sum -= C[i][k] * z[k];
            z[i] = sum / C[i][i];
        }
#pragma unroll
        for (int i = NS - 1; i >= 0; --i) {
            double sum = z[i];
#pragma unroll
            for (int k = i + 1; k < NS; ++k) sum -= C[k][i] * z[k];
            z[i] = sum / C[i][i];
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) Wc[(size_t)s * NS + t] = (is_marg[s] != 0 && is_marg[t] != 0) ? -z[s] : 0.;
    }
    return ok;
}

DL_HD double dl_eg_act_deriv(int act, double z) {   // d act / d z at the pre-activation z (dl_activation)
    if (act == 0) { const double sg = 1. / (1. + exp(-z)); return sg * (1. + z * (1. - sg)); }
    if (act == 1) return z > 0. ? 1. : 0.;
    const double t = tanh(z);
    return 1. - t * t;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "dl_feature_gemm.h"
#include "dl_kernels.h"
#include "dl_marg_solve.h"

// U [B][19][ldu] of 16 points per workgroup: U_m = G . basis by fp64 MFMA, the operand in the fragment order of the feature GEMM (dl_feature_gemm.h), the 19 accumulator
// tiles of a wave stored as they are (the feature GEMM's epilogue contracts them with monomial rows instead).  128 threads = 2 column blocks of 16; blockIdx.y = pair of
// column blocks (at 2048 points, 8 blocks per workgroup were 128 workgroups: half the chip, 59 us; pairs are 512).  The basis comes from the records the theory kernel wrote (feat, this observable at feat_off).
__global__ __launch_bounds__(128) void dl_emu_grad_u_kernel(const double* __restrict__ feat, int64_t feat_ld, int64_t feat_off, int nb_pad, const double* __restrict__ gfrag,
                                                            double* __restrict__ U, int64_t ldu, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int64_t p0 = (int64_t)blockIdx.x * DL_FG_PTS;
    const int stride = dl_fg_lds_stride(nb_pad);
    for (int idx = tid; idx < DL_FG_PTS * nb_pad; idx += 128) {
        const int pt = idx / nb_pad, c = idx - pt * nb_pad;
        const int64_t b = p0 + pt < B ? p0 + pt : B - 1;
        lds[pt * stride + c] = feat[(size_t)b * feat_ld + feat_off + c];
    }
    __syncthreads();
    const int jb = blockIdx.y * 2 + wave, nq = nb_pad / 8;
    const dl_fg_double2* gw = reinterpret_cast<const dl_fg_double2*>(gfrag) + (size_t)jb * nq * DL_FG_NM * 64 + lane;
    const double* arow = lds + col * stride + 2 * g;
    dl_fg_double4 acc[DL_FG_NM];
#pragma unroll
    for (int m = 0; m < DL_FG_NM; ++m) acc[m] = (dl_fg_double4){0., 0., 0., 0.};
    for (int q = 0; q < nq; ++q) {
        dl_fg_double2 bq[DL_FG_NM];
#pragma unroll
        for (int m = 0; m < DL_FG_NM; ++m) bq[m] = gw[(size_t)(q * DL_FG_NM + m) * 64];
        const dl_fg_double2 a = *reinterpret_cast<const dl_fg_double2*>(arow + 8 * q);
#pragma unroll
        for (int m = 0; m < DL_FG_NM; ++m) {
            acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, bq[m].x, acc[m], 0, 0, 0);
            acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, bq[m].y, acc[m], 0, 0, 0);
        }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {   // accumulator register rr of lane (col, g) = U[point g + 4 rr][m][column jb * 16 + col]
        const int64_t p = p0 + g + 4 * rr;
        if (p < B) {
#pragma unroll
            for (int m = 0; m < DL_FG_NM; ++m) U[((size_t)p * DL_FG_NM + m) * ldu + jb * 16 + col] = acc[m][rr];
        }
    }
}

__device__ __forceinline__ double dl_eg_wave_sum(double x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
template <int N>
__device__ __forceinline__ void dl_eg_wave_sums(double (&x)[N]) {   // N independent reductions, interleaved
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] += __shfl_xor(x[i], o, 64);
    }
}

// Adjoint and log-posterior of one point per 64-thread workgroup, NS = n_s solved parameters: rows X = [dt; Tt_1 .. Tt_NS] from U and the record's monomial rows, their
// Gram matrix, the solve of the evaluation path (dl_marg_solve_lane: log-likelihood, solved priors, dx), the priors and the status (dl_marg_store_lane: the log-posterior the
// caller gets), the marginalisation adjoint Wc, y_r, then V [B][19][ldu] (the next GEMM's A operand) and Q [B][(1 + n_var)][19].
// LDS: mono [(1 + n_var)][20] | X [(1 + NS)][N_pad] | y [(1 + NS)][N_pad] | G [(1 + NS)]^2 | dx [NS], Wc [NS][NS].
template <int NS>
__global__ __launch_bounds__(64) void dl_emu_grad_adjoint_kernel(const double* __restrict__ feat, int64_t feat_ld, int64_t feat_off, int nb_pad, int n_var,
                                                                 const double* __restrict__ U, int64_t ldu, int N_pad, const double* __restrict__ bias, const DlMargDev mg,
                                                                 const double* __restrict__ theta, int n_params, const double* __restrict__ priors,
                                                                 double* __restrict__ logpost, int32_t* __restrict__ status,
                                                                 double* __restrict__ V, double* __restrict__ Q, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int NR = 1 + NS;
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int R = 1 + n_var;
    double* mono = lds;                                   // [R][20]
    double* X = mono + (size_t)R * DL_FG_MONO_LD;         // [NR][N_pad]
    double* Y = X + (size_t)NR * N_pad;                   // [NR][N_pad]
    double* Gm = Y + (size_t)NR * N_pad;                  // [NR][NR]
    double* dxw = Gm + (size_t)NR * NR;                   // dx [NS] | Wc [NS][NS]
    int row_of[NR];                                       // record row of X row r, -1: none (a solved parameter with a constant derivative row)
    row_of[0] = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) row_of[1 + s] = mg.var_slot[s] >= 0 ? 1 + mg.var_slot[s] : -1;
    const double* rec = feat + (size_t)b * feat_ld + feat_off + nb_pad;
    for (int i = lane; i < R * DL_FG_MONO_LD; i += 64) mono[i] = rec[i];
    __syncthreads();
    const double* Ub = U + (size_t)b * DL_FG_NM * ldu;
    double gp[NR * (NR + 1) / 2];
#pragma unroll
    for (int i = 0; i < NR * (NR + 1) / 2; ++i) gp[i] = 0.;
    for (int j = lane; j < N_pad; j += 64) {
        double um[DL_FG_NM], xr[NR];
#pragma unroll
        for (int m = 0; m < DL_FG_NM; ++m) um[m] = Ub[(size_t)m * ldu + j];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            double acc = r == 0 ? bias[j] : mg.tconst[(size_t)(r - 1) * N_pad + j];
            if (row_of[r] >= 0) {
#pragma unroll
                for (int m = 0; m < DL_FG_NM; ++m) acc = fma(mono[row_of[r] * DL_FG_MONO_LD + m], um[m], acc);
            }
            xr[r] = acc;
            X[(size_t)r * N_pad + j] = acc;
        }
        int k = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int t = 0; t <= r; ++t) gp[k++] += xr[r] * xr[t];
    }
    dl_eg_wave_sums(gp);
    if (lane == 0) {
        int k = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int t = 0; t <= r; ++t) { Gm[r * NR + t] = gp[k]; Gm[t * NR + r] = gp[k]; ++k; }
        // log-posterior as the evaluation path forms it (dl_marg_solve.h)
        double ll, lps = 0.;
        bool ok = true;
        double* dx = dxw;
        double* Wc = dxw + NS;
        if constexpr (NS > 0) {
            double xsol[NS];
            ll = dl_marg_solve_lane<NS>([&](int i, int j) { return Gm[i * NR + j]; }, mg, xsol, nullptr, lps, ok);
            (void)dl_eg_marg_adjoint<NS>(Gm, NR, mg.x0, mg.loc, mg.prec, mg.is_marg, dx, Wc);
        } else ll = -0.5 * Gm[0];
        double lp;
        int nan_in;
        dl_marg_priors_lane(theta + (size_t)b * n_params, n_params, priors, lp, nan_in);
        dl_marg_store_lane(ll, lps, ok, lp, nan_in != 0, 1, b, logpost, nullptr, status);
    }
    __syncthreads();
    double dx[NS > 0 ? NS : 1], Wc[NS > 0 ? NS * NS : 1];
#pragma unroll
    for (int s = 0; s < NS; ++s) dx[s] = dxw[s];
#pragma unroll
    for (int s = 0; s < NS * NS; ++s) Wc[s] = dxw[NS + s];
    double* Vb = V + (size_t)b * DL_FG_NM * ldu;
    double* Qb = Q + (size_t)b * R * DL_FG_NM;
    for (int j = lane; j < N_pad; j += 64) {
        double xr[NR], y[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) xr[r] = X[(size_t)r * N_pad + j];
        double rs = xr[0];
#pragma unroll
        for (int s = 0; s < NS; ++s) rs = fma(dx[s], xr[1 + s], rs);
        y[0] = -rs;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            double ys = -rs * dx[s];
#pragma unroll
            for (int t = 0; t < NS; ++t) ys = fma(Wc[s * NS + t], xr[1 + t], ys);
            y[1 + s] = ys;
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) Y[(size_t)r * N_pad + j] = y[r];
        // V[m][j] = sum_r c_row(r),m y_r[j]
#pragma unroll
        for (int m = 0; m < DL_FG_NM; ++m) {
            double acc = 0.;
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (row_of[r] >= 0) acc = fma(mono[row_of[r] * DL_FG_MONO_LD + m], y[r], acc);
            Vb[(size_t)m * ldu + j] = acc;
        }
    }
    // Q[row(r)][m] = U_m . y_r  (each lane reads back only its own columns of Y: no barrier needed)
    for (int m = 0; m < DL_FG_NM; ++m) {
        double qp[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) qp[r] = 0.;
        for (int j = lane; j < N_pad; j += 64) {
            const double u = Ub[(size_t)m * ldu + j];
#pragma unroll
            for (int r = 0; r < NR; ++r) qp[r] = fma(u, Y[(size_t)r * N_pad + j], qp[r]);
        }
        dl_eg_wave_sums(qp);
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < NR; ++r) if (row_of[r] >= 0) Qb[row_of[r] * DL_FG_NM + m] = qp[r];
        }
    }
}

struct DlEgWT { const double* w[3]; };   // per engine: the MLP kernels transposed (dl_eg_mlp_backward), null for other engines

// LDS doubles of dl_emu_grad_backprop_kernel: x | scaled-input gradient | scalars | per engine: pre-activations of every layer | two activation / delta buffers
static inline __host__ __device__ int dl_eg_engine_doubles(const DlObsDev::Engine& e) {
    int n = 0, w = 0;
    if (e.type != 0) return 0;
    for (int l = 0; l < e.n_layers; ++l) n += e.widths[l + 1];
    for (int l = 0; l <= e.n_layers; ++l) w = e.widths[l] > w ? e.widths[l] : w;
    return n + 2 * w;
}
static inline __host__ __device__ size_t dl_eg_backprop_doubles(const DlObsDev& o) {
    size_t n = 2 * DL_MAX_X + 32;
    for (int ie = 0; ie < 3; ++ie) n += dl_eg_engine_doubles(o.eng[ie]);
    return n;
}

// forward pass of MLP engine e for one point (64 lanes), keeping every pre-activation z [sum of widths] ; returns the buffer holding the last layer's output
__device__ __forceinline__ const double* dl_eg_mlp_forward(const DlObsDev::Engine& e, bool table, const double* x, int n_x, double* z, double* buf) {
    const int lane = threadIdx.x;
    int w = 0;
    for (int l = 0; l <= e.n_layers; ++l) w = e.widths[l] > w ? e.widths[l] : w;
    double* cur = buf;
    double* nxt = buf + w;
    for (int i = lane; i < n_x; i += 64) cur[i] = (x[i] - e.xlo[i]) * e.xinv[i];
    __syncthreads();
    const double* W = e.weights;
    for (int l = 0; l < e.n_layers; ++l) {
        const int nin = e.widths[l], nout = e.widths[l + 1];
        const bool activate = table || l < e.n_layers - 1;
        for (int o = lane; o < nout; o += 64) {
            double acc = W[(size_t)nin * nout + o], acc2 = 0.;   // (two chains; the weight loads of eight steps are issued ahead)
            int i = 0;
#pragma unroll 4
            for (; i + 2 <= nin; i += 2) { acc = fma(cur[i], W[(size_t)i * nout + o], acc); acc2 = fma(cur[i + 1], W[(size_t)(i + 1) * nout + o], acc2); }
            if (i < nin) acc = fma(cur[i], W[(size_t)i * nout + o], acc);
            acc += acc2;
            z[o] = acc;
            nxt[o] = activate ? dl_activation(e.act, acc) : acc;
        }
        __syncthreads();
        W += (size_t)nin * nout + nout;
        z += nout;
        double* t = cur; cur = nxt; nxt = t;
    }
    return cur;
}

// backward pass: delta [widths[n_layers]] of the last layer's pre-activations (in buf) -> gx [n_x] += d / d x (the x-scaler included).  wT: the engine's kernels
// transposed, [out][in] per layer, packed without biases (dl_eg_transposed_weights): lane i reads column i of a row, 64 lanes one contiguous 512-byte row
__device__ __forceinline__ void dl_eg_mlp_backward(const DlObsDev::Engine& e, const double* __restrict__ wT, int n_x, const double* z_all, double* buf, double* gx) {
    const int lane = threadIdx.x;
    int w = 0, nz = 0;
    for (int l = 0; l <= e.n_layers; ++l) w = e.widths[l] > w ? e.widths[l] : w;
    for (int l = 0; l < e.n_layers; ++l) nz += e.widths[l + 1];
    size_t woff = 0;
    for (int l = 0; l < e.n_layers; ++l) woff += (size_t)e.widths[l] * e.widths[l + 1];
    double* cur = buf;            // delta of layer l (pre-activation)
    double* nxt = buf + w;
    for (int l = e.n_layers - 1; l >= 0; --l) {
        const int nin = e.widths[l], nout = e.widths[l + 1];
        woff -= (size_t)nin * nout;
        nz -= nout;
        const double* W = wT + woff;
        const double* zprev = z_all + nz - nin;   // pre-activations of layer l - 1 (l >= 1)
        for (int i = lane; i < nin; i += 64) {
            double acc = 0., acc2 = 0.;
            int o = 0;
#pragma unroll 4
            for (; o + 2 <= nout; o += 2) { acc = fma(W[(size_t)o * nin + i], cur[o], acc); acc2 = fma(W[(size_t)(o + 1) * nin + i], cur[o + 1], acc2); }
            if (o < nout) acc = fma(W[(size_t)o * nin + i], cur[o], acc);
            acc += acc2;
            if (l > 0) nxt[i] = acc * dl_eg_act_deriv(e.act, zprev[i]);
            else gx[i] += acc * e.xinv[i];
        }
        __syncthreads();
        double* t = cur; cur = nxt; nxt = t;
    }
}

// One point per 64-thread workgroup: forward of the MLP engines (pre-activations kept), the monomial adjoint (dl_eg_mono_vjp), back through the engines, then the
// theta columns and the prior.  gb [n_slabs][B][ldg]: dJ / d basis_h (split-K partial sums of the GEMM, slab_stride apart); Q [B][(1 + n_var)][19]; status: of the log-posterior pass (non-zero: gradient 0).
__global__ __launch_bounds__(64) void dl_emu_grad_backprop_kernel(const DlObsDev o, const double* __restrict__ theta, int n_params, const double* __restrict__ priors,
                                                                  const double* __restrict__ gb, int64_t ldg, int n_slabs, int64_t slab_stride, const double* __restrict__ Q, const int32_t* __restrict__ status,
                                                                  const DlEgWT wT, double* __restrict__ grad, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const double* th = theta + (size_t)b * n_params;
    double* gout = grad + (size_t)b * n_params;
    const bool ok = status == nullptr || status[b] == 0;
    if (!ok) {   // (uniform over the workgroup)
        for (int p = lane; p < n_params; p += 64) gout[p] = 0.;
        return;
    }
    double* x = lds;                    // [DL_MAX_X]
    double* gx = x + DL_MAX_X;          // [DL_MAX_X]
    double* sc = gx + DL_MAX_X;         // [32]: sigma8, fsigma8, g [DL_EG_NIN] at 4
    double* eng_base[3];
    {
        double* q = sc + 32;
        for (int ie = 0; ie < 3; ++ie) { eng_base[ie] = q; q += dl_eg_engine_doubles(o.eng[ie]); }
    }
    for (int i = lane; i < o.n_x; i += 64) { x[i] = dl_get(o.x_in[i], th); gx[i] = 0.; }
    __syncthreads();
    for (int ie = 1; ie < 3; ++ie) {
        const DlObsDev::Engine& e = o.eng[ie];
        if (e.type == 0) {
            int nz = 0;
            for (int l = 0; l < e.n_layers; ++l) nz += e.widths[l + 1];
            const double* out = dl_eg_mlp_forward(e, false, x, o.n_x, eng_base[ie], eng_base[ie] + nz);
            if (lane == 0) sc[ie - 1] = out[0] * e.yscale + e.ylo;
        } else if (lane == 0) sc[ie - 1] = e.cst;
    }
    int nz0 = 0;
    for (int l = 0; l < o.eng[0].n_layers; ++l) nz0 += o.eng[0].widths[l + 1];
    (void)dl_eg_mlp_forward(o.eng[0], true, x, o.n_x, eng_base[0], eng_base[0] + nz0);
    __syncthreads();
    if (lane == 0) {
        double v[DL_N_VPARS];
        for (int c = 0; c < DL_N_VPARS; ++c) v[c] = dl_get(o.vp_in[c], th);
        dl_eg_mono_vjp(o, v, sc[0], sc[1], Q + (size_t)b * (1 + o.n_var) * DL_N_MONO, sc + 4);
    }
    __syncthreads();
    // table engine: delta of the last hidden layer = g_h act'(z)
    {
        const DlObsDev::Engine& e = o.eng[0];
        const int L = e.n_layers, wl = e.widths[L];
        int w = 0;
        for (int l = 0; l <= L; ++l) w = e.widths[l] > w ? e.widths[l] : w;
        double* buf = eng_base[0] + nz0;
        const double* zl = eng_base[0] + nz0 - wl;
        for (int h = lane; h < wl; h += 64) {
            double gh = 0.;
            for (int sl = 0; sl < n_slabs; ++sl) gh += gb[(size_t)sl * slab_stride + (size_t)b * ldg + h];
            buf[h] = gh * dl_eg_act_deriv(e.act, zl[h]);
        }
        __syncthreads();
        dl_eg_mlp_backward(e, wT.w[0], o.n_x, eng_base[0], buf, gx);
    }
    for (int ie = 1; ie < 3; ++ie) {
        const DlObsDev::Engine& e = o.eng[ie];
        if (e.type != 0) continue;
        int nz = 0;
        for (int l = 0; l < e.n_layers; ++l) nz += e.widths[l + 1];
        double* buf = eng_base[ie] + nz;
        if (lane == 0) buf[0] = sc[4 + 10 + ie] * e.yscale;   // (g[11]: sigma8, g[12]: fsigma8; the output layer is linear)
        __syncthreads();
        dl_eg_mlp_backward(e, wT.w[ie], o.n_x, eng_base[ie], buf, gx);
    }
    __syncthreads();
    if (lane == 0) {
        for (int p = 0; p < n_params; ++p) {
            const double* pr = priors + 5 * p;
            gout[p] = pr[0] == 1. ? -(th[p] - pr[3]) / (pr[4] * pr[4]) : 0.;   // parameter.py:2007 differentiated (dl_grad_finalize_kernel)
        }
        for (int i = 0; i < o.n_x; ++i) if (o.x_in[i].col >= 0) gout[o.x_in[i].col] += gx[i];
        for (int c = 0; c < DL_N_VPARS; ++c) if (o.vp_in[c].col >= 0) gout[o.vp_in[c].col] += sc[4 + c];
    }
}
#endif
