// dl_fullshape_jac.h -- analytic Jacobian of the Kaiser full-shape theory vector: the FORWARD-mode twin of dl_fullshape_grad.h (exact derivative rows for the Fisher
// algebra: what the reference's ``Differentiation`` takes from jax, desilike/differentiation.py, and fisher.py:731-750 consumes as dD).
//
// dl_fullshape_grad.h contracts d P_l(k) / d(physical inputs) with Y on the fly and never forms the derivative; here every thread owns its wavenumbers and keeps,
// per wavenumber and multipole, the sums over the mu nodes
//     d P_l(k) / d phys = sum_m w_l(m) (alpha_phys(m) T + beta_phys(m) T'),   phys in (qpar, qper, f, b1X, b1Y)           [pass 0: the template's own spline]
//     d P_l(k) / d dm   = sum_m w_l(m) jac bias(m) S_dm,   d P_l(k) / d dn likewise                                        [passes 1, 2: the splines of d template / d dm, dn]
//     d P_0(k) / d sn0  = 1 / nd
// with the SAME per-mu records (dl_fs_grad_weights), the same knot data (dl_fs_grad_knots) and the same interval polynomials (dl_spline_eval_t2) as the gradient
// phase, one spline held at a time.  The chain rule to the theta columns is linear: its matrix C [DL_NPHYS][P] is dl_fs_grad_chain applied to the unit vectors
// (every AP mode, df, tracer namespaces -- nothing restated here), and each ELEMENT of the rows is  J_p(l, k) = sum_phys C[phys][p] d P_l(k) / d phys.
// Output: rows [P][ldj] of one point; an observable writes its own column block [col_offset, col_offset + n_ell n_kin) of every row (zeros where a parameter does
// not reach it); the workgroup of the last observable also zeroes the padding columns.  No reduction across threads: results are bit-repeatable.
// Scope: dl_fs_grad_applicable (Kaiser tracers, fixed / ShapeFit template on uniform knots, no damping, no counter terms, no pass-through columns).
#pragma once
#include "dl_fullshape_grad.h"

// the chain rule's matrix, C [DL_NPHYS][P]: thread q < DL_NPHYS writes row q = dl_fs_grad_chain(e_q)
DL_HD void dl_fs_jac_chain_matrix(int tid, const DlObsDev& o, const double* th, int P, double* C) {
    if (tid >= DL_NPHYS) return;
    double g[DL_NPHYS];
#pragma unroll
    for (int q = 0; q < DL_NPHYS; ++q) g[q] = q == tid ? 1. : 0.;
    double* row = C + (size_t)tid * P;
    for (int p = 0; p < P; ++p) row[p] = 0.;
    dl_fs_grad_chain(o, th, g, row);
}

// padding columns [k_live, k_pad) of the P rows of one point (they meet zeros of the window operator: they must be finite)
DL_HD void dl_fs_jac_zero_tail(int tid, int nthr, int P, int k_live, int k_pad, double* J, int64_t ldj) {
    const int w = k_pad - k_live;
    for (int idx = tid; idx < P * w; idx += nthr) J[(size_t)(idx / w) * ldj + k_live + idx % w] = 0.;
}

// c a added to v unless c is exactly zero (a column the parameter does not reach stays 0 whatever a holds: NaN inputs of another parameter included)
DL_HD double dl_fs_jac_madd(double c, double a, double v) { return c != 0. ? fma(c, a, v) : v; }

// Jacobian phase 3.  J: row 0 of the point at this observable's first column, row p at J + p ldj, element (l, k_i) at l n_kin + i.
// pass 0 WRITES every row (all P: the zero fill is part of it); passes 1 and 2 add the dm / dn term to the rows whose chain entry is not zero -- the same thread
// wrote the element in pass 0, so the read-modify-write needs no barrier.
// KPT wavenumbers per thread: the accumulators of pass 0 are 5 NL KPT doubles (NL = 3, KPT = 2: 30; NL = 5: KPT = 1, 25).
template <int NL, int KPT>
DL_HD void dl_fs_jac_phase3(int tid, int nthr, const DlObsDev& o, const DlFsShared& s, const double* gw, const double* C, int P, int pass, double* __restrict__ J, int64_t ldj) {
    const int n_kin = o.n_kin, n_mu4 = (o.n_mu + 3) & ~3;
    for (int i0 = tid; i0 < n_kin; i0 += KPT * nthr) {
        double t0[KPT];
#pragma unroll
        for (int q = 0; q < KPT; ++q) {
            const int i = i0 + q * nthr;
            t0[q] = (o.lkin[i < n_kin ? i : n_kin - 1] - o.x0) * o.inv_hx;
        }
        if (pass == 0) {
            double acc[KPT][5][NL];
#pragma unroll
            for (int q = 0; q < KPT; ++q)
#pragma unroll
                for (int c = 0; c < 5; ++c)
#pragma unroll
                    for (int l = 0; l < NL; ++l) acc[q][c][l] = 0.;
            for (int m = 0; m < n_mu4; ++m) {
                const double* r = gw + (size_t)m * DL_GW;
                double w[NL];
#pragma unroll
                for (int l = 0; l < NL; ++l) w[l] = r[DL_GW_W + l];
                const double lqh = r[DL_GW_LQH];
                const double aqpar = r[DL_GW_AQPAR], bqpar = r[DL_GW_BQPAR], aqper = r[DL_GW_AQPER], bqper = r[DL_GW_BQPER], af = r[DL_GW_AF], ab1x = r[DL_GW_AB1X], ab1y = r[DL_GW_AB1Y];
#pragma unroll
                for (int q = 0; q < KPT; ++q) {
                    int j; double u, T, dT;
                    dl_spline_eval_t2(o, s, t0[q] + lqh, j, u, T, dT);
                    const double v[5] = {fma(aqpar, T, bqpar * dT), fma(aqper, T, bqper * dT), af * T, ab1x * T, ab1y * T};
#pragma unroll
                    for (int c = 0; c < 5; ++c)
#pragma unroll
                        for (int l = 0; l < NL; ++l) acc[q][c][l] = fma(w[l], v[c], acc[q][c][l]);
                }
            }
            const double inv_nd = 1. / o.nd;
            for (int p = 0; p < P; ++p) {
                const double cqpar = C[DL_G_QPAR * P + p], cqper = C[DL_G_QPER * P + p], cf = C[DL_G_F * P + p], cb1x = C[DL_G_B1X * P + p], cb1y = C[DL_G_B1Y * P + p];
                const double csn0 = C[DL_G_SN0 * P + p] * inv_nd;
#pragma unroll
                for (int q = 0; q < KPT; ++q) {
                    const int i = i0 + q * nthr;
                    if (i >= n_kin) continue;
#pragma unroll
                    for (int l = 0; l < NL; ++l) {
                        if (l >= o.n_ell) continue;
                        double v = l == o.ell0 ? csn0 : 0.;
                        v = dl_fs_jac_madd(cqpar, acc[q][0][l], v);
                        v = dl_fs_jac_madd(cqper, acc[q][1][l], v);
                        v = dl_fs_jac_madd(cf, acc[q][2][l], v);
                        v = dl_fs_jac_madd(cb1x, acc[q][3][l], v);
                        v = dl_fs_jac_madd(cb1y, acc[q][4][l], v);
                        J[(size_t)p * ldj + (size_t)l * n_kin + i] = v;
                    }
                }
            }
        } else {
            double acc[KPT][NL];
#pragma unroll
            for (int q = 0; q < KPT; ++q)
#pragma unroll
                for (int l = 0; l < NL; ++l) acc[q][l] = 0.;
            for (int m = 0; m < n_mu4; ++m) {
                const double* r = gw + (size_t)m * DL_GW;
                double w[NL];
#pragma unroll
                for (int l = 0; l < NL; ++l) w[l] = r[DL_GW_W + l];
                const double lqh = r[DL_GW_LQH], gg = r[DL_GW_G];
#pragma unroll
                for (int q = 0; q < KPT; ++q) {
                    const double v = gg * dl_spline_eval_t(o, s, t0[q] + lqh);
#pragma unroll
                    for (int l = 0; l < NL; ++l) acc[q][l] = fma(w[l], v, acc[q][l]);
                }
            }
            const double* crow = C + (size_t)(pass == 1 ? DL_G_DM : DL_G_DN) * P;
            for (int p = 0; p < P; ++p) {
                const double c = crow[p];
                if (c == 0.) continue;
#pragma unroll
                for (int q = 0; q < KPT; ++q) {
                    const int i = i0 + q * nthr;
                    if (i >= n_kin) continue;
#pragma unroll
                    for (int l = 0; l < NL; ++l) {
                        if (l >= o.n_ell) continue;
                        double* e = J + (size_t)p * ldj + (size_t)l * n_kin + i;
                        *e = fma(c, acc[q][l], *e);
                    }
                }
            }
        }
    }
}

// LDS doubles of the Jacobian workgroup: the gradient workgroup's layout with the chain matrix [DL_NPHYS][P] in place of the reduction scratch
DL_HD size_t dl_fs_jac_shared_doubles(const DlObsDev& o, int P) {
    return dl_fs_shared_doubles_obs(o, true) + (size_t)DL_MAX_MU * DL_GW + (size_t)DL_NPHYS * P;
}
