// dl_wigglesplit.h -- wiggle-split template (template kind 5; WiggleSplitPowerSpectrumTemplate.calculate, power_template.py:1187-1211 with integrate_sigma_r2, 1038-1076).
//
// Per point, with kp the pivot (0.05) and k_i the reference's inner grid (uniform in log10 k):
//   v_i  = [P_now,tt^fid(k_i) + P_tt^fid(k_i / qbao) - P_now,tt^fid(k_i / qbao)] (k_i / kp)^dm
//   P    = cubic spline of log10 v over log10 k, to the power of ten
//   I    = trapezoid over the reference's 2048 nodes k_q of P(k_q) W^2(k_q r) k_q^3 / (2 pi^2)
//   P_dd(k_t) = P(k_t) df^2 fsigmar_fid^2 / I / (f_fid df)^2
// df cancels; the spline is linear in its data and reproduces the straight line dm log10(k / kp), so P(k) = 10^S(log10 k) (k / kp)^dm with S the spline of
// y_i = log10[P_now,tt^fid(k_i) + w(k_i / qbao)], which depends on qbao alone.  Everything else is constant and tabulated at create (dl_host.hpp, dl_ws_build).
//
// One workgroup per (point, distinct template) runs BEFORE the theory kernel and leaves P_dd at the n_t template knots in a scratch row that the theory kernel's knot
// phase copies (dl_fs_knots): the seven full-shape kernel variants keep their LDS carving and barriers, and observables sharing a template evaluate it once.
// Phases (a barrier after each):
//   1 dl_ws_knots      y_i at the n_i inner knots: two fixed log-log splines at the shifted abscissa (clamped to the fiducial table), two exponentials, one logarithm
//   2 dl_ps_fir        moments of the not-a-knot spline of y on the uniform grid: 57-tap convolution (dl_fullshape.h, shared with the phase-shift template)
//   3-5 dl_ps_end_*    end corrections and end relations (shared)
//   6 dl_ws_quadrature every thread sums its nodes in order
//   7 dl_ws_reduce     16 threads sum 1/16 of the partial sums each, in order
//   8 dl_ws_output     every thread adds the 16 sums in order (the same I everywhere: no broadcast), then P_dd at its template knots
// The order of every sum is fixed by the workgroup size alone: results repeat bit for bit from run to run and from batch to batch.
// LDS: mu^k [2 DL_FIR_PAD + 2] | moments [n_i] | padded y [n_i + 2 DL_FIR_PAD] | partial sums [nthr] | 16 sums: 8 (2 n_i + 130 + nthr + 16) bytes, 31.5 KB at the
// reference's 1828 inner knots.
// Table (dl_ws_tab; in the arena): header [DL_WS_HEAD] | inner knots [n_i][2]: (log10 k_i, P_now,tt^fid(k_i)) | fiducial intervals [n_f - 1][8]: polynomials in the
// fractional index of log10 P_tt^fid, then of log10 P_now,tt^fid | quadrature [n_q][4]: (trapezoid weight W^2 k^3 / (2 pi^2), ln(k_q / kp), interval, fraction) |
// template knots [n_t][4]: (ln(k_t / kp), interval, fraction, 0).
#pragma once
#include "dl_fullshape.h"

#define DL_WS_THREADS 256
#define DL_WS_HEAD 16
#define DL_WS_PARTS 16     // second-level sums of the quadrature
#define DL_WS_NQ 2048      // integrate_sigma_r2: nk
#define DL_LN10 2.302585092994046
enum { DL_WS_NI = 0, DL_WS_NF, DL_WS_NQ_, DL_WS_NT, DL_WS_X0F, DL_WS_INVHF, DL_WS_NORM, DL_WS_E0A, DL_WS_E0B, DL_WS_E1A, DL_WS_E1B };

DL_HD const double* dl_ws_tab(const DlObsDev& o) { return o.band_tab; }   // (kinds 3, 4 and 5 exclude each other: the band template's pointer)
DL_HD const DlInput& dl_ws_qbao(const DlObsDev& o) { return o.band_in[0]; }
DL_HD int dl_ws_n_inner(const DlObsDev& o) { return o.pad_ml; }           // inner knot count, for the launcher (the header of the table lives in device memory)

struct DlWsShared {
    DlPsShared ps;      // mu^k, moments, padded knot values of the inner grid
    double* part;       // [nthr]
    double* sums;       // [DL_WS_PARTS]
};
DL_HD size_t dl_ws_shared_doubles(int n_i, int nthr) { return (2 * DL_FIR_PAD + 2) + 2 * (size_t)n_i + 2 * DL_FIR_PAD + (size_t)nthr + DL_WS_PARTS; }
DL_HD DlWsShared dl_ws_carve(double* lds, int n_i, int nthr) {
    DlWsShared s;
    s.ps.mupow = lds;
    s.ps.m = lds + 2 * DL_FIR_PAD + 2;
    s.ps.y = s.ps.m + n_i + DL_FIR_PAD;
    s.part = s.ps.y + n_i + DL_FIR_PAD;
    s.sums = s.part + nthr;
    return s;
}

struct DlWsTab {
    int n_i, n_f, n_q, n_t;
    const double *head, *inner, *fid, *quad, *knots;
};
DL_HD DlWsTab dl_ws_open(const double* tab) {
    DlWsTab t;
    t.head = tab;
    t.n_i = (int)tab[DL_WS_NI]; t.n_f = (int)tab[DL_WS_NF]; t.n_q = (int)tab[DL_WS_NQ_]; t.n_t = (int)tab[DL_WS_NT];
    t.inner = tab + DL_WS_HEAD;
    t.fid = t.inner + 2 * (size_t)t.n_i;
    t.quad = t.fid + 8 * (size_t)(t.n_f - 1);
    t.knots = t.quad + 4 * (size_t)t.n_q;
    return t;
}

// phase 1: y_i = log10[P_now(k_i) + P_tt(k_i / qbao) - P_now,tt(k_i / qbao)]; zero padding and the mu^k table beside it
DL_HD void dl_ws_knots(int tid, int nthr, const DlWsTab& t, double qbao, const DlPsShared& s) {
    const double x0f = t.head[DL_WS_X0F], inv_hf = t.head[DL_WS_INVHF];
    const double tmax = (double)(t.n_f - 1);
    const int jmax = t.n_f - 2;
    const double lq = log10(qbao);
    for (int i = tid; i < t.n_i; i += nthr) {
        double tt = ((t.inner[2 * i] - lq) - x0f) * inv_hf;
        // clamped to the fiducial table BEFORE indexing: samplers propose any qbao.  Comparisons, not fmin / fmax: a NaN qbao stays NaN (as in dl_bao_ps_knots)
        tt = tt < 0. ? 0. : (tt > tmax ? tmax : tt);
        int j = (int)(tt > 0. ? tt : 0.);            // (0 for a NaN abscissa: u and the value below are NaN)
        j = j > jmax ? jmax : j;
        const double u = tt - (double)j;
        const double* c = t.fid + 8 * (size_t)j;
        const double ltt = fma(fma(fma(c[3], u, c[2]), u, c[1]), u, c[0]);
        const double lnow = fma(fma(fma(c[7], u, c[6]), u, c[5]), u, c[4]);
        const double wiggle = exp(DL_LN10 * ltt) - exp(DL_LN10 * lnow);
        s.y[i] = log10(t.inner[2 * i + 1] + wiggle);
    }
    for (int i = tid; i < 2 * DL_FIR_PAD; i += nthr) s.y[i < DL_FIR_PAD ? i - DL_FIR_PAD : t.n_i + i - DL_FIR_PAD] = 0.;
    for (int k = tid; k <= 2 * DL_FIR_PAD; k += nthr) {
        const double v = exp((double)k * DL_FIR_LN_ABS_MU);
        s.mupow[k] = (k & 1) ? -v : v;
    }
}

// P(k) / kp^-dm at a tabulated abscissa: record (.., ln(k / kp), interval, fraction) -> 10^S (k / kp)^dm
DL_HD double dl_ws_power(const DlPsShared& s, double dm, double lnk, double interval, double u) {
    return exp(fma(DL_LN10, dl_bao_ps_wiggle(s, (int)interval, u), dm * lnk));
}

// phase 6: the thread's share of the sigma_r integral, nodes tid, tid + nthr, ... in that order
DL_HD void dl_ws_quadrature(int tid, int nthr, const DlWsTab& t, double dm, const DlWsShared& s) {
    double acc = 0.;
    for (int q = tid; q < t.n_q; q += nthr) {
        const double* r = t.quad + 4 * (size_t)q;
        acc = fma(r[0], dl_ws_power(s.ps, dm, r[1], r[2], r[3]), acc);
    }
    s.part[tid] = acc;
}

// phase 7: DL_WS_PARTS threads sum nthr / DL_WS_PARTS partial sums each (nthr: a multiple of DL_WS_PARTS)
DL_HD void dl_ws_reduce(int tid, int nthr, const DlWsShared& s) {
    if (tid >= DL_WS_PARTS) return;
    const int len = nthr / DL_WS_PARTS;
    double acc = 0.;
    for (int q = 0; q < len; ++q) acc += s.part[tid * len + q];
    s.sums[tid] = acc;
}

// phase 8: P_dd at the template knots -> the point's scratch row
DL_HD void dl_ws_output(int tid, int nthr, const DlWsTab& t, double dm, const DlWsShared& s, double* row) {
    double integral = 0.;
    for (int q = 0; q < DL_WS_PARTS; ++q) integral += s.sums[q];
    const double norm = t.head[DL_WS_NORM] / integral;       // fsigmar_fid^2 / f_fid^2 / I: df^2 over (f_fid df)^2
    for (int j = tid; j < t.n_t; j += nthr) {
        const double* r = t.knots + 4 * (size_t)j;
        row[j] = dl_ws_power(s.ps, dm, r[0], r[1], r[2]) * norm;
    }
}

// The kernel's sequence (dl_kernels.hip: dl_ws_template_kernel; tests/csrc/emulate_wigglesplit.cpp loops tid for each phase): a barrier between two phases; `carry` is
// the thread's end-corrected moment between phases 2 and 3.  nthr: at least 2 DL_FIR_PAD, a multiple of DL_WS_PARTS.
DL_HD void dl_ws_point_phase(int phase, int tid, int nthr, double qbao, double dm, const DlWsTab& t, const DlWsShared& s, double& carry, double* row) {
    switch (phase) {
        case 0: dl_ws_knots(tid, nthr, t, qbao, s.ps); break;
        case 1: dl_ps_fir(tid, nthr, t.n_i, s.ps); break;
        case 2: carry = dl_ps_end_moment(tid, t.n_i, s.ps); break;
        case 3: dl_ps_end_store(tid, t.n_i, s.ps, carry); break;
        case 4: dl_ps_end_relations(tid, t.n_i, t.head[DL_WS_E0A], t.head[DL_WS_E0B], t.head[DL_WS_E1A], t.head[DL_WS_E1B], s.ps); break;
        case 5: dl_ws_quadrature(tid, nthr, t, dm, s); break;
        case 6: dl_ws_reduce(tid, nthr, s); break;
        default: dl_ws_output(tid, nthr, t, dm, s, row);
    }
}
#define DL_WS_PHASES 8
