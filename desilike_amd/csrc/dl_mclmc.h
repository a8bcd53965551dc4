// dl_mclmc.h -- one integrator stage of microcanonical Langevin Monte Carlo for one chain (dl_mclmc.hip; reference: desilike/samplers/mclmc.py, blackjax.mclmc
// underneath; Robnik, De Luca, Silverstein & Seljak, arXiv:2212.08549), written once for the device (one wavefront per chain, one lane per parameter component) and
// for the host (one thread holds every component: tests/csrc/emulate_mclmc.cpp).
//
// Algorithm.  S = -log-posterior, d = P parameters, the state of a chain is a position x and a unit momentum u.  The dynamics run in preconditioned coordinates
// x = x^ + A z: A = diag(sigma) (kept as its diagonal; blackjax's sqrt_diag_cov) or a dense lower Cholesky factor of a covariance.
//   * momentum update B(eps): g = A^T grad_x S, e = -g / |g|, delta = eps |g| / (d - 1),
//         u <- [u + e (sinh delta + (e.u)(cosh delta - 1))] / [cosh delta + (e.u) sinh delta],   then u <- u / |u|,
//     the exact flow of du/dt = -(1 - u u^T) grad S / (d - 1) at fixed x.  With zeta = exp(-delta), numerator and denominator times 2 zeta:
//         u <- 2 zeta u + e [(1 - zeta^2) + (e.u)(1 - zeta)^2]   (normalised), 1 - zeta^2 = -expm1(-2 delta), 1 - zeta = -expm1(-delta): no overflow, no cancellation;
//     change of kinetic energy  dK = (d - 1) log(cosh delta + (e.u) sinh delta) = (d - 1) [delta - log 2 + log(1 + e.u + (1 - e.u) zeta^2)]
//                                  = (d - 1) [delta + log1p((1 - e.u) (zeta^2 - 1) / 2)]   (the form evaluated: the same quantity, exact for small delta too);
//     |g| = 0 is the identity (dK = 0);
//   * position update A(eps): x <- x + eps A u;
//   * integrators (blackjax.mcmc.integrators): isokinetic_leapfrog  B(eps/2) A(eps) B(eps/2)            -- one gradient per step (the closing B and the next step's
//     opening B use the same gradient, kept with the chain); isokinetic_mclachlan  B(l eps) A(eps/2) B((1 - 2l) eps) A(eps/2) B(l eps), l = 0.1931833275037836 -- two;
//     energy change of the step  dE = sum dK + S(x') - S(x);
//   * partial refresh after every step: u <- (u + nu z) / |u + nu z|, nu = sqrt((exp(2 eps / L) - 1) / d), z standard Gaussians; L = +inf: no refresh;
//   * LEAVING THE SUPPORT.  There is no Metropolis step (blackjax returns NaN from there on).  Here: if the log-posterior (or a gradient component) of ANY pending
//     position of a step is not finite, or dE is not finite, the whole step is undone: the chain goes back to the step's start (x0, its gradient and log-posterior),
//     the momentum becomes -u0 (the chain leaves the way it came), the refresh is still applied, the record's flag is 1 and dE is recorded as 0.  A chain marked so in
//     the first stage of a two-stage step waits at x0 for the step's end (x0 is its pending position: its row is evaluated and ignored);
//   * step-size controller (per chain, switch `adapt`; the energy-variance controller of the paper, blackjax's mclmc_adaptation): after a step with energy change dE
//         xi = dE^2 / (d desired_energy_var) + 1e-8,  w = exp(-(log xi / (6 trust_in_estimate))^2 / 2),
//         a <- gamma a + w xi / eps^6,  b <- gamma b + w,  gamma = (n_eff - 1) / (n_eff + 1),  eps <- (a / b)^(-1/6), capped at eps_max;
//     an undone step leaves a and b alone, sets eps <- 0.8 eps and eps_max to that value from then on;
//   * moments (switch `moments`): per chain sum w, sum w x, sum w x^2 with w = the step size in use, over the steps that were not undone (blackjax's streaming
//     average of its second warm-up phase); the host pools them into the preconditioner.
//
// Stage machine: as in dl_nuts.h the kernel is given the log-posterior and gradient of every chain's PENDING position, finishes the stage (the B update with that
// gradient) and writes the next pending position; the last stage of a step completes it (energy, undo, refresh, controller, moments, record) and -- unless it is
// the last step of the call -- opens the next step (B with the gradient just received, first drift).  All chains are at the same stage: `stage` is a launch argument
// (-1: open a step from the chain's current point).  Between two calls of dl_mclmc_run every chain rests at a step boundary: (x, u, gradient, log-posterior, eps).
// A chain whose record count reached the quota of the batch rests until the next batch.
//
// Random draws: Philox4x32-10 keyed by the seed, counter (step lo, step hi, chain id, stream word), step = the chain's own step counter; streams 48-49
// (dl_ens_fold.h uses 0-4, dl_mh.h 16-21, dl_nuts.h 32-34):
//   DL_MCLMC_STREAM_REFRESH | pair << 8    Box-Muller pair (components 2 pair, 2 pair + 1) of the refresh that closes step `step`
//   DL_MCLMC_STREAM_INIT | pair << 8       the same for the unit momentum z / |z| drawn where a state is set without momenta
// so a chain is reproduced from (seed, chain id, position, momentum, step counter) alone, whatever the rank or chunking that runs it.
// desilike_amd/mclmc.py (_HostMCLMC) is the NumPy statement of the same stage machine.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dl_nuts.h"   // DlNutsVec, dl_nuts_load / store / dot / matvec, DlNutsSerial, dl_philox.h

enum { DL_MCLMC_STREAM_REFRESH = 48, DL_MCLMC_STREAM_INIT = 49 };

#define DL_MCLMC_MAX_P 64      // parameters (one lane each); at least 2: one parameter has no isokinetic dynamics (d - 1 = 0)
#define DL_MCLMC_INFO 3        // per record: energy change dE, flag (1: the step was undone), step size in use
#define DL_MCLMC_LAMBDA 0.1931833275037836

// vector fields of the state, [field][chain][P]: position, its gradient, momentum, momentum at the step's start, pending position, moments
enum { DL_MCLMC_V_X, DL_MCLMC_V_G, DL_MCLMC_V_U, DL_MCLMC_V_U0, DL_MCLMC_V_XN, DL_MCLMC_V_SX, DL_MCLMC_V_SXX, DL_MCLMC_NV };
// double fields, [field][chain]: log-posterior of x (offset included), step size, its cap, the controller's averages, sum of dK of the open step, sum of weights
enum { DL_MCLMC_D_LP, DL_MCLMC_D_EPS, DL_MCLMC_D_EPSMAX, DL_MCLMC_D_CA, DL_MCLMC_D_CB, DL_MCLMC_D_DK, DL_MCLMC_D_SW, DL_MCLMC_ND };
// int fields, [field][chain]; ACTIVE: a step is open; BAD: a pending position of the open step left the support
enum { DL_MCLMC_I_ACTIVE, DL_MCLMC_I_BAD, DL_MCLMC_NI };

struct DlMclmcArgs {
    double* vec;                  // [DL_MCLMC_NV][C][P]
    double* dsc;                  // [DL_MCLMC_ND][C]
    int32_t* isc;                 // [DL_MCLMC_NI][C]
    long long* iter;              // [C] steps completed by each chain
    const int32_t* chain_ids;     // [C]
    const double* fac;            // A: [P] (diagonal) or [P, P] (dense, lower)
    const double* fact;           // A^T [P, P] (dense only)
    const double* lp_new;         // [C] log-posterior of the pending positions (before the offset)
    const double* g_new;          // [C, P] its gradient
    double *out_coords, *out_logp, *out_info;   // records [C, cap, P], [C, cap], [C, cap, DL_MCLMC_INFO]
    int32_t* out_count;           // [C] records of the batch so far
    int32_t C, P, dense, cap, quota, thin_by, nstage, adapt, moments;
    double cb[3], ca[2];          // the integrator: B(cb[0] eps) A(ca[0] eps) B(cb[1] eps) [A(ca[1] eps) B(cb[2] eps)]
    double L, offset, energy_var, trust, gamma;
    uint32_t k0, k1;
};

// the integrator's coefficients; false: unknown integrator (0 isokinetic_leapfrog, 1 isokinetic_mclachlan)
DL_NUTS_HD bool dl_mclmc_integrator(int integrator, int32_t* nstage, double* cb, double* ca) {
    if (integrator == 0) {
        *nstage = 1; cb[0] = 0.5; cb[1] = 0.5; cb[2] = 0.; ca[0] = 1.; ca[1] = 0.;
        return true;
    }
    if (integrator == 1) {
        *nstage = 2; cb[0] = DL_MCLMC_LAMBDA; cb[1] = 1. - 2. * DL_MCLMC_LAMBDA; cb[2] = DL_MCLMC_LAMBDA; ca[0] = 0.5; ca[1] = 0.5;
        return true;
    }
    return false;
}

// standard Gaussian of component i of the draw of `stream` at step `it`
DL_NUTS_HD double dl_mclmc_gauss(long long it, uint32_t chain, int i, uint32_t stream, uint32_t k0, uint32_t k1) {
    const DlPhilox r = dl_philox4x32((uint32_t)it, (uint32_t)((unsigned long long)it >> 32), chain, stream | ((uint32_t)(i >> 1) << 8), k0, k1);
    return dl_box_muller(r, i);
}

// out = A v (transpose = false) or A^T v
template <class L>
DL_NUTS_HD void dl_mclmc_apply(const L& l, const DlMclmcArgs& a, bool transpose, const DlNutsVec<L>& v, DlNutsVec<L>& out) {
    if (a.dense) dl_nuts_matvec(l, transpose ? a.fact : a.fac, v, out);
    else for (int j = 0; j < L::W; ++j) out.x[j] = l.on(j) ? a.fac[l.comp(j)] * v.x[j] : 0.;
}

// u <- u / |u| (left alone where the norm is not positive and finite)
template <class L>
DL_NUTS_HD void dl_mclmc_normalise(const L& l, DlNutsVec<L>& u) {
    const double n = sqrt(dl_nuts_dot(l, u, u));
    if (n > 0. && n < HUGE_VAL) for (int j = 0; j < L::W; ++j) u.x[j] = u.x[j] / n;
}

// B(h): the exact momentum flow over h with the gradient gq of the LOG-POSTERIOR (grad S = -gq) in the coordinates of x; returns dK
template <class L>
DL_NUTS_HD double dl_mclmc_bstep(const L& l, const DlMclmcArgs& a, DlNutsVec<L>& u, const DlNutsVec<L>& gq, double h) {
    DlNutsVec<L> t;
    dl_mclmc_apply(l, a, true, gq, t);      // t = A^T gq = -g: e = t / |t|
    const double n2 = dl_nuts_dot(l, t, t);
    if (!(n2 > 0.)) return 0.;
    const double nrm = sqrt(n2), delta = h * nrm / (a.P - 1), eu = dl_nuts_dot(l, t, u) / nrm;
    const double zeta = exp(-delta), m1 = expm1(-delta), m2 = expm1(-2. * delta);
    const double ce = -m2 + eu * (m1 * m1);
    for (int j = 0; j < L::W; ++j) u.x[j] = (2. * zeta) * u.x[j] + (t.x[j] / nrm) * ce;
    dl_mclmc_normalise(l, u);
    return (a.P - 1) * (delta + log1p(0.5 * (1. - eu) * m2));
}

// opens a step from (x, u, g) with step size eps: u0 kept, B(cb[0] eps), the first drift
template <class L>
DL_NUTS_HD void dl_mclmc_open(const L& l, const DlMclmcArgs& a, int c, const DlNutsVec<L>& x, DlNutsVec<L>& u, const DlNutsVec<L>& g, double eps) {
    const size_t C = a.C, P = a.P;
    auto row = [&](int f) { return a.vec + ((size_t)f * C + c) * P; };
    dl_nuts_store(l, u, row(DL_MCLMC_V_U0));
    const double dk = dl_mclmc_bstep(l, a, u, g, a.cb[0] * eps);
    DlNutsVec<L> au, xn;
    dl_mclmc_apply(l, a, false, u, au);
    for (int j = 0; j < L::W; ++j) xn.x[j] = x.x[j] + (a.ca[0] * eps) * au.x[j];
    dl_nuts_store(l, u, row(DL_MCLMC_V_U));
    dl_nuts_store(l, xn, row(DL_MCLMC_V_XN));
    { a.dsc[DL_MCLMC_D_DK * C + c] = dk; a.isc[DL_MCLMC_I_BAD * C + c] = 0; a.isc[DL_MCLMC_I_ACTIVE * C + c] = 1; }
}

// stage -1: chains below their quota open a step from their current point; stage s in [0, nstage): the stage proper; open_next: the last stage opens the next step
template <class L>
DL_NUTS_HD void dl_mclmc_chain_stage(const L& l, const DlMclmcArgs& a, int c, int stage, int open_next) {
    const size_t C = a.C, P = a.P;
    double* d = a.dsc;
    int32_t* I = a.isc;
    auto row = [&](int f) { return a.vec + ((size_t)f * C + c) * P; };
    DlNutsVec<L> x, u, g;
    if (stage < 0) {
        if (a.out_count[c] >= a.quota) { I[DL_MCLMC_I_ACTIVE * C + c] = 0; return; }
        dl_nuts_load(l, x, row(DL_MCLMC_V_X)); dl_nuts_load(l, u, row(DL_MCLMC_V_U)); dl_nuts_load(l, g, row(DL_MCLMC_V_G));
        dl_mclmc_open(l, a, c, x, u, g, d[DL_MCLMC_D_EPS * C + c]);
        return;
    }
    if (!I[DL_MCLMC_I_ACTIVE * C + c]) return;
    const double eps = d[DL_MCLMC_D_EPS * C + c];
    int bad = I[DL_MCLMC_I_BAD * C + c];
    double dk = d[DL_MCLMC_D_DK * C + c];
    const double sw = d[DL_MCLMC_D_SW * C + c];
    // the pending position's log-posterior and gradient; outside the support (or a gradient that is not finite): the step will be undone
    double lp = a.lp_new[c];
    const bool inside = lp == lp && fabs(lp) < HUGE_VAL;
    lp += a.offset;
    dl_nuts_load(l, g, a.g_new + (size_t)c * P);
    double notfinite[L::W];
    for (int j = 0; j < L::W; ++j) notfinite[j] = l.on(j) && !(fabs(g.x[j]) < HUGE_VAL) ? 1. : 0.;
    if (!inside || l.sum(notfinite) > 0.) bad = 1;
    dl_nuts_load(l, u, row(DL_MCLMC_V_U));
    if (!bad) dk += dl_mclmc_bstep(l, a, u, g, a.cb[stage + 1] * eps);
    if (stage + 1 < a.nstage) {              // the next drift (an undone step waits at its start)
        DlNutsVec<L> xn;
        if (!bad) {
            DlNutsVec<L> au;
            dl_nuts_load(l, xn, row(DL_MCLMC_V_XN));
            dl_mclmc_apply(l, a, false, u, au);
            for (int j = 0; j < L::W; ++j) xn.x[j] += (a.ca[stage + 1] * eps) * au.x[j];
            dl_nuts_store(l, u, row(DL_MCLMC_V_U));
        } else dl_nuts_load(l, xn, row(DL_MCLMC_V_X));
        dl_nuts_store(l, xn, row(DL_MCLMC_V_XN));
        { d[DL_MCLMC_D_DK * C + c] = dk; I[DL_MCLMC_I_BAD * C + c] = bad; }
        return;
    }
    // ---- the step is complete: energy, undo, refresh, controller, moments, record ---------------------------------------------------------------------------
    const double lp0 = d[DL_MCLMC_D_LP * C + c];
    double de = dk - (lp - lp0);
    if (!bad && !(fabs(de) < HUGE_VAL)) bad = 1;
    if (bad) {
        dl_nuts_load(l, x, row(DL_MCLMC_V_X)); dl_nuts_load(l, g, row(DL_MCLMC_V_G)); dl_nuts_load(l, u, row(DL_MCLMC_V_U0));
        for (int j = 0; j < L::W; ++j) u.x[j] = -u.x[j];
        lp = lp0; de = 0.;
    } else {
        dl_nuts_load(l, x, row(DL_MCLMC_V_XN));
        dl_nuts_store(l, x, row(DL_MCLMC_V_X)); dl_nuts_store(l, g, row(DL_MCLMC_V_G));
    }
    const long long it = a.iter[c];
    if (a.L < HUGE_VAL) {
        const double nu = sqrt(expm1(2. * eps / a.L) / a.P);
        const uint32_t chain = (uint32_t)a.chain_ids[c];
        for (int j = 0; j < L::W; ++j) if (l.on(j)) u.x[j] += nu * dl_mclmc_gauss(it, chain, l.comp(j), DL_MCLMC_STREAM_REFRESH, a.k0, a.k1);
        dl_mclmc_normalise(l, u);
    }
    dl_nuts_store(l, u, row(DL_MCLMC_V_U));
    double eps_next = eps;
    if (a.adapt) {
        double epsmax = d[DL_MCLMC_D_EPSMAX * C + c], ca = d[DL_MCLMC_D_CA * C + c], cb = d[DL_MCLMC_D_CB * C + c];
        if (bad) {
            eps_next = 0.8 * eps; epsmax = eps_next;
        } else {
            const double xi = de * de / (a.P * a.energy_var) + 1e-8, r = log(xi) / (6. * a.trust), w = exp(-0.5 * r * r), e2 = eps * eps;
            ca = a.gamma * ca + w * (xi / (e2 * e2 * e2));
            cb = a.gamma * cb + w;
            const double e = pow(ca / cb, -1. / 6.);
            if (e > 0. && e < HUGE_VAL) eps_next = e;
            if (eps_next > epsmax) eps_next = epsmax;
        }
        { d[DL_MCLMC_D_EPS * C + c] = eps_next; d[DL_MCLMC_D_EPSMAX * C + c] = epsmax; d[DL_MCLMC_D_CA * C + c] = ca; d[DL_MCLMC_D_CB * C + c] = cb; }
    }
    if (a.moments && !bad) {
        DlNutsVec<L> sx, sxx;
        dl_nuts_load(l, sx, row(DL_MCLMC_V_SX)); dl_nuts_load(l, sxx, row(DL_MCLMC_V_SXX));
        for (int j = 0; j < L::W; ++j) { sx.x[j] += eps * x.x[j]; sxx.x[j] += eps * (x.x[j] * x.x[j]); }
        dl_nuts_store(l, sx, row(DL_MCLMC_V_SX)); dl_nuts_store(l, sxx, row(DL_MCLMC_V_SXX));
        d[DL_MCLMC_D_SW * C + c] = sw + eps;
    }
    int count = a.out_count[c];
    if ((it + 1) % a.thin_by == 0) {
        const size_t r = (size_t)c * a.cap + count;
        dl_nuts_store(l, x, a.out_coords + r * P);
        {
            a.out_logp[r] = lp;      // (offset included)
            double* info = a.out_info + r * DL_MCLMC_INFO;
            info[0] = de; info[1] = bad; info[2] = eps;
        }
        ++count;
    }
    { d[DL_MCLMC_D_LP * C + c] = lp; a.iter[c] = it + 1; a.out_count[c] = count; }
    if (open_next && count < a.quota) dl_mclmc_open(l, a, c, x, u, g, eps_next);
    else I[DL_MCLMC_I_ACTIVE * C + c] = 0;
}
