// dl_smc.h -- the phases of one iteration of adaptive tempered sequential Monte Carlo for one system of particles (dl_smc.hip; Del Moral, Doucet & Jasra 2006,
// "Sequential Monte Carlo samplers"; the skeleton of PocoMC with precondition=False, sample='rwm' -- none of its flows, t-preconditioned Crank-Nicolson or persistent
// reweighting), written once for the device (a workgroup per system, a wavefront per particle) and for the host (tests/csrc/emulate_smc.cpp).
//
// Algorithm.  A SYSTEM is N particles (position x [P], log-likelihood L, log-prior pi) and the scalars: inverse temperature beta (from 0), logZ (from 0), proposal
// scale s, an iteration counter.  K independent systems run side by side; the target at level beta is pi(x) L(x)^beta (the likelihood alone is tempered).
// One ITERATION of a system:
//   1. next temperature.  Lmax = max_i L_i over the live particles (L finite); incremental weights w_i(D) = exp(D (L_i - Lmax)), exactly 0 where L_i is not finite;
//      ESS(D) = (sum w)^2 / sum w^2.  target = ess_fraction N (ess_fraction x the number of live particles where that number does not exceed ess_fraction N: the
//      level could not be met otherwise).  If ESS(1 - beta) >= target: D = 1 - beta and beta becomes EXACTLY 1.  Otherwise 64 halvings of the bracket (0, 1 - beta)
//      (ESS decreases with D), D = the bracket's midpoint.  A system already at beta = 1 has D = 0: it skips 2 and 3 and only mutates (a "sweep");
//   2. evidence.  logZ += log(sum w / N) + D Lmax;
//   3. moments and resampling.  W_i = w_i / sum w.  Mean and covariance of the particles under W (before resampling), taken about the system's first particle
//      (y = x - x_0: a coordinate all particles share has EXACTLY zero variance): m = sum W y, cov_ij = sum W (y_i - m_i)(y_j - m_j).  C = its lower Cholesky factor;
//      a pivot that is not finite and above 1e-10 of its diagonal entry (a singular covariance: what is left there is rounding error): C = diag(sqrt(cov_ii))
//      instead; there a diagonal entry that is not positive and finite is replaced by the prior's width or scale of that component.  Systematic resampling with
//      one uniform u in (0, 1] per system and iteration: the ancestor of slot i is the first j with cum_j >= min((i + u) / N, cum_{N-1}) on the inclusive
//      prefix sums of W; x, L, pi are gathered through a second buffer (systems that do not resample copy);
//   4. mutation: n_steps random-walk Metropolis sweeps.  x' = x + s (2.38 / sqrt(P)) C z, z standard normal; one evaluation of all K N proposals gives L', pi',
//      status; accepted iff status = 0, L' and pi' finite and log u < beta (L' - L) + (pi' - pi).  After each sweep, a = the system's acceptance fraction:
//      s <- clamp(s exp(a - target_acceptance), 1e-3, 1e3);
//   5. record (beta, logZ, ESS at the chosen D (N for a sweep), mean acceptance of the sweeps, s); the counter advances.  A sweep at beta = 1 also records the N
//      particles and their L + pi + offset.
//
// Sums.  Every sum over particles has a fixed order (a thread's strided partial, the wavefront's butterfly, the wavefronts in index order; the prefix sums: a thread's
// slice in order, 32 threads' totals in order, the groups in order), acceptance counts are integer atomics: two runs give the same bits.
//
// Random draws: Philox4x32-10 keyed by the seed, counter (iteration, sweep, global system id, stream word); streams 50-52 (dl_ens_fold.h uses 0-4, dl_mh.h 16-21,
// dl_nuts.h 32-34, dl_mclmc.h 48-49):
//   DL_SMC_STREAM_PROPOSE | pair << 8 | slot << 16     Box-Muller pair (components 2 pair, 2 pair + 1) of the proposal of particle slot `slot` in sweep `sweep`
//   DL_SMC_STREAM_ACCEPT | slot << 16                  the uniform of its Metropolis test
//   DL_SMC_STREAM_RESAMPLE                             (sweep word 0) 1 - the uniform of the iteration's systematic resampling
// so a system is reproduced from (seed, system id, state, counter) alone, whatever the chunking of the calls.
// desilike_amd/smc.py (_HostSMC) is the NumPy statement of the same stage machine.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dl_nuts.h"   // DlNutsVec, dl_nuts_load / store / matvec, DlNutsSerial, dl_philox.h

enum { DL_SMC_STREAM_PROPOSE = 50, DL_SMC_STREAM_ACCEPT = 51, DL_SMC_STREAM_RESAMPLE = 52 };

#define DL_SMC_MAX_P 64          // parameters (one lane each)
#define DL_SMC_MAX_N 16384       // particles of a system (a multiple of 64): their log-likelihoods fit the LDS of one workgroup
#define DL_SMC_MAX_STEPS 1024    // Metropolis sweeps per iteration
#define DL_SMC_HIST 5            // per record: beta, logZ (offset included), ESS, mean acceptance, scale
#define DL_SMC_THREADS 1024      // threads of the temper and resample workgroups
#define DL_SMC_GROUP 32          // threads whose totals one thread scans (second level of the prefix sums)
#define DL_SMC_PIVOT 1e-10       // a pivot of the Cholesky factor below this fraction of its diagonal entry is rounding error: the covariance is singular
#define DL_SMC_MOMENT_WAVES 16   // wavefronts of a moments workgroup: particles w, w + 16, ... to wavefront w

// per-system scratch doubles [field][K]: D of the iteration, its ESS, beta at the iteration's start
enum { DL_SMC_T_DELTA, DL_SMC_T_ESS, DL_SMC_T_BETA0, DL_SMC_NT };
// mode of a system in the iteration under way: at rest (its quota of records is full), a temperature level, a sweep at beta = 1
enum { DL_SMC_REST, DL_SMC_TEMPER, DL_SMC_SWEEP };

struct DlSmcArgs {
    double *x[2], *L[2], *pi[2];         // the particles, double-buffered: [K, N, P], [K, N], [K, N]; `cur` is the buffer an iteration starts from
    double *beta, *logz, *scale;         // [K]
    long long* iter;                     // [K] iterations completed
    const int32_t* sys_ids;              // [K]
    double *W, *cum;                     // [K, N] normalised weights, their inclusive prefix sums
    int32_t* anc;                        // [K, N] ancestors of the iteration
    double *mean, *cov, *chol;           // [K, P], [K, P, P] (lower triangle), [K, P, P]
    const double* widths;                // [P] the priors' widths or scales
    double* tmp;                         // [DL_SMC_NT][K]
    int32_t* mode;                       // [K]
    double *prop, *Lp, *pip;             // proposals [K, N, P] and their log-likelihoods, log-priors [K, N]
    const int32_t* status;               // [K, N]
    double* sscale;                      // [K, n_steps] scale in use in sweep j
    int32_t* acc;                        // [K, n_steps] proposals accepted in sweep j
    uint8_t* flags;                      // [K, n_steps, N] accept flags of the iteration
    double *hist, *out_coords, *out_logp;   // records [K, quota, DL_SMC_HIST], [K, quota, N, P], [K, quota, N]
    int32_t* out_count;                  // [K, 2] records, particle records of the batch so far
    int32_t K, N, P, n_steps, quota, cur;
    double ess_fraction, target_acceptance, offset;
    uint32_t k0, k1;
};

// ---- draws ------------------------------------------------------------------------------------------------------------------------------------------------------
// standard Gaussian of component i of the proposal of particle `slot`
DL_NUTS_HD double dl_smc_gauss(long long it, int sweep, uint32_t sys, int slot, int i, uint32_t k0, uint32_t k1) {
    const DlPhilox r = dl_philox4x32((uint32_t)it, (uint32_t)sweep, sys, (uint32_t)DL_SMC_STREAM_PROPOSE | ((uint32_t)(i >> 1) << 8) | ((uint32_t)slot << 16), k0, k1);
    return dl_box_muller(r, i);
}

// log of the uniform of the Metropolis test of particle `slot` (-inf for the uniform 0: accepted)
DL_NUTS_HD double dl_smc_log_uniform(long long it, int sweep, uint32_t sys, int slot, uint32_t k0, uint32_t k1) {
    const DlPhilox r = dl_philox4x32((uint32_t)it, (uint32_t)sweep, sys, (uint32_t)DL_SMC_STREAM_ACCEPT | ((uint32_t)slot << 16), k0, k1);
    return log(dl_uniform53(r.x[0], r.x[1]));
}

// the uniform in (0, 1] of the systematic resampling of iteration `it`
DL_NUTS_HD double dl_smc_resample_uniform(long long it, uint32_t sys, uint32_t k0, uint32_t k1) {
    const DlPhilox r = dl_philox4x32((uint32_t)it, 0u, sys, (uint32_t)DL_SMC_STREAM_RESAMPLE, k0, k1);
    return 1. - dl_uniform53(r.x[0], r.x[1]);
}

// ---- 1, 2: temperature and evidence ------------------------------------------------------------------------------------------------------------------------------
// G: the threads that share a system's sums -- int tid, n; sum2(a, b): both sums to every thread, in a fixed order; max(v)
struct DlSmcSerialGroup {
    int tid = 0, n = 1;
    void sum2(double&, double&) const {}
    double max(double v) const { return v; }
};

DL_NUTS_HD bool dl_smc_live(double L) { return fabs(L) < HUGE_VAL; }      // (false for NaN)

DL_NUTS_HD double dl_smc_weight(double L, double lmax, double delta) { return dl_smc_live(L) ? exp(delta * (L - lmax)) : 0.; }

template <class G>
DL_NUTS_HD double dl_smc_ess(const G& g, const double* L, int N, double lmax, double delta, double* sumw) {
    double s1 = 0., s2 = 0.;
    for (int i = g.tid; i < N; i += g.n) {
        const double w = dl_smc_weight(L[i], lmax, delta);
        s1 += w; s2 += w * w;
    }
    g.sum2(s1, s2);
    *sumw = s1;
    return s2 > 0. ? s1 * s1 / s2 : 0.;
}

struct DlSmcLevel {
    double delta, lmax, sumw, ess, beta, dlogz;      // beta: the new one
};

// the next level of a system at `beta` with log-likelihoods L [N] (every thread of the group gets the same result)
template <class G>
DL_NUTS_HD void dl_smc_temper(const G& g, const double* L, int N, double beta, double ess_fraction, DlSmcLevel* t) {
    double lmax = -HUGE_VAL, nlive = 0., unused = 0.;
    for (int i = g.tid; i < N; i += g.n)
        if (dl_smc_live(L[i])) { lmax = L[i] > lmax ? L[i] : lmax; nlive += 1.; }
    lmax = g.max(lmax);
    g.sum2(nlive, unused);
    t->lmax = lmax; t->beta = beta; t->delta = 0.; t->dlogz = 0.; t->sumw = N; t->ess = N;
    if (!(beta < 1.) || !(nlive > 0.)) return;       // a sweep (a system without a live particle cannot be weighted: dl_smc_set_particles refuses it)
    double target = ess_fraction * N;
    if (!(nlive > target)) target = ess_fraction * nlive;
    double hi = 1. - beta, lo = 0., sumw;
    double ess = dl_smc_ess(g, L, N, lmax, hi, &sumw), delta = hi;
    if (ess >= target) t->beta = 1.;
    else {
        for (int h = 0; h < 64; ++h) {
            const double mid = 0.5 * (lo + hi);
            if (dl_smc_ess(g, L, N, lmax, mid, &sumw) > target) lo = mid; else hi = mid;
        }
        delta = 0.5 * (lo + hi);
        ess = dl_smc_ess(g, L, N, lmax, delta, &sumw);
        t->beta = beta + delta;
        if (!(t->beta < 1.)) t->beta = 1.;
    }
    t->delta = delta; t->sumw = sumw; t->ess = ess;
    t->dlogz = log(sumw / N) + delta * lmax;
}

// ---- 3: moments -----------------------------------------------------------------------------------------------------------------------------------------------
// the share of wavefront w (particles w, w + nw, ...) of the weighted sums of row `row` of the covariance (row < 0: of the mean) about ref = the first particle;
// m: the mean of y = x - ref (not read for the mean)
template <class L>
DL_NUTS_HD void dl_smc_moment_partial(const L& l, const double* x, const double* W, int N, int w, int nw, int row, const DlNutsVec<L>& m, double mrow, DlNutsVec<L>& acc) {
    const int P = l.P;
    DlNutsVec<L> ref, v;
    dl_nuts_load(l, ref, x);
    const double refrow = row >= 0 ? x[row] : 0.;
    for (int j = 0; j < L::W; ++j) acc.x[j] = 0.;
    for (int n = w; n < N; n += nw) {
        const double wn = W[n];
        dl_nuts_load(l, v, x + (size_t)n * P);
        if (row < 0) for (int j = 0; j < L::W; ++j) acc.x[j] += wn * (v.x[j] - ref.x[j]);
        else {
            const double f = wn * ((x[(size_t)n * P + row] - refrow) - mrow);
            for (int j = 0; j < L::W; ++j) acc.x[j] += f * ((v.x[j] - ref.x[j]) - m.x[j]);
        }
    }
}

// ---- 3: Cholesky factor with its fallbacks -------------------------------------------------------------------------------------------------------------------
// C [P, P] (shared by the lanes; l.sync() orders a column's stores before the next column's loads) from the lower triangle of A [P, P]; false: a pivot failed
template <class L>
DL_NUTS_HD bool dl_smc_cholesky(const L& l, const double* A, double* C) {
    const int P = l.P;
    for (int j = 0; j < P; ++j) {
        double v[L::W];
        for (int jj = 0; jj < L::W; ++jj) {
            v[jj] = 0.;
            const int i = l.comp(jj);
            if (!l.on(jj) || i < j) continue;
            double s = A[(size_t)i * P + j];
            for (int k = 0; k < j; ++k) s -= C[(size_t)i * P + k] * C[(size_t)j * P + k];
            v[jj] = s;
        }
        const double d = l.at(v, j);
        if (!(d > DL_SMC_PIVOT * A[(size_t)j * P + j]) || !(d < HUGE_VAL)) return false;
        const double r = sqrt(d);
        for (int jj = 0; jj < L::W; ++jj) {
            const int i = l.comp(jj);
            if (l.on(jj)) C[(size_t)i * P + j] = i < j ? 0. : i == j ? r : v[jj] / r;
        }
        l.sync();
    }
    return true;
}

// the factor a system proposes with: the Cholesky factor of cov, or the diagonal fallback
template <class L>
DL_NUTS_HD void dl_smc_factor(const L& l, const double* cov, const double* widths, double* C) {
    const int P = l.P;
    const bool ok = dl_smc_cholesky(l, cov, C);
    l.sync();
    if (ok) return;
    for (int jj = 0; jj < L::W; ++jj) {
        const int i = l.comp(jj);
        if (!l.on(jj)) continue;
        const double d = cov[(size_t)i * P + i];
        for (int k = 0; k < P; ++k) C[(size_t)i * P + k] = 0.;
        C[(size_t)i * P + i] = d > 0. && d < HUGE_VAL ? sqrt(d) : widths[i];
    }
    l.sync();
}

// ---- 3: prefix sums and ancestors ----------------------------------------------------------------------------------------------------------------------------
// four phases of the inclusive prefix sums of W [N] by T threads (a barrier between two phases); tot [T], gtot [T / DL_SMC_GROUP] shared
DL_NUTS_HD void dl_smc_scan_slices(int tid, int T, const double* W, int N, double* cum, double* tot) {
    const int S = (N + T - 1) / T, i0 = tid * S, i1 = i0 + S < N ? i0 + S : N;
    double run = 0.;
    for (int i = i0; i < i1; ++i) { run += W[i]; cum[i] = run; }
    tot[tid] = run;
}

DL_NUTS_HD void dl_smc_scan_groups(int tid, int T, double* tot, double* gtot) {
    if (tid >= T / DL_SMC_GROUP) return;
    double run = 0.;
    for (int t = tid * DL_SMC_GROUP; t < (tid + 1) * DL_SMC_GROUP; ++t) { run += tot[t]; tot[t] = run; }
    gtot[tid] = run;
}

DL_NUTS_HD void dl_smc_scan_top(int tid, int T, double* gtot) {
    if (tid != 0) return;
    double run = 0.;
    for (int g = 0; g < T / DL_SMC_GROUP; ++g) { const double t = gtot[g]; gtot[g] = run; run += t; }
}

DL_NUTS_HD void dl_smc_scan_offsets(int tid, int T, int N, double* cum, const double* tot, const double* gtot) {
    const int S = (N + T - 1) / T, i0 = tid * S, i1 = i0 + S < N ? i0 + S : N;
    const double off = gtot[tid / DL_SMC_GROUP] + (tid % DL_SMC_GROUP ? tot[tid - 1] : 0.);
    for (int i = i0; i < i1; ++i) cum[i] += off;
}

// ancestor of slot i: the first j with cum_j >= min((i + u) / N, cum_{N-1})
DL_NUTS_HD int dl_smc_ancestor(const double* cum, int N, int i, double u) {
    double target = (i + u) / N;
    if (target > cum[N - 1]) target = cum[N - 1];
    int lo = 0, hi = N - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] >= target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// ---- 4: mutation ---------------------------------------------------------------------------------------------------------------------------------------------
DL_NUTS_HD double dl_smc_next_scale(double s, double a, double target_acceptance) {
    s *= exp(a - target_acceptance);
    return s < 1e-3 ? 1e-3 : s > 1e3 ? 1e3 : s;
}

// the scale of sweep j of a system: scale0 for the first, else the update of sweep j - 1's by its acceptance fraction
DL_NUTS_HD double dl_smc_sweep_scale(int j, double scale0, const double* sscale, const int32_t* acc, int N, double target_acceptance) {
    return j == 0 ? scale0 : dl_smc_next_scale(sscale[j - 1], (double)acc[j - 1] / N, target_acceptance);
}

// proposal of particle `slot` at x with scale s and factor C [P, P]
template <class L>
DL_NUTS_HD void dl_smc_propose(const L& l, const double* C, double s, const DlNutsVec<L>& x, long long it, int sweep, uint32_t sys, int slot, uint32_t k0, uint32_t k1,
                               DlNutsVec<L>& xp) {
    DlNutsVec<L> z, cz;
    for (int j = 0; j < L::W; ++j) z.x[j] = l.on(j) ? dl_smc_gauss(it, sweep, sys, slot, l.comp(j), k0, k1) : 0.;
    dl_nuts_matvec(l, C, z, cz);
    const double f = s * (2.38 / sqrt((double)l.P));
    for (int j = 0; j < L::W; ++j) xp.x[j] = x.x[j] + f * cz.x[j];
}

DL_NUTS_HD bool dl_smc_accept(double beta, double L, double pi, double Lp, double pip, int status, double logu) {
    if (status != 0 || !dl_smc_live(Lp) || !dl_smc_live(pip)) return false;
    return logu < beta * (Lp - L) + (pip - pi);
}

// the host's layout: one thread holds every component
struct DlSmcSerial : DlNutsSerial {
    void sync() const {}
};
