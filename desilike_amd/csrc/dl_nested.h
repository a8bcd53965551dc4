// dl_nested.h -- the phases of one iteration of batched nested sampling for one run of live points (dl_nested.hip; Skilling 2006, "Nested sampling for general
// Bayesian computation", with M points deleted per iteration and a random walk under the hard likelihood constraint: none of the arithmetic of the dynesty,
// PolyChord or nautilus the reference wraps), written once for the device (a workgroup per run, a wavefront per replaced point) and for the host
// (tests/csrc/emulate_nested.cpp).
//
// Algorithm.  A RUN is N live points (position x [P], log-likelihood L, log-prior pi, all finite) and the scalars: log X (the log prior volume, from 0), log Z (from
// -inf), the proposal scale s (from 1), an iteration counter, a mode (climbing or at rest).  K independent runs go side by side; M = ndelete points die per
// iteration, 1 <= M <= N / 2.  One ITERATION of a run that is not at rest:
//   1. rank.  The live points ordered by (L, slot) ascending (equal L: the lower slot first; -0 counts as +0).  The M lowest are the dead, in rank order j = 0 .. M - 1;
//      L* = L of rank M - 1;
//   2. evidence.  log X_j = log X_{j-1} - 1 / (N - j) with log X_{-1} = the run's log X, taken as log X - c_j on the inclusive prefix sums c_j of 1 / (N - j);
//      log w_j = log X_{j-1} + log(-expm1(-1 / (N - j))) (= log(X_{j-1} - X_j): the weights of all dead points and the closing X / N of the live ones sum to 1);
//      log Z <- logaddexp(log Z, L* + log sum_j exp(L_j - L* + log w_j)), the sum taken with log X factored out as well (every term is then <= 2 / N whatever log X
//      is: nothing underflows at a small prior volume); log X <- log X_{M-1};
//   3. moments.  Mean and covariance of the N - M survivors with equal weights 1 / (N - M), about the run's first survivor in slot order (dl_smc_moment_partial on
//      the points from that slot on, the dead among them at weight 0); the lower Cholesky factor with the pivot rule and the diagonal fallback of dl_smc_factor;
//   4. seeds.  The dead slot of rank j takes x, L, pi of the survivor of rank M + floor(u (N - M)), one uniform u in [0, 1) per (iteration, run, j);
//   5. mutation: n_steps sweeps over the M replaced slots only.  x' = x + s (2.38 / sqrt(P)) C z; one evaluation of the K M proposals, compacted as [K, M, P]; accepted
//      iff status = 0, L' and pi' finite, L' > L* STRICTLY and log u < pi' - pi.  After each sweep, a = the accepted fraction of the run's M proposals:
//      s <- clamp(s exp(a - target_acceptance), 1e-3, 1e3) (dl_smc_next_scale);
//   6. record.  The M dead: x, L, pi, log w.  One history row: log X, log Z + offset, L*, mean acceptance, s, log Z_rem + offset with log Z_rem = log X +
//      log mean_i exp(L_i) over the new live set.  The run goes to rest when log Z_rem - logaddexp(log Z, log Z_rem) < log(dlogz).  A run at rest does nothing and
//      records nothing.
// The closing contribution (the N live points at weight X / N each), the information and the error of log Z are taken by the caller from the state (desilike_amd/nested.py).
//
// Sums.  Every sum over points has a fixed order (a thread's strided partial, the wavefront's butterfly, the wavefronts in index order; the prefix sums: a thread's
// slice in order, 32 threads' totals in order, the groups in order -- the scan of dl_smc.h), acceptance counts are integer atomics, there is no floating-point atomic:
// two runs give the same bits.  The sort is a bitonic network over (key, slot) pairs, all different: its result does not depend on the network.
//
// Random draws: Philox4x32-10 keyed by the seed, counter (iteration, sweep, global run id, stream word); streams 64-66 (dl_ens_fold.h uses 0-4, dl_mh.h 16-21,
// dl_nuts.h 32-34, dl_mclmc.h 48-49, dl_smc.h 50-52):
//   DL_NESTED_STREAM_PROPOSE | pair << 8 | rank << 16     Box-Muller pair (components 2 pair, 2 pair + 1) of the proposal of the replaced point of rank `rank` in sweep `sweep`
//   DL_NESTED_STREAM_ACCEPT | rank << 16                  the uniform of its Metropolis test
//   DL_NESTED_STREAM_SEED | rank << 16                    (sweep word 0) the uniform that chooses its seed among the survivors
// so a run is reproduced from (seed, run id, state, counter) alone, whatever the chunking of the calls.
// desilike_amd/nested.py (_HostNested) is the NumPy statement of the same stage machine.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "dl_smc.h"   // dl_smc_moment_partial, dl_smc_factor, the scan's upper levels, dl_smc_next_scale / sweep_scale, DlSmcSerial, DlSmcSerialGroup; dl_nuts.h, dl_philox.h

enum { DL_NESTED_STREAM_PROPOSE = 64, DL_NESTED_STREAM_ACCEPT = 65, DL_NESTED_STREAM_SEED = 66 };

#define DL_NESTED_MAX_P 64          // parameters (one lane each)
#define DL_NESTED_MAX_N 8192        // live points of a run (a multiple of 64): keys and slots of a run fit the LDS of one workgroup beside the scan
#define DL_NESTED_MAX_M (DL_NESTED_MAX_N / 2)
#define DL_NESTED_MAX_STEPS 1024    // sweeps per iteration
#define DL_NESTED_HIST 6            // per record: log X, log Z (offset included), L*, mean acceptance, scale, log Z_rem (offset included)
#define DL_NESTED_THREADS 1024      // threads of the rank and finish workgroups

// mode of a run
enum { DL_NESTED_REST, DL_NESTED_CLIMB };
// per-run scratch doubles [field][K]: L* of the iteration
enum { DL_NESTED_T_LSTAR, DL_NESTED_NT };

struct DlNestedArgs {
    double *x, *L, *pi;                  // the live points [K, N, P], [K, N], [K, N]
    double *logx, *logz, *scale;         // [K]
    long long* iter;                     // [K] iterations completed
    int32_t* mode;                       // [K] climbing or at rest (part of the state)
    int32_t* active;                     // [K] the run takes part in the iteration under way (climbing, its quota of records not full)
    const int32_t* sys_ids;              // [K]
    int32_t *rank, *seeds, *first;       // [K, N] slot of every rank; [K, M] slot of the seed of the dead of rank j; [K] first survivor in slot order
    double *W, *logw;                    // [K, N] 1 / (N - M) for a survivor, 0 for a dead point; [K, M] log w of the dead
    double *mean, *cov, *chol;           // [K, P], [K, P, P] (lower triangle), [K, P, P]
    const double* widths;                // [P] the priors' widths or scales
    double* tmp;                         // [DL_NESTED_NT][K]
    double *prop, *Lp, *pip;             // proposals [K, M, P] and their log-likelihoods, log-priors [K, M]
    const int32_t* status;               // [K, M]
    double* sscale;                      // [K, n_steps] scale in use in sweep j
    int32_t* acc;                        // [K, n_steps] proposals accepted in sweep j
    uint8_t* flags;                      // [K, n_steps, M] accept flags of the iteration
    double *hist, *out_coords, *out_L, *out_pi, *out_logw;   // records [K, quota, DL_NESTED_HIST], [K, quota, M, P], 3 x [K, quota, M]
    int32_t *out_count, *out_mode;       // [K] records of the batch so far; [K] the modes after the last iteration
    int32_t K, N, M, P, n_steps, quota;
    double target_acceptance, dlogz, offset;
    uint32_t k0, k1;
};

// ---- draws ------------------------------------------------------------------------------------------------------------------------------------------------------
// standard Gaussian of component i of the proposal of the replaced point of rank j
DL_NUTS_HD double dl_nested_gauss(long long it, int sweep, uint32_t run, int j, int i, uint32_t k0, uint32_t k1) {
    const DlPhilox r = dl_philox4x32((uint32_t)it, (uint32_t)sweep, run, (uint32_t)DL_NESTED_STREAM_PROPOSE | ((uint32_t)(i >> 1) << 8) | ((uint32_t)j << 16), k0, k1);
    return dl_box_muller(r, i);
}

// log of the uniform of the Metropolis test of the replaced point of rank j (-inf for the uniform 0)
DL_NUTS_HD double dl_nested_log_uniform(long long it, int sweep, uint32_t run, int j, uint32_t k0, uint32_t k1) {
    const DlPhilox r = dl_philox4x32((uint32_t)it, (uint32_t)sweep, run, (uint32_t)DL_NESTED_STREAM_ACCEPT | ((uint32_t)j << 16), k0, k1);
    return log(dl_uniform53(r.x[0], r.x[1]));
}

// the uniform in [0, 1) that chooses the seed of the dead point of rank j
DL_NUTS_HD double dl_nested_seed_uniform(long long it, uint32_t run, int j, uint32_t k0, uint32_t k1) {
    const DlPhilox r = dl_philox4x32((uint32_t)it, 0u, run, (uint32_t)DL_NESTED_STREAM_SEED | ((uint32_t)j << 16), k0, k1);
    return dl_uniform53(r.x[0], r.x[1]);
}

// ---- 1: rank ----------------------------------------------------------------------------------------------------------------------------------------------------
// order-preserving 64-bit key of a double that is not NaN (-0 as +0): a < b  <=>  key(a) < key(b)
DL_NUTS_HD uint64_t dl_nested_key(double L) {
    L += 0.;
    uint64_t b;
    memcpy(&b, &L, sizeof(b));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

DL_NUTS_HD int dl_nested_pow2(int N) {
    int n2 = 64;
    while (n2 < N) n2 <<= 1;
    return n2;
}

// keys [n2], slots [n2] of the run: entries N .. n2 - 1 hold the key above every double
DL_NUTS_HD void dl_nested_load_keys(int tid, int T, const double* L, int N, int n2, uint64_t* keys, int32_t* slots) {
    for (int i = tid; i < n2; i += T) {
        keys[i] = i < N ? dl_nested_key(L[i]) : ~0ull;
        slots[i] = i;
    }
}

// the compare-exchanges of thread tid in one stage (size, stride) of the bitonic network over n2 pairs (a barrier between two stages)
DL_NUTS_HD void dl_nested_bitonic_stage(int tid, int T, uint64_t* keys, int32_t* slots, int n2, int size, int stride) {
    for (int t = tid; t < n2 / 2; t += T) {
        const int i = ((t / stride) * 2 * stride) + (t % stride), j = i + stride;
        const bool up = (i & size) == 0;
        const uint64_t ki = keys[i], kj = keys[j];
        const int32_t si = slots[i], sj = slots[j];
        const bool greater = ki > kj || (ki == kj && si > sj);
        if (greater == up) { keys[i] = kj; keys[j] = ki; slots[i] = sj; slots[j] = si; }
    }
}

// ---- 2: evidence ------------------------------------------------------------------------------------------------------------------------------------------------
// first phase of the inclusive prefix sums cum [M] of 1 / (N - j) by T threads (then dl_smc_scan_groups, dl_smc_scan_top, dl_smc_scan_offsets with M for N)
DL_NUTS_HD void dl_nested_scan_slices(int tid, int T, int N, int M, double* cum, double* tot) {
    const int S = (M + T - 1) / T, i0 = tid * S, i1 = i0 + S < M ? i0 + S : M;
    double run = 0.;
    for (int i = i0; i < i1; ++i) { run += 1. / (double)(N - i); cum[i] = run; }
    tot[tid] = run;
}

// log w_j of the dead point of rank j of a run at log prior volume logx
DL_NUTS_HD double dl_nested_logw(double logx, const double* cum, int N, int j) {
    return (logx - (j ? cum[j - 1] : 0.)) + log(-expm1(-1. / (double)(N - j)));
}

struct DlNestedLevel {
    double lstar, logx, logz;      // L* and the run's log X, log Z after the iteration
};

// G: the threads that share a run's sums (dl_smc.h); L [N] by slot, slots [>= M] by rank; every thread of the group gets the same result
template <class G>
DL_NUTS_HD void dl_nested_evidence(const G& g, const double* L, const int32_t* slots, const double* cum, int N, int M, double logx, double logz, DlNestedLevel* t) {
    const double lstar = L[slots[M - 1]];
    double s = 0., unused = 0.;
    for (int j = g.tid; j < M; j += g.n) s += exp((L[slots[j]] - lstar) + dl_nested_logw(0., cum, N, j));
    g.sum2(s, unused);
    t->lstar = lstar;
    t->logx = logx - cum[M - 1];
    t->logz = dl_nuts_logaddexp(logz, (lstar + logx) + log(s));
}

// ---- 4: seeds ---------------------------------------------------------------------------------------------------------------------------------------------------
// rank of the survivor that seeds a dead point
DL_NUTS_HD int dl_nested_seed_rank(double u, int N, int M) {
    int r = (int)(u * (double)(N - M));
    if (r > N - M - 1) r = N - M - 1;
    return M + r;
}

// ---- 5: mutation ------------------------------------------------------------------------------------------------------------------------------------------------
// proposal of the replaced point of rank j at x with scale s and factor C [P, P]
template <class L>
DL_NUTS_HD void dl_nested_propose(const L& l, const double* C, double s, const DlNutsVec<L>& x, long long it, int sweep, uint32_t run, int j, uint32_t k0, uint32_t k1,
                                  DlNutsVec<L>& xp) {
    DlNutsVec<L> z, cz;
    for (int c = 0; c < L::W; ++c) z.x[c] = l.on(c) ? dl_nested_gauss(it, sweep, run, j, l.comp(c), k0, k1) : 0.;
    dl_nuts_matvec(l, C, z, cz);
    const double f = s * (2.38 / sqrt((double)l.P));
    for (int c = 0; c < L::W; ++c) xp.x[c] = x.x[c] + f * cz.x[c];
}

DL_NUTS_HD bool dl_nested_accept(double lstar, double pi, double Lp, double pip, int status, double logu) {
    if (status != 0 || !dl_smc_live(Lp) || !dl_smc_live(pip)) return false;
    return Lp > lstar && logu < pip - pi;
}

// ---- 6: record --------------------------------------------------------------------------------------------------------------------------------------------------
// log Z_rem = logx + log mean_i exp(L_i) over the live points L [N]
template <class G>
DL_NUTS_HD double dl_nested_remaining(const G& g, const double* L, int N, double logx) {
    double lmax = -HUGE_VAL, s = 0., unused = 0.;
    for (int i = g.tid; i < N; i += g.n) lmax = L[i] > lmax ? L[i] : lmax;
    lmax = g.max(lmax);
    for (int i = g.tid; i < N; i += g.n) s += exp(L[i] - lmax);
    g.sum2(s, unused);
    return (logx + lmax) + log(s / N);
}

DL_NUTS_HD bool dl_nested_at_rest(double logz, double logzrem, double dlogz) { return logzrem - dl_nuts_logaddexp(logz, logzrem) < log(dlogz); }
