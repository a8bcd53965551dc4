// dl_nuts.h -- one step of the No-U-Turn sampler for one chain (dl_nuts.hip; reference: desilike/samplers/nuts.py, blackjax.nuts underneath), written once for
// the device (one wavefront per chain, one lane per parameter component) and for the host (one thread holds every component: tests/csrc/emulate_nuts.cpp).
//
// Algorithm: multinomial NUTS (Hoffman & Gelman 2014; Betancourt 2017, "A Conceptual Introduction to Hamiltonian Monte Carlo", appendix A) as Stan and blackjax run it:
//   * velocity-Verlet leapfrog, one step size eps per chain, inverse mass matrix Minv diagonal (kept as its diagonal) or dense; momentum p ~ N(0, M), M = Minv^-1:
//     p = z / sqrt(Minv_ii) or p = L_M z with L_M the Cholesky factor of M (computed once on the host), z standard Gaussians;
//   * H = -logposterior + p.Minv.p / 2; a leaf's log weight is H0 - H (H0: energy of the trajectory's start);
//   * the trajectory doubles up to max_num_doublings times; doubling d draws a direction v = +-1 and builds a subtree of 2^d leaves from the trajectory's end in
//     that direction, ONE LEAF PER STEP (no recursion);
//   * inside a subtree the proposal is chosen by uniform progressive sampling (leaf n replaces the subtree's candidate with probability w_n / sum_{m <= n} w_m);
//     when the completed subtree is joined, by biased progressive sampling (its candidate replaces the trajectory's with probability min(1, W_subtree / W_old));
//   * U-turn criterion: the generalised one, p#_a . rho > 0 and p#_b . rho > 0 (p# = Minv p, rho = sum of the momenta from end a to end b). Inside a subtree it is
//     checked on every sub-subtree that a leaf completes, from checkpoints (NumPyro's iterative_build_tree): at an even leaf n the checkpoint idx_max(n) keeps rho
//     before the leaf and p# of the leaf; an odd leaf completes the sub-subtrees whose first leaves are the checkpoints idx_min(n) .. idx_max(n).  A U-turn inside
//     a subtree drops the subtree and ends the trajectory.  When a subtree is joined, the criterion is checked on the whole trajectory and, as Stan >= 2.26 and
//     blackjax do, across the join: (left part + the right part's first leaf) and (the left part's last leaf + right part); any failure ends the trajectory
//     (the join, and its proposal, stand);
//   * divergence: H - H0 > divergence_threshold or H NaN; the divergent subtree is dropped and the trajectory ends.  The record's flag tells the two causes apart:
//     1 an energy error, 2 a leaf outside the support (log-posterior -inf: a prior bound; both are divergent for Stan and blackjax);
//   * acceptance statistic of a trajectory: mean over its leaves (the divergent one included) of min(1, exp(H0 - H_leaf)); reported depth: number of doublings
//     attempted (Stan's treedepth).
//
// Asynchronous chains: every step advances every moving chain by one leapfrog step.  The state of a chain is a fixed-size record (both ends (q, p, gradient), the
// trajectory's and the subtree's candidates (q, gradient, logposterior, energy), rho of the trajectory and of the subtree, the two log-sums of weights, depth, leaf,
// direction, max_num_doublings checkpoint vectors of rho and of p#, the pending leaf's position and half-kicked momentum).  dl_nuts_chain_step takes the
// log-posterior and gradient of the pending position, finishes its kick, processes the leaf and sets up the next pending leaf: the same subtree's next leaf, the
// first leaf of the next doubling from the trajectory's end, or -- when the trajectory ends -- the record, the dual-averaging update, a fresh momentum and the
// first drift of the next trajectory from the chosen point.  A chain that has recorded its quota of the current batch stops (idle) at its trajectory's end.
//
// Random draws: Philox4x32-10 keyed by the seed, counter (iteration lo, iteration hi, chain id, stream word), iteration = the chain's own trajectory counter;
// streams 32-34 (dl_ens_fold.h uses 0-4, dl_mh.h 16-21):
//   DL_NUTS_STREAM_MOMENTUM | pair << 8    Box-Muller pair (components 2 pair, 2 pair + 1)
//   DL_NUTS_STREAM_DIRECTION | d << 8      direction of doubling d (top bit of word 0) and the join uniform of doubling d (words 2, 3)
//   DL_NUTS_STREAM_SELECT | d << 8 | n << 12   selection uniform of leaf n of doubling d
// so a chain is reproduced from (seed, chain id, position, iteration counter) alone, whatever the rank, batch or chunking that runs it.
// desilike_amd/nuts.py (_HostNUTS) is the NumPy statement of the same step.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dl_philox.h"

#if defined(__HIPCC__)
#define DL_NUTS_HD __host__ __device__ inline
#else
#define DL_NUTS_HD inline
#endif

enum { DL_NUTS_STREAM_MOMENTUM = 32, DL_NUTS_STREAM_DIRECTION = 33, DL_NUTS_STREAM_SELECT = 34 };

#define DL_NUTS_MAX_P 64       // parameters (one lane each)
#define DL_NUTS_MAX_DEPTH 15   // max_num_doublings (leaf index of the selection stream: 2^15 leaves fit its bits 12 .. 26)
#define DL_NUTS_INFO 5         // per record: depth, leapfrog steps, divergent (0, 1 energy error, 2 left the support), acceptance statistic, energy

// vector fields of the state, [field][chain][P]; checkpoint k of rho at DL_NUTS_V_CK + k, of p# at DL_NUTS_V_CK + D + k
enum { DL_NUTS_V_QL, DL_NUTS_V_PL, DL_NUTS_V_GL, DL_NUTS_V_QR, DL_NUTS_V_PR, DL_NUTS_V_GR, DL_NUTS_V_QP, DL_NUTS_V_GP, DL_NUTS_V_QS, DL_NUTS_V_GS,
       DL_NUTS_V_QN, DL_NUTS_V_PN, DL_NUTS_V_PF, DL_NUTS_V_RHO, DL_NUTS_V_RHOS, DL_NUTS_V_CK };
// double fields, [field][chain]
enum { DL_NUTS_D_LPP, DL_NUTS_D_HP, DL_NUTS_D_LPS, DL_NUTS_D_HS, DL_NUTS_D_H0, DL_NUTS_D_LW, DL_NUTS_D_LWS, DL_NUTS_D_SACC,
       DL_NUTS_D_LOGEPS, DL_NUTS_D_HBAR, DL_NUTS_D_LOGBAR, DL_NUTS_D_MU, DL_NUTS_D_DACOUNT, DL_NUTS_ND };
// int fields, [field][chain]; ACTIVE: a leaf is pending (else the chain waits at a trajectory boundary for its next batch)
enum { DL_NUTS_I_DEPTH, DL_NUTS_I_LEAF, DL_NUTS_I_DIR, DL_NUTS_I_NLEAF, DL_NUTS_I_ACTIVE, DL_NUTS_NI };

struct DlNutsArgs {
    double* vec;                  // [DL_NUTS_V_CK + 2 D][C][P]
    double* dsc;                  // [DL_NUTS_ND][C]
    int32_t* isc;                 // [DL_NUTS_NI][C]
    long long* iter;              // [C] trajectories completed by each chain
    const int32_t* chain_ids;     // [C]
    const double* minv;           // [P] or [P, P]
    const double* lmass;          // [P, P] lower Cholesky factor of M = Minv^-1 (dense only)
    const double* lp_new;         // [C] log-posterior of the pending positions (before the offset)
    const double* g_new;          // [C, P] its gradient
    double *out_coords, *out_logp, *out_info;   // records [C, cap, P], [C, cap], [C, cap, DL_NUTS_INFO]
    int32_t* out_count;           // [C] records of the batch so far
    int32_t C, P, D, dense, cap, quota, thin_by, adapt;
    double threshold, offset, target;
    uint32_t k0, k1;
};

DL_NUTS_HD double dl_nuts_logaddexp(double a, double b) {
    if (a == -HUGE_VAL) return b;
    if (b == -HUGE_VAL) return a;
    const double m = a > b ? a : b;
    return m + log1p(exp(-fabs(a - b)));
}

// standard Gaussian of component i of the momentum of trajectory `it`
DL_NUTS_HD double dl_nuts_gauss(long long it, uint32_t chain, int i, uint32_t k0, uint32_t k1) {
    const DlPhilox r = dl_philox4x32((uint32_t)it, (uint32_t)((unsigned long long)it >> 32), chain, (uint32_t)DL_NUTS_STREAM_MOMENTUM | ((uint32_t)(i >> 1) << 8), k0, k1);
    return dl_box_muller(r, i);
}

// direction (+1 / -1) of doubling d and the uniform of its join
DL_NUTS_HD int dl_nuts_direction(long long it, uint32_t chain, int d, uint32_t k0, uint32_t k1, double* u_join) {
    const DlPhilox r = dl_philox4x32((uint32_t)it, (uint32_t)((unsigned long long)it >> 32), chain, (uint32_t)DL_NUTS_STREAM_DIRECTION | ((uint32_t)d << 8), k0, k1);
    if (u_join) *u_join = dl_uniform53(r.x[2], r.x[3]);
    return (r.x[0] >> 31) ? 1 : -1;
}

// selection uniform of leaf n of doubling d
DL_NUTS_HD double dl_nuts_select_uniform(long long it, uint32_t chain, int d, int n, uint32_t k0, uint32_t k1) {
    const DlPhilox r = dl_philox4x32((uint32_t)it, (uint32_t)((unsigned long long)it >> 32), chain,
                                     (uint32_t)DL_NUTS_STREAM_SELECT | ((uint32_t)d << 8) | ((uint32_t)n << 12), k0, k1);
    return dl_uniform53(r.x[0], r.x[1]);
}

// checkpoints of leaf n (NumPyro's _leaf_idx_to_ckpt_idxs): idx_max = number of set bits of n >> 1; idx_min = idx_max - (number of trailing ones of n) + 1
DL_NUTS_HD void dl_nuts_ckpt_range(int n, int* idx_min, int* idx_max) {
    int mx = 0, ones = 0;
    for (int m = n >> 1; m > 0; m >>= 1) mx += m & 1;
    for (int m = n; m & 1; m >>= 1) ++ones;
    *idx_max = mx;
    *idx_min = mx - ones + 1;
}

// dual averaging of log eps towards the target acceptance (Nesterov 2009 as Hoffman & Gelman 2014, algorithm 5; constants of desilike_amd/hmc.py: gamma 0.05,
// t0 10, kappa 0.75); s = {logeps, hbar, logbar, mu, count}
DL_NUTS_HD void dl_nuts_dual_averaging(double* s, double target, double accept) {
    const double count = s[4] + 1., t0 = 10., gamma = 0.05, kappa = 0.75;
    s[1] = (1. - 1. / (count + t0)) * s[1] + (target - accept) / (count + t0);
    s[0] = s[3] - sqrt(count) / gamma * s[1];
    const double eta = pow(count, -kappa);
    s[2] = eta * s[0] + (1. - eta) * s[2];
    s[4] = count;
}

// ---- vector operations over the components of one chain: L::W components per thread (device: 1, lane = component; host: DL_NUTS_MAX_P, one thread) -----------
template <class L>
struct DlNutsVec {
    double x[L::W];
};

template <class L>
DL_NUTS_HD void dl_nuts_load(const L& l, DlNutsVec<L>& v, const double* row) {
    for (int j = 0; j < L::W; ++j) v.x[j] = l.on(j) ? row[l.comp(j)] : 0.;
}

template <class L>
DL_NUTS_HD void dl_nuts_store(const L& l, const DlNutsVec<L>& v, double* row) {
    for (int j = 0; j < L::W; ++j) if (l.on(j)) row[l.comp(j)] = v.x[j];
}

template <class L>
DL_NUTS_HD double dl_nuts_dot(const L& l, const DlNutsVec<L>& a, const DlNutsVec<L>& b) {
    double s[L::W];
    for (int j = 0; j < L::W; ++j) s[j] = a.x[j] * b.x[j];
    return l.sum(s);
}

// out = A x for a [P, P] row-major matrix (dense inverse mass matrix, Cholesky factor), A's rows beyond P never read
template <class L>
DL_NUTS_HD void dl_nuts_matvec(const L& l, const double* A, const DlNutsVec<L>& x, DlNutsVec<L>& out) {
    for (int j = 0; j < L::W; ++j) out.x[j] = 0.;
    for (int k = 0; k < l.P; ++k) {
        const double xk = l.at(x.x, k);
        for (int j = 0; j < L::W; ++j) if (l.on(j)) out.x[j] += A[(size_t)l.comp(j) * l.P + k] * xk;
    }
}

template <class L>
DL_NUTS_HD void dl_nuts_sharp(const L& l, const DlNutsArgs& a, const DlNutsVec<L>& p, DlNutsVec<L>& ps) {
    if (a.dense) dl_nuts_matvec(l, a.minv, p, ps);
    else for (int j = 0; j < L::W; ++j) ps.x[j] = l.on(j) ? a.minv[l.comp(j)] * p.x[j] : 0.;
}

// generalised criterion: the segment with ends of p# a, b and momentum sum rho keeps going (no U-turn)
template <class L>
DL_NUTS_HD bool dl_nuts_no_uturn(const L& l, const DlNutsVec<L>& a, const DlNutsVec<L>& b, const DlNutsVec<L>& rho) {
    return dl_nuts_dot(l, a, rho) > 0. && dl_nuts_dot(l, b, rho) > 0.;
}

// ---- the step -----------------------------------------------------------------------------------------------------------------------------------------------
// pending leaf from (q, p, g): half kick and drift with the chain's step size in direction v
template <class L>
DL_NUTS_HD void dl_nuts_launch_leaf(const L& l, const DlNutsArgs& a, int c, int v, const DlNutsVec<L>& q, const DlNutsVec<L>& p, const DlNutsVec<L>& g) {
    const size_t C = a.C, P = a.P;
    const double h = v * exp(a.dsc[DL_NUTS_D_LOGEPS * C + c]);
    DlNutsVec<L> ph, ps, qn;
    for (int j = 0; j < L::W; ++j) ph.x[j] = p.x[j] + (0.5 * h) * g.x[j];
    dl_nuts_sharp(l, a, ph, ps);
    for (int j = 0; j < L::W; ++j) qn.x[j] = q.x[j] + h * ps.x[j];
    dl_nuts_store(l, ph, a.vec + ((size_t)DL_NUTS_V_PN * C + c) * P);
    dl_nuts_store(l, qn, a.vec + ((size_t)DL_NUTS_V_QN * C + c) * P);
    a.isc[DL_NUTS_I_ACTIVE * C + c] = 1;
}

// new trajectory from the chain's current point (the last proposal): fresh momentum of iteration iter[c], energy, ends, first direction, first drift
template <class L>
DL_NUTS_HD void dl_nuts_start(const L& l, const DlNutsArgs& a, int c) {
    const size_t C = a.C, P = a.P;
    double* V = a.vec;
    auto row = [&](int f) { return V + ((size_t)f * C + c) * P; };
    const long long it = a.iter[c];
    const uint32_t chain = (uint32_t)a.chain_ids[c];
    DlNutsVec<L> z, p, ps, q, g;
    for (int j = 0; j < L::W; ++j) z.x[j] = l.on(j) ? dl_nuts_gauss(it, chain, l.comp(j), a.k0, a.k1) : 0.;
    if (a.dense) dl_nuts_matvec(l, a.lmass, z, p);
    else for (int j = 0; j < L::W; ++j) p.x[j] = l.on(j) ? z.x[j] / sqrt(a.minv[l.comp(j)]) : 0.;
    dl_nuts_sharp(l, a, p, ps);
    const double h0 = -a.dsc[DL_NUTS_D_LPP * C + c] + 0.5 * dl_nuts_dot(l, p, ps);
    dl_nuts_load(l, q, row(DL_NUTS_V_QP));
    dl_nuts_load(l, g, row(DL_NUTS_V_GP));
    dl_nuts_store(l, q, row(DL_NUTS_V_QL)); dl_nuts_store(l, p, row(DL_NUTS_V_PL)); dl_nuts_store(l, g, row(DL_NUTS_V_GL));
    dl_nuts_store(l, q, row(DL_NUTS_V_QR)); dl_nuts_store(l, p, row(DL_NUTS_V_PR)); dl_nuts_store(l, g, row(DL_NUTS_V_GR));
    dl_nuts_store(l, p, row(DL_NUTS_V_RHO));
    {
        a.dsc[DL_NUTS_D_H0 * C + c] = h0; a.dsc[DL_NUTS_D_HP * C + c] = h0;
        a.dsc[DL_NUTS_D_LW * C + c] = 0.; a.dsc[DL_NUTS_D_SACC * C + c] = 0.;
        a.isc[DL_NUTS_I_DEPTH * C + c] = 0; a.isc[DL_NUTS_I_LEAF * C + c] = 0; a.isc[DL_NUTS_I_NLEAF * C + c] = 0;
    }
    const int v = dl_nuts_direction(it, chain, 0, a.k0, a.k1, nullptr);
    a.isc[DL_NUTS_I_DIR * C + c] = v;
    dl_nuts_launch_leaf(l, a, c, v, q, p, g);
}

// end of the trajectory: record, adapt, and either start the next trajectory or wait for the next batch
template <class L>
DL_NUTS_HD void dl_nuts_finish(const L& l, const DlNutsArgs& a, int c, int depth_attempted, int divergent) {
    const size_t C = a.C, P = a.P;
    double* d = a.dsc;
    const int nleaf = a.isc[DL_NUTS_I_NLEAF * C + c];
    const double accept = d[DL_NUTS_D_SACC * C + c] / nleaf;
    const long long it = a.iter[c] + 1;
    int count = a.out_count[c];
    if (it % a.thin_by == 0) {
        const size_t r = (size_t)c * a.cap + count;
        DlNutsVec<L> q;
        dl_nuts_load(l, q, a.vec + ((size_t)DL_NUTS_V_QP * C + c) * P);
        dl_nuts_store(l, q, a.out_coords + r * P);
        {
            a.out_logp[r] = d[DL_NUTS_D_LPP * C + c];      // (offset included)
            double* info = a.out_info + r * DL_NUTS_INFO;
            info[0] = depth_attempted; info[1] = nleaf; info[2] = divergent; info[3] = accept; info[4] = d[DL_NUTS_D_HP * C + c];
        }
        ++count;
    }
    if (a.adapt) {
        double s[5] = {d[DL_NUTS_D_LOGEPS * C + c], d[DL_NUTS_D_HBAR * C + c], d[DL_NUTS_D_LOGBAR * C + c], d[DL_NUTS_D_MU * C + c], d[DL_NUTS_D_DACOUNT * C + c]};
        dl_nuts_dual_averaging(s, a.target, accept);
        {
            d[DL_NUTS_D_LOGEPS * C + c] = s[0]; d[DL_NUTS_D_HBAR * C + c] = s[1]; d[DL_NUTS_D_LOGBAR * C + c] = s[2]; d[DL_NUTS_D_DACOUNT * C + c] = s[4];
        }
    }
    { a.iter[c] = it; a.out_count[c] = count; a.isc[DL_NUTS_I_ACTIVE * C + c] = 0; }
    if (count < a.quota) dl_nuts_start(l, a, c);
}

// mode 0: chains waiting at a trajectory boundary start their next trajectory (first launch of a batch call); mode 1: the step proper
template <class L>
DL_NUTS_HD void dl_nuts_chain_step(const L& l, const DlNutsArgs& a, int c, int mode) {
    const size_t C = a.C, P = a.P;
    double* V = a.vec;
    double* d = a.dsc;
    int32_t* I = a.isc;
    auto row = [&](int f) { return V + ((size_t)f * C + c) * P; };
    if (a.out_count[c] >= a.quota) return;
    const int active = I[DL_NUTS_I_ACTIVE * C + c];
    if (mode == 0) {
        if (!active) dl_nuts_start(l, a, c);
        return;
    }
    if (!active) return;
    const long long it = a.iter[c];
    const uint32_t chain = (uint32_t)a.chain_ids[c];
    const int depth = I[DL_NUTS_I_DEPTH * C + c], leaf = I[DL_NUTS_I_LEAF * C + c], v = I[DL_NUTS_I_DIR * C + c];
    const double h = v * exp(d[DL_NUTS_D_LOGEPS * C + c]), h0 = d[DL_NUTS_D_H0 * C + c];
    // the new leaf: second half kick with the gradient of the pending position; rows without a finite log-posterior: -inf and a zero gradient
    double lp = a.lp_new[c];
    lp = lp == lp && lp < HUGE_VAL ? lp + a.offset : -HUGE_VAL;
    DlNutsVec<L> q, p, g, ps;
    dl_nuts_load(l, q, row(DL_NUTS_V_QN));
    dl_nuts_load(l, p, row(DL_NUTS_V_PN));
    dl_nuts_load(l, g, a.g_new + (size_t)c * P);
    for (int j = 0; j < L::W; ++j) {
        if (!(lp > -HUGE_VAL) || !(fabs(g.x[j]) < HUGE_VAL)) g.x[j] = 0.;
        p.x[j] += (0.5 * h) * g.x[j];
    }
    dl_nuts_sharp(l, a, p, ps);
    const double H = -lp + 0.5 * dl_nuts_dot(l, p, ps), dH = H - h0;
    const int nleaf = I[DL_NUTS_I_NLEAF * C + c] + 1;
    const double acc = dH == dH ? (dH > 0. ? exp(-dH) : 1.) : 0.;
    const double sacc = d[DL_NUTS_D_SACC * C + c] + acc;
    { I[DL_NUTS_I_NLEAF * C + c] = nleaf; d[DL_NUTS_D_SACC * C + c] = sacc; }
    if (!(dH <= a.threshold)) {                 // divergent (or NaN): the subtree is dropped; flag 2 when the leaf left the support (log-posterior -inf)
        dl_nuts_finish(l, a, c, depth + 1, lp > -HUGE_VAL ? 1 : 2);
        return;
    }
    const double lw_leaf = -dH;
    // uniform progressive sampling inside the subtree, momentum sum, first leaf
    DlNutsVec<L> before, rhos;     // rho of the subtree before and after this leaf
    bool take;
    double lws;
    if (leaf == 0) {
        take = true; lws = lw_leaf;
        for (int j = 0; j < L::W; ++j) before.x[j] = 0.;
        dl_nuts_store(l, p, row(DL_NUTS_V_PF));
    } else {
        dl_nuts_load(l, before, row(DL_NUTS_V_RHOS));
        lws = dl_nuts_logaddexp(d[DL_NUTS_D_LWS * C + c], lw_leaf);
        take = dl_nuts_select_uniform(it, chain, depth, leaf, a.k0, a.k1) < exp(lw_leaf - lws);
    }
    for (int j = 0; j < L::W; ++j) rhos.x[j] = before.x[j] + p.x[j];
    if (take) {
        dl_nuts_store(l, q, row(DL_NUTS_V_QS));
        dl_nuts_store(l, g, row(DL_NUTS_V_GS));
    }
    // checkpoints and the U-turns of the sub-subtrees this leaf completes
    bool turning = false;
    if (leaf % 2 == 0) {
        int imin, imax;
        dl_nuts_ckpt_range(leaf, &imin, &imax);
        dl_nuts_store(l, before, row(DL_NUTS_V_CK + imax));
        dl_nuts_store(l, ps, row(DL_NUTS_V_CK + a.D + imax));
    } else {
        int imin, imax;
        dl_nuts_ckpt_range(leaf, &imin, &imax);
        for (int i = imax; i >= imin && !turning; --i) {
            DlNutsVec<L> ckr, cks, r;
            dl_nuts_load(l, ckr, row(DL_NUTS_V_CK + i));
            dl_nuts_load(l, cks, row(DL_NUTS_V_CK + a.D + i));
            for (int j = 0; j < L::W; ++j) r.x[j] = rhos.x[j] - ckr.x[j];
            turning = !dl_nuts_no_uturn(l, cks, ps, r);
        }
    }
    {
        d[DL_NUTS_D_LWS * C + c] = lws;
        if (take) { d[DL_NUTS_D_LPS * C + c] = lp; d[DL_NUTS_D_HS * C + c] = H; }
    }
    if (turning) {                              // U-turn inside the subtree: dropped
        dl_nuts_finish(l, a, c, depth + 1, 0);
        return;
    }
    if (leaf + 1 < (1 << depth)) {              // the subtree goes on from this leaf
        dl_nuts_store(l, rhos, row(DL_NUTS_V_RHOS));
        I[DL_NUTS_I_LEAF * C + c] = leaf + 1;
        dl_nuts_launch_leaf(l, a, c, v, q, p, g);
        return;
    }
    // ---- the subtree is complete: join (biased progressive sampling), U-turn of the trajectory and across the join ------------------------------------------------
    double u_join;
    dl_nuts_direction(it, chain, depth, a.k0, a.k1, &u_join);
    const double lw = d[DL_NUTS_D_LW * C + c];
    const bool swap = u_join < exp(lws - lw);
    DlNutsVec<L> rho, pf, pl, pr, psf, psl, psr, t1, t2, rho_new;
    dl_nuts_load(l, rho, row(DL_NUTS_V_RHO));
    dl_nuts_load(l, pf, row(DL_NUTS_V_PF));
    dl_nuts_load(l, pl, row(DL_NUTS_V_PL));
    dl_nuts_load(l, pr, row(DL_NUTS_V_PR));
    dl_nuts_sharp(l, a, pf, psf);
    dl_nuts_sharp(l, a, pl, psl);
    dl_nuts_sharp(l, a, pr, psr);
    for (int j = 0; j < L::W; ++j) rho_new.x[j] = rho.x[j] + rhos.x[j];
    bool go;
    if (v > 0) {     // old trajectory on the left, subtree (first leaf pf, last leaf p) on the right
        for (int j = 0; j < L::W; ++j) { t1.x[j] = rho.x[j] + pf.x[j]; t2.x[j] = pr.x[j] + rhos.x[j]; }
        go = dl_nuts_no_uturn(l, psl, ps, rho_new) && dl_nuts_no_uturn(l, psl, psf, t1) && dl_nuts_no_uturn(l, psr, ps, t2);
    } else {         // subtree (last leaf p on the far left, first leaf pf) on the left, old trajectory on the right
        for (int j = 0; j < L::W; ++j) { t1.x[j] = rhos.x[j] + pl.x[j]; t2.x[j] = pf.x[j] + rho.x[j]; }
        go = dl_nuts_no_uturn(l, ps, psr, rho_new) && dl_nuts_no_uturn(l, ps, psl, t1) && dl_nuts_no_uturn(l, psf, psr, t2);
    }
    if (swap) {
        DlNutsVec<L> qs, gs;
        dl_nuts_load(l, qs, row(DL_NUTS_V_QS));
        dl_nuts_load(l, gs, row(DL_NUTS_V_GS));
        dl_nuts_store(l, qs, row(DL_NUTS_V_QP));
        dl_nuts_store(l, gs, row(DL_NUTS_V_GP));
    }
    const int e = v > 0 ? DL_NUTS_V_QR : DL_NUTS_V_QL;     // the new end: this leaf
    dl_nuts_store(l, q, row(e)); dl_nuts_store(l, p, row(e + 1)); dl_nuts_store(l, g, row(e + 2));
    dl_nuts_store(l, rho_new, row(DL_NUTS_V_RHO));
    const double lps = d[DL_NUTS_D_LPS * C + c], hs = d[DL_NUTS_D_HS * C + c];
    {
        d[DL_NUTS_D_LW * C + c] = dl_nuts_logaddexp(lw, lws);
        if (swap) { d[DL_NUTS_D_LPP * C + c] = lps; d[DL_NUTS_D_HP * C + c] = hs; }
    }
    if (!go || depth + 1 >= a.D) {
        dl_nuts_finish(l, a, c, depth + 1, 0);
        return;
    }
    // next doubling: direction, and its first leaf from the trajectory's end on that side
    const int w = dl_nuts_direction(it, chain, depth + 1, a.k0, a.k1, nullptr);
    { I[DL_NUTS_I_DEPTH * C + c] = depth + 1; I[DL_NUTS_I_LEAF * C + c] = 0; I[DL_NUTS_I_DIR * C + c] = w; }
    const int f = w > 0 ? DL_NUTS_V_QR : DL_NUTS_V_QL;
    DlNutsVec<L> qe, pe, ge;
    dl_nuts_load(l, qe, row(f)); dl_nuts_load(l, pe, row(f + 1)); dl_nuts_load(l, ge, row(f + 2));
    dl_nuts_launch_leaf(l, a, c, w, qe, pe, ge);
}

// the host's component layout: one thread holds every component of a chain
struct DlNutsSerial {
    static constexpr int W = DL_NUTS_MAX_P;
    int P;
    int comp(int j) const { return j; }
    bool on(int j) const { return j < P; }
    double sum(const double* x) const {
        double s = 0.;
        for (int j = 0; j < P; ++j) s += x[j];
        return s;
    }
    double at(const double* x, int k) const { return x[k]; }
};
