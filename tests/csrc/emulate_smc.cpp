// emulate_smc.cpp -- TEST INFRASTRUCTURE: runs the phases of tempered sequential Monte Carlo of desilike_amd/csrc/dl_smc.h on the CPU (the threads of a workgroup one
// after the other, a barrier = the end of a loop; one thread holds every component of a particle), so that the `not gpu` suite checks the device arithmetic against
// the NumPy statement (desilike_amd/smc.py _HostSMC).  It is NOT a fallback: nothing in desilike_amd/ links or loads it.
// With -DEMU_SMC_MAIN: a stand-alone program that runs every phase over the shapes of the tests, for the sanitizers.
#include <string.h>

#include <vector>

#include "../../desilike_amd/csrc/dl_smc.h"

static DlSmcSerial layout(int P) {
    DlSmcSerial l;
    l.P = P;
    return l;
}

extern "C" {

// the next level of one system: out = {delta, lmax, sumw, ess, new beta, dlogz}; W [N] the normalised weights (untouched for a sweep)
int emu_smc_temper(const double* L, int32_t N, double beta, double ess_fraction, double* out, double* W) {
    if (N < 1 || N > DL_SMC_MAX_N) return 1;
    DlSmcLevel t;
    dl_smc_temper(DlSmcSerialGroup(), L, N, beta, ess_fraction, &t);
    out[0] = t.delta; out[1] = t.lmax; out[2] = t.sumw; out[3] = t.ess; out[4] = t.beta; out[5] = t.dlogz;
    if (t.delta > 0.) for (int i = 0; i < N; ++i) W[i] = dl_smc_weight(L[i], t.lmax, t.delta) / t.sumw;
    return 0;
}

// dl_smc_moments_kernel for one system: mean [P], cov [P, P] (lower triangle written)
int emu_smc_moments(const double* x, const double* W, int32_t N, int32_t P, double* mean, double* cov) {
    if (P < 1 || P > DL_SMC_MAX_P || N < 1) return 1;
    const DlSmcSerial l = layout(P);
    const int nw = DL_SMC_MOMENT_WAVES;
    DlNutsVec<DlSmcSerial> m, acc;
    for (int j = 0; j < DlSmcSerial::W; ++j) m.x[j] = 0.;
    std::vector<double> sum(P);
    auto combine = [&](int row) {
        for (int j = 0; j < P; ++j) sum[j] = 0.;
        for (int w = 0; w < nw; ++w) {
            dl_smc_moment_partial(l, x, W, N, w, nw, row, m, row >= 0 ? m.x[row] : 0., acc);
            for (int j = 0; j < P; ++j) sum[j] += acc.x[j];
        }
    };
    combine(-1);
    for (int j = 0; j < P; ++j) { m.x[j] = sum[j]; mean[j] = x[j] + sum[j]; }
    for (int row = 0; row < P; ++row) {
        combine(row);
        for (int j = 0; j <= row; ++j) cov[(size_t)row * P + j] = sum[j];
    }
    return 0;
}

// dl_smc_cholesky_kernel for one system: C [P, P]
int emu_smc_factor(const double* cov, const double* widths, int32_t P, double* C) {
    if (P < 1 || P > DL_SMC_MAX_P) return 1;
    memset(C, 0, sizeof(double) * P * P);
    dl_smc_factor(layout(P), cov, widths, C);
    return 0;
}

// the scan and the ancestor search of dl_smc_resample_kernel for one system: cum [N], anc [N]; *u the uniform drawn
int emu_smc_resample(const double* W, int32_t N, long long it, int32_t sys, uint64_t seed, double* cum, int32_t* anc, double* u) {
    if (N < 1 || N > DL_SMC_MAX_N) return 1;
    const int T = DL_SMC_THREADS;
    std::vector<double> tot(T), gtot(T / DL_SMC_GROUP);
    for (int t = 0; t < T; ++t) dl_smc_scan_slices(t, T, W, N, cum, tot.data());
    for (int t = 0; t < T; ++t) dl_smc_scan_groups(t, T, tot.data(), gtot.data());
    for (int t = 0; t < T; ++t) dl_smc_scan_top(t, T, gtot.data());
    for (int t = 0; t < T; ++t) dl_smc_scan_offsets(t, T, N, cum, tot.data(), gtot.data());
    *u = dl_smc_resample_uniform(it, (uint32_t)sys, (uint32_t)seed, (uint32_t)(seed >> 32));
    for (int i = 0; i < N; ++i) anc[i] = dl_smc_ancestor(cum, N, i, *u);
    return 0;
}

// dl_smc_propose_kernel for one system: prop [N, P]
int emu_smc_propose(const double* C, double s, const double* x, int32_t N, int32_t P, long long it, int32_t sweep, int32_t sys, uint64_t seed, double* prop) {
    if (P < 1 || P > DL_SMC_MAX_P) return 1;
    const DlSmcSerial l = layout(P);
    DlNutsVec<DlSmcSerial> v, vp;
    for (int i = 0; i < N; ++i) {
        dl_nuts_load(l, v, x + (size_t)i * P);
        dl_smc_propose(l, C, s, v, it, sweep, (uint32_t)sys, i, (uint32_t)seed, (uint32_t)(seed >> 32), vp);
        dl_nuts_store(l, vp, prop + (size_t)i * P);
    }
    return 0;
}

// the Metropolis test of dl_smc_accept_kernel for one system: flags [N], logu [N]; returns the number accepted through *naccepted
int emu_smc_accept(double beta, const double* L, const double* pi, const double* Lp, const double* pip, const int32_t* status, int32_t N, long long it, int32_t sweep, int32_t sys,
                   uint64_t seed, uint8_t* flags, double* logu, int32_t* naccepted) {
    *naccepted = 0;
    for (int i = 0; i < N; ++i) {
        logu[i] = dl_smc_log_uniform(it, sweep, (uint32_t)sys, i, (uint32_t)seed, (uint32_t)(seed >> 32));
        flags[i] = dl_smc_accept(beta, L[i], pi[i], Lp[i], pip[i], status[i], logu[i]) ? 1 : 0;
        *naccepted += flags[i];
    }
    return 0;
}

double emu_smc_next_scale(double s, double a, double target_acceptance) { return dl_smc_next_scale(s, a, target_acceptance); }

}

#ifdef EMU_SMC_MAIN
#include <stdio.h>

// every phase over N in {64, 320, 16384} x P in {1, 2, 15, 64} on a Gaussian toy likelihood, with the edge inputs of tests/test_smc.py: some L = -inf, all live L
// equal, a coordinate all particles share
int main() {
    const int Ns[3] = {64, 320, 16384}, Ps[4] = {1, 2, 15, 64};
    const uint64_t seed = 12345;
    int bad = 0;
    for (int N : Ns)
        for (int P : Ps)
            for (int edge = 0; edge < 4; ++edge) {
                std::vector<double> x((size_t)N * P), L(N), pi(N, 0.), W(N), cum(N), mean(P), cov((size_t)P * P, 0.), C((size_t)P * P), widths(P, 2.), prop((size_t)N * P), logu(N);
                std::vector<int32_t> anc(N), status(N, 0);
                std::vector<uint8_t> flags(N);
                for (int i = 0; i < N; ++i) {
                    double s = 0.;
                    for (int j = 0; j < P; ++j) {
                        const double z = dl_smc_gauss(7, 0, 3, i, j, (uint32_t)seed, 0);
                        x[(size_t)i * P + j] = edge == 3 && j == P - 1 ? 0.25 : z;
                        s += z * z;
                    }
                    L[i] = edge == 2 ? -1.5 : -2. * s;
                    if ((edge == 1 || edge == 2) && i % 3 == 0) L[i] = -HUGE_VAL;
                }
                double out[6], u;
                int32_t nacc;
                bad += emu_smc_temper(L.data(), N, 0., 0.5, out, W.data());
                if (!(out[0] > 0.) || !(out[3] > 0.)) ++bad;
                if (edge == 2 && out[4] != 1.) ++bad;
                bad += emu_smc_moments(x.data(), W.data(), N, P, mean.data(), cov.data());
                bad += emu_smc_factor(cov.data(), widths.data(), P, C.data());
                if (edge == 3 && C[(size_t)(P - 1) * P + P - 1] != 2.) ++bad;      // the shared coordinate: the prior's width
                bad += emu_smc_resample(W.data(), N, 7, 3, seed, cum.data(), anc.data(), &u);
                for (int i = 0; i < N; ++i) if (anc[i] < 0 || anc[i] >= N || !(W[anc[i]] > 0.)) ++bad;
                bad += emu_smc_propose(C.data(), 0.7, x.data(), N, P, 7, 1, 3, seed, prop.data());
                std::vector<double> Lp(N);
                for (int i = 0; i < N; ++i) {
                    double s = 0.;
                    for (int j = 0; j < P; ++j) s += prop[(size_t)i * P + j] * prop[(size_t)i * P + j];
                    Lp[i] = -2. * s;
                    if (i % 7 == 0) status[i] = 1;
                }
                bad += emu_smc_accept(out[4], L.data(), pi.data(), Lp.data(), pi.data(), status.data(), N, 7, 1, 3, seed, flags.data(), logu.data(), &nacc);
                if (nacc < 0 || nacc > N) ++bad;
                (void)emu_smc_next_scale(1., (double)nacc / N, 0.234);
            }
    printf("emulate_smc: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
