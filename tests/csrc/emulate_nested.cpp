// emulate_nested.cpp -- TEST INFRASTRUCTURE: runs the phases of batched nested sampling of desilike_amd/csrc/dl_nested.h on the CPU (the threads of a workgroup one
// after the other, a barrier = the end of a loop; one thread holds every component of a point), so that the `not gpu` suite checks the device arithmetic against
// the NumPy statement (desilike_amd/nested.py _HostNested).  It is NOT a fallback: nothing in desilike_amd/ links or loads it.
// With -DEMU_NESTED_MAIN: a stand-alone program that runs every phase over the shapes of the tests, for the sanitizers.
#include <string.h>

#include <vector>

#include "../../desilike_amd/csrc/dl_nested.h"

static DlSmcSerial layout(int P) {
    DlSmcSerial l;
    l.P = P;
    return l;
}

static bool shape_ok(int N, int M) { return N >= 64 && N <= DL_NESTED_MAX_N && N % 64 == 0 && M >= 1 && M <= N / 2; }

extern "C" {

// the sort of dl_nested_rank_kernel for one run: rank [N] the slot of every rank, W [N] the survivors' weights, *first the first survivor in slot order
int emu_nested_rank(const double* L, int32_t N, int32_t M, int32_t* rank, double* W, int32_t* first) {
    if (!shape_ok(N, M)) return 1;
    const int T = DL_NESTED_THREADS, n2 = dl_nested_pow2(N);
    std::vector<uint64_t> keys(n2);
    std::vector<int32_t> slots(n2);
    for (int t = 0; t < T; ++t) dl_nested_load_keys(t, T, L, N, n2, keys.data(), slots.data());
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride >= 1; stride >>= 1)
            for (int t = 0; t < T; ++t) dl_nested_bitonic_stage(t, T, keys.data(), slots.data(), n2, size, stride);
    *first = N;
    for (int r = 0; r < N; ++r) {
        rank[r] = slots[r];
        if (slots[r] < 0 || slots[r] >= N) return 2;      // (a padding entry among the first N ranks)
        W[slots[r]] = r >= M ? 1. / (double)(N - M) : 0.;
        if (r >= M && slots[r] < *first) *first = slots[r];
    }
    return 0;
}

// the scan and the evidence of dl_nested_rank_kernel for one run: out = {L*, new log X, new log Z}; cum [M], logw [M]
int emu_nested_evidence(const double* L, const int32_t* rank, int32_t N, int32_t M, double logx, double logz, double* out, double* cum, double* logw) {
    if (!shape_ok(N, M)) return 1;
    const int T = DL_NESTED_THREADS;
    std::vector<double> tot(T), gtot(T / DL_SMC_GROUP);
    for (int t = 0; t < T; ++t) dl_nested_scan_slices(t, T, N, M, cum, tot.data());
    for (int t = 0; t < T; ++t) dl_smc_scan_groups(t, T, tot.data(), gtot.data());
    for (int t = 0; t < T; ++t) dl_smc_scan_top(t, T, gtot.data());
    for (int t = 0; t < T; ++t) dl_smc_scan_offsets(t, T, M, cum, tot.data(), gtot.data());
    DlNestedLevel lv;
    dl_nested_evidence(DlSmcSerialGroup(), L, rank, cum, N, M, logx, logz, &lv);
    out[0] = lv.lstar; out[1] = lv.logx; out[2] = lv.logz;
    for (int j = 0; j < M; ++j) logw[j] = dl_nested_logw(logx, cum, N, j);
    return 0;
}

// dl_nested_moments_kernel for one run: mean [P], cov [P, P] (lower triangle written) of the points from slot `first` on under the weights W
int emu_nested_moments(const double* x, const double* W, int32_t first, int32_t N, int32_t P, double* mean, double* cov) {
    if (P < 1 || P > DL_NESTED_MAX_P || first < 0 || first >= N) return 1;
    const DlSmcSerial l = layout(P);
    const int nw = DL_SMC_MOMENT_WAVES, n = N - first;
    const double *xs = x + (size_t)first * P, *Ws = W + first;
    DlNutsVec<DlSmcSerial> m, acc;
    for (int j = 0; j < DlSmcSerial::W; ++j) m.x[j] = 0.;
    std::vector<double> sum(P);
    auto combine = [&](int row) {
        for (int j = 0; j < P; ++j) sum[j] = 0.;
        for (int w = 0; w < nw; ++w) {
            dl_smc_moment_partial(l, xs, Ws, n, w, nw, row, m, row >= 0 ? m.x[row] : 0., acc);
            for (int j = 0; j < P; ++j) sum[j] += acc.x[j];
        }
    };
    combine(-1);
    for (int j = 0; j < P; ++j) { m.x[j] = sum[j]; mean[j] = xs[j] + sum[j]; }
    for (int row = 0; row < P; ++row) {
        combine(row);
        for (int j = 0; j <= row; ++j) cov[(size_t)row * P + j] = sum[j];
    }
    return 0;
}

// dl_nested_cholesky_kernel for one run: C [P, P]
int emu_nested_factor(const double* cov, const double* widths, int32_t P, double* C) {
    if (P < 1 || P > DL_NESTED_MAX_P) return 1;
    memset(C, 0, sizeof(double) * P * P);
    dl_smc_factor(layout(P), cov, widths, C);
    return 0;
}

// the seeds of dl_nested_seed_kernel for one run: seeds [M] the slot that seeds the dead point of rank j, u [M] the uniforms
int emu_nested_seeds(const int32_t* rank, int32_t N, int32_t M, long long it, int32_t run, uint64_t seed, int32_t* seeds, double* u) {
    if (!shape_ok(N, M)) return 1;
    for (int j = 0; j < M; ++j) {
        u[j] = dl_nested_seed_uniform(it, (uint32_t)run, j, (uint32_t)seed, (uint32_t)(seed >> 32));
        const int r = dl_nested_seed_rank(u[j], N, M);
        if (r < M || r >= N) return 2;
        seeds[j] = rank[r];
    }
    return 0;
}

// dl_nested_propose_kernel for one run: x [M, P] the replaced points in rank order, prop [M, P]
int emu_nested_propose(const double* C, double s, const double* x, int32_t M, int32_t P, long long it, int32_t sweep, int32_t run, uint64_t seed, double* prop) {
    if (P < 1 || P > DL_NESTED_MAX_P) return 1;
    const DlSmcSerial l = layout(P);
    DlNutsVec<DlSmcSerial> v, vp;
    for (int j = 0; j < M; ++j) {
        dl_nuts_load(l, v, x + (size_t)j * P);
        dl_nested_propose(l, C, s, v, it, sweep, (uint32_t)run, j, (uint32_t)seed, (uint32_t)(seed >> 32), vp);
        dl_nuts_store(l, vp, prop + (size_t)j * P);
    }
    return 0;
}

// the constrained test of dl_nested_accept_kernel for one run: flags [M], logu [M]; the number accepted through *naccepted
int emu_nested_accept(double lstar, const double* pi, const double* Lp, const double* pip, const int32_t* status, int32_t M, long long it, int32_t sweep, int32_t run, uint64_t seed,
                      uint8_t* flags, double* logu, int32_t* naccepted) {
    *naccepted = 0;
    for (int j = 0; j < M; ++j) {
        logu[j] = dl_nested_log_uniform(it, sweep, (uint32_t)run, j, (uint32_t)seed, (uint32_t)(seed >> 32));
        flags[j] = dl_nested_accept(lstar, pi[j], Lp[j], pip[j], status[j], logu[j]) ? 1 : 0;
        *naccepted += flags[j];
    }
    return 0;
}

// dl_nested_finish_kernel for one run: out = {log Z_rem, 1 if the run goes to rest}
int emu_nested_finish(const double* L, int32_t N, double logx, double logz, double dlogz, double* out) {
    if (N < 1) return 1;
    out[0] = dl_nested_remaining(DlSmcSerialGroup(), L, N, logx);
    out[1] = dl_nested_at_rest(logz, out[0], dlogz) ? 1. : 0.;
    return 0;
}

uint64_t emu_nested_key(double L) { return dl_nested_key(L); }

}

#ifdef EMU_NESTED_MAIN
#include <stdio.h>

// every phase over N in {64, 320, 8192} x M in {1, 24, N / 2} x P in {1, 2, 15, 64} on a Gaussian toy likelihood, with the edge inputs of tests/test_nested.py: equal L,
// a coordinate all points share, a proposal with L' = L*
int main() {
    const int Ns[3] = {64, 320, 8192}, Ps[4] = {1, 2, 15, 64};
    const uint64_t seed = 12345;
    int bad = 0;
    for (int N : Ns)
        for (int m = 0; m < 3; ++m)
            for (int P : Ps)
                for (int edge = 0; edge < 3; ++edge) {
                    const int M = m == 0 ? 1 : m == 1 ? 24 : N / 2;
                    std::vector<double> x((size_t)N * P), L(N), W(N), cum(M), logw(M), mean(P), cov((size_t)P * P, 0.), C((size_t)P * P), widths(P, 2.), xs((size_t)M * P),
                        prop((size_t)M * P), logu(M), u(M), pi(M, 0.), Lp(M);
                    std::vector<int32_t> rank(N), seeds(M), status(M, 0);
                    std::vector<uint8_t> flags(M);
                    for (int i = 0; i < N; ++i) {
                        double s = 0.;
                        for (int j = 0; j < P; ++j) {
                            const double z = dl_nested_gauss(7, 0, 3, i % 4096, j + 2 * (i / 4096), (uint32_t)seed, 0);
                            x[(size_t)i * P + j] = edge == 2 && j == P - 1 ? 0.25 : z;
                            s += z * z;
                        }
                        L[i] = edge == 1 ? -1.5 - (i % 3) : -2. * s;
                    }
                    int32_t first, nacc;
                    double out[3], fin[2];
                    bad += emu_nested_rank(L.data(), N, M, rank.data(), W.data(), &first);
                    for (int r = 1; r < N; ++r)
                        if (L[rank[r - 1]] > L[rank[r]] || (L[rank[r - 1]] == L[rank[r]] && rank[r - 1] > rank[r])) ++bad;
                    bad += emu_nested_evidence(L.data(), rank.data(), N, M, -0.5, -3., out, cum.data(), logw.data());
                    if (!(out[1] < -0.5) || !(out[2] >= -3.) || out[0] != L[rank[M - 1]]) ++bad;
                    bad += emu_nested_moments(x.data(), W.data(), first, N, P, mean.data(), cov.data());
                    bad += emu_nested_factor(cov.data(), widths.data(), P, C.data());
                    if (edge == 2 && C[(size_t)(P - 1) * P + P - 1] != 2.) ++bad;      // the shared coordinate: the prior's width
                    bad += emu_nested_seeds(rank.data(), N, M, 7, 3, seed, seeds.data(), u.data());
                    for (int j = 0; j < M; ++j) {
                        if (!(W[seeds[j]] > 0.)) ++bad;
                        memcpy(&xs[(size_t)j * P], &x[(size_t)seeds[j] * P], sizeof(double) * P);
                    }
                    bad += emu_nested_propose(C.data(), 0.7, xs.data(), M, P, 7, 1, 3, seed, prop.data());
                    for (int j = 0; j < M; ++j) {
                        double s = 0.;
                        for (int c = 0; c < P; ++c) s += prop[(size_t)j * P + c] * prop[(size_t)j * P + c];
                        Lp[j] = j % 5 == 0 ? out[0] : -2. * s;       // L' = L*: rejected
                        if (j % 7 == 0) status[j] = 1;
                    }
                    bad += emu_nested_accept(out[0], pi.data(), Lp.data(), pi.data(), status.data(), M, 7, 1, 3, seed, flags.data(), logu.data(), &nacc);
                    for (int j = 0; j < M; ++j) if (flags[j] && (j % 5 == 0 || j % 7 == 0)) ++bad;
                    bad += emu_nested_finish(L.data(), N, out[1], out[2], 0.01, fin);
                    if (!(fin[0] == fin[0])) ++bad;
                }
    printf("emulate_nested: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
