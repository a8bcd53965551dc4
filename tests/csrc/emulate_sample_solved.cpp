// CPU build of the lane function of the draw kernel (desilike_amd/csrc/dl_sample_solved.h): the same source the device compiles, one "lane" after the other.
// Shared object for tests/test_sample_solved.py (ctypes); with -DSS_STANDALONE a program of its own for the sanitizer run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../desilike_amd/csrc/dl_sample_solved.h"

struct SsMarg {   // the fields of DlMargDev the lane function reads
    int32_t n_s, n_marg;
    int32_t is_marg[DL_MAX_SOLVED];
    double prec[DL_MAX_SOLVED];
};

template <int NS>
static void ss_run_ns(const SsMarg& mg, const double* hessian, const double* xhat, const double* loglike, const double* logprior, const int32_t* status_in, int64_t B,
                      int64_t index0, int size, uint64_t seed, double* solved_out, double* loglike_out, double* logprior_out, int32_t* status_out) {
    for (int64_t b = 0; b < B; ++b)
        status_out[b] = dl_sample_solved_lane<NS>(hessian + b * NS * NS, xhat + b * NS, mg, loglike[b], logprior[b], status_in[b], index0 + b, size, (uint32_t)seed,
                                                  (uint32_t)(seed >> 32), solved_out + b * size * NS, loglike_out + b * size, logprior_out + b * size);
}

// hessian [B, ns, ns], xhat [B, ns], prec [ns], is_marg [ns], loglike / logprior / status_in [B] -> solved_out [B, size, ns], loglike_out / logprior_out [B, size],
// status_out [B].  Returns 0, or 1 for ns outside 1 .. 16.
extern "C" int ss_sample_solved(int32_t ns, const double* hessian, const double* xhat, const double* prec, const int32_t* is_marg, const double* loglike,
                                const double* logprior, const int32_t* status_in, int64_t B, int64_t index0, int32_t size, uint64_t seed, double* solved_out,
                                double* loglike_out, double* logprior_out, int32_t* status_out) {
    if (ns < 1 || ns > DL_MAX_SOLVED) return 1;
    SsMarg mg;
    memset(&mg, 0, sizeof(mg));
    mg.n_s = ns;
    for (int s = 0; s < ns; ++s) { mg.is_marg[s] = is_marg[s]; mg.prec[s] = prec[s]; mg.n_marg += is_marg[s] != 0; }
#define SS_CASE(N) case N: ss_run_ns<N>(mg, hessian, xhat, loglike, logprior, status_in, B, index0, size, seed, solved_out, loglike_out, logprior_out, status_out); break;
    switch (ns) {
        SS_CASE(1) SS_CASE(2) SS_CASE(3) SS_CASE(4) SS_CASE(5) SS_CASE(6) SS_CASE(7) SS_CASE(8) SS_CASE(9) SS_CASE(10) SS_CASE(11) SS_CASE(12) SS_CASE(13) SS_CASE(14)
        SS_CASE(15) SS_CASE(16)
    }
#undef SS_CASE
    return 0;
}

#ifdef SS_STANDALONE
// every size 1 .. 16, all / some / none of the parameters marginalised, flat and Gaussian priors, a row with a non-positive pivot and a row with a bad status:
// the residual |C^T (x - x^) - z| is not checked here (tests/test_sample_solved.py does, against NumPy) -- this run is for the sanitizers; it checks what needs no
// second implementation: finite draws on good rows, NaN on bad ones, the statuses, and that draw d does not depend on size.
int main() {
    const int64_t B = 7;
    const int size = 3;
    uint64_t lcg = 12345;
    auto uniform = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg >> 11) / 9007199254740992. - 0.5; };
    int nfail = 0;
    for (int ns = 1; ns <= DL_MAX_SOLVED; ++ns) {
        for (int mode = 0; mode < 3; ++mode) {   // 0 all marginalised, 1 every other one, 2 none
            std::vector<double> hessian(B * ns * ns), xhat(B * ns), prec(ns), loglike(B), logprior(B);
            std::vector<int32_t> is_marg(ns), status_in(B, 0), status(B), status1(B);
            for (int s = 0; s < ns; ++s) { is_marg[s] = mode == 0 ? 1 : mode == 1 ? (s & 1) : 0; prec[s] = (s % 3 == 0) ? 0.25 * (1 + s) : 0.; }
            for (int64_t b = 0; b < B; ++b) {
                std::vector<double> T(ns * (ns + 3));
                for (auto& t : T) t = uniform();
                for (int i = 0; i < ns; ++i) {
                    xhat[b * ns + i] = uniform();
                    for (int j = 0; j < ns; ++j) {
                        double sum = 0.;
                        for (int k = 0; k < ns + 3; ++k) sum += T[i * (ns + 3) + k] * T[j * (ns + 3) + k];
                        hessian[(b * ns + i) * ns + j] = -sum;
                    }
                }
                loglike[b] = -10. + uniform(); logprior[b] = uniform();
            }
            hessian[(2 * ns + ns - 1) * ns + ns - 1] = 1.;   // row 2: a negative diagonal entry of A (prec of the last parameter is below 1)
            if (prec[ns - 1] >= 1.) hessian[(2 * ns + ns - 1) * ns + ns - 1] = 1. + prec[ns - 1];
            status_in[4] = 1;
            std::vector<double> x(B * size * ns), ll(B * size), lp(B * size), x1(B * ns), ll1(B), lp1(B);
            if (ss_sample_solved(ns, hessian.data(), xhat.data(), prec.data(), is_marg.data(), loglike.data(), logprior.data(), status_in.data(), B, 1000, size, 42, x.data(),
                                 ll.data(), lp.data(), status.data())) return 2;
            if (ss_sample_solved(ns, hessian.data(), xhat.data(), prec.data(), is_marg.data(), loglike.data(), logprior.data(), status_in.data(), B, 1000, 1, 42, x1.data(),
                                 ll1.data(), lp1.data(), status1.data())) return 2;
            for (int64_t b = 0; b < B; ++b) {
                const bool bad = b == 2 || b == 4;
                if (status[b] != (b == 2 ? 2 : b == 4 ? 1 : 0) || status1[b] != status[b]) nfail++;
                for (int d = 0; d < size; ++d) {
                    for (int s = 0; s < ns; ++s) if (bad != (x[(b * size + d) * ns + s] != x[(b * size + d) * ns + s])) nfail++;
                    if (bad != (ll[b * size + d] != ll[b * size + d]) || bad != (lp[b * size + d] != lp[b * size + d])) nfail++;
                }
                if (!bad) {
                    for (int s = 0; s < ns; ++s) if (x1[b * ns + s] != x[b * size * ns + s]) nfail++;
                    if (ll1[b] != ll[b * size] || lp1[b] != lp[b * size]) nfail++;
                }
            }
        }
    }
    if (nfail) { printf("%d checks failed\n", nfail); return 1; }
    printf("sizes 1 .. %d, three marginalisation patterns: statuses, NaN rows and draw addressing agree\n", DL_MAX_SOLVED);
    return 0;
}
#endif
