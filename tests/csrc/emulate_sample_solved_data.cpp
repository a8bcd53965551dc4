// CPU run of the per-pair draw of dl_sample_solved_data (desilike_amd/csrc/dl_sample_solved_data.h): the functions the device compiles -- the record of the point
// (host twin dl_dbm_point_host), dl_dbm_pair, dl_ssd_status, dl_ssd_draw -- here with g++.  A program of its own (tests/test_sample_solved_data.py runs the plain build
// and the build under the address / undefined-behaviour sanitizers; nothing of it is loaded into python).
//
// Input (argv[1]): a file of float64 -- n, n_s, M, n_rows, size, index0, seed low word, seed high word, m_lo, m_hi, lp | prec [n_s] | x0 [n_s] | loc [n_s] |
// '.marg' mask [n_s] | whitened biases [M][n] | per row: y [n], Tt [n_s][n].  Row i is point index0 + i; it is taken against the data indices m_lo .. m_hi - 1 (an
// index outside [0, M) is the kernel's bad index: the table is not read); lp is the log-prior of the sampled parameters written into every record.
// Output, %.17g:
//   P row m status ll lps hld xhat_0 .. xhat_{n_s - 1} H_00 .. H_{n_s - 1, n_s - 1}     one line per (row, data index): the inputs of the draws
//   D row m draw loglike logprior x_0 .. x_{n_s - 1}                                     one line per draw
// Besides, for every draw: the largest compiled size (NSP = 16: record and constants padded) must give the BITS of the size the launcher picks.  Exit status 1 if not.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../desilike_amd/csrc/dl_sample_solved_data.h"

struct Pair { int status; double ll, lps, dx[16]; };
struct Draw { double loglike, logprior, x[17]; };

template <int NSP>
static Pair pair(const double* y, const double* const* t_rows, int n_s, const double* bias, int n, const double* rec, const DlDbmConst& k, bool bad) {
    Pair r;
    memset(&r, 0, sizeof(r));
    if (bad) {   // (the kernel runs the finish on zero partial sums: nothing of it is used)
        r.status = dl_ssd_status(rec, 0., true);
        return r;
    }
    dl_dbm_pair<NSP>(y, t_rows, n_s, bias, n, rec, k, r.ll, r.lps, r.dx);
    r.status = dl_ssd_status(rec, r.ll, false);
    return r;
}

template <int NSP>
static Draw draw(const Pair& p, const double* rec, const DlDbmConst& k, int n_s, int64_t index, uint32_t d, uint32_t k0, uint32_t k1) {
    Draw r;
    memset(&r, 0, sizeof(r));
    if (p.status != 0) {
        r.loglike = r.logprior = NAN;
        for (int s = 0; s < n_s; ++s) r.x[s] = NAN;
        return r;
    }
    dl_ssd_draw<NSP>(rec + DL_DBM_C, rec[DL_DBM_HLD], k, n_s, p.dx, p.ll, rec[DL_DBM_LP] + p.lps, index, d, k0, k1, r.x, r.loglike, r.logprior);
    return r;
}

static bool same_bits(const Draw& a, const Draw& b, int n_s) {
    return memcmp(&a.loglike, &b.loglike, sizeof(double)) == 0 && memcmp(&a.logprior, &b.logprior, sizeof(double)) == 0 && memcmp(a.x, b.x, n_s * sizeof(double)) == 0;
}

struct Input {
    int n, n_s, M, n_rows, size, m_lo, m_hi;
    int64_t index0;
    uint32_t k0, k1;
    double lp;
    const double *prec, *x0, *loc, *bias, *rows;
    int32_t is_marg[DL_MAX_SOLVED];
};

template <int NSP>
static int run(const Input& in) {
    DlDbmConst k;
    for (int s = 0; s < DL_MAX_SOLVED; ++s) { k.x0[s] = s < in.n_s ? in.x0[s] : 0.; k.loc[s] = s < in.n_s ? in.loc[s] : 0.; k.prec[s] = s < in.n_s ? in.prec[s] : 0.; }
    int nfail = 0;
    const int n = in.n, n_s = in.n_s;
    std::vector<double> rec(DL_DBM_REC);
    for (int i = 0; i < in.n_rows; ++i) {
        const double* y = in.rows + (size_t)i * (1 + n_s) * n;
        std::vector<const double*> t_rows(n_s);
        for (int s = 0; s < n_s; ++s) t_rows[s] = y + (size_t)(1 + s) * n;
        dl_dbm_point_host(t_rows.data(), n, n_s, in.prec, in.is_marg, in.lp, rec.data());
        for (int m = in.m_lo; m < in.m_hi; ++m) {
            const bool bad = m < 0 || m >= in.M;
            const double* b = in.bias + (size_t)(bad ? 0 : m) * n;
            const Pair p = pair<NSP>(y, t_rows.data(), n_s, b, n, rec.data(), k, bad), p16 = pair<16>(y, t_rows.data(), n_s, b, n, rec.data(), k, bad);
            printf("P %d %d %d %.17g %.17g %.17g", i, m, p.status, p.ll, p.lps, rec[DL_DBM_HLD]);
            for (int s = 0; s < n_s; ++s) printf(" %.17g", in.x0[s] + p.dx[s]);
            for (int s = 0; s < n_s; ++s)
                for (int t = 0; t < n_s; ++t) printf(" %.17g", rec[DL_DBM_H + s * 16 + t]);
            printf("\n");
            for (int d = 0; d < in.size; ++d) {
                const Draw r = draw<NSP>(p, rec.data(), k, n_s, in.index0 + i, (uint32_t)d, in.k0, in.k1);
                const Draw r16 = draw<16>(p16, rec.data(), k, n_s, in.index0 + i, (uint32_t)d, in.k0, in.k1);
                if (p.status == 0 && !same_bits(r, r16, n_s)) { fprintf(stderr, "row %d data vector %d draw %d: the compiled sizes DIFFER\n", i, m, d); nfail++; }
                printf("D %d %d %d %.17g %.17g", i, m, d, r.loglike, r.logprior);
                for (int s = 0; s < n_s; ++s) printf(" %.17g", r.x[s]);
                printf("\n");
            }
        }
    }
    return nfail;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s input-file\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    double head[11];
    if (fread(head, sizeof(double), 11, f) != 11) { fclose(f); return 2; }
    Input in;
    in.n = (int)head[0]; in.n_s = (int)head[1]; in.M = (int)head[2]; in.n_rows = (int)head[3]; in.size = (int)head[4];
    in.index0 = (int64_t)head[5]; in.k0 = (uint32_t)head[6]; in.k1 = (uint32_t)head[7]; in.m_lo = (int)head[8]; in.m_hi = (int)head[9]; in.lp = head[10];
    if (in.n < 1 || in.n > 512 || in.n_s < 1 || in.n_s > DL_MAX_SOLVED || in.M < 1 || in.n_rows < 1 || in.size < 1 || in.index0 < 0) {
        fclose(f); fprintf(stderr, "sizes out of range\n"); return 2;
    }
    const int n = in.n, n_s = in.n_s;
    const size_t count = 4 * (size_t)n_s + (size_t)in.M * n + (size_t)in.n_rows * (1 + n_s) * n;
    std::vector<double> buf(count);
    const size_t got = fread(buf.data(), sizeof(double), count, f);
    fclose(f);
    if (got != count) { fprintf(stderr, "short input: %zu of %zu values\n", got, count); return 2; }
    in.prec = buf.data(); in.x0 = in.prec + n_s; in.loc = in.x0 + n_s;
    const double* mask = in.loc + n_s;
    in.bias = mask + n_s; in.rows = in.bias + (size_t)in.M * n;
    for (int s = 0; s < DL_MAX_SOLVED; ++s) in.is_marg[s] = s < n_s && mask[s] != 0.;
    int nfail = 0;
    switch (dl_dbm_nsp(n_s)) {
        case 1: nfail = run<1>(in); break;
        case 2: nfail = run<2>(in); break;
        case 3: nfail = run<3>(in); break;
        case 4: nfail = run<4>(in); break;
        case 5: nfail = run<5>(in); break;
        case 6: nfail = run<6>(in); break;
        case 8: nfail = run<8>(in); break;
        case 12: nfail = run<12>(in); break;
        default: nfail = run<16>(in); break;
    }
    if (nfail) { fprintf(stderr, "%d checks failed\n", nfail); return 1; }
    return 0;
}
