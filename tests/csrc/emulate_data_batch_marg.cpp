// CPU run of the per-pair arithmetic of the data-batch kernels of contexts with solved parameters (desilike_amd/csrc/dl_data_batch_marg.h): the same functions the
// device compiles, here with g++.  A program of its own (tests/test_data_batch_marg.py runs the plain build and the build under the address / undefined-behaviour
// sanitizers; nothing of it is loaded into python).
//
// Input (argv[1]): a file of float64 -- n, n_s, M, n_rows | prec [n_s] | x0 [n_s] | loc [n_s] | '.marg' mask [n_s] | whitened biases [M][n] | per row: y [n], Tt [n_s][n].
// Output: one line per (row, data vector): row m ok ll lps x_0 .. x_{n_s - 1}, %.17g.
// Besides, for every pair: the cross kernel's order (chunks of DL_DBM_JC columns, columns beyond n staged as zeros) and the largest compiled size (NSP = 16: record
// and constants padded) must give the BITS of dl_dbm_pair at the size the launcher picks.  Exit status 1 if they do not.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../desilike_amd/csrc/dl_data_batch_marg.h"

struct Result { double ll, lps, dx[16]; };

template <int NSP>
static Result pair(const double* y, const double* const* t_rows, int n_s, const double* bias, int n, const double* rec, const DlDbmConst& k) {
    Result r;
    memset(&r, 0, sizeof(r));
    dl_dbm_pair<NSP>(y, t_rows, n_s, bias, n, rec, k, r.ll, r.lps, r.dx);
    return r;
}

// the cross kernel's order for one pair: chunks of DL_DBM_JC columns, columns beyond n staged as zeros, column c of a chunk on chain c % DL_DB_NP
template <int NSP>
static Result cross_order(const double* y, const double* const* t_rows, int n_s, const double* bias, int n, const double* rec, const DlDbmConst& k) {
    double p[DL_DB_NP], g[NSP], ys[DL_DBM_JC], bs[DL_DBM_JC], ts[DL_DBM_JC][NSP];
    for (int q = 0; q < DL_DB_NP; ++q) p[q] = 0.;
    for (int s = 0; s < NSP; ++s) g[s] = 0.;
    for (int base = 0; base < n; base += DL_DBM_JC) {
        for (int c = 0; c < DL_DBM_JC; ++c) {
            const bool in = base + c < n;
            ys[c] = in ? y[base + c] : 0.;
            bs[c] = in ? bias[base + c] : 0.;
            for (int s = 0; s < NSP; ++s) ts[c][s] = (in && s < n_s) ? t_rows[s][base + c] : 0.;
        }
        for (int c = 0; c < DL_DBM_JC; ++c) dl_dbm_step<NSP>(p[c % DL_DB_NP], g, ys[c], bs[c], ts[c]);
    }
    Result r;
    memset(&r, 0, sizeof(r));
    dl_dbm_pair_finish<NSP>(dl_db_tree(p), g, rec, k, r.ll, r.lps, r.dx);
    return r;
}

static bool same_bits(const Result& a, const Result& b, int n_s) {
    return memcmp(&a.ll, &b.ll, sizeof(double)) == 0 && memcmp(&a.lps, &b.lps, sizeof(double)) == 0 && memcmp(a.dx, b.dx, n_s * sizeof(double)) == 0;
}

template <int NSP>
static int run(int n, int n_s, int M, int n_rows, const double* prec, const double* x0, const double* loc, const int32_t* is_marg, const double* bias, const double* rows) {
    static_assert(DL_DBM_JC % DL_DB_NP == 0, "a staged chunk holds whole groups of chains");
    DlDbmConst k;
    for (int s = 0; s < DL_MAX_SOLVED; ++s) { k.x0[s] = s < n_s ? x0[s] : 0.; k.loc[s] = s < n_s ? loc[s] : 0.; k.prec[s] = s < n_s ? prec[s] : 0.; }
    int nfail = 0;
    std::vector<double> rec(DL_DBM_REC);
    for (int i = 0; i < n_rows; ++i) {
        const double* y = rows + (size_t)i * (1 + n_s) * n;
        std::vector<const double*> t_rows(n_s);
        for (int s = 0; s < n_s; ++s) t_rows[s] = y + (size_t)(1 + s) * n;
        const bool ok = dl_dbm_point_host(t_rows.data(), n, n_s, prec, is_marg, 0., rec.data());
        for (int m = 0; m < M; ++m) {
            const double* b = bias + (size_t)m * n;
            const Result r = pair<NSP>(y, t_rows.data(), n_s, b, n, rec.data(), k);
            const Result rc = cross_order<NSP>(y, t_rows.data(), n_s, b, n, rec.data(), k), r16 = pair<16>(y, t_rows.data(), n_s, b, n, rec.data(), k);
            if (!same_bits(r, rc, n_s) || !same_bits(r, r16, n_s)) { fprintf(stderr, "row %d data vector %d: the kernel orders DIFFER\n", i, m); nfail++; }
            printf("%d %d %d %.17g %.17g", i, m, ok ? 1 : 0, r.ll, r.lps);
            for (int s = 0; s < n_s; ++s) printf(" %.17g", x0[s] + r.dx[s]);
            printf("\n");
        }
    }
    return nfail;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s input-file\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    double head[4];
    if (fread(head, sizeof(double), 4, f) != 4) { fclose(f); return 2; }
    const int n = (int)head[0], n_s = (int)head[1], M = (int)head[2], n_rows = (int)head[3];
    if (n < 1 || n > 512 || n_s < 1 || n_s > DL_MAX_SOLVED || M < 1 || n_rows < 1) { fclose(f); fprintf(stderr, "sizes out of range\n"); return 2; }
    const size_t count = 4 * (size_t)n_s + (size_t)M * n + (size_t)n_rows * (1 + n_s) * n;
    std::vector<double> buf(count);
    const size_t got = fread(buf.data(), sizeof(double), count, f);
    fclose(f);
    if (got != count) { fprintf(stderr, "short input: %zu of %zu values\n", got, count); return 2; }
    const double *prec = buf.data(), *x0 = prec + n_s, *loc = x0 + n_s, *mask = loc + n_s, *bias = mask + n_s, *rows = bias + (size_t)M * n;
    int32_t is_marg[DL_MAX_SOLVED];
    for (int s = 0; s < n_s; ++s) is_marg[s] = mask[s] != 0.;
    int nfail = 0;
    switch (dl_dbm_nsp(n_s)) {
        case 1: nfail = run<1>(n, n_s, M, n_rows, prec, x0, loc, is_marg, bias, rows); break;
        case 2: nfail = run<2>(n, n_s, M, n_rows, prec, x0, loc, is_marg, bias, rows); break;
        case 3: nfail = run<3>(n, n_s, M, n_rows, prec, x0, loc, is_marg, bias, rows); break;
        case 4: nfail = run<4>(n, n_s, M, n_rows, prec, x0, loc, is_marg, bias, rows); break;
        case 5: nfail = run<5>(n, n_s, M, n_rows, prec, x0, loc, is_marg, bias, rows); break;
        case 6: nfail = run<6>(n, n_s, M, n_rows, prec, x0, loc, is_marg, bias, rows); break;
        case 8: nfail = run<8>(n, n_s, M, n_rows, prec, x0, loc, is_marg, bias, rows); break;
        case 12: nfail = run<12>(n, n_s, M, n_rows, prec, x0, loc, is_marg, bias, rows); break;
        default: nfail = run<16>(n, n_s, M, n_rows, prec, x0, loc, is_marg, bias, rows); break;
    }
    if (nfail) { fprintf(stderr, "%d checks failed\n", nfail); return 1; }
    return 0;
}
