// CPU run of the per-pair reduction of the data-batch kernels (desilike_amd/csrc/dl_data_batch.h): the same functions the device compiles, here with g++.
// A program of its own (tests/test_data_batch.py runs the plain build and the build under the address / undefined-behaviour sanitizers).
//   1. dl_db_pair_chi2 and dl_db_slab_sum against long-double sums for n in {1, 63, 64, 65, 120, 257} and 1 .. 19 slabs;
//   2. the two ways the kernels distribute that statement -- the cross kernel's staged chunks of DL_DB_JC columns padded with zeros, the paired kernel's eight lanes
//      striding a staged chunk of DL_DB_PC columns -- replayed sequentially: both must give the BITS of dl_db_pair_chi2 (the tested contract cross == paired).
// Bound of 1.: chi2 is a sum of non-negative terms d^2, d = y + bias (one rounding: relative 2^-53, so 2^-52 on d^2 to first order), each added by one fma to a
// chain of ceil(n / 8) terms (one rounding per link, relative to a partial sum that never exceeds the total), the eight chains added by a tree of depth 3:
// |error| <= (ceil(n / 8) + 3 + 2) 2^-53 chi2 to first order; the program allows (ceil(n / 8) + 8) 2^-52, twice that and change.  The slab sum is a sum of
// n_slabs terms of either sign in ceil(n_slabs / 8) + 1 groups of depth-3 trees: |error| <= (ceil(n_slabs / 8) + 4) 2^-53 sum |t|, allowed: twice that.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../desilike_amd/csrc/dl_data_batch.h"

static uint64_t lcg_state = 20240607;
static double uniform() {   // (-0.5, 0.5)
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(lcg_state >> 11) / 9007199254740992. - 0.5;
}

// the cross kernel's order for one pair: chunks of DL_DB_JC columns, columns beyond n staged as zeros, column c of a chunk on chain c % DL_DB_NP
static double cross_order(const double* y, const double* bias, int n) {
    double p[DL_DB_NP], ys[DL_DB_JC], bs[DL_DB_JC];
    for (int q = 0; q < DL_DB_NP; ++q) p[q] = 0.;
    for (int base = 0; base < n; base += DL_DB_JC) {
        for (int c = 0; c < DL_DB_JC; ++c) { ys[c] = base + c < n ? y[base + c] : 0.; bs[c] = base + c < n ? bias[base + c] : 0.; }
        for (int c = 0; c < DL_DB_JC; ++c) dl_db_step(p[c % DL_DB_NP], ys[c], bs[c]);
    }
    return dl_db_tree(p);
}

// the paired kernel's order: per chunk of DL_DB_PC columns, lane q < DL_DB_NP runs c = q, q + DL_DB_NP .. over the staged row; the partial sums are then gathered
static double paired_order(const double* y, const double* bias, int n) {
    double p[DL_DB_NP], ys[DL_DB_PC];
    for (int q = 0; q < DL_DB_NP; ++q) p[q] = 0.;
    for (int base = 0; base < n; base += DL_DB_PC) {
        const int width = n - base < DL_DB_PC ? n - base : DL_DB_PC;
        for (int c = 0; c < width; ++c) ys[c] = y[base + c];
        for (int lane = 0; lane < DL_DB_NP; ++lane)
            for (int c = lane; c < width; c += DL_DB_NP) dl_db_step(p[lane], ys[c], bias[base + c]);
    }
    return dl_db_tree(p);
}

int main() {
    static_assert(DL_DB_JC % DL_DB_NP == 0 && DL_DB_PC % DL_DB_NP == 0, "a staged chunk holds whole groups of chains");
    const int sizes[] = {1, 63, 64, 65, 120, 257, 600, 1031};   // (the last two: more than one chunk of the paired kernel)
    int nfail = 0;
    for (int n : sizes) {
        // y of the size of a whitened theory vector (1e2 - 1e3 per entry), bias its near opposite: the residual is of order one, as in a fit
        std::vector<double> y(n), bias(n);
        long double ref = 0.L;
        for (int j = 0; j < n; ++j) {
            y[j] = 2000. * uniform();
            bias[j] = -y[j] + 2. * uniform();
            const long double d = (long double)y[j] + (long double)bias[j];
            ref += d * d;
        }
        const double chi2 = dl_db_pair_chi2(y.data(), bias.data(), n);
        const double err = (double)fabsl((long double)chi2 - ref), bound = ((n + DL_DB_NP - 1) / DL_DB_NP + 8) * DBL_EPSILON * (double)ref;
        const double cross = cross_order(y.data(), bias.data(), n), paired = paired_order(y.data(), bias.data(), n);
        const bool same = memcmp(&cross, &chi2, sizeof(double)) == 0 && memcmp(&paired, &chi2, sizeof(double)) == 0;
        printf("n = %4d  chi2 = %.17g  error = %.3e  bound = %.3e  cross / paired orders %s\n", n, chi2, err, bound, same ? "same bits" : "DIFFER");
        if (!(err <= bound) || !same) nfail++;
    }
    for (int n_slabs = 1; n_slabs <= 19; ++n_slabs) {
        const int64_t stride = 7;
        std::vector<double> slabs(n_slabs * stride);
        long double ref = 0.L, mag = 0.L;
        for (auto& v : slabs) v = 1e300;   // (entries between the strided ones are not read: a read would show as an overflowing sum)
        for (int s = 0; s < n_slabs; ++s) { slabs[s * stride] = 1000. * uniform(); ref += slabs[s * stride]; mag += fabsl(slabs[s * stride]); }
        const double sum = dl_db_slab_sum(slabs.data(), n_slabs, stride);
        const double err = (double)fabsl((long double)sum - ref), bound = ((n_slabs + 7) / 8 + 4) * DBL_EPSILON * (double)mag;
        if (!(err <= bound)) { printf("slab sum of %d slabs: error %.3e above %.3e\n", n_slabs, err, bound); nfail++; }
    }
    // an empty row: chi2 = 0 exactly
    if (dl_db_pair_chi2(nullptr, nullptr, 0) != 0.) nfail++;
    if (nfail) { printf("%d checks failed\n", nfail); return 1; }
    printf("data batch reduction: sizes and slab counts agree with the long-double sums, kernel orders give the same bits\n");
    return 0;
}
