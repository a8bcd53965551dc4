// CPU run of the residual row of a (point, data vector) pair (desilike_amd/csrc/dl_data_batch.h: dl_db_resid, dl_db_resid_entry, dl_db_resid_row and the per-thread
// statement dl_db_resid_pair of dl_data_resid_kernel): the same functions the device compiles, here with g++.  A program of its own (tests/test_data_batch_analytic.py
// runs the plain build and the build under the address / undefined-behaviour sanitizers).
// For n in {1, 7, 8, 9, 120, 513} x n_slabs in {1, 2, 3, 9}, three points against a table of two data vectors, checked indices {1, -1, 0}:
//   1. the live entries of a row are the d_j of dl_db_step, bit for bit: d_j = dl_db_slab_sum(column j) + bias[m][j], and fma(d_j, d_j, 0) is what one dl_db_step leaves
//      in an empty chain;
//   2. the tail [n, N_pad) is exact +0.0;
//   3. the row of the point whose checked index is -1 is NaN in its live columns, zero in its tail;
//   4. the kernel's distribution -- thread t owns columns (2 c, 2 c + 1) of row t / (N_pad / 2) -- replayed sequentially gives the bits of dl_db_resid_row, the pair
//      that straddles an odd n included.
// Every buffer holds exactly what the contract allows to be touched -- slabs n_slabs x B x N_pad, table M x N_pad, output B x N_pad doubles, each its own heap block --
// so that the sanitizer build sees any read or write outside [0, B) x [0, N_pad) or outside the table.  What this program shows about a point without a data vector
// is that the shared functions, given NO row of the table (a null pointer), read none and return NaN; the mapping from a checked index of -1 to that null pointer is one
// line of dl_data_resid_kernel (`m < 0 ? nullptr : bias_tab + m ldb`), replayed here, not taken from the kernel: the device side of it is the GPU test of bad indices.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../desilike_amd/csrc/dl_data_batch.h"

// two doubles with the operations dl_db_slab_sum_t / dl_db_resid_entry ask of their value type (the device uses a 16-byte vector).  may_alias: dl_db_resid_pair reads
// the rows of doubles through a pointer to this type, as the device reads them through a pointer to its vector; without the attribute that is an aliasing violation
// g++ -O2 may act on and no sanitizer reports
struct __attribute__((may_alias)) pair2 {
    double x, y;
    pair2() : x(0.), y(0.) {}
    explicit pair2(double v) : x(v), y(v) {}
    pair2(double a, double b) : x(a), y(b) {}
    pair2 operator+(const pair2& o) const { return pair2(x + o.x, y + o.y); }
    pair2& operator+=(const pair2& o) { x += o.x; y += o.y; return *this; }
};

static uint64_t lcg_state = 20250311;
static double uniform() {   // (-0.5, 0.5)
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(lcg_state >> 11) / 9007199254740992. - 0.5;
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0; }

int main() {
    const int sizes[] = {1, 7, 8, 9, 120, 513}, slab_counts[] = {1, 2, 3, 9};
    const int B = 3, M = 2, checked[B] = {1, -1, 0};
    int nfail = 0;
    for (int n : sizes)
        for (int n_slabs : slab_counts) {
            const int N_pad = (n + 127) / 128 * 128;
            const int64_t slab_stride = (int64_t)B * N_pad;
            std::vector<double> slabs((size_t)n_slabs * B * N_pad), table((size_t)M * N_pad), out((size_t)B * N_pad, -7.), dist((size_t)B * N_pad, -7.);
            // slab entries of the size of a whitened theory vector split over the slabs, the bias their near opposite: a residual of order one, as in a fit;
            // the padding columns of the slabs hold what an earlier, wider call may have left (finite, not zero)
            for (auto& v : slabs) v = 2000. * uniform();
            for (int m = 0; m < M; ++m)
                for (int j = 0; j < N_pad; ++j) table[(size_t)m * N_pad + j] = j < n ? -1000. * uniform() : 0.;
            for (int b = 0; b < B; ++b)
                dl_db_resid_row(slabs.data() + (size_t)b * N_pad, n_slabs, slab_stride, table.data(), N_pad, checked[b], n, N_pad, out.data() + (size_t)b * N_pad);
            int bad = 0;
            for (int b = 0; b < B; ++b)
                for (int j = 0; j < N_pad; ++j) {
                    const double v = out[(size_t)b * N_pad + j];
                    if (j >= n) { if (!same_bits(v, 0.)) bad++; continue; }
                    if (checked[b] < 0) { if (v == v) bad++; continue; }
                    const double y = dl_db_slab_sum(slabs.data() + (size_t)b * N_pad + j, n_slabs, slab_stride), bias = table[(size_t)checked[b] * N_pad + j];
                    const double d = y + bias;
                    double p = 0.;
                    dl_db_step(p, y, bias);
                    if (!same_bits(v, d) || !same_bits(p, fma(v, v, 0.))) bad++;
                }
            // the kernel's distribution over threads
            const int half = N_pad / 2;
            for (int64_t t = 0; t < (int64_t)B * half; ++t) {
                const int64_t b = t / half;
                const int j = 2 * (int)(t - b * half), m = checked[b];
                const pair2 v = dl_db_resid_pair<pair2>(slabs.data() + (size_t)b * N_pad, n_slabs, slab_stride, m < 0 ? nullptr : table.data() + (size_t)m * N_pad, j, n);
                dist[(size_t)b * N_pad + j] = v.x;
                dist[(size_t)b * N_pad + j + 1] = v.y;
            }
            const bool same = memcmp(dist.data(), out.data(), out.size() * sizeof(double)) == 0;
            printf("n = %3d  N_pad = %3d  slabs = %d  entries off: %d  thread distribution %s\n", n, N_pad, n_slabs, bad, same ? "same bits" : "DIFFERS");
            if (bad || !same) nfail++;
        }
    // a point without a data vector next to a table it must not read: no table at all
    {
        const int n = 9, N_pad = 128;
        std::vector<double> slabs((size_t)2 * N_pad, 1.), out(N_pad, -7.);
        dl_db_resid_row(slabs.data(), 2, N_pad, nullptr, N_pad, -1, n, N_pad, out.data());
        for (int j = 0; j < N_pad; ++j)
            if (j < n ? out[j] == out[j] : !same_bits(out[j], 0.)) nfail++;
        for (int j = 0; j < N_pad; j += 2) {
            const pair2 v = dl_db_resid_pair<pair2>(slabs.data(), 2, N_pad, nullptr, j, n);
            if (j + 1 < n ? (v.x == v.x || v.y == v.y) : j < n ? (v.x == v.x || !same_bits(v.y, 0.)) : (!same_bits(v.x, 0.) || !same_bits(v.y, 0.))) nfail++;
        }
    }
    if (nfail) { printf("%d checks failed\n", nfail); return 1; }
    printf("data batch residual rows: live entries are the d_j of dl_db_step bit for bit, tails are zero, rows without a data vector are NaN and read no table\n");
    return 0;
}
