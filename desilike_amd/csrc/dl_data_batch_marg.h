// dl_data_batch_marg.h -- data batch of a context with analytically solved parameters (include/desilike_amd.h: dl_data_set_solved, dl_eval_logposterior_data,
// dl_eval_solved_data): log-posteriors of a batch of points against a batch of data vectors when the n_s linear parameters are solved per point AND per data vector.
//
// Notation of dl_marg_solve.h.  Of the whitened residual d = y + bias_m only the additive term depends on the data (dl_data_batch.h); the derivative rows Tt [n_s, n]
// (tconst_s, plus a device row of the point where var_slot[s] >= 0) do not.  So, per POINT b (dl_dbm_point_kernel, one wavefront per point, once whatever M):
//     y = the slabs of residual row 0 summed as dl_db_slab_sum does;  Tt_s likewise for the point-dependent rows;
//     H = Tt Tt^T;  A = H + diag(prec) = C C^T;  1/2 logdet of A (of its '.marg' sub-block when n_marg < n_s);  the log-prior lp and the NaN flag of the sampled parameters
// and per PAIR (b, m) (dl_dbm_cross_kernel on tiles of points x data vectors; dl_dbm_paired_kernel, one wavefront per point):
//     d = y + bias_m;  G00 = |d|^2;  gd = Tt d;  rhs = -gd - (x0 - loc) prec;  dx = A^-1 rhs (two substitutions with the point's C);
//     ll = -1/2 G00 - 1/2 dx H dx - gd . dx - 1/2 logdet;  lps = sum -1/2 (x0 + dx - loc)^2 prec;  out = ll + lp + lps.
// G00 and gd are formed from the DIRECT difference d (the expanded form |y|^2 + 2 y . bias + |bias|^2 loses four to five digits: dl_data_batch.h); no intermediate has
// an M dimension, so nothing is chunked over M.
//
// Order of the arithmetic of a pair (a function of n and n_s only: not of the tile, the batch, the number of data vectors or the kernel):
//   d_j  = y_j + bias_mj;
//   G00  : dl_db_step / dl_db_tree of dl_data_batch.h -- eight chains over j = q, q + 8 .., then the tree;
//   gd_s = fma(Tt_sj, d_j, gd_s) over j = 0 .. n - 1 in increasing order, ONE chain per solved parameter (columns staged as zeros add +0 and change no bit);
//   the solve, the quadratic forms and lps: dl_dbm_pair_finish below, every product that feeds a sum written as an explicit fma (nothing is left to contraction,
//   so that the two kernels and the CPU program tests/csrc/emulate_data_batch_marg.cpp give the same bits from the same record).
// NSP >= n_s is the compiled size (1, 2, 3, 4, 5, 6, 8, 12, 16): the record of a point is padded with a unit factor, zero rows of H, zero prec / x0 / loc, which adds
// exact zeros.
//
// Record of a point (DL_DBM_REC doubles, written by the point kernel or by dl_dbm_point_host): H [16][16] | C [16][16] (lower triangle, zeros above) |
// 1 / C_ii [16] | 1/2 logdet, lp, flags (bit 0: NaN input, bit 1: a pivot was not positive), -.  The rows themselves -- y and the point-dependent Tt_s, slabs summed,
// tconst added -- go to a row workspace [B, 1 + n_var, ld]; constant rows are read from tconst where they are.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dl_data_batch.h"

#define DL_DBM_REC 536
#define DL_DBM_H 0
#define DL_DBM_C 256
#define DL_DBM_INV 512
#define DL_DBM_HLD 528   // 1/2 logdet
#define DL_DBM_LP 529
#define DL_DBM_FLAGS 530
#define DL_DBM_JC 16     // columns staged at a time by the cross kernel (two groups of DL_DB_NP chains)

// the constants of the solved parameters, padded with zeros to DL_MAX_SOLVED
struct DlDbmConst {
    double x0[DL_MAX_SOLVED], loc[DL_MAX_SOLVED], prec[DL_MAX_SOLVED];
};

// one column of one pair: the chain of G00 the column belongs to, and the chains of gd
template <int NSP>
DL_HD void dl_dbm_step(double& p, double* g, double y, double bias, const double* t) {
    const double d = y + bias;
    p = fma(d, d, p);
#pragma unroll
    for (int s = 0; s < NSP; ++s) g[s] = fma(t[s], d, g[s]);
}

// from G00, gd [NSP] and the record of the point: log-likelihood ll, log-prior of the solved parameters lps, dx [NSP]
template <int NSP>
DL_HD void dl_dbm_pair_finish(double g00, const double* gd, const double* rec, const DlDbmConst& k, double& ll, double& lps, double* dx) {
    const double* H = rec + DL_DBM_H;
    const double* C = rec + DL_DBM_C;
    const double* inv = rec + DL_DBM_INV;
#pragma unroll
    for (int i = 0; i < NSP; ++i) {   // forward substitution C z = rhs
        double sum = fma(-(k.x0[i] - k.loc[i]), k.prec[i], -gd[i]);
#pragma unroll
        for (int j = 0; j < i; ++j) sum = fma(-C[i * 16 + j], dx[j], sum);
        dx[i] = sum * inv[i];
    }
#pragma unroll
    for (int i = NSP - 1; i >= 0; --i) {   // backward substitution C^T dx = z
        double sum = dx[i];
#pragma unroll
        for (int j = i + 1; j < NSP; ++j) sum = fma(-C[j * 16 + i], dx[j], sum);
        dx[i] = sum * inv[i];
    }
    double quad = 0., lin = 0.;
    lps = 0.;
#pragma unroll
    for (int s = 0; s < NSP; ++s) {
        double rowsum = 0.;
#pragma unroll
        for (int t = 0; t < NSP; ++t) rowsum = fma(H[s * 16 + t], dx[t], rowsum);
        quad = fma(dx[s], rowsum, quad);
        lin = fma(gd[s], dx[s], lin);
        const double e = (k.x0[s] + dx[s]) - k.loc[s];
        const double he = (-0.5 * e) * e;
        lps = fma(he, k.prec[s], lps);
    }
    ll = (fma(-0.5, quad, -0.5 * g00) - lin) - rec[DL_DBM_HLD];
}

// the whole pair from the rows: y [n], Tt rows t_rows[s] [n] (s < n_s), bias [n] -- the statement the kernels distribute over lanes
template <int NSP>
DL_HD void dl_dbm_pair(const double* y, const double* const* t_rows, int n_s, const double* bias, int n, const double* rec, const DlDbmConst& k, double& ll, double& lps,
                       double* dx) {
    double p[DL_DB_NP], g[NSP], t[NSP];
    for (int q = 0; q < DL_DB_NP; ++q) p[q] = 0.;
    for (int s = 0; s < NSP; ++s) g[s] = 0.;
    for (int j = 0; j < n; ++j) {
        for (int s = 0; s < NSP; ++s) t[s] = s < n_s ? t_rows[s][j] : 0.;
        dl_dbm_step<NSP>(p[j % DL_DB_NP], g, y[j], bias[j], t);
    }
    dl_dbm_pair_finish<NSP>(dl_db_tree(p), g, rec, k, ll, lps, dx);
}

// compiled size for n_s solved parameters
DL_HD int dl_dbm_nsp(int n_s) { return n_s <= 6 ? n_s : n_s <= 8 ? 8 : n_s <= 12 ? 12 : 16; }

// The record of a point on the HOST (plain sqrt and log: the twin of the point kernel's factorisation, for the CPU program).  t_rows[s] [n], prec / is_marg [n_s].
// Returns false when a pivot is not positive (the record then carries flag bit 1).
inline bool dl_dbm_point_host(const double* const* t_rows, int n, int n_s, const double* prec, const int32_t* is_marg, double lp, double* rec) {
    for (int e = 0; e < DL_DBM_REC; ++e) rec[e] = 0.;
    double* H = rec + DL_DBM_H;
    double* C = rec + DL_DBM_C;
    double* inv = rec + DL_DBM_INV;
    for (int s = 0; s < n_s; ++s)
        for (int t = 0; t <= s; ++t) {
            double acc = 0.;
            for (int j = 0; j < n; ++j) acc = fma(t_rows[s][j], t_rows[t][j], acc);
            H[s * 16 + t] = H[t * 16 + s] = acc;
        }
    bool ok = true;
    for (int i = 0; i < 16; ++i) { C[i * 16 + i] = 1.; inv[i] = 1.; }
    auto cholesky = [&](const bool* use, double* L, double* invd) {   // factor of the sub-block of A on the rows with use[i]; others: unit rows.  Returns log det.
        double logdet = 0.;
        for (int j = 0; j < n_s; ++j) {
            double d = use[j] ? H[j * 16 + j] + prec[j] : 1.;
            for (int q = 0; q < j; ++q) d -= L[j * 16 + q] * L[j * 16 + q];
            if (!(d > 0.) || d == HUGE_VAL) { ok = false; d = 1.; }
            logdet += log(d);
            const double r = sqrt(d);
            L[j * 16 + j] = r;
            invd[j] = 1. / r;
            for (int i = j + 1; i < n_s; ++i) {
                double sum = (use[i] && use[j]) ? H[i * 16 + j] : 0.;
                for (int q = 0; q < j; ++q) sum -= L[i * 16 + q] * L[j * 16 + q];
                L[i * 16 + j] = sum / r;
            }
        }
        return logdet;
    };
    bool all[16], marg[16];
    int n_marg = 0;
    for (int s = 0; s < 16; ++s) { all[s] = s < n_s; marg[s] = s < n_s && is_marg[s] != 0; n_marg += marg[s]; }
    const double logdet_all = cholesky(all, C, inv);
    double hld = 0.;
    if (n_marg == n_s) hld = 0.5 * logdet_all;
    else if (n_marg > 0) {
        double S[256] = {0.}, invs[16];
        hld = 0.5 * cholesky(marg, S, invs);
    }
    rec[DL_DBM_HLD] = hld;
    rec[DL_DBM_LP] = lp;
    rec[DL_DBM_FLAGS] = ok ? 0. : 2.;
    return ok;
}

#if defined(__HIPCC__)
#include "dl_kernels.h"
// out: [B, M] (index == nullptr: cross) or [B] (paired); solved [B, n_s] (paired only, may be null); rows_ws [B, rows_per_point, ld], rec_ws [B, DL_DBM_REC]
void dl_launch_data_marg(const double* dtilde, int64_t ld, int n, int rows_per_point, int n_slabs, int64_t slab_stride, const DlMargDev& mg, const double* bias_tab, int64_t ldb,
                         int M, const int32_t* index, const double* theta, int n_params, const double* priors, int64_t B, double* rows_ws, double* rec_ws, double* out,
                         int32_t* status, double* solved, hipStream_t stream);
// the point kernel alone (the first launch of dl_launch_data_marg): rows and records of the B points, for a consumer of its own (dl_sample_solved_data.h)
void dl_launch_data_marg_points(const double* dtilde, int64_t ld, int n, int rows_per_point, int n_slabs, int64_t slab_stride, const DlMargDev& mg, const double* theta,
                                int n_params, const double* priors, int64_t B, double* rows_ws, double* rec_ws, hipStream_t stream);

// row of solved parameter s of point b: its point-dependent row in the row workspace, or the constant one (shared by the pair kernels and by the draw kernel of
// dl_sample_solved_data.hip, whose row phase must stay the paired kernel's)
__device__ __forceinline__ const double* dl_dbm_trow(const DlMargDev& mg, int s, const double* __restrict__ rows_ws, int64_t b, int rows_per_point, int64_t ld) {
    int vs = -1;
#pragma unroll
    for (int q = 0; q < DL_MAX_SOLVED; ++q) if (q == s) vs = mg.var_slot[q];
    return vs >= 0 ? rows_ws + ((size_t)b * rows_per_point + 1 + vs) * ld : mg.tconst + (size_t)s * ld;
}
#endif

#if defined(__HIPCC__) && defined(DL_DBM_KERNELS)   // (dl_kernels.hip: after dl_wave_sum, dl_grouplane, dl_lane_cholesky)
// ---- point kernel: one wavefront (one workgroup) per point -----------------------------------------------------------------------------------------------------------
// Dynamic LDS: X [1 + n_s][nx] (row 0: y, row 1 + s: Tt_s; nx = n rounded up to 8) | Hs [16][16] | Cm [16][16].
// H_st = the wave sum (dl_wave_sum: a fixed butterfly) of the lanes' chains over the columns j = lane, lane + 64 ..: a function of n only.
__global__ __launch_bounds__(64) void dl_dbm_point_kernel(const double* __restrict__ dtilde, int64_t ld, int n, int rows_per_point, int n_slabs, int64_t slab_stride,
                                                          DlMargDev mg, const double* __restrict__ theta, int n_params, const double* __restrict__ priors, int64_t B,
                                                          double* __restrict__ rows_ws, double* __restrict__ rec_ws) {
    extern __shared__ __attribute__((aligned(16))) double dl_dbm_dyn[];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (b >= B) return;
    const int ns = mg.n_s, nx = (n + 7) & ~7;
    double* X = dl_dbm_dyn;
    double* Hs = X + (size_t)(1 + ns) * nx;
    double* Cm = Hs + 256;
    const double* row0 = dtilde + (size_t)b * rows_per_point * ld;
    double* out_rows = rows_ws + (size_t)b * rows_per_point * ld;
    // priors of the sampled parameters
    double lp = 0.;
    int nan_in = 0;
    for (int p = lane; p < n_params; p += 64) {
        const double x = theta[(size_t)b * n_params + p];
        if (x != x) nan_in = 1;
        lp += dl_prior_logpdf(priors + 5 * p, x);
    }
    lp = dl_wave_sum(lp);
    nan_in = __any(nan_in);
    // rows: slabs summed once; the point-dependent ones also go to the row workspace
    for (int c = lane; c < nx; c += 64) {
        const double v = c < n ? dl_db_slab_sum(row0 + c, n_slabs, slab_stride) : 0.;
        X[c] = v;
        if (c < n) out_rows[c] = v;
    }
    for (int s = 0; s < ns; ++s) {
        const int vs = mg.var_slot[s];
        const double* cp = mg.tconst + (size_t)s * ld;
        for (int c = lane; c < nx; c += 64) {
            double v = 0.;
            if (c < n) {
                v = cp[c];
                if (vs >= 0) {
                    v += dl_db_slab_sum(row0 + (size_t)(1 + vs) * ld + c, n_slabs, slab_stride);
                    out_rows[(size_t)(1 + vs) * ld + c] = v;
                }
            }
            X[(size_t)(1 + s) * nx + c] = v;
        }
    }
    for (int e = lane; e < 256; e += 64) Hs[e] = 0.;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int s = 0; s < ns; ++s) {
        const double* xs = X + (size_t)(1 + s) * nx;
        for (int t = 0; t <= s; ++t) {
            const double* xt = X + (size_t)(1 + t) * nx;
            double acc = 0.;
            for (int c = lane; c < nx; c += 64) acc = fma(xs[c], xt[c], acc);
            acc = dl_wave_sum(acc);
            if (lane == 0) { Hs[s * 16 + t] = acc; Hs[t * 16 + s] = acc; }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // A = H + diag(prec) = C C^T: the four groups of 16 lanes factor the same system (lane li of a group owns row li), group 0 stores
    const int li = lane & 15;
    double prec_i = 0.;
    int marg_i = 0;
#pragma unroll
    for (int s = 0; s < DL_MAX_SOLVED; ++s) if (s == li) { prec_i = mg.prec[s]; marg_i = mg.is_marg[s]; }
    const bool mine = li < ns;
    double a[16], invc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = (mine && k < ns) ? Hs[li * 16 + k] + (k == li ? prec_i : 0.) : (k == li ? 1. : 0.);
    bool ok = true;
    const double logdet_all = dl_lane_cholesky<true>(a, invc, ns, li, ok);
    double hld = 0.;
    if (mg.n_marg == ns) hld = 0.5 * logdet_all;
    else if (mg.n_marg > 0) {   // the compacted '.marg' sub-block (dl_finalize_marg_kernel)
        int pos_i = 0;
#pragma unroll
        for (int s = 0; s < DL_MAX_SOLVED; ++s) if (s < li && s < ns && mg.is_marg[s]) pos_i++;
        if (lane < 16 && mine && marg_i) {
            int pos_k = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < ns && mg.is_marg[k]) { Cm[pos_i * 16 + pos_k] = Hs[li * 16 + k] + (k == li ? prec_i : 0.); pos_k++; }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int nm = mg.n_marg;
        double sub[16], invs[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) sub[k] = (li < nm && k < nm) ? Cm[li * 16 + k] : (k == li ? 1. : 0.);
        hld = 0.5 * dl_lane_cholesky<true>(sub, invs, nm, li, ok);
    }
    ok = __all(ok);
    double* rec = rec_ws + (size_t)b * DL_DBM_REC;
    if (lane < 16) {
        double inv_i = 1.;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            rec[DL_DBM_H + li * 16 + k] = Hs[li * 16 + k];
            rec[DL_DBM_C + li * 16 + k] = k <= li ? a[k] : 0.;
            if (k == li) inv_i = invc[k];
        }
        rec[DL_DBM_INV + li] = inv_i;
        if (lane < DL_DBM_REC - DL_DBM_HLD)
            rec[DL_DBM_HLD + lane] = lane == 0 ? hld : lane == 1 ? lp : lane == 2 ? (double)((nan_in ? 1 : 0) | (ok ? 0 : 2)) : 0.;
    }
}

// status rules of include/desilike_amd.h, the samplers' conventions of dl_marg_store_lane (post_mode)
__device__ __forceinline__ double dl_dbm_logposterior(double ll, double lps, const double* __restrict__ rec, int& st) {
    const double inf = __builtin_huge_val();
    const double lp = rec[DL_DBM_LP];
    const int flags = (int)rec[DL_DBM_FLAGS];
    st = DL_ST_OK;
    if (flags & 1) st = DL_ST_NAN_INPUT;
    else if (lp == -inf) st = DL_ST_OUT_OF_PRIOR;
    else if ((flags & 2) || !(ll == ll) || ll == inf || ll == -inf) st = DL_ST_NONFINITE;
    return st == DL_ST_OK ? ll + (lp + lps) : -inf;
}

// ---- cross: out[b, m] for a tile of TB = 2 TBX points x TM = 2 (256 / TBX) data vectors; thread (tb, tm) owns the 2 x 2 pairs (2 tb + {0, 1}, 2 tm + {0, 1}) ----------------
// The 1 + NSP rows of the tile's points and the bias rows of its data vectors are staged transposed in LDS, DL_DBM_JC columns at a time: per column a thread reads
// 2 + NSP 16-byte words for 4 (1 + NSP) FMAs.  TBX = 16 (32 x 32) up to NSP = 8: 43.5 KB; TBX = 8 (16 x 64) above: 47.6 KB at NSP = 16.  Rows and columns beyond B, M, n
// and parameters beyond n_s are staged as zeros; nothing outside [0, B) x [0, M) is read or written.  status: by the tiles of data vector 0.
template <int NSP, int TBX>
__global__ __launch_bounds__(256) void dl_dbm_cross_kernel(const double* __restrict__ rows_ws, int64_t ld, int n, int rows_per_point, const double* __restrict__ rec_ws,
                                                           DlMargDev mg, DlDbmConst kc, const double* __restrict__ bias_tab, int64_t ldb, int M, int64_t B,
                                                           double* __restrict__ out, int32_t* __restrict__ status) {
    constexpr int TMX = 256 / TBX, TB = 2 * TBX, TM = 2 * TMX, JC = DL_DBM_JC;
    __shared__ __attribute__((aligned(16))) double xT[1 + NSP][JC][TB + 2];   // (+2 doubles: 16-byte aligned rows that do not all start on one bank)
    __shared__ __attribute__((aligned(16))) double bT[JC][TM + 2];
    const int tid = threadIdx.x, tm = tid % TMX, tb = tid / TMX;
    const int64_t b0 = (int64_t)blockIdx.x * TB;
    const int m0 = (int)blockIdx.y * TM;
    const int ns = mg.n_s;
    double p[2][2][DL_DB_NP], g[2][2][NSP];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int q = 0; q < DL_DB_NP; ++q) p[i][k][q] = 0.;
#pragma unroll
            for (int s = 0; s < NSP; ++s) g[i][k][s] = 0.;
        }
    for (int base = 0; base < n; base += JC) {
        // stage: element e = tid + 256 u -> column e % 16 (consecutive lanes read consecutive columns of one row), row e / 16
#pragma unroll
        for (int r = 0; r <= NSP; ++r) {
#pragma unroll
            for (int u = 0; u < TB * JC / 256; ++u) {
                const int e = tid + 256 * u, c = e & (JC - 1), pt = e / JC, j = base + c;
                const int64_t b = b0 + pt;
                double v = 0.;
                if (b < B && j < n && r <= ns) v = (r == 0 ? rows_ws + (size_t)b * rows_per_point * ld : dl_dbm_trow(mg, r - 1, rows_ws, b, rows_per_point, ld))[j];
                xT[r][c][pt] = v;
            }
        }
#pragma unroll
        for (int u = 0; u < TM * JC / 256; ++u) {
            const int e = tid + 256 * u, c = e & (JC - 1), r = e / JC, j = base + c;
            const int m = m0 + r;
            bT[c][r] = (m < M && j < n) ? bias_tab[(size_t)m * ldb + j] : 0.;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < JC; ++c) {
            const dl_double2 y2 = *reinterpret_cast<const dl_double2*>(&xT[0][c][2 * tb]);
            const dl_double2 b2 = *reinterpret_cast<const dl_double2*>(&bT[c][2 * tm]);
            double t0[NSP], t1[NSP];
#pragma unroll
            for (int s = 0; s < NSP; ++s) {
                const dl_double2 t2 = *reinterpret_cast<const dl_double2*>(&xT[1 + s][c][2 * tb]);
                t0[s] = t2.x; t1[s] = t2.y;
            }
            dl_dbm_step<NSP>(p[0][0][c % DL_DB_NP], g[0][0], y2.x, b2.x, t0);
            dl_dbm_step<NSP>(p[0][1][c % DL_DB_NP], g[0][1], y2.x, b2.y, t0);
            dl_dbm_step<NSP>(p[1][0][c % DL_DB_NP], g[1][0], y2.y, b2.x, t1);
            dl_dbm_step<NSP>(p[1][1][c % DL_DB_NP], g[1][1], y2.y, b2.y, t1);
        }
        __syncthreads();   // the chunk has been read: the next one may overwrite it
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int64_t b = b0 + 2 * tb + i;
            const int m = m0 + 2 * tm + k;
            if (b >= B || m >= M) continue;
            const double* rec = rec_ws + (size_t)b * DL_DBM_REC;
            double ll, lps, dx[NSP];
            dl_dbm_pair_finish<NSP>(dl_db_tree(p[i][k]), g[i][k], rec, kc, ll, lps, dx);
            int st;
            const double v = dl_dbm_logposterior(ll, lps, rec, st);
            out[(size_t)b * M + m] = v;
            if (status && m == 0) status[b] = st;
        }
}

// ---- paired: out[b] against data vector index[b], one wavefront per point; solved [B, n_s] = x0 + dx of the pair (may be null) ------------------------------------------------
// The lanes form d = y + bias into the wavefront's LDS row; lanes 0 .. 7 run the eight chains of G00 over it, lane 8 + s the chain of gd_s: the order of the cross
// kernel.  An index outside [0, M): NaN (solved too) and DL_STATUS_NAN_INPUT; the table is not read for that row.
template <int NSP>
__global__ __launch_bounds__(256) void dl_dbm_paired_kernel(const double* __restrict__ rows_ws, int64_t ld, int n, int rows_per_point, const double* __restrict__ rec_ws,
                                                            DlMargDev mg, DlDbmConst kc, const double* __restrict__ bias_tab, int64_t ldb, int M,
                                                            const int32_t* __restrict__ index, int64_t B, double* __restrict__ out, int32_t* __restrict__ status,
                                                            double* __restrict__ solved) {
    __shared__ double dbuf[4][64 * DL_MARG_NJ];   // (n <= 512: the limit of solved contexts)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= B) return;   // (whole wavefronts leave: no workgroup barrier below)
    const int ns = mg.n_s;
    const int m = index[b];
    const bool bad = m < 0 || m >= M;
    const double* brow = bias_tab + (size_t)(bad ? 0 : m) * ldb;
    const double* yrow = rows_ws + (size_t)b * rows_per_point * ld;
    double* dw = dbuf[wave];
    double pq = 0., gs = 0.;
    if (!bad) {
        for (int c = lane; c < n; c += 64) dw[c] = yrow[c];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (!bad) {
        if (lane < DL_DB_NP) {
            for (int c = lane; c < n; c += DL_DB_NP) dl_db_step(pq, dw[c], brow[c]);
        } else if (lane < DL_DB_NP + ns) {
            const double* trow = dl_dbm_trow(mg, lane - DL_DB_NP, rows_ws, b, rows_per_point, ld);
            for (int c = 0; c < n; ++c) {
                const double d = dw[c] + brow[c];
                gs = fma(trow[c], d, gs);
            }
        }
    }
    double p[DL_DB_NP], g[NSP];
#pragma unroll
    for (int q = 0; q < DL_DB_NP; ++q) p[q] = __shfl(pq, q, 64);
#pragma unroll
    for (int s = 0; s < NSP; ++s) g[s] = __shfl(gs, DL_DB_NP + s, 64);
    if (lane == 0) {
        const double* rec = rec_ws + (size_t)b * DL_DBM_REC;
        double ll, lps, dx[NSP];
        dl_dbm_pair_finish<NSP>(dl_db_tree(p), g, rec, kc, ll, lps, dx);
        int st;
        double v = dl_dbm_logposterior(ll, lps, rec, st);
        if (bad) { v = __builtin_nan(""); st = DL_ST_NAN_INPUT; }
        out[b] = v;
        if (status) status[b] = st;
        if (solved) {
#pragma unroll
            for (int s = 0; s < NSP; ++s)
                if (s < ns) solved[(size_t)b * ns + s] = bad ? __builtin_nan("") : kc.x0[s] + dx[s];
        }
    }
}

template <int NSP>
static void dl_dbm_launch_pairs(const DlMargDev& mg, const DlDbmConst& kc, const double* rows_ws, int64_t ld, int n, int rows_per_point, const double* rec_ws,
                                const double* bias_tab, int64_t ldb, int M, const int32_t* index, int64_t B, double* out, int32_t* status, double* solved, hipStream_t stream) {
    constexpr int TBX = NSP <= 8 ? 16 : 8, TB = 2 * TBX, TM = 2 * (256 / TBX);
    if (index)
        DL_LAUNCH(dl_dbm_paired_kernel<NSP>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, rows_ws, ld, n, rows_per_point, rec_ws, mg, kc, bias_tab, ldb, M, index, B, out,
                  status, solved);
    else
        DL_LAUNCH((dl_dbm_cross_kernel<NSP, TBX>), dim3((unsigned)((B + TB - 1) / TB), (unsigned)((M + TM - 1) / TM)), dim3(256), 0, stream, rows_ws, ld, n, rows_per_point, rec_ws,
                  mg, kc, bias_tab, ldb, M, B, out, status);
}

void dl_launch_data_marg_points(const double* dtilde, int64_t ld, int n, int rows_per_point, int n_slabs, int64_t slab_stride, const DlMargDev& mg, const double* theta,
                                int n_params, const double* priors, int64_t B, double* rows_ws, double* rec_ws, hipStream_t stream) {
    const size_t shm = ((size_t)(1 + mg.n_s) * ((n + 7) & ~7) + 512) * sizeof(double);   // <= 17 x 512 + 512 doubles = 73 728 B
    if (shm > 48 * 1024) (void)hipFuncSetAttribute((const void*)dl_dbm_point_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    DL_LAUNCH(dl_dbm_point_kernel, dim3((unsigned)B), dim3(64), shm, stream, dtilde, ld, n, rows_per_point, n_slabs, slab_stride, mg, theta, n_params, priors, B, rows_ws, rec_ws);
}

void dl_launch_data_marg(const double* dtilde, int64_t ld, int n, int rows_per_point, int n_slabs, int64_t slab_stride, const DlMargDev& mg, const double* bias_tab, int64_t ldb,
                         int M, const int32_t* index, const double* theta, int n_params, const double* priors, int64_t B, double* rows_ws, double* rec_ws, double* out,
                         int32_t* status, double* solved, hipStream_t stream) {
    const int ns = mg.n_s;
    dl_launch_data_marg_points(dtilde, ld, n, rows_per_point, n_slabs, slab_stride, mg, theta, n_params, priors, B, rows_ws, rec_ws, stream);
    DlDbmConst kc;
    for (int s = 0; s < DL_MAX_SOLVED; ++s) { kc.x0[s] = s < ns ? mg.x0[s] : 0.; kc.loc[s] = s < ns ? mg.loc[s] : 0.; kc.prec[s] = s < ns ? mg.prec[s] : 0.; }
    auto launch = [&](auto tag) {
        dl_dbm_launch_pairs<decltype(tag)::value>(mg, kc, rows_ws, ld, n, rows_per_point, rec_ws, bias_tab, ldb, M, index, B, out, status, solved, stream);
    };
    switch (dl_dbm_nsp(ns)) {
        case 1: launch(std::integral_constant<int, 1>()); break;
        case 2: launch(std::integral_constant<int, 2>()); break;
        case 3: launch(std::integral_constant<int, 3>()); break;
        case 4: launch(std::integral_constant<int, 4>()); break;
        case 5: launch(std::integral_constant<int, 5>()); break;
        case 6: launch(std::integral_constant<int, 6>()); break;
        case 8: launch(std::integral_constant<int, 8>()); break;
        case 12: launch(std::integral_constant<int, 12>()); break;
        default: launch(std::integral_constant<int, 16>()); break;
    }
}
#endif
