// dl_emu_jac.h -- analytic Jacobian of an emulated (velocileptors-table) full-shape theory: the exact derivative rows dl_eval_fisher_analytic feeds to the Gram product for
// BASELINE configs[2], the forward-mode twin of dl_emu_grad.h (the reference's Differentiation takes these derivatives from jax, desilike/differentiation.py).
//
// Notation (one centre, whitened data space, columns j < N_pad; dl_feature_gemm.h:1-9, dl_emu_grad.h:4-6).  The context is created with the solved parameters varied
// (Fisher does so), so there is one monomial row c(theta) [19] and
//   d~[j] = sum_m c_m U_m[j] + bias[j],   U_m[j] = sum_h G[(m, j)][h] basis_h(x(theta)):
// bilinear in the monomials c and the basis.  x [n_x] are the emulator inputs; x_q is theta column col_q or a constant; q runs over the n_xv <= DL_MAX_X inputs that ARE
// theta columns.  The derivative row of theta_p is
//   D~_p[j] = sum_m (d c_m / d theta_p) U_m[j] + sum_q [col_q == p] sum_m c_m (G . d basis / d x_q)_m[j].
// First term: c depends on 13 inputs -- the eleven velocileptors 'pars' inputs v (theta columns vp_in, or constants), sigma8 and fsigma8 (scalar engines of x):
//   d c_m / d theta_p = sum_k [vp_in[k].col == p] J[k][m] + sum_q [col_q == p] (J[11][m] d sigma8 / d x_q + J[12][m] d fsigma8 / d x_q),
// J [13][19] = d c / d (v, sigma8, fsigma8): forward mode of dl_velocileptors_prelude / _row0 (dl_ej_mono_jvp_row below, all four mono_modes, the REPT co-evolution shift;
// its transpose is dl_eg_mono_vjp of dl_emu_grad.h: y^T (J v) = v^T vjp(y)).  The chain entries [vp_in[k].col == p], [col_q == p] are structural, and a scalar-engine
// tangent that is exactly zero (a constant engine) is skipped, not multiplied: a parameter that reaches nothing leaves an exactly zero row.
// Second term: the basis and its tangents go through the SAME operator, so (G . d basis / d x_q) is one more row of the U GEMM: per centre 1 + n_xv basis rows
// [basis; d basis / d x_1 .. d basis / d x_n_xv] in the record layout dl_emu_grad_u_kernel reads (nb_pad doubles, zero beyond n_basis).
// Engines, value z and one tangent z'_q per varied input carried side by side:
//   MLP: x-scaler xs_i = (x_i - lo_i) inv_i, xs'_q,i = [i == q] inv_q; layer z = b + W^T a, z'_q = W^T a'_q; a = act(z), a'_q = act'(z) z'_q (relu: act'(0) = 0, jax's
//        convention); scalar engines end y = v yscale + ylo, y'_q = v'_q yscale; the table engine stops after its last hidden layer, its constant basis function has tangent 0;
//   Taylor: basis_t = prod_p (x_p - c_p)^k_tp, d / d x_q = k_tq (x_q - c_q)^(k_tq - 1) prod_{p != q} (x_p - c_p)^k_tp (0 when k_tq = 0); scalar engines sum with coef.
//
// Launch sequence per pass (dl_api.hip): dl_emu_jac_tangent_kernel (one wavefront per centre: basis rows, c, d c / d theta) -> dl_emu_grad_u_kernel over (1 + n_xv) rows per
// centre (fp64 MFMA, unchanged) -> dl_emu_jac_rows_kernel (X = [d~; D~_1 .. D~_P], fixed summation order, no atomics: two calls give the same bits; padding columns
// [N_live, N_pad) zero) -> dl_fisher_kernel<TILES, GIVEN = true>.
//
// Scope (dl_eval_fisher_analytic returns 2 otherwise): ONE emulated observable on the feature path (theory 3, n_mono == DL_N_MONO, n_pass == 0), table engine an MLP or a
// Taylor engine, sigma8 / fsigma8 engines MLP, Taylor or constant, no transform, no solved parameter, P <= 31.  The stacked layout, several observables, emulated xi_l: not covered.
//
// The per-point arithmetic (dl_ej_mono_jvp_row, dl_ej_engine) is host-buildable (tests/csrc/emulate_emu_jac.cpp): the layer / engine functions take (lane0, stride) --
// (threadIdx.x, 64) on the device with a barrier between layers, (0, 1) on the host.
#pragma once
#include "dl_emu_grad.h"

#define DL_EJ_NIN DL_EG_NIN   // inputs of the monomials: the eleven 'pars' inputs, sigma8, fsigma8

#if defined(__HIP_DEVICE_COMPILE__)
#define DL_EJ_SYNC __syncthreads();
#else
#define DL_EJ_SYNC
#endif

// the emulator inputs that are theta columns: tangent r < n_xv differentiates with respect to input xq[r], which is theta column col[r]
struct DlEjCols { int32_t n_xv, pad; int32_t xq[DL_MAX_X], col[DL_MAX_X]; };
DL_HD DlEjCols dl_ej_cols(const DlObsDev& o) {
    DlEjCols c;
    c.n_xv = 0; c.pad = 0;
    for (int i = 0; i < DL_MAX_X; ++i) { c.xq[i] = -1; c.col[i] = -1; }
    for (int i = 0; i < o.n_x && i < DL_MAX_X; ++i)
        if (o.x_in[i].col >= 0) { c.xq[c.n_xv] = i; c.col[c.n_xv] = o.x_in[i].col; ++c.n_xv; }
    return c;
}

// row k of J [13][19]: d c_m / d input_k, inputs k < 11: v[k], 11: sigma8, 12: fsigma8 (forward mode of dl_velocileptors_prelude + _row0)
DL_HD void dl_ej_mono_jvp_row(const DlObsDev& o, const double* v, double sigma8, double fsigma8, int k, double* row) {
    DlVeloPre p;
    dl_velocileptors_prelude(o, v, sigma8, fsigma8, p);
    const bool rept = (o.mono_mode == 2 || o.mono_mode == 4);
    double dq0, dq1, dq2, dq3, dp4, dp5, dp6, dp7, dp8, dp9, dp10;
    if (p.physical) {
        const double s = sigma8, is = 1. / s, is2 = is * is, is3 = is2 * is, one = p.one_b1L, f = p.f;
        // one = v0 / s, f = fsigma8 / s, b2L = v1 / s^2, bsL = v2 / s^2, b3L = v3 / s^3
        const double d_one = k == 0 ? is : k == 11 ? -v[0] * is2 : 0.;
        const double d_f = k == 12 ? is : k == 11 ? -fsigma8 * is2 : 0.;
        const double d_b2L = k == 1 ? is2 : k == 11 ? -2. * v[1] * is3 : 0.;
        const double d_bsL = k == 2 ? is2 : k == 11 ? -2. * v[2] * is3 : 0.;
        const double d_b3L = k == 3 ? is3 : k == 11 ? -3. * v[3] * is3 * is : 0.;
        const double dv4 = k == 4 ? 1. : 0., dv5 = k == 5 ? 1. : 0., dv6 = k == 6 ? 1. : 0.;
        dq0 = d_one;
        dq1 = rept ? (8. / 21.) * d_one + d_b2L : d_b2L;
        dq2 = d_bsL;
        dq3 = d_b3L;
        dp4 = 2. * one * d_one * v[4] + one * one * dv4;
        dp5 = (d_f * one + f * d_one) * (v[4] + v[5]) + f * one * (dv4 + dv5);
        dp6 = d_f * (f * v[5] + one * v[6]) + f * (d_f * v[5] + f * dv5 + d_one * v[6] + one * dv6);
        dp7 = 2. * f * d_f * v[6] + f * f * dv6;
        dp8 = k == 8 ? p.sn_scale[0] : 0.;
        dp9 = k == 9 ? p.sn_scale[1] : 0.;
        dp10 = k == 10 ? p.sn_scale[2] : 0.;
    } else {
        dq0 = k == 0 ? 1. : 0.; dq1 = k == 1 ? 1. : 0.; dq2 = k == 2 ? 1. : 0.; dq3 = k == 3 ? 1. : 0.;
        dp4 = k == 4 ? 1. : 0.; dp5 = k == 5 ? 1. : 0.; dp6 = k == 6 ? 1. : 0.; dp7 = k == 7 ? 1. : 0.;
        dp8 = k == 8 ? 1. : 0.; dp9 = k == 9 ? 1. : 0.; dp10 = k == 10 ? 1. : 0.;
    }
    // co-evolution (full_shape.py:1481-1485): bs = q2 - 2/7 (q0 - 1), b3 = 3 q3 + (q0 - 1)
    const double db1 = dq0, db2 = dq1, dbs = rept ? dq2 - (2. / 7.) * dq0 : dq2, db3 = rept ? 3. * dq3 + dq0 : dq3;
    const double b1 = p.pars[0], b2 = p.pars[1], bs = p.pars[2], b3 = p.pars[3];
    row[0] = 0.; row[1] = db1; row[2] = 2. * b1 * db1; row[3] = db2; row[4] = db1 * b2 + b1 * db2; row[5] = 2. * b2 * db2; row[6] = dbs; row[7] = db1 * bs + b1 * dbs;
    row[8] = db2 * bs + b2 * dbs; row[9] = 2. * bs * dbs; row[10] = db3; row[11] = db1 * b3 + b1 * db3; row[12] = dp4; row[13] = dp5; row[14] = dp6; row[15] = dp7;
    row[16] = dp8 / o.nd; row[17] = dp9 / o.nd; row[18] = dp10 / o.nd;
}

// one dense layer, value row 0 and NT tangent rows (row stride ldb): out[0][u] = act(z_u), out[1 + r][u] = act'(z_u) z'_r,u; units u = lane0, lane0 + stride, ...
template <int NT>
DL_HD void dl_ej_mlp_layer(int lane0, int stride, const DlObsDev::Engine& e, int layer, const double* w, const double* in, double* out, int ldb, bool activate) {
    const int nin = e.widths[layer], nout = e.widths[layer + 1];
    for (int u = lane0; u < nout; u += stride) {
        double acc[1 + NT];
        acc[0] = w[(size_t)nin * nout + u];
#pragma unroll
        for (int r = 1; r <= NT; ++r) acc[r] = 0.;
        for (int i = 0; i < nin; ++i) {
            const double wi = w[(size_t)i * nout + u];
#pragma unroll
            for (int r = 0; r <= NT; ++r) acc[r] = fma(in[(size_t)r * ldb + i], wi, acc[r]);
        }
        const double d = activate ? dl_eg_act_deriv(e.act, acc[0]) : 1.;
        out[u] = activate ? dl_activation(e.act, acc[0]) : acc[0];
#pragma unroll
        for (int r = 1; r <= NT; ++r) out[(size_t)r * ldb + u] = d * acc[r];
    }
}

// engine ie at the inputs x [n_x]: value (row 0) and the tangents with respect to the inputs cols.xq[r], r < NT (rows 1 + r; rows of r >= cols.n_xv are zero), row stride ldb,
// in the returned buffer (bufa or bufb, each [(1 + NT)][ldb]).  Table engine: the basis functions (MLP: widths[n_layers] of them; Taylor: n_terms).  Scalar engines: entry 0.
template <int NT>
DL_HD double* dl_ej_engine(int lane0, int stride, const DlObsDev& o, int ie, const DlEjCols& cols, const double* x, double* bufa, double* bufb, int ldb) {
    const DlObsDev::Engine& e = o.eng[ie];
    double* cur = bufa;
    double* nxt = bufb;
    if (e.type == 0) {
        for (int i = lane0; i < o.n_x; i += stride) {
            cur[i] = (x[i] - e.xlo[i]) * e.xinv[i];
#pragma unroll
            for (int r = 0; r < NT; ++r) cur[(size_t)(1 + r) * ldb + i] = cols.xq[r] == i ? e.xinv[i] : 0.;
        }
        DL_EJ_SYNC
        const double* w = e.weights;
        for (int layer = 0; layer < e.n_layers; ++layer) {
            const bool activate = ie == 0 || layer < e.n_layers - 1;
            dl_ej_mlp_layer<NT>(lane0, stride, e, layer, w, cur, nxt, ldb, activate);
            DL_EJ_SYNC
            w += (size_t)e.widths[layer] * e.widths[layer + 1] + e.widths[layer + 1];
            double* t = cur; cur = nxt; nxt = t;
        }
        if (ie != 0) {
            if (lane0 == 0) {
                cur[0] = cur[0] * e.yscale + e.ylo;
#pragma unroll
                for (int r = 1; r <= NT; ++r) cur[(size_t)r * ldb] *= e.yscale;
            }
            DL_EJ_SYNC
        }
        return cur;
    }
    // Taylor (dl_emu_engine): the value with the factors in the order of the evaluation path
    for (int t = lane0; t < e.n_terms; t += stride) {
        const double* pw = e.powers + (size_t)t * o.n_x;
        double mon = 1.;
        for (int p = 0; p < o.n_x; ++p) mon *= dl_ipow(x[p] - e.center[p], (int)pw[p]);
        cur[t] = mon;
#pragma unroll
        for (int r = 0; r < NT; ++r) {
            const int q = cols.xq[r];
            double d = 0.;
            if (q >= 0 && (int)pw[q] > 0) {
                d = pw[q] * dl_ipow(x[q] - e.center[q], (int)pw[q] - 1);
                for (int p = 0; p < o.n_x; ++p) if (p != q) d *= dl_ipow(x[p] - e.center[p], (int)pw[p]);
            }
            cur[(size_t)(1 + r) * ldb + t] = d;
        }
    }
    DL_EJ_SYNC
    if (ie != 0) {
        if (lane0 == 0) {
            double sum[1 + NT];
#pragma unroll
            for (int r = 0; r <= NT; ++r) sum[r] = 0.;
            for (int t = 0; t < e.n_terms; ++t) {
#pragma unroll
                for (int r = 0; r <= NT; ++r) sum[r] = fma(e.coef[t], cur[(size_t)r * ldb + t], sum[r]);
            }
#pragma unroll
            for (int r = 0; r <= NT; ++r) nxt[(size_t)r * ldb] = sum[r];
        }
        DL_EJ_SYNC
        return nxt;
    }
    return cur;
}

// row stride of the engine buffers: the widest layer (or term list) of the three engines, even
DL_HD int dl_ej_ldb(const DlObsDev& o) {
    int w = o.n_x;
    for (int ie = 0; ie < 3; ++ie) {
        const DlObsDev::Engine& e = o.eng[ie];
        if (e.type == 0) { for (int l = 0; l <= e.n_layers; ++l) w = e.widths[l] > w ? e.widths[l] : w; }
        else if (e.type == 1) w = e.n_terms > w ? e.n_terms : w;
    }
    return (w + 1) / 2 * 2;
}
// LDS doubles of dl_emu_jac_tangent_kernel<NT>: x [DL_MAX_X] | v [12] | scalars [2][(1 + NT)] | J [13][20 = DL_FG_MONO_LD] | two engine buffers [(1 + NT)][ldb]
DL_HD size_t dl_ej_tangent_doubles(const DlObsDev& o, int NT) {
    return DL_MAX_X + 12 + 2 * (size_t)(1 + NT) + (size_t)DL_EJ_NIN * 20 + 2 * (size_t)(1 + NT) * dl_ej_ldb(o);
}

#if defined(__HIPCC__)

// One centre per 64-thread workgroup, NT >= n_xv tangents (4, 8 or 16: compile-time, so that the accumulators of a unit live in registers): the three engines forward with
// value and tangents, then basis_rows [B (1 + n_xv)][nb_pad] (the rows of the U GEMM), cmono [B][20] (the monomials) and dmono [B][P][20] (d c / d theta_p).
template <int NT>
__global__ __launch_bounds__(64) void dl_emu_jac_tangent_kernel(const DlObsDev o, const DlEjCols cols, const double* __restrict__ theta, int n_params,
                                                                double* __restrict__ basis_rows, double* __restrict__ cmono, double* __restrict__ dmono, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const double* th = theta + (size_t)b * n_params;
    const int ldb = dl_ej_ldb(o), n_xv = cols.n_xv;
    double* x = lds;                                   // [DL_MAX_X]
    double* v = x + DL_MAX_X;                          // [12]
    double* sc = v + 12;                               // [2][(1 + NT)]: sigma8 and its tangents, fsigma8 and its tangents
    double* J = sc + 2 * (1 + NT);                     // [13][20]
    double* bufa = J + DL_EJ_NIN * DL_FG_MONO_LD;
    double* bufb = bufa + (size_t)(1 + NT) * ldb;
    for (int i = lane; i < o.n_x; i += 64) x[i] = dl_get(o.x_in[i], th);
    for (int c = lane; c < DL_N_VPARS; c += 64) v[c] = dl_get(o.vp_in[c], th);
    __syncthreads();
    for (int ie = 1; ie < 3; ++ie) {
        double* s = sc + (size_t)(ie - 1) * (1 + NT);
        if (o.eng[ie].type < 0) {
            if (lane <= NT) s[lane] = lane == 0 ? o.eng[ie].cst : 0.;
        } else {
            const double* out = dl_ej_engine<NT>(lane, 64, o, ie, cols, x, bufa, bufb, ldb);
            if (lane <= NT) s[lane] = out[(size_t)lane * ldb];
        }
        __syncthreads();
    }
    const double* basis = dl_ej_engine<NT>(lane, 64, o, 0, cols, x, bufa, bufb, ldb);
    // the basis rows: value, then one tangent per varied input; the constant basis function of an MLP table engine has value 1 and tangent 0
    const int nb_live = o.eng[0].type == 0 ? o.n_basis - 1 : o.n_basis;
    double* rows = basis_rows + (size_t)b * (1 + n_xv) * o.nb_pad;
    for (int idx = lane; idx < (1 + n_xv) * o.nb_pad; idx += 64) {
        const int r = idx / o.nb_pad, h = idx - r * o.nb_pad;
        rows[idx] = h < nb_live ? basis[(size_t)r * ldb + h] : (h < o.n_basis && r == 0) ? 1. : 0.;
    }
    if (lane < DL_EJ_NIN) {
        double* row = J + lane * DL_FG_MONO_LD;
        dl_ej_mono_jvp_row(o, v, sc[0], sc[1 + NT], lane, row);
        row[19] = 0.;
    } else if (lane == DL_EJ_NIN) {
        DlVeloPre p;
        double r0[20];
        dl_velocileptors_prelude(o, v, sc[0], sc[1 + NT], p);
        dl_velocileptors_row0(o, p, r0);
#pragma unroll
        for (int m = 0; m < 20; ++m) cmono[(size_t)b * DL_FG_MONO_LD + m] = r0[m];
    }
    __syncthreads();
    const bool s8_live = o.eng[1].type >= 0, fs8_live = o.eng[2].type >= 0;
    double* dm = dmono + (size_t)b * n_params * DL_FG_MONO_LD;
    for (int idx = lane; idx < n_params * DL_FG_MONO_LD; idx += 64) {
        const int p = idx / DL_FG_MONO_LD, m = idx - p * DL_FG_MONO_LD;
        double acc = 0.;
        for (int k = 0; k < DL_N_VPARS; ++k) if (o.vp_in[k].col == p) acc += J[k * DL_FG_MONO_LD + m];
        for (int r = 0; r < n_xv; ++r) {
            if (cols.col[r] != p) continue;
            const double d8 = sc[1 + r], df8 = sc[1 + NT + 1 + r];
            if (s8_live && d8 != 0.) acc = fma(J[11 * DL_FG_MONO_LD + m], d8, acc);
            if (fs8_live && df8 != 0.) acc = fma(J[12 * DL_FG_MONO_LD + m], df8, acc);
        }
        dm[idx] = acc;
    }
}

// X = [d~; D~_1 .. D~_P] of one centre per 128-thread workgroup from U [B (1 + n_xv)][19][ldu], the monomials cmono [B][20] and dmono [B][P][20]:
//   resid [B][ldr]: d~[j] = bias[j] + sum_m c_m U_0m[j] (the order of dl_emu_grad_adjoint_kernel);  rows [B P][ld]: D~_p[j] = sum_m dc_pm U_0m[j] (zero entries skipped)
//   + sum_{r: col_r == p} sum_m c_m U_(1 + r)m[j].  Each thread owns its columns, every sum runs in index order; columns [n_live, N_pad) are written as zeros.
// data_index (dl_eval_fisher_analytic_data; null: as above): `bias` is the table [M, ldb] of whitened bias rows of the data batch and the sum of centre b starts from
// row data_index[b] of it -- CHECKED indices (dl_data_batch.h): -1 starts it from NaN and the table is not read.  The order of the sum is the same.
__global__ __launch_bounds__(128) void dl_emu_jac_rows_kernel(const DlEjCols cols, const double* __restrict__ U, int64_t ldu, const double* __restrict__ cmono,
                                                              const double* __restrict__ dmono, const double* __restrict__ bias, int n_params, int n_live, int N_pad,
                                                              double* __restrict__ resid, int64_t ldr, double* __restrict__ rows, int64_t ld, int64_t B,
                                                              const int32_t* __restrict__ data_index, int64_t ldb) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, n_xv = cols.n_xv;
    const int64_t b = blockIdx.x;
    const int data_row = data_index ? data_index[b] : 0;
    const double* brow = data_index ? (data_row >= 0 ? bias + (size_t)data_row * ldb : nullptr) : bias;
    double* c = lds;                          // [20]
    double* dc = lds + DL_FG_MONO_LD;         // [P][20]
    for (int i = tid; i < DL_FG_MONO_LD; i += 128) c[i] = cmono[(size_t)b * DL_FG_MONO_LD + i];
    for (int i = tid; i < n_params * DL_FG_MONO_LD; i += 128) dc[i] = dmono[(size_t)b * n_params * DL_FG_MONO_LD + i];
    __syncthreads();
    const double* Ub = U + (size_t)b * (1 + n_xv) * DL_FG_NM * ldu;
    for (int j = tid; j < N_pad; j += 128) {
        const bool live = j < n_live;
        double um[DL_FG_NM];
#pragma unroll
        for (int m = 0; m < DL_FG_NM; ++m) um[m] = Ub[(size_t)m * ldu + j];
        double acc = brow ? brow[j] : __builtin_nan("");
#pragma unroll
        for (int m = 0; m < DL_FG_NM; ++m) acc = fma(c[m], um[m], acc);
        resid[(size_t)b * ldr + j] = live ? acc : 0.;
        for (int p = 0; p < n_params; ++p) {
            double d = 0.;
#pragma unroll
            for (int m = 0; m < DL_FG_NM; ++m) {
                const double g = dc[p * DL_FG_MONO_LD + m];
                if (g != 0.) d = fma(g, um[m], d);
            }
            for (int r = 0; r < n_xv; ++r) {
                if (cols.col[r] != p) continue;
                const double* Ur = Ub + (size_t)(1 + r) * DL_FG_NM * ldu + j;
                double t = 0.;
#pragma unroll
                for (int m = 0; m < DL_FG_NM; ++m) t = fma(c[m], Ur[(size_t)m * ldu], t);
                d += t;
            }
            rows[((size_t)b * n_params + p) * ld + j] = live ? d : 0.;
        }
    }
}
#endif
