// emulate_emu_jac.cpp -- TEST INFRASTRUCTURE: the per-point arithmetic of the emulated analytic Jacobian (desilike_amd/csrc/dl_emu_jac.h: the forward mode of the
// monomials, the MLP / Taylor engines with their tangents) built for the host, so that the `not gpu` suite checks it against torch autograd (tests/test_emu_jac.py).
// It is NOT a fallback: nothing in desilike_amd/ links or loads it.  With -DEMU_EJ_MAIN it is a stand-alone program (its own main) that runs a few cases of every
// function: the form built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../desilike_amd/csrc/dl_emu_jac.h"

static void emu_ej_obs(DlObsDev& o, int mono_mode, double nd, double snd, double fsat, double sigv) {
    std::memset(&o, 0, sizeof(o));
    o.mono_mode = mono_mode; o.nd = nd; o.snd = snd; o.fsat = fsat; o.sigv = sigv; o.n_mono = DL_N_MONO;
    for (int c = 0; c < DL_N_VPARS; ++c) { o.vp_in[c].col = c; o.vp_slot[c] = -1; }
}

template <int NT>
static int emu_ej_run_engine(DlObsDev& o, int ie, const double* x, double* value, double* tangent) {
    const DlEjCols cols = dl_ej_cols(o);
    const int ldb = dl_ej_ldb(o);
    std::vector<double> bufa((size_t)(1 + NT) * ldb, 0.), bufb((size_t)(1 + NT) * ldb, 0.);
    const double* out = dl_ej_engine<NT>(0, 1, o, ie, cols, x, bufa.data(), bufb.data(), ldb);
    const DlObsDev::Engine& e = o.eng[ie];
    const int nout = ie != 0 ? 1 : e.type == 0 ? e.widths[e.n_layers] : e.n_terms;
    for (int u = 0; u < nout; ++u) {
        value[u] = out[u];
        for (int r = 0; r < cols.n_xv; ++r) tangent[(size_t)r * nout + u] = out[(size_t)(1 + r) * ldb + u];
    }
    return 0;
}

static int emu_ej_dispatch(DlObsDev& o, int ie, int nt, const double* x, double* value, double* tangent) {
    if (dl_ej_cols(o).n_xv > nt) return 2;
    if (nt == 4) return emu_ej_run_engine<4>(o, ie, x, value, tangent);
    if (nt == 8) return emu_ej_run_engine<8>(o, ie, x, value, tangent);
    if (nt == 16) return emu_ej_run_engine<16>(o, ie, x, value, tangent);
    return 2;
}

extern "C" {

// J [13][19] = d mono / d (v [11], sigma8, fsigma8)
int emu_ej_mono_jvp(int mono_mode, double nd, double snd, double fsat, double sigv, const double* v, double sigma8, double fsigma8, double* J) {
    DlObsDev o;
    emu_ej_obs(o, mono_mode, nd, snd, fsat, sigv);
    for (int k = 0; k < DL_EJ_NIN; ++k) dl_ej_mono_jvp_row(o, v, sigma8, fsigma8, k, J + (size_t)k * DL_N_MONO);
    return 0;
}

// MLP engine (table != 0: every layer activated, the hidden units are the outputs; else a scalar engine: last layer linear, y = v yscale + ylo) at x [n_x]:
// value [nout], tangent [n_xv][nout] with respect to the inputs with varied[i] != 0; nt: the instantiation (4, 8, 16)
int emu_ej_mlp(int n_x, int n_layers, const int32_t* widths, int act, int table, const double* xlo, const double* xinv, const double* weights, double ylo, double yscale,
               const int32_t* varied, int nt, const double* x, double* value, double* tangent) {
    DlObsDev o;
    std::memset(&o, 0, sizeof(o));
    o.n_x = n_x;
    for (int i = 0; i < n_x; ++i) o.x_in[i].col = varied[i] ? i : -1;
    for (int ie = 0; ie < 3; ++ie) o.eng[ie].type = -1;
    const int ie = table ? 0 : 1;
    DlObsDev::Engine& e = o.eng[ie];
    e.type = 0; e.n_layers = n_layers; e.act = act; e.ylo = ylo; e.yscale = yscale; e.xlo = xlo; e.xinv = xinv; e.weights = weights;
    for (int l = 0; l <= n_layers; ++l) e.widths[l] = widths[l];
    return emu_ej_dispatch(o, ie, nt, x, value, tangent);
}

// Taylor engine (coef == NULL: the table engine, the n_terms monomials are the outputs; else a scalar engine) at x [n_x]
int emu_ej_taylor(int n_x, int n_terms, const double* center, const double* powers, const double* coef, const int32_t* varied, int nt, const double* x, double* value,
                  double* tangent) {
    DlObsDev o;
    std::memset(&o, 0, sizeof(o));
    o.n_x = n_x;
    for (int i = 0; i < n_x; ++i) o.x_in[i].col = varied[i] ? i : -1;
    for (int ie = 0; ie < 3; ++ie) o.eng[ie].type = -1;
    const int ie = coef ? 1 : 0;
    DlObsDev::Engine& e = o.eng[ie];
    e.type = 1; e.n_terms = n_terms; e.center = center; e.powers = powers; e.coef = coef;
    return emu_ej_dispatch(o, ie, nt, x, value, tangent);
}

}

#ifdef EMU_EJ_MAIN
// a few cases of every function, the results compared with central differences of the values (1e-6: the differences' own error at h = 1e-5)
static double emu_ej_check(double a, double b, double scale) { const double d = a - b; return (d < 0 ? -d : d) / scale; }

int main() {
    double worst = 0.;
    const double h = 1e-5;
    for (int mode = 1; mode <= 4; ++mode) {
        double v[11] = {1.1, 0.7, -0.4, 0.3, 1.5, -2., 0.8, 0.2, 0.6, -0.3, 0.9}, s8 = 0.81, fs8 = 0.46, J[13 * 19];
        emu_ej_mono_jvp(mode, 3e-4, 0.8, 0.1, 5., v, s8, fs8, J);
        for (int k = 0; k < 13; ++k) {
            double in[13], mp[6 * 19], mm[6 * 19];
            int32_t slots[11];
            for (int c = 0; c < 11; ++c) { in[c] = v[c]; slots[c] = -1; }
            in[11] = s8; in[12] = fs8;
            DlObsDev o;
            emu_ej_obs(o, mode, 3e-4, 0.8, 0.1, 5.);
            in[k] += h; dl_velocileptors_monomials(o, in, in[11], in[12], mp);
            in[k] -= 2 * h; dl_velocileptors_monomials(o, in, in[11], in[12], mm);
            for (int m = 0; m < 19; ++m) { const double e = emu_ej_check(J[k * 19 + m], (mp[m] - mm[m]) / (2 * h), 1e4); worst = e > worst ? e : worst; }
        }
    }
    for (int act = 0; act < 3; ++act)
        for (int width : {5, 64, 65}) {
            const int n_x = 3;
            int32_t widths[4] = {n_x, width, width, 1}, varied[3] = {1, 0, 1};
            std::vector<double> w;
            unsigned state = 12345u + act * 7 + width;
            auto rnd = [&]() { state = state * 1664525u + 1013904223u; return ((state >> 8) & 0xffff) / 65536. - 0.5; };
            for (int l = 0; l < 3; ++l) for (int i = 0; i < widths[l] * widths[l + 1] + widths[l + 1]; ++i) w.push_back(rnd() * 1.5 / (widths[l] < 8 ? 2. : 8.));
            double xlo[3] = {0.9, 0.9, -0.1}, xinv[3] = {5., 5., 5.}, x[3] = {1.013, 0.97, 0.021};
            for (int table = 0; table < 2; ++table) {
                const int nl = table ? 2 : 3, nout = table ? width : 1;
                std::vector<double> val(nout), tan(2 * nout), vp(nout), vm(nout), dummy(2 * nout);
                for (int nt : {4, 8, 16}) {
                    if (emu_ej_mlp(n_x, nl, widths, act, table, xlo, xinv, w.data(), 0.4, 0.2, varied, nt, x, val.data(), tan.data())) return 1;
                    for (int r = 0; r < 2; ++r) {
                        const int q = r == 0 ? 0 : 2;
                        double xs[3] = {x[0], x[1], x[2]};
                        xs[q] += h; emu_ej_mlp(n_x, nl, widths, act, table, xlo, xinv, w.data(), 0.4, 0.2, varied, nt, xs, vp.data(), dummy.data());
                        xs[q] -= 2 * h; emu_ej_mlp(n_x, nl, widths, act, table, xlo, xinv, w.data(), 0.4, 0.2, varied, nt, xs, vm.data(), dummy.data());
                        for (int u = 0; u < nout; ++u) { const double e = emu_ej_check(tan[r * nout + u], (vp[u] - vm[u]) / (2 * h), 10.); worst = e > worst ? e : worst; }
                    }
                }
            }
        }
    {
        const double powers[7 * 3] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 1, 0, 2, 0, 2, 0, 0}, center[3] = {1., 1., 0.}, coef[7] = {0.8, 0.1, -0.2, 0.16, 0.3, 0.05, 0.08};
        int32_t varied[3] = {1, 1, 1};
        double x[3] = {1.02, 0.97, 0.03};
        for (int scalar = 0; scalar < 2; ++scalar) {
            const int nout = scalar ? 1 : 7;
            double val[7], tan[21], vp[7], vm[7], dummy[21];
            if (emu_ej_taylor(3, 7, center, powers, scalar ? coef : nullptr, varied, 4, x, val, tan)) return 1;
            for (int q = 0; q < 3; ++q) {
                double xs[3] = {x[0], x[1], x[2]};
                xs[q] += h; emu_ej_taylor(3, 7, center, powers, scalar ? coef : nullptr, varied, 4, xs, vp, dummy);
                xs[q] -= 2 * h; emu_ej_taylor(3, 7, center, powers, scalar ? coef : nullptr, varied, 4, xs, vm, dummy);
                for (int u = 0; u < nout; ++u) { const double e = emu_ej_check(tan[q * nout + u], (vp[u] - vm[u]) / (2 * h), 1.); worst = e > worst ? e : worst; }
            }
        }
    }
    std::printf("emulate_emu_jac: worst difference to central differences %.3e\n", worst);
    return worst <= 1e-6 ? 0 : 1;
}
#endif
