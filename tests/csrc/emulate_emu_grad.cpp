// emulate_emu_grad.cpp -- TEST INFRASTRUCTURE: the per-point arithmetic of the emulated analytic gradient (desilike_amd/csrc/dl_emu_grad.h: the monomial adjoint and the
// marginalisation adjoint) built for the host, so that the `not gpu` suite checks it against torch autograd (tests/test_emu_grad.py).
// It is NOT a fallback: nothing in desilike_amd/ links or loads it.
#include <cstring>
#include "../../desilike_amd/csrc/dl_emu_grad.h"

static void emu_eg_obs(DlObsDev& o, int mono_mode, double nd, double snd, double fsat, double sigv, const int32_t* vp_slot, int n_var) {
    std::memset(&o, 0, sizeof(o));
    o.mono_mode = mono_mode; o.nd = nd; o.snd = snd; o.fsat = fsat; o.sigv = sigv; o.n_var = n_var; o.n_mono = DL_N_MONO;
    for (int c = 0; c < DL_N_VPARS; ++c) { o.vp_in[c].col = c; o.vp_slot[c] = vp_slot[c]; }
}

extern "C" {

// monomial rows [(1 + n_var)][19] at the inputs v [11] (dl_velocileptors_monomials)
int emu_eg_mono(int mono_mode, double nd, double snd, double fsat, double sigv, const int32_t* vp_slot, int n_var, const double* v, double sigma8, double fsigma8, double* mono) {
    DlObsDev o;
    emu_eg_obs(o, mono_mode, nd, snd, fsat, sigv, vp_slot, n_var);
    dl_velocileptors_monomials(o, v, sigma8, fsigma8, mono);
    return 0;
}

// g [13] = Q . d mono / d (v [11], sigma8, fsigma8)
int emu_eg_mono_vjp(int mono_mode, double nd, double snd, double fsat, double sigv, const int32_t* vp_slot, int n_var, const double* v, double sigma8, double fsigma8,
                    const double* Q, double* g) {
    DlObsDev o;
    emu_eg_obs(o, mono_mode, nd, snd, fsat, sigv, vp_slot, n_var);
    dl_eg_mono_vjp(o, v, sigma8, fsigma8, Q, g);
    return 0;
}

// G [(1 + ns)][(1 + ns)] -> dx [ns], Wc [ns][ns]; returns 1 if a pivot is not positive
int emu_eg_marg_adjoint(int ns, const double* G, const double* x0, const double* loc, const double* prec, const int32_t* is_marg, double* dx, double* Wc) {
    bool ok = false;
    switch (ns) {
#define EMU_EG_CASE(n) case n: ok = dl_eg_marg_adjoint<n>(G, 1 + n, x0, loc, prec, is_marg, dx, Wc); break;
        EMU_EG_CASE(1) EMU_EG_CASE(2) EMU_EG_CASE(3) EMU_EG_CASE(4) EMU_EG_CASE(5) EMU_EG_CASE(6) EMU_EG_CASE(7) EMU_EG_CASE(8)
        EMU_EG_CASE(9) EMU_EG_CASE(10) EMU_EG_CASE(11) EMU_EG_CASE(12) EMU_EG_CASE(13) EMU_EG_CASE(14) EMU_EG_CASE(15) EMU_EG_CASE(16)
#undef EMU_EG_CASE
        default: return 2;
    }
    return ok ? 0 : 1;
}

}
