// emulate_jac.cpp -- TEST INFRASTRUCTURE: the Jacobian workgroup (dl_fullshape_jac_kernel, desilike_amd/csrc/dl_kernels.hip) run on the CPU through the device's own phase
// functions (desilike_amd/csrc/dl_fullshape_jac.h), one barrier-separated phase after the other, so that the `not gpu` suite checks the derivative rows against the
// oracle's stencil and against the gradient phase (tests/test_jacobian.py), also under AddressSanitizer / UndefinedBehaviorSanitizer.
// It is NOT a fallback: nothing in desilike_amd/ links or loads it.
#include "emulate.cpp"   // the forward / gradient emulation (run_point, run_point_grad) and the configuration store
#include "../../desilike_amd/csrc/dl_fullshape_jac.h"

// rows [P][ldj] of one point: this observable's column block at J (already offset by col_offset)
static bool run_point_jac(const DlObsDev& o, const double* th, int P, double* J, int64_t ldj) {
    if (!dl_fs_grad_applicable(o)) return false;
    std::vector<double> lds(dl_fs_jac_shared_doubles(o, P), 0.);   // (exactly the device's size: the sanitizer sees an access beyond it)
    const bool toep = o.toeplitz && !o.fixed_spline;
    DlFsShared s = dl_fs_shared_carve(lds.data(), o.n_t, o.n_in, dl_fs_n_dd0(o), toep);
    double* gw = s.pt + DL_PT_SIZE_FAST;
    double* C = gw + (size_t)DL_MAX_MU * DL_GW;
    const int nthr = DL_FS_THREADS, KT = DL_FS_KT;
    std::vector<DlMuCarry> carry(nthr);
    auto mu_lane = [&](int tid) { return tid >= KT && tid - KT < o.n_mu; };
    for (int tid = 0; tid < nthr; ++tid) {
        if (tid >= KT) {
            dl_fs_mu_partA(o, th, mu_lane(tid) ? tid - KT : 0, carry[tid]);
            dl_fs_mu_partB(carry[tid]);
            if (mu_lane(tid)) { dl_fs_mu_partC(o, s, tid - KT, carry[tid], false); dl_fs_grad_weights(o, tid - KT, carry[tid], gw); }
            if (tid == nthr - 1) { dl_fs_scalars(o, th, s, carry[tid], false); dl_fs_grad_weights_pad(o, gw); }
            dl_fs_jac_chain_matrix(tid - KT, o, th, P, C);
        } else dl_fs_knots(tid, KT, o, th, s);
    }
    auto build = [&]() {
        for (int tid = 0; tid < KT; ++tid) dl_fs_phase2_fir(tid, KT, o, s);
        for (int tid = 0; tid < KT; ++tid) {
            double dlt_pref[DL_TOEP_PREF];
            for (int it = 0; it < DL_TOEP_PREF; ++it) dlt_pref[it] = (tid + it * KT < o.n_t - 1) ? o.dlt[tid + it * KT] : 0.;
            dl_fs_phase2d_toep(tid, KT, o, s, dlt_pref);
        }
    };
    auto rows = [&](int pass) {
        for (int tid = 0; tid < nthr; ++tid) {
            if (o.n_ell <= 3) dl_fs_jac_phase3<3, 2>(tid, nthr, o, s, gw, C, P, pass, J, ldj);
            else dl_fs_jac_phase3<DL_MAX_ELL, 1>(tid, nthr, o, s, gw, C, P, pass, J, ldj);
        }
    };
    if (toep) build();
    rows(0);
    if (toep && o.templ == 1) {
        for (int which = 0; which < 2; ++which) {
            if (which == 0 ? o.dm.col < 0 : o.dn.col < 0) continue;
            for (int tid = 0; tid < KT; ++tid) dl_fs_grad_knots(tid, KT, o, th, s, which);
            build();
            rows(1 + which);
        }
    }
    return true;
}

static bool emu_jac_build(const dl_config* cfg, DlArena& arena, std::vector<DlObsHost>& obs, std::vector<int>& col0, int& K) {
    const int P = cfg->i("n_params", -1), nobs = cfg->i("n_obs", -1);
    obs.resize(nobs);
    K = 0;
    for (int i = 0; i < nobs; ++i) {
        if (!dl_build_obs(*cfg, i, P, obs[i], arena, g_err)) return false;
        col0.push_back(K);
        K += obs[i].n_cols();
    }
    for (int i = 0; i < nobs; ++i) { obs[i].rebase(arena.data.data()); obs[i].dev.col_offset = col0[i]; }
    return true;
}

extern "C" {

// columns of the concatenated theory vector (every observable's [n_ell][n_kin] block); -1 on error
int64_t emu_jac_ncols(const dl_config* cfg) {
    DlArena arena; std::vector<DlObsHost> obs; std::vector<int> col0; int K = 0;
    return emu_jac_build(cfg, arena, obs, col0, K) ? K : -1;
}

// jac [B, P, k_pad]: d(theory vector) / d theta_p; the rows are NOT cleared first (the phase functions must write every column up to k_pad).  Returns 2 outside the scope.
int emu_eval_jac(const dl_config* cfg, const double* theta, int64_t B, int64_t k_pad, double* jac) {
    const int P = cfg->i("n_params", -1);
    DlArena arena; std::vector<DlObsHost> obs; std::vector<int> col0; int K = 0;
    if (!emu_jac_build(cfg, arena, obs, col0, K)) return 1;
    if (k_pad < K) { g_err = "emu_eval_jac: k_pad below the number of columns"; return 1; }
    for (int64_t b = 0; b < B; ++b) {
        double* Jpoint = jac + (size_t)b * P * k_pad;
        for (size_t i = 0; i < obs.size(); ++i) {
            if (!run_point_jac(obs[i].dev, theta + b * P, P, Jpoint + col0[i], k_pad)) return 2;
            if (i + 1 == obs.size())
                for (int tid = 0; tid < DL_FS_THREADS; ++tid) dl_fs_jac_zero_tail(tid, DL_FS_THREADS, P, K, (int)k_pad, Jpoint, k_pad);
        }
    }
    return 0;
}

// the gradient phase (reverse mode) on a GIVEN Y [B, K]: grad [B, P] = chain rule of the per-observable contractions (what J . Y must equal)
int emu_eval_grad_given_y(const dl_config* cfg, const double* theta, int64_t B, const double* Y, double* grad) {
    const int P = cfg->i("n_params", -1);
    DlArena arena; std::vector<DlObsHost> obs; std::vector<int> col0; int K = 0;
    if (!emu_jac_build(cfg, arena, obs, col0, K)) return 1;
    for (int64_t b = 0; b < B; ++b) {
        double* g = grad + b * P;
        std::fill(g, g + P, 0.);
        for (size_t i = 0; i < obs.size(); ++i) {
            double gphys[DL_NPHYS];
            if (!run_point_grad(obs[i].dev, theta + b * P, Y + b * K + col0[i], gphys)) return 2;
            dl_fs_grad_chain(obs[i].dev, theta + b * P, gphys, g);
        }
    }
    return 0;
}

}  // extern "C"
