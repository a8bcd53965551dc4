// emulate_wigglesplit.cpp -- TEST INFRASTRUCTURE: the phases of the wiggle-split template kernel (dl_ws_template_kernel, desilike_amd/csrc/dl_kernels.hip) run on the
// CPU from the same phase functions (desilike_amd/csrc/dl_wigglesplit.h: dl_ws_point_phase, with the shared spline phases dl_ps_* of dl_fullshape.h) and the same host-side
// tables (dl_host.hpp: dl_ws_build), one workgroup emulated by looping tid over [0, nthr) for each barrier-separated phase; then the theory kernel's general form on the
// scratch row the template left (dl_fs_phase01 ... dl_fs_phase4, as tests/csrc/emulate.cpp runs them).
// Built twice by tests/wigglesplit_utils.py: as a shared object loaded by ctypes, and (-DWS_STANDALONE) as a program of its own under the address / undefined-behaviour
// sanitizers.  It is NOT a fallback: nothing in desilike_amd/ links or loads it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../desilike_amd/csrc/dl_host.hpp"

static std::string g_err;

// the template of one point at the knots: row [n_t]; the LDS image is exactly as large as the kernel's: the sanitizers see any index past it
static void ws_run_template(const DlObsDev& o, const double* th, int nthr, double* row) {
    const DlWsTab t = dl_ws_open(dl_ws_tab(o));
    std::vector<double> lds(dl_ws_shared_doubles(t.n_i, nthr), 0.);
    const DlWsShared s = dl_ws_carve(lds.data(), t.n_i, nthr);
    const double qbao = dl_get(dl_ws_qbao(o), th), dm = dl_get(o.dm, th);
    std::vector<double> carry(nthr, 0.);
    for (int phase = 0; phase < DL_WS_PHASES; ++phase)
        for (int tid = 0; tid < nthr; ++tid) dl_ws_point_phase(phase, tid, nthr, qbao, dm, t, s, carry[tid], row);
}

// the theory kernel's general form (dl_fullshape_kernel<false, 5, true>) for one point, its knot phase reading the scratch row
static void ws_run_theory(const DlObsDev& o, const double* th, double* prow) {
    const int nthr = DL_FS_THREADS;
    std::vector<double> lds(dl_fs_shared_doubles_obs(o, false), 0.);
    const bool toep = o.toeplitz && !o.fixed_spline;
    const DlFsShared s = dl_fs_shared_carve(lds.data(), o.n_t, o.n_in, dl_fs_n_dd0(o), toep);
    std::vector<double> lk(DL_P3_PREF * nthr, 0.);
    for (int tid = 0; tid < nthr; ++tid) dl_fs_phase01<true>(tid, nthr, o, th, s, 0);
    if (toep) {
        for (int tid = 0; tid < nthr; ++tid) dl_fs_phase2_fir(tid, nthr, o, s);
        for (int tid = 0; tid < nthr; ++tid) {
            double dlt_pref[DL_TOEP_PREF];
            for (int it = 0; it < DL_TOEP_PREF; ++it) dlt_pref[it] = (tid + it * nthr < o.n_t - 1) ? o.dlt[tid + it * nthr] : 0.;
            dl_fs_phase2d_toep(tid, nthr, o, s, dlt_pref);
        }
    } else {
        for (int tid = 0; tid < nthr; ++tid) dl_fs_phase2a(tid, nthr, o, s);
        for (int tid = 0; tid < nthr; ++tid) dl_fs_phase2b_dot(tid, nthr, o, s);
        for (int tid = 0; tid < nthr; ++tid) dl_fs_phase2b(tid, nthr, o, s);
        for (int tid = 0; tid < nthr; ++tid) dl_fs_phase2c_dot(tid, nthr, o, s);
        for (int tid = 0; tid < nthr; ++tid) dl_fs_phase2c(tid, nthr, o, s);
        for (int tid = 0; tid < nthr; ++tid) dl_fs_phase2d(tid, nthr, o, s);
    }
    for (int tid = 0; tid < nthr; ++tid) {
        double lk_pref[DL_P3_PREF];
        for (int it = 0; it < DL_P3_PREF; ++it) lk_pref[it] = (tid + it * nthr < o.n_kin) ? o.lkin[tid + it * nthr] : 0.;
        dl_fs_phase3<false, 5, true>(tid, nthr, o, s, nullptr, lk_pref);
    }
    for (int tid = 0; tid < nthr; ++tid) dl_fs_phase4(tid, nthr, o, s, th, prow, o.n_in);
}

// template [B, n_t] and power [B, n_in] of observable iobs with nthr emulated threads in the template kernel; 1: the configuration is refused (ws_last_error)
static int ws_eval(const dl_config& cfg, const double* theta, int64_t B, int iobs, int nthr, double* templ, double* power) {
    const int P = cfg.i("n_params", -1);
    if (nthr < 2 * DL_FIR_PAD || nthr % DL_WS_PARTS != 0) { g_err = "the template kernel needs at least 64 threads, a multiple of 16"; return 1; }
    DlArena arena;
    DlObsHost oh;
    if (!dl_build_obs(cfg, iobs, P, oh, arena, g_err)) return 1;
    if (oh.dev.templ != 5) { g_err = "not a wiggle-split observable"; return 2; }
    oh.rebase(arena.data.data());
    oh.dev.col_offset = 0;
    std::vector<double> scratch(oh.dev.n_t), row(oh.n_cols() + 8);
    oh.dev.coef_w = scratch.data(); oh.dev.n_band = oh.dev.n_t;   // (dl_ws_scratch, dl_ws_scratch_ld: one point at a time)
    for (int64_t b = 0; b < B; ++b) {
        ws_run_template(oh.dev, theta + b * P, nthr, scratch.data());
        if (templ) std::copy(scratch.begin(), scratch.end(), templ + b * oh.dev.n_t);
        if (power) {
            ws_run_theory(oh.dev, theta + b * P, row.data());
            std::copy(row.begin(), row.begin() + oh.dev.n_in, power + b * oh.dev.n_in);
        }
    }
    return 0;
}

extern "C" {

dl_config* ws_config_new(void) { return new dl_config(); }
void ws_config_free(dl_config* cfg) { delete cfg; }
int ws_config_set_f64(dl_config* cfg, const char* key, const double* data, int64_t n) { cfg->f64[key] = std::vector<double>(data, data + n); return 0; }
int ws_config_set_i32(dl_config* cfg, const char* key, const int32_t* data, int64_t n) { cfg->i32[key] = std::vector<int32_t>(data, data + n); return 0; }
const char* ws_last_error(void) { return g_err.c_str(); }
int ws_n_t(const dl_config* cfg, int iobs) { return (int)cfg->F("obs" + std::to_string(iobs) + ".k_t").size(); }
int ws_n_in(const dl_config* cfg, int iobs) { return (int)(cfg->I("obs" + std::to_string(iobs) + ".ells_in").size() * cfg->F("obs" + std::to_string(iobs) + ".kin").size()); }
int ws_eval_point(const dl_config* cfg, const double* theta, int64_t B, int iobs, int nthr, double* templ, double* power) { return ws_eval(*cfg, theta, B, iobs, nthr, templ, power); }

}

#ifdef WS_STANDALONE
// Flat file: records (int32 kind: 0 f64, 1 i32, 2 end of the keys | int32 length of the key | key | int64 count | values), then int64 B, int64 P, theta [B, P].
// Runs the template of every observable with 256 (the kernel's) and 64 emulated threads.  Exit status 0: fine; 1: unreadable file / refused configuration; 2: a
// template value of a row with qbao inside (0.75, 1.25) is not finite or not positive.  Rows outside only have to index inside the tables: that is the sanitizers' call.
int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s spec-file\n", argv[0]); return 1; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    dl_config cfg;
    auto get = [&](void* dst, size_t size, size_t count) { return std::fread(dst, size, count, f) == count; };
    for (;;) {
        int32_t kind = 2, len = 0;
        int64_t count = 0;
        if (!get(&kind, sizeof(kind), 1)) { std::fclose(f); return 1; }
        if (kind == 2) break;
        if (!get(&len, sizeof(len), 1) || len < 0 || len > 256) { std::fclose(f); return 1; }
        std::string key((size_t)len, ' ');
        if (len && !get(&key[0], 1, (size_t)len)) { std::fclose(f); return 1; }
        if (!get(&count, sizeof(count), 1) || count < 0 || count > (int64_t)1 << 26) { std::fclose(f); return 1; }
        if (kind == 0) { std::vector<double> v((size_t)count); if (count && !get(v.data(), sizeof(double), (size_t)count)) { std::fclose(f); return 1; } cfg.f64[key] = v; }
        else { std::vector<int32_t> v((size_t)count); if (count && !get(v.data(), sizeof(int32_t), (size_t)count)) { std::fclose(f); return 1; } cfg.i32[key] = v; }
    }
    int64_t B = 0, P = 0;
    if (!get(&B, sizeof(B), 1) || !get(&P, sizeof(P), 1) || B < 1 || P < 1 || B * P > (int64_t)1 << 24 || P != cfg.i("n_params", -1)) { std::fclose(f); return 1; }
    std::vector<double> theta((size_t)(B * P));
    if (!get(theta.data(), sizeof(double), theta.size())) { std::fclose(f); return 1; }
    std::fclose(f);
    const int n_obs = cfg.i("n_obs", 1);
    for (int iobs = 0; iobs < n_obs; ++iobs) {
        if (cfg.i("obs" + std::to_string(iobs) + ".template", 0) != 5) continue;
        const auto& qin = cfg.F("obs" + std::to_string(iobs) + ".in.qbao");
        const int qcol = qin.size() >= 2 ? (int)std::lround(qin[0]) : -1;
        const int n_t = ws_n_t(&cfg, iobs), n_in = ws_n_in(&cfg, iobs);
        std::vector<double> templ((size_t)B * n_t), power((size_t)B * n_in);
        const int sizes[2] = {256, 64};
        for (int is = 0; is < 2; ++is) {
            if (ws_eval(cfg, theta.data(), B, iobs, sizes[is], templ.data(), is == 0 ? power.data() : nullptr)) { std::fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
            for (int64_t b = 0; b < B; ++b) {
                const double qbao = qcol >= 0 ? theta[(size_t)(b * P + qcol)] : 1.;
                if (!(qbao > 0.75 && qbao < 1.25)) continue;
                for (int j = 0; j < n_t; ++j)
                    if (!(templ[(size_t)b * n_t + j] > 0.) || !std::isfinite(templ[(size_t)b * n_t + j])) { std::fprintf(stderr, "obs %d, %d threads: row %lld knot %d is not a positive number\n", iobs, sizes[is], (long long)b, j); return 2; }
            }
        }
        std::printf("obs %d: %lld points x %d knots, 256 and 64 threads ran inside their tables\n", iobs, (long long)B, n_t);
    }
    return 0;
}
#endif
