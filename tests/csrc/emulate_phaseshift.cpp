// emulate_phaseshift.cpp -- TEST INFRASTRUCTURE: the phases of the BAO kernel's phase-shift instantiations (dl_bao_kernel<MODEL, true>, desilike_amd/csrc/dl_kernels.hip)
// run on the CPU from the same phase functions (desilike_amd/csrc/dl_fullshape.h: dl_bao_phaseA, dl_bao_ps_*, dl_bao_phaseB_m<MODEL, true>) and the same host-side
// constant folding (dl_host.hpp), one workgroup emulated by looping tid over [0, nthr) for each barrier-separated phase -- with nthr = 64, 128, 192, 256: the workgroup
// sizes dl_bao_threads gives (64 / 128 by the batch; below, the wavenumbers rounded up to whole waves: 192 for the 168 of the P_ell fixtures, 256 for 300).
// Built twice by tests/test_bao_phaseshift.py: as a shared object loaded by ctypes, and (-DPS_STANDALONE) as a program of its own under the address /
// undefined-behaviour sanitizers.  It is NOT a fallback: nothing in desilike_amd/ links or loads it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../desilike_amd/csrc/dl_host.hpp"

static std::string g_err;

// one point of one observable: power row [n_in + n_pass]
static void ps_run_point(const DlObsDev& o, const double* th, int nthr, double* prow) {
    std::vector<double> lds(dl_bao_ps_shared_doubles(o.n_t, o.n_in), 0.);
    const DlPsShared ps = dl_bao_ps_carve(lds.data(), o.n_t, o.n_in);
    std::vector<double> end(nthr);
    for (int tid = 0; tid < nthr; ++tid) { dl_bao_phaseA(tid, nthr, o, th, lds.data()); dl_bao_ps_knots(tid, nthr, o, th, ps); }
    for (int tid = 0; tid < nthr; ++tid) dl_bao_ps_fir(tid, nthr, o, ps);
    for (int tid = 0; tid < nthr; ++tid) end[tid] = dl_bao_ps_end_moment(tid, o, ps);
    for (int tid = 0; tid < nthr; ++tid) dl_bao_ps_end_store(tid, o, ps, end[tid]);
    for (int tid = 0; tid < nthr; ++tid) dl_bao_ps_end_relations(tid, o, ps);
    const int model = o.bao_mode >> 4;
    for (int tid = 0; tid < nthr; ++tid) {
        if (model == 0) dl_bao_phaseB_m<0, true>(tid, nthr, o, lds.data());
        else if (model & 32) dl_bao_phaseB_m<3, true>(tid, nthr, o, lds.data());
        else if (model & 16) dl_bao_phaseB_m<2, true>(tid, nthr, o, lds.data());
        else dl_bao_phaseB_m<1, true>(tid, nthr, o, lds.data());
    }
    for (int tid = 0; tid < nthr; ++tid) dl_store_with_pass(tid, nthr, o, th, lds.data() + DL_BAO_PT, prow);
}

// power [B, n_in] of observable iobs with nthr emulated threads; 1: the configuration is refused (ps_last_error), 2: not a phase-shift observable
static int ps_eval(const dl_config& cfg, const double* theta, int64_t B, int iobs, int nthr, double* power) {
    const int P = cfg.i("n_params", -1);
    DlArena arena;
    DlObsHost oh;
    if (!dl_build_obs(cfg, iobs, P, oh, arena, g_err)) return 1;
    if (oh.dev.theory != 2 || oh.dev.templ != 4) { g_err = "not a phase-shift BAO observable"; return 2; }
    oh.rebase(arena.data.data());
    oh.dev.col_offset = 0;
    std::vector<double> row(oh.n_cols());
    for (int64_t b = 0; b < B; ++b) {
        ps_run_point(oh.dev, theta + b * P, nthr, row.data());
        std::copy(row.begin(), row.begin() + oh.dev.n_in, power + b * oh.dev.n_in);
    }
    return 0;
}

extern "C" {

dl_config* ps_config_new(void) { return new dl_config(); }
void ps_config_free(dl_config* cfg) { delete cfg; }
int ps_config_set_f64(dl_config* cfg, const char* key, const double* data, int64_t n) { cfg->f64[key] = std::vector<double>(data, data + n); return 0; }
int ps_config_set_i32(dl_config* cfg, const char* key, const int32_t* data, int64_t n) { cfg->i32[key] = std::vector<int32_t>(data, data + n); return 0; }
const char* ps_last_error(void) { return g_err.c_str(); }
int ps_n_in(const dl_config* cfg, int iobs) { return (int)(cfg->I("obs" + std::to_string(iobs) + ".ells_in").size() * cfg->F("obs" + std::to_string(iobs) + ".kin").size()); }
int ps_eval_theory(const dl_config* cfg, const double* theta, int64_t B, int iobs, int nthr, double* power) { return ps_eval(*cfg, theta, B, iobs, nthr, power); }

}

#ifdef PS_STANDALONE
// Flat file: records (int32 kind: 0 f64, 1 i32, 2 end of the keys | int32 length of the key | key | int64 count | values), then int64 B, int64 P, theta [B, P].
// Runs every observable with 64, 128, 192 and 256 emulated threads: they must agree (the partition of the knots among the threads does not change a single
// operation) and be finite.  Exit status 0: fine; 1: unreadable file / refused configuration; 2: the workgroup sizes disagree or a value is not finite.
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
        const size_t n = (size_t)B * ps_n_in(&cfg, iobs);
        std::vector<double> first(n), other(n);
        const int sizes[4] = {64, 128, 192, 256};
        for (int is = 0; is < 4; ++is) {
            std::vector<double>& out = is == 0 ? first : other;
            if (ps_eval(cfg, theta.data(), B, iobs, sizes[is], out.data())) { std::fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
            for (size_t i = 0; i < n; ++i) {
                if (!std::isfinite(out[i])) { std::fprintf(stderr, "obs %d, %d threads: entry %zu is not finite\n", iobs, sizes[is], i); return 2; }
                if (is > 0 && out[i] != first[i]) { std::fprintf(stderr, "obs %d: %d and 64 threads disagree at entry %zu\n", iobs, sizes[is], i); return 2; }
            }
        }
        std::printf("obs %d: %lld points x %d values, 64 / 128 / 192 / 256 threads agree\n", iobs, (long long)B, ps_n_in(&cfg, iobs));
    }
    return 0;
}
#endif
