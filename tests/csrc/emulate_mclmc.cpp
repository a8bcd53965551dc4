// emulate_mclmc.cpp -- TEST INFRASTRUCTURE: runs the microcanonical Langevin stage of desilike_amd/csrc/dl_mclmc.h on the CPU (one thread holds every component of
// a chain, the chains one after the other), so that the `not gpu` suite checks the device arithmetic against the NumPy statement (desilike_amd/mclmc.py _HostMCLMC)
// and the momentum update against the differential equation it solves.  It is NOT a fallback: nothing in desilike_amd/ links or loads it.
#include <string.h>

#include "../../desilike_amd/csrc/dl_mclmc.h"

extern "C" {

// B(h) on one chain with A = diag(sigma): u [P] updated in place, g [P] the gradient of the log-posterior; returns dK through *dk
int emu_mclmc_bstep(int32_t P, double* u, const double* g, const double* sigma, double h, double* dk) {
    if (P < 2 || P > DL_MCLMC_MAX_P) return 1;
    DlMclmcArgs a;
    memset(&a, 0, sizeof(a));
    a.P = P; a.C = 1; a.fac = sigma;
    const DlNutsSerial l{P};
    DlNutsVec<DlNutsSerial> uu, gg;
    dl_nuts_load(l, uu, u);
    dl_nuts_load(l, gg, g);
    *dk = dl_mclmc_bstep(l, a, uu, gg, h);
    dl_nuts_store(l, uu, u);
    return 0;
}

// one launch of dl_mclmc_stage_kernel, every pointer a host array laid out as the device's; hyper = {L, offset, desired_energy_var, trust_in_estimate, gamma}
int emu_mclmc_kernel(double* vec, double* dsc, int32_t* isc, long long* iter, const int32_t* chain_ids, const double* fac, const double* fact, const double* lp_new,
                     const double* g_new, double* out_coords, double* out_logp, double* out_info, int32_t* out_count, int32_t C, int32_t P, int32_t dense, int32_t quota,
                     int32_t thin_by, int32_t integrator, int32_t adapt, int32_t moments, const double* hyper, uint64_t seed, int32_t stage, int32_t open_next) {
    if (P < 2 || P > DL_MCLMC_MAX_P) return 1;
    DlMclmcArgs a;
    memset(&a, 0, sizeof(a));
    if (!dl_mclmc_integrator(integrator, &a.nstage, a.cb, a.ca)) return 2;
    a.vec = vec; a.dsc = dsc; a.isc = isc; a.iter = iter; a.chain_ids = chain_ids; a.fac = fac; a.fact = fact; a.lp_new = lp_new; a.g_new = g_new;
    a.out_coords = out_coords; a.out_logp = out_logp; a.out_info = out_info; a.out_count = out_count;
    a.C = C; a.P = P; a.dense = dense; a.cap = quota; a.quota = quota; a.thin_by = thin_by; a.adapt = adapt; a.moments = moments;
    a.L = hyper[0]; a.offset = hyper[1]; a.energy_var = hyper[2]; a.trust = hyper[3]; a.gamma = hyper[4];
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    const DlNutsSerial l{P};
    for (int c = 0; c < C; ++c) dl_mclmc_chain_stage(l, a, c, stage, open_next);
    return 0;
}

// unit momentum of a state set without momenta: z / |z| of the DL_MCLMC_STREAM_INIT draw at the chain's counter
int emu_mclmc_initial_momentum(int32_t P, long long it, int32_t chain, uint64_t seed, double* u) {
    if (P < 2 || P > DL_MCLMC_MAX_P) return 1;
    const DlNutsSerial l{P};
    DlNutsVec<DlNutsSerial> z;
    for (int j = 0; j < DlNutsSerial::W; ++j) z.x[j] = j < P ? dl_mclmc_gauss(it, (uint32_t)chain, j, DL_MCLMC_STREAM_INIT, (uint32_t)seed, (uint32_t)(seed >> 32)) : 0.;
    dl_mclmc_normalise(l, z);
    dl_nuts_store(l, z, u);
    return 0;
}

}
