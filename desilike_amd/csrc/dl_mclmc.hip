// dl_mclmc.hip -- device-resident microcanonical Langevin sampler (include/desilike_amd.h, dl_mclmc_*; the algorithm and the per-chain record: dl_mclmc.h).
//
// A step of every chain is one (isokinetic_leapfrog) or two (isokinetic_mclachlan) stages; a stage is two launches, nothing synchronises with the host:
//
//     gradient of the pending positions [C, P]  ->  dl_mclmc_stage_kernel (the B update with that gradient and the next drift -- or, closing the step: the energy
//                                                  change, the undo of a step that left the support, the partial refresh, the step-size controller, the moments,
//                                                  the record, and the opening B and drift of the next step)
//
// There is no accept / reject and no tree: every gradient row is used, every chain is at the same stage.  The gradient is dl_eval_logposterior_grad where the context
// is in its scope; otherwise central differences of dl_eval_logposterior, of which a value that is not finite undoes the step (dl_fd_gradient.hip: the route NUTS shares).
// One wavefront per chain, one lane per parameter component (P <= 64): |g|, e.u and the normalisations are wavefront reductions (xor butterflies: every lane holds
// the same sum), a state row is one coalesced load.  Every lane computes the same chain scalars and stores them (one address): no lane reads another lane's store.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/desilike_amd.h"
#include "dl_sampler_dev.h"   // DlWave, DlBlock, dl_fail, DL_HIP_CHECK, dl_dev_alloc / free
#include "dl_mclmc.h"

#define DL_MCLMC_WAVES 4    // chains per workgroup

struct dl_mclmc {
    dl_ctx* ctx = nullptr;
    int device = 0;
    int C = 0, P = 0, integrator = 1;
    bool have_fac = false, have_state = false, have_hyper = false, adapt = false, moments = false, dense = false;
    double offset = 0., L = 1., energy_var = 5e-4, trust = 1.5, gamma = 149. / 151.;
    uint64_t seed = 0;
    int64_t steps = 0;
    std::vector<int32_t> ids;
    // device
    double *vec = nullptr, *dsc = nullptr, *fac = nullptr, *fact = nullptr;
    DlFdGradient g;       // log-posterior and gradient of the pending positions
    int32_t *isc = nullptr, *chain_ids = nullptr;
    long long* iter = nullptr;
};

namespace {

__global__ __launch_bounds__(64 * DL_MCLMC_WAVES) void dl_mclmc_stage_kernel(DlMclmcArgs a, int stage, int open_next) {
    const int c = blockIdx.x * DL_MCLMC_WAVES + (int)(threadIdx.x >> 6);
    if (c >= a.C) return;     // (whole wavefronts)
    const DlWave l{a.P, (int)(threadIdx.x & 63)};
    dl_mclmc_chain_stage(l, a, c, stage, open_next);
}

DlMclmcArgs dl_mclmc_args(const dl_mclmc* m) {
    DlMclmcArgs a;
    std::memset(&a, 0, sizeof(a));
    dl_mclmc_integrator(m->integrator, &a.nstage, a.cb, a.ca);
    a.vec = m->vec; a.dsc = m->dsc; a.isc = m->isc; a.iter = m->iter; a.chain_ids = m->chain_ids; a.fac = m->fac; a.fact = m->fact;
    a.lp_new = m->g.lp; a.g_new = m->g.grad;
    a.C = m->C; a.P = m->P; a.dense = m->dense ? 1 : 0; a.adapt = m->adapt ? 1 : 0; a.moments = m->moments ? 1 : 0;
    a.L = m->L; a.offset = m->offset; a.energy_var = m->energy_var; a.trust = m->trust; a.gamma = m->gamma;
    a.k0 = (uint32_t)m->seed; a.k1 = (uint32_t)(m->seed >> 32);
    return a;
}

// every chain's entry of double field f <- value
int dl_mclmc_fill(dl_mclmc* m, int f, double value, hipStream_t stream) {
    std::vector<double> v((size_t)m->C, value);
    DL_HIP_CHECK(hipMemcpyAsync(m->dsc + (size_t)f * m->C, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));   // the host buffer is pageable
    return 0;
}

}  // namespace

extern "C" {

void dl_mclmc_destroy(dl_mclmc* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    dl_fd_gradient_destroy(&m->g);
    dl_dev_free({(void**)&m->vec, (void**)&m->dsc, (void**)&m->fac, (void**)&m->fact, (void**)&m->isc, (void**)&m->chain_ids, (void**)&m->iter});
    delete m;
}

int dl_mclmc_create(dl_mclmc** out, dl_ctx* ctx, int32_t nchains, const int32_t* chain_ids, int32_t integrator, uint64_t seed, double offset, int32_t gradient_mode,
                    const double* fd_delta, const double* fd_limits) {
    if (!out || !ctx) return dl_fail("dl_mclmc_create: null argument");
    *out = nullptr;
    const int P = (int)dl_info(ctx, "n_params");
    if (P < 2 || P > DL_MCLMC_MAX_P)
        return dl_fail("dl_mclmc_create: the sampler takes 2 .. 64 parameters (one parameter has no isokinetic dynamics: d - 1 = 0), the context has " + std::to_string(P));
    if (nchains < 1) return dl_fail("dl_mclmc_create: nchains must be >= 1");
    int32_t nstage;
    double cb[3], ca[2];
    if (!dl_mclmc_integrator(integrator, &nstage, cb, ca)) return dl_fail("dl_mclmc_create: integrator must be 0 (isokinetic_leapfrog) or 1 (isokinetic_mclachlan)");
    if (gradient_mode < 0 || gradient_mode > 2) return dl_fail("dl_mclmc_create: gradient_mode must be 0 (auto), 1 (analytic) or 2 (finite)");
    if (gradient_mode == 2 && (!fd_delta || !fd_limits)) return dl_fail("dl_mclmc_create: the finite-difference mode needs fd_delta and fd_limits");
    std::vector<int32_t> ids(nchains);
    for (int c = 0; c < nchains; ++c) {
        ids[c] = chain_ids ? chain_ids[c] : c;
        if (ids[c] < 0) return dl_fail("dl_mclmc_create: chain ids must be non-negative");
    }
    dl_mclmc* m = new dl_mclmc();
    m->ctx = ctx; m->device = (int)dl_info(ctx, "device"); m->C = nchains; m->P = P; m->integrator = integrator;
    m->seed = seed; m->offset = offset; m->ids = ids;
    auto bail = [&](const std::string& msg) { dl_mclmc_destroy(m); return dl_fail(msg); };
    if (hipSetDevice(m->device) != hipSuccess) return bail("dl_mclmc_create: hipSetDevice failed");
    const size_t C = nchains, p = P;
    bool ok = dl_dev_alloc(&m->vec, DL_MCLMC_NV * C * p) && dl_dev_alloc(&m->dsc, DL_MCLMC_ND * C) && dl_dev_alloc(&m->isc, DL_MCLMC_NI * C) && dl_dev_alloc(&m->iter, C) &&
              dl_dev_alloc(&m->chain_ids, C) && dl_dev_alloc(&m->fac, p * p) && dl_dev_alloc(&m->fact, p * p) &&
              dl_fd_gradient_create(&m->g, C, p, gradient_mode, fd_delta, fd_limits);
    if (!ok) return bail("dl_mclmc_create: device allocation failed");
    ok = hipMemcpy(m->chain_ids, ids.data(), C * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) return bail("dl_mclmc_create: initialisation of the device arrays failed");
    *out = m;
    return 0;
}

int dl_mclmc_set_preconditioner(dl_mclmc* m, const double* factor, int32_t dense, void* hip_stream) {
    if (!m || !factor) return dl_fail("dl_mclmc_set_preconditioner: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int P = m->P;
    std::vector<double> fac(dense ? (size_t)P * P : (size_t)P, 0.), fact((size_t)P * P, 0.);
    if (!dense) {
        for (int i = 0; i < P; ++i) {
            fac[i] = factor[i];
            if (!(fac[i] > 0.) || !std::isfinite(fac[i])) return dl_fail("dl_mclmc_set_preconditioner: the diagonal preconditioner must be positive and finite");
        }
    } else {
        for (int i = 0; i < P; ++i)
            for (int j = 0; j <= i; ++j) {      // the lower triangle (entries above the diagonal are not read)
                const double v = factor[(size_t)i * P + j];
                if (!std::isfinite(v) || (i == j && !(v > 0.))) return dl_fail("dl_mclmc_set_preconditioner: the dense factor must be finite, lower triangular, with a positive diagonal");
                fac[(size_t)i * P + j] = v; fact[(size_t)j * P + i] = v;
            }
    }
    DL_HIP_CHECK(hipSetDevice(m->device));
    DL_HIP_CHECK(hipMemcpyAsync(m->fac, fac.data(), fac.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->fact, fact.data(), fact.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));   // the host buffers are pageable
    m->dense = dense != 0;
    m->have_fac = true;
    return 0;
}

int dl_mclmc_set_hyper(dl_mclmc* m, double step_size, double L, void* hip_stream) {
    if (!m) return dl_fail("dl_mclmc_set_hyper: null sampler");
    if (!(step_size > 0.) || !std::isfinite(step_size)) return dl_fail("dl_mclmc_set_hyper: step_size must be positive and finite");
    if (!(L > 0.)) return dl_fail("dl_mclmc_set_hyper: L must be positive (+inf: no refresh)");
    hipStream_t stream = (hipStream_t)hip_stream;
    DL_HIP_CHECK(hipSetDevice(m->device));
    if (dl_mclmc_fill(m, DL_MCLMC_D_EPS, step_size, stream)) return 1;
    m->L = L;
    m->have_hyper = true;
    return 0;
}

int dl_mclmc_set_state(dl_mclmc* m, const double* coords, const double* momenta, const double* logposterior, const int64_t* step_counters, void* hip_stream) {
    if (!m || !coords) return dl_fail("dl_mclmc_set_state: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t C = m->C, P = m->P;
    for (size_t k = 0; k < C * P; ++k)
        if (!std::isfinite(coords[k])) return dl_fail("dl_mclmc_set_state: the starting positions must be finite");
    std::vector<long long> it(C, 0);
    if (step_counters)
        for (size_t c = 0; c < C; ++c) {
            if (step_counters[c] < 0) return dl_fail("dl_mclmc_set_state: negative step counter");
            it[c] = step_counters[c];
        }
    std::vector<double> u(C * P);
    const DlNutsSerial l{(int)P};
    for (size_t c = 0; c < C; ++c) {
        if (momenta) {
            double n2 = 0.;
            for (size_t i = 0; i < P; ++i) { u[c * P + i] = momenta[c * P + i]; n2 += u[c * P + i] * u[c * P + i]; }
            if (!(std::fabs(n2 - 1.) < 1e-6)) return dl_fail("dl_mclmc_set_state: the momenta must be unit vectors");
        } else {                // z / |z| of the chain's counter
            DlNutsVec<DlNutsSerial> z;
            for (int j = 0; j < DlNutsSerial::W; ++j)
                z.x[j] = j < (int)P ? dl_mclmc_gauss(it[c], (uint32_t)m->ids[c], j, DL_MCLMC_STREAM_INIT, (uint32_t)m->seed, (uint32_t)(m->seed >> 32)) : 0.;
            dl_mclmc_normalise(l, z);
            dl_nuts_store(l, z, u.data() + c * P);
        }
    }
    DL_HIP_CHECK(hipSetDevice(m->device));
    double* x = m->vec + (size_t)DL_MCLMC_V_X * C * P;
    DL_HIP_CHECK(hipMemcpyAsync(x, coords, C * P * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->vec + (size_t)DL_MCLMC_V_XN * C * P, coords, C * P * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->vec + (size_t)DL_MCLMC_V_U * C * P, u.data(), C * P * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->iter, it.data(), C * sizeof(long long), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemsetAsync(m->isc, 0, DL_MCLMC_NI * C * sizeof(int32_t), stream));
    // log-posterior and gradient of the starting points
    if (dl_fd_gradient_eval(&m->g, m->ctx, "dl_mclmc", x, m->C, m->P, stream)) return 1;
    std::vector<double> lp(C), g(C * P);
    DL_HIP_CHECK(hipMemcpyAsync(lp.data(), m->g.lp, C * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipMemcpyAsync(g.data(), m->g.grad, C * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    for (size_t c = 0; c < C; ++c) {
        lp[c] = logposterior ? logposterior[c] : lp[c] + m->offset;
        if (!std::isfinite(lp[c])) return dl_fail("dl_mclmc_set_state: the log-posterior of starting position " + std::to_string(c) + " is not finite");
        for (size_t i = 0; i < P; ++i)
            if (!std::isfinite(g[c * P + i])) return dl_fail("dl_mclmc_set_state: the gradient at starting position " + std::to_string(c) + " is not finite");
    }
    DL_HIP_CHECK(hipMemcpyAsync(m->dsc + DL_MCLMC_D_LP * C, lp.data(), C * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->vec + (size_t)DL_MCLMC_V_G * C * P, m->g.grad, C * P * sizeof(double), hipMemcpyDeviceToDevice, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    m->have_state = true;
    return 0;
}

int dl_mclmc_get_state(dl_mclmc* m, double* coords, double* momenta, double* logposterior, int64_t* step_counters, double* step_size, void* hip_stream) {
    if (!m) return dl_fail("dl_mclmc_get_state: null sampler");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t C = m->C, P = m->P;
    DL_HIP_CHECK(hipSetDevice(m->device));
    if (coords) DL_HIP_CHECK(hipMemcpyAsync(coords, m->vec + (size_t)DL_MCLMC_V_X * C * P, C * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (momenta) DL_HIP_CHECK(hipMemcpyAsync(momenta, m->vec + (size_t)DL_MCLMC_V_U * C * P, C * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (logposterior) DL_HIP_CHECK(hipMemcpyAsync(logposterior, m->dsc + DL_MCLMC_D_LP * C, C * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (step_counters) DL_HIP_CHECK(hipMemcpyAsync(step_counters, m->iter, C * sizeof(long long), hipMemcpyDeviceToHost, stream));
    if (step_size) DL_HIP_CHECK(hipMemcpyAsync(step_size, m->dsc + DL_MCLMC_D_EPS * C, C * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int dl_mclmc_set_adaptation(dl_mclmc* m, int32_t step_size_on, int32_t moments_on, double desired_energy_var, double trust_in_estimate, double num_effective_samples,
                            void* hip_stream) {
    if (!m) return dl_fail("dl_mclmc_set_adaptation: null sampler");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t C = m->C, P = m->P;
    DL_HIP_CHECK(hipSetDevice(m->device));
    if (step_size_on) {
        if (!(desired_energy_var > 0.) || !(trust_in_estimate > 0.) || !(num_effective_samples >= 1.) || !std::isfinite(desired_energy_var + trust_in_estimate + num_effective_samples))
            return dl_fail("dl_mclmc_set_adaptation: desired_energy_var and trust_in_estimate must be positive, num_effective_samples >= 1");
        m->energy_var = desired_energy_var; m->trust = trust_in_estimate; m->gamma = (num_effective_samples - 1.) / (num_effective_samples + 1.);
        // the controller restarts: a = b = 0, no cap
        if (dl_mclmc_fill(m, DL_MCLMC_D_CA, 0., stream) || dl_mclmc_fill(m, DL_MCLMC_D_CB, 0., stream) ||
            dl_mclmc_fill(m, DL_MCLMC_D_EPSMAX, std::numeric_limits<double>::infinity(), stream)) return 1;
    }
    if (moments_on) {           // the sums restart
        DL_HIP_CHECK(hipMemsetAsync(m->vec + (size_t)DL_MCLMC_V_SX * C * P, 0, 2 * C * P * sizeof(double), stream));
        DL_HIP_CHECK(hipMemsetAsync(m->dsc + DL_MCLMC_D_SW * C, 0, C * sizeof(double), stream));
        DL_HIP_CHECK(hipStreamSynchronize(stream));
    }
    m->adapt = step_size_on != 0;
    m->moments = moments_on != 0;
    return 0;
}

int dl_mclmc_get_moments(dl_mclmc* m, double* sum_w, double* sum_wx, double* sum_wxx, void* hip_stream) {
    if (!m) return dl_fail("dl_mclmc_get_moments: null sampler");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t C = m->C, P = m->P;
    DL_HIP_CHECK(hipSetDevice(m->device));
    if (sum_w) DL_HIP_CHECK(hipMemcpyAsync(sum_w, m->dsc + DL_MCLMC_D_SW * C, C * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (sum_wx) DL_HIP_CHECK(hipMemcpyAsync(sum_wx, m->vec + (size_t)DL_MCLMC_V_SX * C * P, C * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (sum_wxx) DL_HIP_CHECK(hipMemcpyAsync(sum_wxx, m->vec + (size_t)DL_MCLMC_V_SXX * C * P, C * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int dl_mclmc_run(dl_mclmc* m, int64_t nsteps, int32_t quota, int32_t thin_by, double* out_coords_dev, double* out_logp_dev, double* out_info_dev, int32_t* out_count_dev,
                 void* hip_stream) {
    if (!m) return dl_fail("dl_mclmc_run: null sampler");
    if (nsteps < 0 || quota < 1 || thin_by < 1) return dl_fail("dl_mclmc_run: invalid argument");
    if (!out_coords_dev || !out_logp_dev || !out_info_dev || !out_count_dev) return dl_fail("dl_mclmc_run: the record buffers are required");
    if (!m->have_fac) return dl_fail("dl_mclmc_run: no preconditioner (dl_mclmc_set_preconditioner)");
    if (!m->have_hyper) return dl_fail("dl_mclmc_run: no step size (dl_mclmc_set_hyper)");
    if (!m->have_state) return dl_fail("dl_mclmc_run: no state (dl_mclmc_set_state)");
    if (!nsteps) return 0;
    hipStream_t stream = (hipStream_t)hip_stream;
    DL_HIP_CHECK(hipSetDevice(m->device));
    DlMclmcArgs a = dl_mclmc_args(m);
    a.out_coords = out_coords_dev; a.out_logp = out_logp_dev; a.out_info = out_info_dev; a.out_count = out_count_dev;
    a.cap = quota; a.quota = quota; a.thin_by = thin_by;
    const unsigned grid = (unsigned)((m->C + DL_MCLMC_WAVES - 1) / DL_MCLMC_WAVES);
    const double* xn = m->vec + (size_t)DL_MCLMC_V_XN * m->C * m->P;
    hipLaunchKernelGGL(dl_mclmc_stage_kernel, dim3(grid), dim3(64 * DL_MCLMC_WAVES), 0, stream, a, -1, 0);     // every chain below its quota opens a step
    for (int64_t s = 0; s < nsteps; ++s)
        for (int stage = 0; stage < a.nstage; ++stage) {
            if (dl_fd_gradient_eval(&m->g, m->ctx, "dl_mclmc", xn, m->C, m->P, stream)) return 1;
            hipLaunchKernelGGL(dl_mclmc_stage_kernel, dim3(grid), dim3(64 * DL_MCLMC_WAVES), 0, stream, a, stage, s + 1 < nsteps ? 1 : 0);
        }
    DL_HIP_CHECK(hipGetLastError());
    m->steps += nsteps;
    return 0;
}

int64_t dl_mclmc_info(const dl_mclmc* m, const char* key) {
    if (!m || !key) return -1;
    const std::string k(key);
    if (k == "nchains") return m->C;
    if (k == "n_params") return m->P;
    if (k == "steps") return m->steps;
    if (k == "integrator") return m->integrator;
    if (k == "gradients_per_step") return m->integrator == 0 ? 1 : 2;
    if (k == "finite") return m->g.finite ? 1 : 0;
    if (k == "dense") return m->dense ? 1 : 0;
    if (k == "adapt") return m->adapt ? 1 : 0;
    if (k == "moments") return m->moments ? 1 : 0;
    return -1;
}

}  // extern "C"
