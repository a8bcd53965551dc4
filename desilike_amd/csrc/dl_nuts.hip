// dl_nuts.hip -- device-resident No-U-Turn sampler (include/desilike_amd.h, dl_nuts_*; the algorithm and the per-chain record: dl_nuts.h).
//
// A step advances every chain by one leapfrog step and is two launches, nothing synchronises with the host:
//
//     gradient of the pending positions [C, P]  ->  dl_nuts_step_kernel (finish the leaf's kick, energy, weight, U-turns, selection, termination; the next leaf's
//                                                  half kick and drift -- or the record, the dual averaging, a fresh momentum and the first drift of the next trajectory)
//
// The gradient is dl_eval_logposterior_grad where the context is in its scope; otherwise central differences of dl_eval_logposterior, whose non-finite values the step
// kernel zeroes (dl_fd_gradient.hip: the route MCLMC shares).
// One wavefront per chain, one lane per parameter component (P <= 64): the kinetic energy and the U-turn dot products are wavefront reductions, a state row is one
// coalesced load.  Every lane computes the same chain scalars and stores them (one address): no lane reads another lane's store.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/desilike_amd.h"
#include "dl_sampler_dev.h"   // DlWave, DlBlock, dl_fail, DL_HIP_CHECK, dl_dev_alloc / free
#include "dl_nuts.h"

#define DL_NUTS_WAVES 4    // chains per workgroup

struct dl_nuts {
    dl_ctx* ctx = nullptr;
    int device = 0;
    int C = 0, P = 0, D = 10;
    bool have_mass = false, have_state = false, adapt = false, dense = false;
    double threshold = 1000., offset = 0., target = 0.8;
    uint64_t seed = 0;
    int64_t steps = 0;
    // device
    double *vec = nullptr, *dsc = nullptr, *minv = nullptr, *lmass = nullptr;
    DlFdGradient g;       // log-posterior and gradient of the pending positions
    int32_t *isc = nullptr, *chain_ids = nullptr;
    long long* iter = nullptr;
};

namespace {

__global__ __launch_bounds__(64 * DL_NUTS_WAVES) void dl_nuts_step_kernel(DlNutsArgs a, int mode) {
    const int c = blockIdx.x * DL_NUTS_WAVES + (int)(threadIdx.x >> 6);
    if (c >= a.C) return;     // (whole wavefronts)
    const DlWave l{a.P, (int)(threadIdx.x & 63)};
    dl_nuts_chain_step(l, a, c, mode);
}

DlNutsArgs dl_nuts_args(const dl_nuts* n) {
    DlNutsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.vec = n->vec; a.dsc = n->dsc; a.isc = n->isc; a.iter = n->iter; a.chain_ids = n->chain_ids; a.minv = n->minv; a.lmass = n->lmass;
    a.lp_new = n->g.lp; a.g_new = n->g.grad;
    a.C = n->C; a.P = n->P; a.D = n->D; a.dense = n->dense ? 1 : 0; a.adapt = n->adapt ? 1 : 0;
    a.threshold = n->threshold; a.offset = n->offset; a.target = n->target;
    a.k0 = (uint32_t)n->seed; a.k1 = (uint32_t)(n->seed >> 32);
    return a;
}

}  // namespace

extern "C" {

void dl_nuts_destroy(dl_nuts* n) {
    if (!n) return;
    (void)hipSetDevice(n->device);
    dl_fd_gradient_destroy(&n->g);
    dl_dev_free({(void**)&n->vec, (void**)&n->dsc, (void**)&n->minv, (void**)&n->lmass, (void**)&n->isc, (void**)&n->chain_ids, (void**)&n->iter});
    delete n;
}

int dl_nuts_create(dl_nuts** out, dl_ctx* ctx, int32_t nchains, const int32_t* chain_ids, int32_t max_num_doublings, double divergence_threshold, uint64_t seed,
                   double offset, int32_t gradient_mode, const double* fd_delta, const double* fd_limits) {
    if (!out || !ctx) return dl_fail("dl_nuts_create: null argument");
    *out = nullptr;
    const int P = (int)dl_info(ctx, "n_params");
    if (P < 1 || P > DL_NUTS_MAX_P) return dl_fail("dl_nuts_create: the sampler takes 1 .. 64 parameters, the context has " + std::to_string(P));
    if (nchains < 1) return dl_fail("dl_nuts_create: nchains must be >= 1");
    if (max_num_doublings < 1 || max_num_doublings > DL_NUTS_MAX_DEPTH) return dl_fail("dl_nuts_create: max_num_doublings must be in [1, 15]");
    if (!(divergence_threshold > 0.)) return dl_fail("dl_nuts_create: divergence_threshold must be positive");
    if (gradient_mode < 0 || gradient_mode > 2) return dl_fail("dl_nuts_create: gradient_mode must be 0 (auto), 1 (analytic) or 2 (finite)");
    if (gradient_mode == 2 && (!fd_delta || !fd_limits)) return dl_fail("dl_nuts_create: the finite-difference mode needs fd_delta and fd_limits");
    std::vector<int32_t> ids(nchains);
    for (int c = 0; c < nchains; ++c) {
        ids[c] = chain_ids ? chain_ids[c] : c;
        if (ids[c] < 0) return dl_fail("dl_nuts_create: chain ids must be non-negative");
    }
    dl_nuts* n = new dl_nuts();
    n->ctx = ctx; n->device = (int)dl_info(ctx, "device"); n->C = nchains; n->P = P; n->D = max_num_doublings;
    n->threshold = divergence_threshold; n->seed = seed; n->offset = offset;
    auto bail = [&](const std::string& msg) { dl_nuts_destroy(n); return dl_fail(msg); };
    if (hipSetDevice(n->device) != hipSuccess) return bail("dl_nuts_create: hipSetDevice failed");
    const size_t C = nchains, p = P, nv = DL_NUTS_V_CK + 2 * (size_t)n->D;
    bool ok = dl_dev_alloc(&n->vec, nv * C * p) && dl_dev_alloc(&n->dsc, DL_NUTS_ND * C) && dl_dev_alloc(&n->isc, DL_NUTS_NI * C) && dl_dev_alloc(&n->iter, C) &&
              dl_dev_alloc(&n->chain_ids, C) && dl_dev_alloc(&n->minv, p * p) && dl_dev_alloc(&n->lmass, p * p) &&
              dl_fd_gradient_create(&n->g, C, p, gradient_mode, fd_delta, fd_limits);
    if (!ok) return bail("dl_nuts_create: device allocation failed");
    ok = hipMemcpy(n->chain_ids, ids.data(), C * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) return bail("dl_nuts_create: initialisation of the device arrays failed");
    *out = n;
    return 0;
}

int dl_nuts_set_mass(dl_nuts* n, const double* inverse_mass, int32_t dense, double step_size, void* hip_stream) {
    if (!n || !inverse_mass) return dl_fail("dl_nuts_set_mass: null argument");
    if (!(step_size > 0.) || !std::isfinite(step_size)) return dl_fail("dl_nuts_set_mass: step_size must be positive");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int P = n->P;
    std::vector<double> minv(dense ? (size_t)P * P : (size_t)P, 0.), lmass((size_t)P * P, 0.);
    if (!dense) {
        for (int i = 0; i < P; ++i) {
            minv[i] = inverse_mass[i];
            if (!(minv[i] > 0.) || !std::isfinite(minv[i])) return dl_fail("dl_nuts_set_mass: the diagonal inverse mass matrix must be positive and finite");
        }
    } else {
        // M = Minv^-1 by Cholesky factorisations: Minv = U U^T (U lower), M = U^-T U^-1, then L_M = chol(M)
        std::vector<double> A(inverse_mass, inverse_mass + (size_t)P * P), Uinv((size_t)P * P, 0.), M((size_t)P * P, 0.);
        for (int i = 0; i < P; ++i)
            for (int j = 0; j < P; ++j)
                if (!std::isfinite(A[(size_t)i * P + j]) || A[(size_t)i * P + j] != A[(size_t)j * P + i]) return dl_fail("dl_nuts_set_mass: the inverse mass matrix must be finite and symmetric");
        auto cholesky = [P](std::vector<double>& a) {    // in place, lower; false if not positive definite
            for (int j = 0; j < P; ++j) {
                double s = a[(size_t)j * P + j];
                for (int k = 0; k < j; ++k) s -= a[(size_t)j * P + k] * a[(size_t)j * P + k];
                if (!(s > 0.)) return false;
                a[(size_t)j * P + j] = std::sqrt(s);
                for (int i = j + 1; i < P; ++i) {
                    double t = a[(size_t)i * P + j];
                    for (int k = 0; k < j; ++k) t -= a[(size_t)i * P + k] * a[(size_t)j * P + k];
                    a[(size_t)i * P + j] = t / a[(size_t)j * P + j];
                }
                for (int k = j + 1; k < P; ++k) a[(size_t)j * P + k] = 0.;
            }
            return true;
        };
        std::vector<double> U = A;
        if (!cholesky(U)) return dl_fail("dl_nuts_set_mass: the inverse mass matrix is not positive definite");
        for (int j = 0; j < P; ++j) {            // U^-1 (lower), column by column
            Uinv[(size_t)j * P + j] = 1. / U[(size_t)j * P + j];
            for (int i = j + 1; i < P; ++i) {
                double s = 0.;
                for (int k = j; k < i; ++k) s += U[(size_t)i * P + k] * Uinv[(size_t)k * P + j];
                Uinv[(size_t)i * P + j] = -s / U[(size_t)i * P + i];
            }
        }
        for (int i = 0; i < P; ++i)
            for (int j = 0; j < P; ++j) {
                double s = 0.;
                for (int k = 0; k < P; ++k) s += Uinv[(size_t)k * P + i] * Uinv[(size_t)k * P + j];
                M[(size_t)i * P + j] = s;
            }
        if (!cholesky(M)) return dl_fail("dl_nuts_set_mass: the mass matrix is not positive definite");
        minv = A; lmass = M;
    }
    DL_HIP_CHECK(hipSetDevice(n->device));
    DL_HIP_CHECK(hipMemcpyAsync(n->minv, minv.data(), minv.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(n->lmass, lmass.data(), lmass.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    // every chain's step size (the chains wait at trajectory boundaries between batches: the new values apply from their next trajectory)
    const size_t C = n->C;
    std::vector<double> logeps(C, std::log(step_size));
    DL_HIP_CHECK(hipMemcpyAsync(n->dsc + DL_NUTS_D_LOGEPS * C, logeps.data(), C * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(n->dsc + DL_NUTS_D_LOGBAR * C, logeps.data(), C * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));   // the host buffers are pageable
    n->dense = dense != 0;
    n->have_mass = true;
    return 0;
}

int dl_nuts_set_state(dl_nuts* n, const double* coords, const double* logposterior, const int64_t* iteration_counters, void* hip_stream) {
    if (!n || !coords) return dl_fail("dl_nuts_set_state: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t C = n->C, P = n->P;
    for (size_t k = 0; k < C * P; ++k)
        if (!std::isfinite(coords[k])) return dl_fail("dl_nuts_set_state: the starting positions must be finite");
    std::vector<long long> it(C, 0);
    if (iteration_counters)
        for (size_t c = 0; c < C; ++c) {
            if (iteration_counters[c] < 0) return dl_fail("dl_nuts_set_state: negative iteration counter");
            it[c] = iteration_counters[c];
        }
    DL_HIP_CHECK(hipSetDevice(n->device));
    double* qp = n->vec + (size_t)DL_NUTS_V_QP * C * P;
    DL_HIP_CHECK(hipMemcpyAsync(qp, coords, C * P * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(n->vec + (size_t)DL_NUTS_V_QN * C * P, coords, C * P * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(n->iter, it.data(), C * sizeof(long long), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemsetAsync(n->isc + DL_NUTS_I_ACTIVE * C, 0, C * sizeof(int32_t), stream));
    // log-posterior and gradient of the starting points: the proposal the first trajectory starts from
    if (dl_fd_gradient_eval(&n->g, n->ctx, "dl_nuts", qp, n->C, n->P, stream)) return 1;
    std::vector<double> lp(C);
    DL_HIP_CHECK(hipMemcpyAsync(lp.data(), n->g.lp, C * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    for (size_t c = 0; c < C; ++c) {
        lp[c] = logposterior ? logposterior[c] : lp[c] + n->offset;
        if (!std::isfinite(lp[c])) return dl_fail("dl_nuts_set_state: the log-posterior of starting position " + std::to_string(c) + " is not finite");
    }
    DL_HIP_CHECK(hipMemcpyAsync(n->dsc + DL_NUTS_D_LPP * C, lp.data(), C * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(n->vec + (size_t)DL_NUTS_V_GP * C * P, n->g.grad, C * P * sizeof(double), hipMemcpyDeviceToDevice, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    n->have_state = true;
    return 0;
}

int dl_nuts_get_state(dl_nuts* n, double* coords, double* logposterior, int64_t* iteration_counters, double* log_step_size, void* hip_stream) {
    if (!n) return dl_fail("dl_nuts_get_state: null sampler");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t C = n->C, P = n->P;
    DL_HIP_CHECK(hipSetDevice(n->device));
    if (coords) DL_HIP_CHECK(hipMemcpyAsync(coords, n->vec + (size_t)DL_NUTS_V_QP * C * P, C * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (logposterior) DL_HIP_CHECK(hipMemcpyAsync(logposterior, n->dsc + DL_NUTS_D_LPP * C, C * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (iteration_counters) DL_HIP_CHECK(hipMemcpyAsync(iteration_counters, n->iter, C * sizeof(long long), hipMemcpyDeviceToHost, stream));
    if (log_step_size) DL_HIP_CHECK(hipMemcpyAsync(log_step_size, n->dsc + DL_NUTS_D_LOGBAR * C, C * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int dl_nuts_set_adaptation(dl_nuts* n, int32_t enabled, double target_acceptance, double initial_log_step_size, void* hip_stream) {
    if (!n) return dl_fail("dl_nuts_set_adaptation: null sampler");
    n->adapt = enabled != 0;
    if (!n->adapt) return 0;
    if (!(target_acceptance > 0. && target_acceptance < 1.) || !std::isfinite(initial_log_step_size)) return dl_fail("dl_nuts_set_adaptation: invalid target or step size");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t C = n->C;
    n->target = target_acceptance;
    // per chain: log eps = log eps_bar = initial, mu = log(10 eps), hbar = 0, count = 0
    std::vector<double> init(C, initial_log_step_size), mu(C, std::log(10.) + initial_log_step_size);
    DL_HIP_CHECK(hipSetDevice(n->device));
    DL_HIP_CHECK(hipMemcpyAsync(n->dsc + DL_NUTS_D_LOGEPS * C, init.data(), C * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(n->dsc + DL_NUTS_D_LOGBAR * C, init.data(), C * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(n->dsc + DL_NUTS_D_MU * C, mu.data(), C * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemsetAsync(n->dsc + DL_NUTS_D_HBAR * C, 0, C * sizeof(double), stream));
    DL_HIP_CHECK(hipMemsetAsync(n->dsc + DL_NUTS_D_DACOUNT * C, 0, C * sizeof(double), stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int dl_nuts_run(dl_nuts* n, int64_t nsteps, int32_t quota, int32_t thin_by, double* out_coords_dev, double* out_logp_dev, double* out_info_dev, int32_t* out_count_dev,
                void* hip_stream) {
    if (!n) return dl_fail("dl_nuts_run: null sampler");
    if (nsteps < 0 || quota < 1 || thin_by < 1) return dl_fail("dl_nuts_run: invalid argument");
    if (!out_coords_dev || !out_logp_dev || !out_info_dev || !out_count_dev) return dl_fail("dl_nuts_run: the record buffers are required");
    if (!n->have_mass) return dl_fail("dl_nuts_run: no inverse mass matrix (dl_nuts_set_mass)");
    if (!n->have_state) return dl_fail("dl_nuts_run: no state (dl_nuts_set_state)");
    hipStream_t stream = (hipStream_t)hip_stream;
    DL_HIP_CHECK(hipSetDevice(n->device));
    DlNutsArgs a = dl_nuts_args(n);
    a.out_coords = out_coords_dev; a.out_logp = out_logp_dev; a.out_info = out_info_dev; a.out_count = out_count_dev;
    a.cap = quota; a.quota = quota; a.thin_by = thin_by;
    const unsigned grid = (unsigned)((n->C + DL_NUTS_WAVES - 1) / DL_NUTS_WAVES);
    const double* qn = n->vec + (size_t)DL_NUTS_V_QN * n->C * n->P;
    hipLaunchKernelGGL(dl_nuts_step_kernel, dim3(grid), dim3(64 * DL_NUTS_WAVES), 0, stream, a, 0);     // chains waiting at a boundary start
    for (int64_t s = 0; s < nsteps; ++s) {
        if (dl_fd_gradient_eval(&n->g, n->ctx, "dl_nuts", qn, n->C, n->P, stream)) return 1;
        hipLaunchKernelGGL(dl_nuts_step_kernel, dim3(grid), dim3(64 * DL_NUTS_WAVES), 0, stream, a, 1);
    }
    DL_HIP_CHECK(hipGetLastError());
    n->steps += nsteps;
    return 0;
}

int64_t dl_nuts_info(const dl_nuts* n, const char* key) {
    if (!n || !key) return -1;
    const std::string k(key);
    if (k == "nchains") return n->C;
    if (k == "n_params") return n->P;
    if (k == "steps") return n->steps;
    if (k == "max_num_doublings") return n->D;
    if (k == "finite") return n->g.finite ? 1 : 0;
    if (k == "dense") return n->dense ? 1 : 0;
    if (k == "adapt") return n->adapt ? 1 : 0;
    return -1;
}

}  // extern "C"
