// dl_nuts.hip -- device-resident No-U-Turn sampler (include/desilike_amd.h, dl_nuts_*; the algorithm and the per-chain record: dl_nuts.h).
//
// A step advances every chain by one leapfrog step and is two launches, nothing synchronises with the host:
//
//     gradient of the pending positions [C, P]  ->  dl_nuts_step_kernel (finish the leaf's kick, energy, weight, U-turns, selection, termination; the next leaf's
//                                                  half kick and drift -- or the record, the dual averaging, a fresh momentum and the first drift of the next trajectory)
//
// The gradient is dl_eval_logposterior_grad where the context is in its scope; otherwise central differences: dl_nuts_stencil_kernel writes the C (2 P + 1) rows
// q, q -+ step e_i (steps: Parameter.delta, shortened near a prior bound), dl_eval_logposterior evaluates them, dl_nuts_diff_kernel forms log-posterior and gradient.
// One wavefront per chain, one lane per parameter component (P <= 64): the kinetic energy and the U-turn dot products are wavefront reductions, a state row is one
// coalesced load.  Every lane computes the same chain scalars and stores them (one address): no lane reads another lane's store.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/desilike_amd.h"
#include "dl_kernels.h"   // dl_set_last_error
#include "dl_nuts.h"

#define DL_NUTS_WAVES 4    // chains per workgroup

struct dl_nuts {
    dl_ctx* ctx = nullptr;
    int device = 0;
    int C = 0, P = 0, D = 10, mode = 0;       // gradient mode: 0 auto, 1 analytic, 2 finite
    bool finite = false, have_mass = false, have_state = false, adapt = false, dense = false;
    double threshold = 1000., offset = 0., target = 0.8;
    uint64_t seed = 0;
    int64_t steps = 0;
    // device
    double *vec = nullptr, *dsc = nullptr, *minv = nullptr, *lmass = nullptr, *lp = nullptr, *grad = nullptr;
    double *fd_rows = nullptr, *fd_vals = nullptr, *fd_delta = nullptr, *fd_limits = nullptr;
    int32_t *isc = nullptr, *chain_ids = nullptr;
    long long* iter = nullptr;
};

namespace {

int fail(const std::string& msg) {
    dl_set_last_error(msg.c_str());
    return 1;
}

#define DL_NUTS_HIP(call)                                                                             \
    do {                                                                                              \
        hipError_t err__ = (call);                                                                    \
        if (err__ != hipSuccess) return fail(std::string(#call) + ": " + hipGetErrorString(err__));   \
    } while (0)

// the device's component layout: lane = component
struct DlNutsWave {
    static constexpr int W = 1;
    int P, lane;
    __device__ int comp(int) const { return lane; }
    __device__ bool on(int) const { return lane < P; }
    __device__ double sum(const double* x) const {
        double v = x[0];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        return v;
    }
    __device__ double at(const double* x, int k) const { return __shfl(x[0], k, 64); }
};

__global__ __launch_bounds__(64 * DL_NUTS_WAVES) void dl_nuts_step_kernel(DlNutsArgs a, int mode) {
    const int c = blockIdx.x * DL_NUTS_WAVES + (int)(threadIdx.x >> 6);
    if (c >= a.C) return;     // (whole wavefronts)
    const DlNutsWave l{a.P, (int)(threadIdx.x & 63)};
    dl_nuts_chain_step(l, a, c, mode);
}

// finite-difference stencil of the pending positions: row (c, 0) = q, (c, 1 + 2 i) = q - lower_i e_i, (c, 2 + 2 i) = q + upper_i e_i
__device__ inline void dl_nuts_fd_steps(const double* q, const double* delta, const double* limits, int i, double* lower, double* upper) {
    *lower = fmax(fmin(delta[2 * i], q[i] - limits[2 * i]), 0.);
    *upper = fmax(fmin(delta[2 * i + 1], limits[2 * i + 1] - q[i]), 0.);
}

__global__ void dl_nuts_stencil_kernel(const double* qn, const double* delta, const double* limits, int C, int P, double* rows) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x, R = 2 * P + 1;
    if (idx >= (long long)C * R * P) return;
    const int i = (int)(idx % P);
    const long long cr = idx / P;
    const int r = (int)(cr % R), c = (int)(cr / R);
    const double* q = qn + (size_t)c * P;
    double value = q[i];
    if (r > 0 && (r - 1) / 2 == i) {
        double lower, upper;
        dl_nuts_fd_steps(q, delta, limits, i, &lower, &upper);
        value = (r & 1) ? q[i] - lower : q[i] + upper;
    }
    rows[idx] = value;
}

__global__ void dl_nuts_diff_kernel(const double* qn, const double* delta, const double* limits, const double* vals, int C, int P, double* lp, double* grad) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)C * P) return;
    const int i = (int)(idx % P), c = (int)(idx / P);
    const double* v = vals + (size_t)c * (2 * P + 1);
    double lower, upper;
    dl_nuts_fd_steps(qn + (size_t)c * P, delta, limits, i, &lower, &upper);
    grad[idx] = (v[2 + 2 * i] - v[1 + 2 * i]) / (lower + upper);     // (non-finite values are zeroed by the step kernel)
    if (i == 0) lp[c] = v[0];
}

// log-posterior [C] and gradient [C, P] of rows q [C, P] into n->lp / n->grad (analytic, or central differences)
int dl_nuts_gradient(dl_nuts* n, const double* q, hipStream_t stream) {
    const int C = n->C, P = n->P;
    if (!n->finite) {
        const int rc = dl_eval_logposterior_grad(n->ctx, q, C, n->lp, n->grad, nullptr, stream);
        if (rc == 1) return 1;
        if (rc == 0) return 0;
        if (n->mode == 1) return fail("dl_nuts: the context is outside the analytic gradient's scope (use the finite-difference mode)");
        n->finite = true;
    }
    if (!n->fd_rows) return fail("dl_nuts: central differences need the steps and limits given to dl_nuts_create");
    const long long nrow = (long long)C * (2 * P + 1);
    hipLaunchKernelGGL(dl_nuts_stencil_kernel, dim3((unsigned)((nrow * P + 255) / 256)), dim3(256), 0, stream, q, n->fd_delta, n->fd_limits, C, P, n->fd_rows);
    if (dl_eval_logposterior(n->ctx, n->fd_rows, nrow, n->fd_vals, nullptr, stream)) return 1;
    hipLaunchKernelGGL(dl_nuts_diff_kernel, dim3((unsigned)(((long long)C * P + 255) / 256)), dim3(256), 0, stream, q, n->fd_delta, n->fd_limits, n->fd_vals, C, P,
                       n->lp, n->grad);
    return 0;
}

DlNutsArgs dl_nuts_args(const dl_nuts* n) {
    DlNutsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.vec = n->vec; a.dsc = n->dsc; a.isc = n->isc; a.iter = n->iter; a.chain_ids = n->chain_ids; a.minv = n->minv; a.lmass = n->lmass;
    a.lp_new = n->lp; a.g_new = n->grad;
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
    for (void* p : {(void*)n->vec, (void*)n->dsc, (void*)n->minv, (void*)n->lmass, (void*)n->lp, (void*)n->grad, (void*)n->fd_rows, (void*)n->fd_vals,
                    (void*)n->fd_delta, (void*)n->fd_limits, (void*)n->isc, (void*)n->chain_ids, (void*)n->iter})
        if (p) (void)hipFree(p);
    delete n;
}

int dl_nuts_create(dl_nuts** out, dl_ctx* ctx, int32_t nchains, const int32_t* chain_ids, int32_t max_num_doublings, double divergence_threshold, uint64_t seed,
                   double offset, int32_t gradient_mode, const double* fd_delta, const double* fd_limits) {
    if (!out || !ctx) return fail("dl_nuts_create: null argument");
    *out = nullptr;
    const int P = (int)dl_info(ctx, "n_params");
    if (P < 1 || P > DL_NUTS_MAX_P) return fail("dl_nuts_create: the sampler takes 1 .. 64 parameters, the context has " + std::to_string(P));
    if (nchains < 1) return fail("dl_nuts_create: nchains must be >= 1");
    if (max_num_doublings < 1 || max_num_doublings > DL_NUTS_MAX_DEPTH) return fail("dl_nuts_create: max_num_doublings must be in [1, 15]");
    if (!(divergence_threshold > 0.)) return fail("dl_nuts_create: divergence_threshold must be positive");
    if (gradient_mode < 0 || gradient_mode > 2) return fail("dl_nuts_create: gradient_mode must be 0 (auto), 1 (analytic) or 2 (finite)");
    if (gradient_mode == 2 && (!fd_delta || !fd_limits)) return fail("dl_nuts_create: the finite-difference mode needs fd_delta and fd_limits");
    std::vector<int32_t> ids(nchains);
    for (int c = 0; c < nchains; ++c) {
        ids[c] = chain_ids ? chain_ids[c] : c;
        if (ids[c] < 0) return fail("dl_nuts_create: chain ids must be non-negative");
    }
    dl_nuts* n = new dl_nuts();
    n->ctx = ctx; n->device = (int)dl_info(ctx, "device"); n->C = nchains; n->P = P; n->D = max_num_doublings; n->mode = gradient_mode; n->finite = gradient_mode == 2;
    n->threshold = divergence_threshold; n->seed = seed; n->offset = offset;
    auto bail = [&](const std::string& msg) { dl_nuts_destroy(n); return fail(msg); };
    if (hipSetDevice(n->device) != hipSuccess) return bail("dl_nuts_create: hipSetDevice failed");
    const size_t C = nchains, nv = DL_NUTS_V_CK + 2 * (size_t)n->D, nrow = C * (2 * P + 1);
    bool ok = hipMalloc((void**)&n->vec, nv * C * P * sizeof(double)) == hipSuccess && hipMalloc((void**)&n->dsc, DL_NUTS_ND * C * sizeof(double)) == hipSuccess &&
              hipMalloc((void**)&n->isc, DL_NUTS_NI * C * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&n->iter, C * sizeof(long long)) == hipSuccess &&
              hipMalloc((void**)&n->chain_ids, C * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&n->minv, (size_t)P * P * sizeof(double)) == hipSuccess &&
              hipMalloc((void**)&n->lmass, (size_t)P * P * sizeof(double)) == hipSuccess && hipMalloc((void**)&n->lp, C * sizeof(double)) == hipSuccess &&
              hipMalloc((void**)&n->grad, C * P * sizeof(double)) == hipSuccess;
    if (ok && fd_delta && fd_limits)
        ok = hipMalloc((void**)&n->fd_rows, nrow * P * sizeof(double)) == hipSuccess && hipMalloc((void**)&n->fd_vals, nrow * sizeof(double)) == hipSuccess &&
             hipMalloc((void**)&n->fd_delta, 2 * (size_t)P * sizeof(double)) == hipSuccess && hipMalloc((void**)&n->fd_limits, 2 * (size_t)P * sizeof(double)) == hipSuccess &&
             hipMemcpy(n->fd_delta, fd_delta, 2 * (size_t)P * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(n->fd_limits, fd_limits, 2 * (size_t)P * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) return bail("dl_nuts_create: device allocation failed");
    ok = hipMemset(n->vec, 0, nv * C * P * sizeof(double)) == hipSuccess && hipMemset(n->dsc, 0, DL_NUTS_ND * C * sizeof(double)) == hipSuccess &&
         hipMemset(n->isc, 0, DL_NUTS_NI * C * sizeof(int32_t)) == hipSuccess && hipMemset(n->iter, 0, C * sizeof(long long)) == hipSuccess &&
         hipMemset(n->minv, 0, (size_t)P * P * sizeof(double)) == hipSuccess && hipMemset(n->lmass, 0, (size_t)P * P * sizeof(double)) == hipSuccess &&
         hipMemcpy(n->chain_ids, ids.data(), C * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) return bail("dl_nuts_create: initialisation of the device arrays failed");
    *out = n;
    return 0;
}

int dl_nuts_set_mass(dl_nuts* n, const double* inverse_mass, int32_t dense, double step_size, void* hip_stream) {
    if (!n || !inverse_mass) return fail("dl_nuts_set_mass: null argument");
    if (!(step_size > 0.) || !std::isfinite(step_size)) return fail("dl_nuts_set_mass: step_size must be positive");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int P = n->P;
    std::vector<double> minv(dense ? (size_t)P * P : (size_t)P, 0.), lmass((size_t)P * P, 0.);
    if (!dense) {
        for (int i = 0; i < P; ++i) {
            minv[i] = inverse_mass[i];
            if (!(minv[i] > 0.) || !std::isfinite(minv[i])) return fail("dl_nuts_set_mass: the diagonal inverse mass matrix must be positive and finite");
        }
    } else {
        // M = Minv^-1 by Cholesky factorisations: Minv = U U^T (U lower), M = U^-T U^-1, then L_M = chol(M)
        std::vector<double> A(inverse_mass, inverse_mass + (size_t)P * P), Uinv((size_t)P * P, 0.), M((size_t)P * P, 0.);
        for (int i = 0; i < P; ++i)
            for (int j = 0; j < P; ++j)
                if (!std::isfinite(A[(size_t)i * P + j]) || A[(size_t)i * P + j] != A[(size_t)j * P + i]) return fail("dl_nuts_set_mass: the inverse mass matrix must be finite and symmetric");
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
        if (!cholesky(U)) return fail("dl_nuts_set_mass: the inverse mass matrix is not positive definite");
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
        if (!cholesky(M)) return fail("dl_nuts_set_mass: the mass matrix is not positive definite");
        minv = A; lmass = M;
    }
    DL_NUTS_HIP(hipSetDevice(n->device));
    DL_NUTS_HIP(hipMemcpyAsync(n->minv, minv.data(), minv.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_NUTS_HIP(hipMemcpyAsync(n->lmass, lmass.data(), lmass.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    // every chain's step size (the chains wait at trajectory boundaries between batches: the new values apply from their next trajectory)
    const size_t C = n->C;
    std::vector<double> logeps(C, std::log(step_size));
    DL_NUTS_HIP(hipMemcpyAsync(n->dsc + DL_NUTS_D_LOGEPS * C, logeps.data(), C * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_NUTS_HIP(hipMemcpyAsync(n->dsc + DL_NUTS_D_LOGBAR * C, logeps.data(), C * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_NUTS_HIP(hipStreamSynchronize(stream));   // the host buffers are pageable
    n->dense = dense != 0;
    n->have_mass = true;
    return 0;
}

int dl_nuts_set_state(dl_nuts* n, const double* coords, const double* logposterior, const int64_t* iteration_counters, void* hip_stream) {
    if (!n || !coords) return fail("dl_nuts_set_state: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t C = n->C, P = n->P;
    for (size_t k = 0; k < C * P; ++k)
        if (!std::isfinite(coords[k])) return fail("dl_nuts_set_state: the starting positions must be finite");
    std::vector<long long> it(C, 0);
    if (iteration_counters)
        for (size_t c = 0; c < C; ++c) {
            if (iteration_counters[c] < 0) return fail("dl_nuts_set_state: negative iteration counter");
            it[c] = iteration_counters[c];
        }
    DL_NUTS_HIP(hipSetDevice(n->device));
    double* qp = n->vec + (size_t)DL_NUTS_V_QP * C * P;
    DL_NUTS_HIP(hipMemcpyAsync(qp, coords, C * P * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_NUTS_HIP(hipMemcpyAsync(n->vec + (size_t)DL_NUTS_V_QN * C * P, coords, C * P * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_NUTS_HIP(hipMemcpyAsync(n->iter, it.data(), C * sizeof(long long), hipMemcpyHostToDevice, stream));
    DL_NUTS_HIP(hipMemsetAsync(n->isc + DL_NUTS_I_ACTIVE * C, 0, C * sizeof(int32_t), stream));
    // log-posterior and gradient of the starting points: the proposal the first trajectory starts from
    if (dl_nuts_gradient(n, qp, stream)) return 1;
    std::vector<double> lp(C);
    DL_NUTS_HIP(hipMemcpyAsync(lp.data(), n->lp, C * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_NUTS_HIP(hipStreamSynchronize(stream));
    for (size_t c = 0; c < C; ++c) {
        lp[c] = logposterior ? logposterior[c] : lp[c] + n->offset;
        if (!std::isfinite(lp[c])) return fail("dl_nuts_set_state: the log-posterior of starting position " + std::to_string(c) + " is not finite");
    }
    DL_NUTS_HIP(hipMemcpyAsync(n->dsc + DL_NUTS_D_LPP * C, lp.data(), C * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_NUTS_HIP(hipMemcpyAsync(n->vec + (size_t)DL_NUTS_V_GP * C * P, n->grad, C * P * sizeof(double), hipMemcpyDeviceToDevice, stream));
    DL_NUTS_HIP(hipStreamSynchronize(stream));
    n->have_state = true;
    return 0;
}

int dl_nuts_get_state(dl_nuts* n, double* coords, double* logposterior, int64_t* iteration_counters, double* log_step_size, void* hip_stream) {
    if (!n) return fail("dl_nuts_get_state: null sampler");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t C = n->C, P = n->P;
    DL_NUTS_HIP(hipSetDevice(n->device));
    if (coords) DL_NUTS_HIP(hipMemcpyAsync(coords, n->vec + (size_t)DL_NUTS_V_QP * C * P, C * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (logposterior) DL_NUTS_HIP(hipMemcpyAsync(logposterior, n->dsc + DL_NUTS_D_LPP * C, C * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (iteration_counters) DL_NUTS_HIP(hipMemcpyAsync(iteration_counters, n->iter, C * sizeof(long long), hipMemcpyDeviceToHost, stream));
    if (log_step_size) DL_NUTS_HIP(hipMemcpyAsync(log_step_size, n->dsc + DL_NUTS_D_LOGBAR * C, C * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_NUTS_HIP(hipStreamSynchronize(stream));
    return 0;
}

int dl_nuts_set_adaptation(dl_nuts* n, int32_t enabled, double target_acceptance, double initial_log_step_size, void* hip_stream) {
    if (!n) return fail("dl_nuts_set_adaptation: null sampler");
    n->adapt = enabled != 0;
    if (!n->adapt) return 0;
    if (!(target_acceptance > 0. && target_acceptance < 1.) || !std::isfinite(initial_log_step_size)) return fail("dl_nuts_set_adaptation: invalid target or step size");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t C = n->C;
    n->target = target_acceptance;
    // per chain: log eps = log eps_bar = initial, mu = log(10 eps), hbar = 0, count = 0
    std::vector<double> init(C, initial_log_step_size), mu(C, std::log(10.) + initial_log_step_size);
    DL_NUTS_HIP(hipSetDevice(n->device));
    DL_NUTS_HIP(hipMemcpyAsync(n->dsc + DL_NUTS_D_LOGEPS * C, init.data(), C * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_NUTS_HIP(hipMemcpyAsync(n->dsc + DL_NUTS_D_LOGBAR * C, init.data(), C * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_NUTS_HIP(hipMemcpyAsync(n->dsc + DL_NUTS_D_MU * C, mu.data(), C * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_NUTS_HIP(hipMemsetAsync(n->dsc + DL_NUTS_D_HBAR * C, 0, C * sizeof(double), stream));
    DL_NUTS_HIP(hipMemsetAsync(n->dsc + DL_NUTS_D_DACOUNT * C, 0, C * sizeof(double), stream));
    DL_NUTS_HIP(hipStreamSynchronize(stream));
    return 0;
}

int dl_nuts_run(dl_nuts* n, int64_t nsteps, int32_t quota, int32_t thin_by, double* out_coords_dev, double* out_logp_dev, double* out_info_dev, int32_t* out_count_dev,
                void* hip_stream) {
    if (!n) return fail("dl_nuts_run: null sampler");
    if (nsteps < 0 || quota < 1 || thin_by < 1) return fail("dl_nuts_run: invalid argument");
    if (!out_coords_dev || !out_logp_dev || !out_info_dev || !out_count_dev) return fail("dl_nuts_run: the record buffers are required");
    if (!n->have_mass) return fail("dl_nuts_run: no inverse mass matrix (dl_nuts_set_mass)");
    if (!n->have_state) return fail("dl_nuts_run: no state (dl_nuts_set_state)");
    hipStream_t stream = (hipStream_t)hip_stream;
    DL_NUTS_HIP(hipSetDevice(n->device));
    DlNutsArgs a = dl_nuts_args(n);
    a.out_coords = out_coords_dev; a.out_logp = out_logp_dev; a.out_info = out_info_dev; a.out_count = out_count_dev;
    a.cap = quota; a.quota = quota; a.thin_by = thin_by;
    const unsigned grid = (unsigned)((n->C + DL_NUTS_WAVES - 1) / DL_NUTS_WAVES);
    const double* qn = n->vec + (size_t)DL_NUTS_V_QN * n->C * n->P;
    hipLaunchKernelGGL(dl_nuts_step_kernel, dim3(grid), dim3(64 * DL_NUTS_WAVES), 0, stream, a, 0);     // chains waiting at a boundary start
    for (int64_t s = 0; s < nsteps; ++s) {
        if (dl_nuts_gradient(n, qn, stream)) return 1;
        hipLaunchKernelGGL(dl_nuts_step_kernel, dim3(grid), dim3(64 * DL_NUTS_WAVES), 0, stream, a, 1);
    }
    DL_NUTS_HIP(hipGetLastError());
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
    if (k == "finite") return n->finite ? 1 : 0;
    if (k == "dense") return n->dense ? 1 : 0;
    if (k == "adapt") return n->adapt ? 1 : 0;
    return -1;
}

}  // extern "C"
