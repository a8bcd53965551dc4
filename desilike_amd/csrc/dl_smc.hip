// dl_smc.hip -- device-resident tempered sequential Monte Carlo with log-evidence (include/desilike_amd.h, dl_smc_*; the algorithm, the sums and the draws: dl_smc.h).
//
// One iteration of all K systems is a fixed sequence of launches -- the host never reads beta to decide what to enqueue, nothing synchronises or allocates:
//
//     dl_smc_temper_kernel     a workgroup per system, L in LDS: the ESS at 1 - beta, the 64 bisection reductions, the evidence, the normalised weights W
//     dl_smc_moments_kernel    a workgroup per (system, row of the covariance): the mean, then the row's lower triangle, wavefront partials added in index order
//     dl_smc_cholesky_kernel   a wavefront per system: the factor C, or its diagonal fallback
//     dl_smc_resample_kernel   a workgroup per system: prefix sums of W, the ancestors by binary search, the gather into the second particle buffer
//     n_steps x [ dl_smc_propose_kernel  ->  dl_eval_batch on the K N proposals  ->  dl_smc_accept_kernel ]      a wavefront per particle, a lane per component
//     dl_smc_finish_kernel     a thread per system: the last scale update, the record, the counters
//
// A system at beta = 1 (a sweep) leaves the moments and Cholesky kernels at once and copies in the resample kernel: every system gathers or copies, so the host flips
// the two particle buffers once per iteration.  The scale of sweep j is computed in the prologue of its propose kernel, by every wavefront, from the integer count of
// sweep j - 1 (order-independent); the accept kernel is not fused with the next propose kernel: the evaluation of the proposals lies between them either way.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/desilike_amd.h"
#include "dl_sampler_dev.h"   // DlWave, DlBlock, dl_fail, DL_HIP_CHECK, dl_dev_alloc / free
#include "dl_smc.h"

#define DL_SMC_WAVES 4    // particles per workgroup of the propose and accept kernels

struct dl_smc {
    dl_ctx* ctx = nullptr;
    int device = 0;
    int K = 0, N = 0, P = 0, n_steps = 0, cur = 0;
    bool have_hyper = false, have_state = false;
    double offset = 0., ess_fraction = 0.5, target_acceptance = 0.234;
    uint64_t seed = 0;
    int64_t iterations = 0, evaluations = 0;
    std::vector<int32_t> ids;
    // device
    double *x[2] = {nullptr, nullptr}, *L[2] = {nullptr, nullptr}, *pi[2] = {nullptr, nullptr};
    double *beta = nullptr, *logz = nullptr, *scale = nullptr, *W = nullptr, *cum = nullptr, *mean = nullptr, *cov = nullptr, *chol = nullptr, *widths = nullptr, *tmp = nullptr;
    double *prop = nullptr, *Lp = nullptr, *pip = nullptr, *sscale = nullptr;
    int32_t *sys_ids = nullptr, *anc = nullptr, *mode = nullptr, *status = nullptr, *acc = nullptr;
    uint8_t* flags = nullptr;
    long long* iter = nullptr;
};

namespace {

__global__ __launch_bounds__(DL_SMC_THREADS) void dl_smc_temper_kernel(DlSmcArgs a) {
    __shared__ double Ls[DL_SMC_MAX_N];
    __shared__ double red[2 * DL_SMC_THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x, K = a.K, N = a.N;
    const bool rest = a.out_count[2 * k] >= a.quota;
    const double beta = a.beta[k];
    const double* L = a.L[a.cur] + (size_t)k * N;
    for (int i = tid; i < N; i += DL_SMC_THREADS) Ls[i] = L[i];
    for (int j = tid; j < a.n_steps; j += DL_SMC_THREADS) a.acc[(size_t)k * a.n_steps + j] = 0;
    __syncthreads();
    if (rest) {
        if (tid == 0) a.mode[k] = DL_SMC_REST;
        return;
    }
    const DlBlock g{tid, DL_SMC_THREADS, red};
    DlSmcLevel t;
    dl_smc_temper(g, Ls, N, beta, a.ess_fraction, &t);
    const bool temper = t.delta > 0.;
    if (temper) {
        double* W = a.W + (size_t)k * N;
        for (int i = tid; i < N; i += DL_SMC_THREADS) W[i] = dl_smc_weight(Ls[i], t.lmax, t.delta) / t.sumw;
    }
    if (tid == 0) {
        a.mode[k] = temper ? DL_SMC_TEMPER : DL_SMC_SWEEP;
        a.tmp[DL_SMC_T_DELTA * K + k] = t.delta; a.tmp[DL_SMC_T_ESS * K + k] = t.ess; a.tmp[DL_SMC_T_BETA0 * K + k] = beta;
        if (temper) { a.beta[k] = t.beta; a.logz[k] += t.dlogz; }
    }
}

__global__ __launch_bounds__(64 * DL_SMC_MOMENT_WAVES) void dl_smc_moments_kernel(DlSmcArgs a) {
    const int k = blockIdx.x, row = blockIdx.y, N = a.N, P = a.P;
    if (a.mode[k] != DL_SMC_TEMPER) return;      // (the whole workgroup)
    dl_pop_moments_row(a, a.x[a.cur] + (size_t)k * N * P, a.W + (size_t)k * N, N, k, row);
}

__global__ __launch_bounds__(64) void dl_smc_cholesky_kernel(DlSmcArgs a) {
    const int k = blockIdx.x, P = a.P;
    if (a.mode[k] != DL_SMC_TEMPER) return;
    dl_pop_cholesky(P, a.cov + (size_t)k * P * P, a.widths, a.chol + (size_t)k * P * P);
}

__global__ __launch_bounds__(DL_SMC_THREADS) void dl_smc_resample_kernel(DlSmcArgs a) {
    __shared__ double tot[DL_SMC_THREADS];
    __shared__ double gtot[DL_SMC_THREADS / DL_SMC_GROUP];
    const int k = blockIdx.x, tid = threadIdx.x, N = a.N, P = a.P, T = DL_SMC_THREADS;
    int32_t* anc = a.anc + (size_t)k * N;
    if (a.mode[k] == DL_SMC_TEMPER) {
        const double* W = a.W + (size_t)k * N;
        double* cum = a.cum + (size_t)k * N;
        dl_smc_scan_slices(tid, T, W, N, cum, tot);
        __syncthreads();
        dl_smc_scan_groups(tid, T, tot, gtot);
        __syncthreads();
        dl_smc_scan_top(tid, T, gtot);
        __syncthreads();
        dl_smc_scan_offsets(tid, T, N, cum, tot, gtot);
        __syncthreads();      // (a workgroup's own global stores are visible to it after the barrier)
        const double u = dl_smc_resample_uniform(a.iter[k], (uint32_t)a.sys_ids[k], a.k0, a.k1);
        for (int i = tid; i < N; i += T) anc[i] = dl_smc_ancestor(cum, N, i, u);
    } else
        for (int i = tid; i < N; i += T) anc[i] = i;
    __syncthreads();
    const int from = a.cur, to = 1 - a.cur;
    const double* xs = a.x[from] + (size_t)k * N * P;
    double* xd = a.x[to] + (size_t)k * N * P;
    for (int e = tid; e < N * P; e += T) {
        const int i = e / P, c = e - i * P;
        xd[e] = xs[(size_t)anc[i] * P + c];
    }
    for (int i = tid; i < N; i += T) {
        const size_t s = (size_t)k * N + anc[i], d = (size_t)k * N + i;
        a.L[to][d] = a.L[from][s]; a.pi[to][d] = a.pi[from][s];
    }
}

// (a.cur: the buffer the mutation works in)
__global__ __launch_bounds__(64 * DL_SMC_WAVES) void dl_smc_propose_kernel(DlSmcArgs a, int sweep) {
    const int N = a.N, P = a.P, lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * DL_SMC_WAVES + (threadIdx.x >> 6);
    if (r >= (long long)a.K * N) return;     // (whole wavefronts)
    const int k = (int)(r / N), i = (int)(r - (long long)k * N);
    const DlWave l{P, lane};
    DlNutsVec<DlWave> x, xp;
    dl_nuts_load(l, x, a.x[a.cur] + (size_t)r * P);
    if (a.mode[k] == DL_SMC_REST) {          // its row is evaluated and ignored
        dl_nuts_store(l, x, a.prop + (size_t)r * P);
        return;
    }
    const size_t ks = (size_t)k * a.n_steps;
    const double s = dl_smc_sweep_scale(sweep, a.scale[k], a.sscale + ks, a.acc + ks, N, a.target_acceptance);
    if (i == 0 && lane == 0) a.sscale[ks + sweep] = s;      // (read by later launches only)
    dl_smc_propose(l, a.chol + (size_t)k * P * P, s, x, a.iter[k], sweep, (uint32_t)a.sys_ids[k], i, a.k0, a.k1, xp);
    dl_nuts_store(l, xp, a.prop + (size_t)r * P);
}

__global__ __launch_bounds__(64 * DL_SMC_WAVES) void dl_smc_accept_kernel(DlSmcArgs a, int sweep, int last) {
    const int N = a.N, P = a.P, K = a.K, lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * DL_SMC_WAVES + (threadIdx.x >> 6);
    if (r >= (long long)K * N) return;
    const int k = (int)(r / N), i = (int)(r - (long long)k * N);
    if (a.mode[k] == DL_SMC_REST) return;
    const DlWave l{P, lane};
    double *L = a.L[a.cur] + r, *pi = a.pi[a.cur] + r, *x = a.x[a.cur] + (size_t)r * P;
    const double logu = dl_smc_log_uniform(a.iter[k], sweep, (uint32_t)a.sys_ids[k], i, a.k0, a.k1);
    double Lc = *L, pic = *pi;
    const bool accept = dl_smc_accept(a.beta[k], Lc, pic, a.Lp[r], a.pip[r], a.status[r], logu);
    DlNutsVec<DlWave> v;
    if (accept) {
        dl_nuts_load(l, v, a.prop + (size_t)r * P);
        dl_nuts_store(l, v, x);
        Lc = a.Lp[r]; pic = a.pip[r];
    }
    if (lane == 0) {
        if (accept) { *L = Lc; *pi = pic; atomicAdd(a.acc + (size_t)k * a.n_steps + sweep, 1); }
        a.flags[((size_t)k * a.n_steps + sweep) * N + i] = accept ? 1 : 0;
    }
    if (last && !(a.tmp[DL_SMC_T_BETA0 * K + k] < 1.)) {       // a sweep at beta = 1: the particle is recorded
        const size_t rec = ((size_t)k * a.quota + a.out_count[2 * k + 1]) * N + i;
        if (!accept) dl_nuts_load(l, v, x);
        dl_nuts_store(l, v, a.out_coords + rec * P);
        if (lane == 0) a.out_logp[rec] = Lc + pic + a.offset;
    }
}

__global__ void dl_smc_finish_kernel(DlSmcArgs a) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, K = a.K, N = a.N, n = a.n_steps;
    if (k >= K || a.mode[k] == DL_SMC_REST) return;
    const size_t ks = (size_t)k * n;
    const double s = dl_smc_next_scale(a.sscale[ks + n - 1], (double)a.acc[ks + n - 1] / N, a.target_acceptance);
    long long total = 0;
    for (int j = 0; j < n; ++j) total += a.acc[ks + j];
    const int count = a.out_count[2 * k];
    double* h = a.hist + ((size_t)k * a.quota + count) * DL_SMC_HIST;
    h[0] = a.beta[k]; h[1] = a.logz[k] + a.offset; h[2] = a.tmp[DL_SMC_T_ESS * K + k]; h[3] = (double)total / ((double)n * N); h[4] = s;
    a.scale[k] = s;
    a.iter[k] += 1;
    a.out_count[2 * k] = count + 1;
    if (!(a.tmp[DL_SMC_T_BETA0 * K + k] < 1.)) a.out_count[2 * k + 1] += 1;
}

DlSmcArgs dl_smc_args(const dl_smc* m) {
    DlSmcArgs a;
    std::memset(&a, 0, sizeof(a));
    for (int b = 0; b < 2; ++b) { a.x[b] = m->x[b]; a.L[b] = m->L[b]; a.pi[b] = m->pi[b]; }
    a.beta = m->beta; a.logz = m->logz; a.scale = m->scale; a.iter = m->iter; a.sys_ids = m->sys_ids; a.W = m->W; a.cum = m->cum; a.anc = m->anc;
    a.mean = m->mean; a.cov = m->cov; a.chol = m->chol; a.widths = m->widths; a.tmp = m->tmp; a.mode = m->mode; a.prop = m->prop; a.Lp = m->Lp; a.pip = m->pip;
    a.status = m->status; a.sscale = m->sscale; a.acc = m->acc; a.flags = m->flags;
    a.K = m->K; a.N = m->N; a.P = m->P; a.n_steps = m->n_steps; a.cur = m->cur;
    a.ess_fraction = m->ess_fraction; a.target_acceptance = m->target_acceptance; a.offset = m->offset;
    a.k0 = (uint32_t)m->seed; a.k1 = (uint32_t)(m->seed >> 32);
    return a;
}

}  // namespace

extern "C" {

void dl_smc_destroy(dl_smc* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    dl_dev_free({(void**)&m->sscale, (void**)&m->acc, (void**)&m->flags});
    for (void* p : {(void*)m->x[0], (void*)m->x[1], (void*)m->L[0], (void*)m->L[1], (void*)m->pi[0], (void*)m->pi[1], (void*)m->beta, (void*)m->logz, (void*)m->scale,
                    (void*)m->W, (void*)m->cum, (void*)m->mean, (void*)m->cov, (void*)m->chol, (void*)m->widths, (void*)m->tmp, (void*)m->prop, (void*)m->Lp, (void*)m->pip,
                    (void*)m->sys_ids, (void*)m->anc, (void*)m->mode, (void*)m->status, (void*)m->iter})
        if (p) (void)hipFree(p);
    delete m;
}

int dl_smc_create(dl_smc** out, dl_ctx* ctx, int32_t nsystems, int32_t nparticles, const int32_t* system_ids, uint64_t seed, double offset, const double* widths) {
    if (!out || !ctx || !widths) return dl_fail("dl_smc_create: null argument");
    *out = nullptr;
    const int P = (int)dl_info(ctx, "n_params");
    if (P < 1 || P > DL_SMC_MAX_P) return dl_fail("dl_smc_create: the sampler takes 1 .. 64 parameters, the context has " + std::to_string(P));
    if (nsystems < 1) return dl_fail("dl_smc_create: nsystems must be >= 1");
    if (nparticles < 64 || nparticles > DL_SMC_MAX_N || nparticles % 64) return dl_fail("dl_smc_create: nparticles must be a multiple of 64 between 64 and 16384");
    if (!std::isfinite(offset)) return dl_fail("dl_smc_create: the offset must be finite");
    std::vector<int32_t> ids(nsystems);
    for (int k = 0; k < nsystems; ++k) {
        ids[k] = system_ids ? system_ids[k] : k;
        if (ids[k] < 0) return dl_fail("dl_smc_create: system ids must be non-negative");
    }
    for (int i = 0; i < P; ++i)
        if (!(widths[i] > 0.) || !std::isfinite(widths[i])) return dl_fail("dl_smc_create: the priors' widths must be positive and finite");
    dl_smc* m = new dl_smc();
    m->ctx = ctx; m->device = (int)dl_info(ctx, "device"); m->K = nsystems; m->N = nparticles; m->P = P; m->seed = seed; m->offset = offset; m->ids = ids;
    auto bail = [&](const std::string& msg) { dl_smc_destroy(m); return dl_fail(msg); };
    if (hipSetDevice(m->device) != hipSuccess) return bail("dl_smc_create: hipSetDevice failed");
    const size_t K = nsystems, N = nparticles, p = P;
    bool ok = true;
    for (int b = 0; b < 2; ++b) ok = ok && dl_dev_alloc(&m->x[b], K * N * p) && dl_dev_alloc(&m->L[b], K * N) && dl_dev_alloc(&m->pi[b], K * N);
    ok = ok && dl_dev_alloc(&m->beta, K) && dl_dev_alloc(&m->logz, K) && dl_dev_alloc(&m->scale, K) && dl_dev_alloc(&m->W, K * N) && dl_dev_alloc(&m->cum, K * N) &&
         dl_dev_alloc(&m->mean, K * p) && dl_dev_alloc(&m->cov, K * p * p) && dl_dev_alloc(&m->chol, K * p * p) && dl_dev_alloc(&m->widths, p) &&
         dl_dev_alloc(&m->tmp, (size_t)DL_SMC_NT * K) && dl_dev_alloc(&m->prop, K * N * p) && dl_dev_alloc(&m->Lp, K * N) && dl_dev_alloc(&m->pip, K * N) &&
         dl_dev_alloc(&m->sys_ids, K) && dl_dev_alloc(&m->anc, K * N) && dl_dev_alloc(&m->mode, K) && dl_dev_alloc(&m->status, K * N) && dl_dev_alloc(&m->iter, K);
    if (!ok) return bail("dl_smc_create: device allocation failed");
    ok = hipMemcpy(m->sys_ids, ids.data(), K * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(m->widths, widths, p * sizeof(double), hipMemcpyHostToDevice) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) return bail("dl_smc_create: initialisation of the device arrays failed");
    *out = m;
    return 0;
}

int dl_smc_set_hyper(dl_smc* m, double ess_fraction, int32_t n_steps, double target_acceptance, double scale, void* hip_stream) {
    if (!m) return dl_fail("dl_smc_set_hyper: null sampler");
    if (!(ess_fraction > 0.) || !(ess_fraction < 1.)) return dl_fail("dl_smc_set_hyper: ess_fraction must lie in (0, 1)");
    if (n_steps < 1 || n_steps > DL_SMC_MAX_STEPS) return dl_fail("dl_smc_set_hyper: n_steps must lie in 1 .. 1024");
    if (!(target_acceptance > 0.) || !(target_acceptance < 1.)) return dl_fail("dl_smc_set_hyper: target_acceptance must lie in (0, 1)");
    if (!(scale >= 1e-3) || !(scale <= 1e3)) return dl_fail("dl_smc_set_hyper: scale must lie in 1e-3 .. 1e3");
    hipStream_t stream = (hipStream_t)hip_stream;
    DL_HIP_CHECK(hipSetDevice(m->device));
    const size_t K = m->K, N = m->N;
    if (n_steps != m->n_steps) {
        DL_HIP_CHECK(hipDeviceSynchronize());      // kernels of earlier calls may still use the buffers about to be freed
        dl_dev_free({(void**)&m->sscale, (void**)&m->acc, (void**)&m->flags});
        m->n_steps = 0;
        if (!(dl_dev_alloc(&m->sscale, K * n_steps) && dl_dev_alloc(&m->acc, K * n_steps) && dl_dev_alloc(&m->flags, K * n_steps * N)))
            return dl_fail("dl_smc_set_hyper: device allocation failed");
        DL_HIP_CHECK(hipDeviceSynchronize());
        m->n_steps = n_steps;
    }
    std::vector<double> s(K, scale);
    DL_HIP_CHECK(hipMemcpyAsync(m->scale, s.data(), K * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));   // the host buffer is pageable
    m->ess_fraction = ess_fraction; m->target_acceptance = target_acceptance;
    m->have_hyper = true;
    return 0;
}

int dl_smc_set_particles(dl_smc* m, const double* coords, void* hip_stream) {
    if (!m || !coords) return dl_fail("dl_smc_set_particles: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t K = m->K, N = m->N, P = m->P;
    for (size_t e = 0; e < K * N * P; ++e)
        if (!std::isfinite(coords[e])) return dl_fail("dl_smc_set_particles: the particles must be finite");
    m->have_state = false;
    DL_HIP_CHECK(hipSetDevice(m->device));
    DL_HIP_CHECK(hipMemcpyAsync(m->x[0], coords, K * N * P * sizeof(double), hipMemcpyHostToDevice, stream));
    if (dl_eval_batch(m->ctx, m->x[0], (int64_t)(K * N), m->L[0], m->pi[0], nullptr, m->status, nullptr, stream)) return 1;
    std::vector<double> L(K * N), pi(K * N);
    std::vector<int32_t> status(K * N);
    DL_HIP_CHECK(hipMemcpyAsync(L.data(), m->L[0], K * N * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipMemcpyAsync(pi.data(), m->pi[0], K * N * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipMemcpyAsync(status.data(), m->status, K * N * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    m->evaluations += (int64_t)(K * N);
    for (size_t k = 0; k < K; ++k) {
        size_t live = 0;
        for (size_t i = 0; i < N; ++i) {
            const size_t r = k * N + i;
            if (!std::isfinite(pi[r]))
                return dl_fail("dl_smc_set_particles: particle " + std::to_string(i) + " of system " + std::to_string(k) + " lies outside the prior (its log-prior is not finite)");
            if (status[r] != 0 || !std::isfinite(L[r])) L[r] = -HUGE_VAL;      // a dead particle: weight 0 at every temperature
            else ++live;
        }
        if (!live) return dl_fail("dl_smc_set_particles: no particle of system " + std::to_string(k) + " has a finite log-likelihood");
    }
    DL_HIP_CHECK(hipMemcpyAsync(m->L[0], L.data(), K * N * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemsetAsync(m->beta, 0, K * sizeof(double), stream));
    DL_HIP_CHECK(hipMemsetAsync(m->logz, 0, K * sizeof(double), stream));
    DL_HIP_CHECK(hipMemsetAsync(m->iter, 0, K * sizeof(long long), stream));
    DL_HIP_CHECK(hipMemsetAsync(m->chol, 0, K * P * P * sizeof(double), stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    m->cur = 0; m->iterations = 0;
    m->have_state = true;
    return 0;
}

int dl_smc_set_state(dl_smc* m, const double* coords, const double* loglike, const double* logprior, const double* beta, const double* logz, const int64_t* counters,
                     const double* scale, const double* factor, void* hip_stream) {
    if (!m || !coords || !loglike || !logprior || !beta || !logz || !counters || !scale || !factor) return dl_fail("dl_smc_set_state: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t K = m->K, N = m->N, P = m->P;
    std::vector<long long> it(K);
    for (size_t k = 0; k < K; ++k) {
        if (!(beta[k] >= 0.) || !(beta[k] <= 1.)) return dl_fail("dl_smc_set_state: beta must lie in 0 .. 1");
        if (counters[k] < 0) return dl_fail("dl_smc_set_state: negative iteration counter");
        if (!(scale[k] >= 1e-3) || !(scale[k] <= 1e3)) return dl_fail("dl_smc_set_state: scale must lie in 1e-3 .. 1e3");
        if (!std::isfinite(logz[k])) return dl_fail("dl_smc_set_state: logz must be finite");
        it[k] = counters[k];
    }
    for (size_t e = 0; e < K * N * P; ++e)
        if (!std::isfinite(coords[e])) return dl_fail("dl_smc_set_state: the particles must be finite");
    for (size_t e = 0; e < K * N; ++e)
        if (!std::isfinite(logprior[e]) || std::isnan(loglike[e]) || loglike[e] == HUGE_VAL) return dl_fail("dl_smc_set_state: log-priors must be finite, log-likelihoods finite or -inf");
    for (size_t e = 0; e < K * P * P; ++e)
        if (!std::isfinite(factor[e])) return dl_fail("dl_smc_set_state: the factor must be finite");
    DL_HIP_CHECK(hipSetDevice(m->device));
    DL_HIP_CHECK(hipMemcpyAsync(m->x[0], coords, K * N * P * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->L[0], loglike, K * N * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->pi[0], logprior, K * N * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->beta, beta, K * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->logz, logz, K * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->iter, it.data(), K * sizeof(long long), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->scale, scale, K * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->chol, factor, K * P * P * sizeof(double), hipMemcpyHostToDevice, stream));
    // the workspaces of the context sized for the K N rows of a sweep before dl_smc_run (which does not allocate): one evaluation of the particles, results unused
    if (dl_eval_batch(m->ctx, m->x[0], (int64_t)(K * N), m->Lp, m->pip, nullptr, m->status, nullptr, stream)) return 1;
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    m->evaluations += (int64_t)(K * N);
    m->cur = 0;
    m->have_state = true;
    return 0;
}

int dl_smc_get_state(dl_smc* m, double* coords, double* loglike, double* logprior, double* beta, double* logz, int64_t* counters, double* scale, double* factor,
                     void* hip_stream) {
    if (!m) return dl_fail("dl_smc_get_state: null sampler");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t K = m->K, N = m->N, P = m->P;
    const int c = m->cur;
    DL_HIP_CHECK(hipSetDevice(m->device));
    if (coords) DL_HIP_CHECK(hipMemcpyAsync(coords, m->x[c], K * N * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (loglike) DL_HIP_CHECK(hipMemcpyAsync(loglike, m->L[c], K * N * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (logprior) DL_HIP_CHECK(hipMemcpyAsync(logprior, m->pi[c], K * N * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (beta) DL_HIP_CHECK(hipMemcpyAsync(beta, m->beta, K * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (logz) DL_HIP_CHECK(hipMemcpyAsync(logz, m->logz, K * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (counters) DL_HIP_CHECK(hipMemcpyAsync(counters, m->iter, K * sizeof(long long), hipMemcpyDeviceToHost, stream));
    if (scale) DL_HIP_CHECK(hipMemcpyAsync(scale, m->scale, K * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (factor) DL_HIP_CHECK(hipMemcpyAsync(factor, m->chol, K * P * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int dl_smc_get_decisions(dl_smc* m, int32_t* ancestors, uint8_t* accepts, double* mean, double* covariance, void* hip_stream) {
    if (!m) return dl_fail("dl_smc_get_decisions: null sampler");
    if (!m->n_steps) return dl_fail("dl_smc_get_decisions: no hyper-parameters (dl_smc_set_hyper)");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t K = m->K, N = m->N, P = m->P;
    DL_HIP_CHECK(hipSetDevice(m->device));
    if (ancestors) DL_HIP_CHECK(hipMemcpyAsync(ancestors, m->anc, K * N * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (accepts) DL_HIP_CHECK(hipMemcpyAsync(accepts, m->flags, K * m->n_steps * N, hipMemcpyDeviceToHost, stream));
    if (mean) DL_HIP_CHECK(hipMemcpyAsync(mean, m->mean, K * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (covariance) DL_HIP_CHECK(hipMemcpyAsync(covariance, m->cov, K * P * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int dl_smc_run(dl_smc* m, int64_t niterations, int32_t quota, double* history_dev, double* coords_dev, double* logp_dev, int32_t* count_dev, void* hip_stream) {
    if (!m) return dl_fail("dl_smc_run: null sampler");
    if (niterations < 0 || quota < 1) return dl_fail("dl_smc_run: invalid argument");
    if (!history_dev || !coords_dev || !logp_dev || !count_dev) return dl_fail("dl_smc_run: the record buffers are required");
    if (!m->have_hyper) return dl_fail("dl_smc_run: no hyper-parameters (dl_smc_set_hyper)");
    if (!m->have_state) return dl_fail("dl_smc_run: no particles (dl_smc_set_particles or dl_smc_set_state)");
    if (!niterations) return 0;
    hipStream_t stream = (hipStream_t)hip_stream;
    DL_HIP_CHECK(hipSetDevice(m->device));
    DlSmcArgs a = dl_smc_args(m);
    a.hist = history_dev; a.out_coords = coords_dev; a.out_logp = logp_dev; a.out_count = count_dev; a.quota = quota;
    const int K = m->K, P = m->P;
    const int64_t rows = (int64_t)K * m->N;
    const unsigned pgrid = (unsigned)((rows + DL_SMC_WAVES - 1) / DL_SMC_WAVES);
    for (int64_t it = 0; it < niterations; ++it) {
        a.cur = m->cur;
        hipLaunchKernelGGL(dl_smc_temper_kernel, dim3(K), dim3(DL_SMC_THREADS), 0, stream, a);
        hipLaunchKernelGGL(dl_smc_moments_kernel, dim3(K, P), dim3(64 * DL_SMC_MOMENT_WAVES), 0, stream, a);
        hipLaunchKernelGGL(dl_smc_cholesky_kernel, dim3(K), dim3(64), 0, stream, a);
        hipLaunchKernelGGL(dl_smc_resample_kernel, dim3(K), dim3(DL_SMC_THREADS), 0, stream, a);
        m->cur = 1 - m->cur;
        a.cur = m->cur;
        for (int j = 0; j < m->n_steps; ++j) {
            hipLaunchKernelGGL(dl_smc_propose_kernel, dim3(pgrid), dim3(64 * DL_SMC_WAVES), 0, stream, a, j);
            if (dl_eval_batch(m->ctx, m->prop, rows, m->Lp, m->pip, nullptr, m->status, nullptr, stream)) return 1;
            hipLaunchKernelGGL(dl_smc_accept_kernel, dim3(pgrid), dim3(64 * DL_SMC_WAVES), 0, stream, a, j, j + 1 == m->n_steps ? 1 : 0);
        }
        hipLaunchKernelGGL(dl_smc_finish_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, stream, a);
        m->evaluations += rows * m->n_steps;
    }
    DL_HIP_CHECK(hipGetLastError());
    m->iterations += niterations;
    return 0;
}

int64_t dl_smc_info(const dl_smc* m, const char* key) {
    if (!m || !key) return -1;
    const std::string k(key);
    if (k == "nsystems") return m->K;
    if (k == "nparticles") return m->N;
    if (k == "n_params") return m->P;
    if (k == "iterations") return m->iterations;
    if (k == "evaluations") return m->evaluations;
    if (k == "n_steps") return m->n_steps;
    return -1;
}

}  // extern "C"
