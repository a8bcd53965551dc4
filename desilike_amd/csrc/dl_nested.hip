// dl_nested.hip -- device-resident batched nested sampling (include/desilike_amd.h, dl_nested_*; the algorithm, the sums and the draws: dl_nested.h).
//
// One iteration of all K runs is a fixed sequence of launches -- the host never reads a mode to decide what to enqueue, nothing synchronises or allocates:
//
//     dl_nested_rank_kernel       a workgroup per run: the bitonic sort of (key of L, slot) in LDS, the survivors' weights and first slot, the prefix sums of
//                                 1 / (N - j), log w of the dead, the evidence update
//     dl_nested_moments_kernel    a workgroup per (run, row of the covariance): the survivors' mean, then the row's lower triangle (dl_smc_moment_partial)
//     dl_nested_cholesky_kernel   a wavefront per run: the factor C, or its diagonal fallback (dl_smc_factor)
//     dl_nested_seed_kernel       a wavefront per dead point: its record, then x, L, pi of its seed gathered into its slot
//     n_steps x [ dl_nested_propose_kernel  ->  dl_eval_batch on the K M proposals  ->  dl_nested_accept_kernel ]      a wavefront per replaced point, a lane per component
//     dl_nested_finish_kernel     a workgroup per run: log Z_rem over the new live set, the last scale update, the record, the mode
//
// LDS of the rank kernel: 8192 keys (65536 bytes) + 8192 slots (32768) + 4096 prefix sums (32768) + the scan's 1024 thread totals (8192) and 32 group totals (256) +
// the reduction scratch (256 + 64) = 139840 bytes of the 163840 of a CU: N <= 8192.  The evidence shares the rank kernel's launch (the sorted slots are in LDS there).
// Only survivors are read and only dead slots are written by the seed kernel, only a wavefront's own slot by the accept kernel: the live points need no second buffer.
// A run at rest leaves every kernel at once; its rows of the proposal batch are evaluated and ignored.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/desilike_amd.h"
#include "dl_sampler_dev.h"   // DlWave, DlBlock, dl_fail, DL_HIP_CHECK, dl_dev_alloc / free
#include "dl_nested.h"

static_assert(DL_NESTED_MAX_P == DL_SMC_MAX_P, "dl_pop_cholesky holds a DL_SMC_MAX_P square in LDS");

#define DL_NESTED_WAVES 4    // points per workgroup of the seed, propose and accept kernels

struct dl_nested {
    dl_ctx* ctx = nullptr;
    int device = 0;
    int K = 0, N = 0, P = 0, M = 0, n_steps = 0;
    bool have_hyper = false, have_state = false;
    double offset = 0., target_acceptance = 0.234, dlogz = 0.01;
    uint64_t seed = 0;
    int64_t iterations = 0, evaluations = 0;
    std::vector<int32_t> ids;
    // device
    double *x = nullptr, *L = nullptr, *pi = nullptr, *logx = nullptr, *logz = nullptr, *scale = nullptr, *W = nullptr, *logw = nullptr, *mean = nullptr, *cov = nullptr,
           *chol = nullptr, *widths = nullptr, *tmp = nullptr, *prop = nullptr, *Lp = nullptr, *pip = nullptr, *sscale = nullptr;
    int32_t *sys_ids = nullptr, *mode = nullptr, *active = nullptr, *rank = nullptr, *seeds = nullptr, *first = nullptr, *status = nullptr, *acc = nullptr;
    uint8_t* flags = nullptr;
    long long* iter = nullptr;
};

namespace {

__global__ __launch_bounds__(DL_NESTED_THREADS) void dl_nested_rank_kernel(DlNestedArgs a) {
    __shared__ uint64_t keys[DL_NESTED_MAX_N];
    __shared__ int32_t slots[DL_NESTED_MAX_N];
    __shared__ double cum[DL_NESTED_MAX_M];
    __shared__ double tot[DL_NESTED_THREADS];
    __shared__ double gtot[DL_NESTED_THREADS / DL_SMC_GROUP];
    __shared__ double red[2 * DL_NESTED_THREADS / 64];
    __shared__ int32_t firsts[DL_NESTED_THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x, K = a.K, N = a.N, M = a.M, T = DL_NESTED_THREADS;
    for (int j = tid; j < a.n_steps; j += T) a.acc[(size_t)k * a.n_steps + j] = 0;
    const bool active = a.mode[k] != DL_NESTED_REST && a.out_count[k] < a.quota;      // (the whole workgroup)
    if (tid == 0) a.active[k] = active ? 1 : 0;
    if (!active) return;
    const double* L = a.L + (size_t)k * N;
    const int n2 = dl_nested_pow2(N);
    dl_nested_load_keys(tid, T, L, N, n2, keys, slots);
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            dl_nested_bitonic_stage(tid, T, keys, slots, n2, size, stride);
            __syncthreads();
        }
    // the ranks, the survivors' weights and the first survivor in slot order
    const double w = 1. / (double)(N - M);
    int f = N;
    for (int r = tid; r < N; r += T) {
        const int s = slots[r];
        a.rank[(size_t)k * N + r] = s;
        a.W[(size_t)k * N + s] = r >= M ? w : 0.;
        if (r >= M && s < f) f = s;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(f, off, 64); f = o < f ? o : f; }
    if ((tid & 63) == 0) firsts[tid >> 6] = f;
    // the prefix sums of 1 / (N - j)
    dl_nested_scan_slices(tid, T, N, M, cum, tot);
    __syncthreads();
    dl_smc_scan_groups(tid, T, tot, gtot);
    __syncthreads();
    dl_smc_scan_top(tid, T, gtot);
    __syncthreads();
    dl_smc_scan_offsets(tid, T, M, cum, tot, gtot);
    __syncthreads();
    const DlBlock g{tid, T, red};
    const double logx = a.logx[k], logz = a.logz[k];
    DlNestedLevel t;
    dl_nested_evidence(g, L, slots, cum, N, M, logx, logz, &t);
    for (int j = tid; j < M; j += T) a.logw[(size_t)k * M + j] = dl_nested_logw(logx, cum, N, j);
    if (tid == 0) {
        for (int v = 0; v < T / 64; ++v) f = firsts[v] < f ? firsts[v] : f;
        a.first[k] = f;
        a.tmp[DL_NESTED_T_LSTAR * K + k] = t.lstar;
        a.logx[k] = t.logx; a.logz[k] = t.logz;
    }
}

__global__ __launch_bounds__(64 * DL_SMC_MOMENT_WAVES) void dl_nested_moments_kernel(DlNestedArgs a) {
    const int k = blockIdx.x, row = blockIdx.y;
    if (!a.active[k]) return;      // (the whole workgroup)
    const int first = a.first[k], N = a.N - first;
    const double *x = a.x + ((size_t)k * a.N + first) * a.P, *W = a.W + (size_t)k * a.N + first;
    dl_pop_moments_row(a, x, W, N, k, row);
}

__global__ __launch_bounds__(64) void dl_nested_cholesky_kernel(DlNestedArgs a) {
    const int k = blockIdx.x, P = a.P;
    if (!a.active[k]) return;
    dl_pop_cholesky(P, a.cov + (size_t)k * P * P, a.widths, a.chol + (size_t)k * P * P);
}

__global__ __launch_bounds__(64 * DL_NESTED_WAVES) void dl_nested_seed_kernel(DlNestedArgs a) {
    const int N = a.N, M = a.M, P = a.P, lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * DL_NESTED_WAVES + (threadIdx.x >> 6);
    if (r >= (long long)a.K * M) return;     // (whole wavefronts)
    const int k = (int)(r / M), j = (int)(r - (long long)k * M);
    if (!a.active[k]) return;
    const DlWave l{P, lane};
    const int32_t* rank = a.rank + (size_t)k * N;
    const int dead = rank[j];
    const int src = rank[dl_nested_seed_rank(dl_nested_seed_uniform(a.iter[k], (uint32_t)a.sys_ids[k], j, a.k0, a.k1), N, M)];
    const size_t d = (size_t)k * N + dead, s = (size_t)k * N + src, rec = ((size_t)k * a.quota + a.out_count[k]) * M + j;
    DlNutsVec<DlWave> v;
    dl_nuts_load(l, v, a.x + d * P);
    dl_nuts_store(l, v, a.out_coords + rec * P);
    dl_nuts_load(l, v, a.x + s * P);
    dl_nuts_store(l, v, a.x + d * P);
    if (lane == 0) {
        a.out_L[rec] = a.L[d]; a.out_pi[rec] = a.pi[d]; a.out_logw[rec] = a.logw[r];
        a.L[d] = a.L[s]; a.pi[d] = a.pi[s];
        a.seeds[r] = src;
    }
}

__global__ __launch_bounds__(64 * DL_NESTED_WAVES) void dl_nested_propose_kernel(DlNestedArgs a, int sweep) {
    const int N = a.N, M = a.M, P = a.P, lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * DL_NESTED_WAVES + (threadIdx.x >> 6);
    if (r >= (long long)a.K * M) return;     // (whole wavefronts)
    const int k = (int)(r / M), j = (int)(r - (long long)k * M);
    const DlWave l{P, lane};
    DlNutsVec<DlWave> x, xp;
    dl_nuts_load(l, x, a.x + ((size_t)k * N + a.rank[(size_t)k * N + j]) * P);      // (a run at rest: the slot of its last iteration, or slot 0)
    if (!a.active[k]) {                      // its row is evaluated and ignored
        dl_nuts_store(l, x, a.prop + (size_t)r * P);
        return;
    }
    const size_t ks = (size_t)k * a.n_steps;
    const double s = dl_smc_sweep_scale(sweep, a.scale[k], a.sscale + ks, a.acc + ks, M, a.target_acceptance);
    if (j == 0 && lane == 0) a.sscale[ks + sweep] = s;      // (read by later launches only)
    dl_nested_propose(l, a.chol + (size_t)k * P * P, s, x, a.iter[k], sweep, (uint32_t)a.sys_ids[k], j, a.k0, a.k1, xp);
    dl_nuts_store(l, xp, a.prop + (size_t)r * P);
}

__global__ __launch_bounds__(64 * DL_NESTED_WAVES) void dl_nested_accept_kernel(DlNestedArgs a, int sweep) {
    const int N = a.N, M = a.M, P = a.P, K = a.K, lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * DL_NESTED_WAVES + (threadIdx.x >> 6);
    if (r >= (long long)K * M) return;
    const int k = (int)(r / M), j = (int)(r - (long long)k * M);
    if (!a.active[k]) return;
    const DlWave l{P, lane};
    const size_t d = (size_t)k * N + a.rank[(size_t)k * N + j];
    const double logu = dl_nested_log_uniform(a.iter[k], sweep, (uint32_t)a.sys_ids[k], j, a.k0, a.k1);
    const bool accept = dl_nested_accept(a.tmp[DL_NESTED_T_LSTAR * K + k], a.pi[d], a.Lp[r], a.pip[r], a.status[r], logu);
    if (accept) {
        DlNutsVec<DlWave> v;
        dl_nuts_load(l, v, a.prop + (size_t)r * P);
        dl_nuts_store(l, v, a.x + d * P);
    }
    if (lane == 0) {
        if (accept) { a.L[d] = a.Lp[r]; a.pi[d] = a.pip[r]; atomicAdd(a.acc + (size_t)k * a.n_steps + sweep, 1); }
        a.flags[((size_t)k * a.n_steps + sweep) * M + j] = accept ? 1 : 0;
    }
}

__global__ __launch_bounds__(DL_NESTED_THREADS) void dl_nested_finish_kernel(DlNestedArgs a) {
    __shared__ double red[2 * DL_NESTED_THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x, K = a.K, N = a.N, M = a.M, n = a.n_steps;
    if (!a.active[k]) {      // (the whole workgroup)
        if (tid == 0) a.out_mode[k] = a.mode[k];
        return;
    }
    const DlBlock g{tid, DL_NESTED_THREADS, red};
    const double logx = a.logx[k], logz = a.logz[k];
    const double rem = dl_nested_remaining(g, a.L + (size_t)k * N, N, logx);
    if (tid != 0) return;
    const size_t ks = (size_t)k * n;
    const double s = dl_smc_next_scale(a.sscale[ks + n - 1], (double)a.acc[ks + n - 1] / M, a.target_acceptance);
    long long total = 0;
    for (int j = 0; j < n; ++j) total += a.acc[ks + j];
    const int count = a.out_count[k];
    double* h = a.hist + ((size_t)k * a.quota + count) * DL_NESTED_HIST;
    h[0] = logx; h[1] = logz + a.offset; h[2] = a.tmp[DL_NESTED_T_LSTAR * K + k]; h[3] = (double)total / ((double)n * M); h[4] = s; h[5] = rem + a.offset;
    const int mode = dl_nested_at_rest(logz, rem, a.dlogz) ? DL_NESTED_REST : DL_NESTED_CLIMB;
    a.scale[k] = s;
    a.iter[k] += 1;
    a.out_count[k] = count + 1;
    a.mode[k] = mode; a.out_mode[k] = mode;
}

DlNestedArgs dl_nested_args(const dl_nested* m) {
    DlNestedArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = m->x; a.L = m->L; a.pi = m->pi; a.logx = m->logx; a.logz = m->logz; a.scale = m->scale; a.iter = m->iter; a.mode = m->mode; a.active = m->active;
    a.sys_ids = m->sys_ids; a.rank = m->rank; a.seeds = m->seeds; a.first = m->first; a.W = m->W; a.logw = m->logw; a.mean = m->mean; a.cov = m->cov; a.chol = m->chol;
    a.widths = m->widths; a.tmp = m->tmp; a.prop = m->prop; a.Lp = m->Lp; a.pip = m->pip; a.status = m->status; a.sscale = m->sscale; a.acc = m->acc; a.flags = m->flags;
    a.K = m->K; a.N = m->N; a.M = m->M; a.P = m->P; a.n_steps = m->n_steps;
    a.target_acceptance = m->target_acceptance; a.dlogz = m->dlogz; a.offset = m->offset;
    a.k0 = (uint32_t)m->seed; a.k1 = (uint32_t)(m->seed >> 32);
    return a;
}

// what dl_nested_set_live and dl_nested_set_state share: the scalars of the runs
int dl_nested_check_live(const char* who, const dl_nested* m, const double* coords, const double* loglike, const double* logprior) {
    const size_t K = m->K, N = m->N, P = m->P;
    if (coords)
        for (size_t e = 0; e < K * N * P; ++e)
            if (!std::isfinite(coords[e])) return dl_fail(std::string(who) + ": the live points must be finite");
    for (size_t e = 0; e < K * N; ++e) {
        if (!std::isfinite(logprior[e]))
            return dl_fail(std::string(who) + ": live point " + std::to_string(e % N) + " of run " + std::to_string(e / N) + " lies outside the prior (its log-prior is not finite)");
        if (!std::isfinite(loglike[e]))
            return dl_fail(std::string(who) + ": live point " + std::to_string(e % N) + " of run " + std::to_string(e / N) + " has no finite log-likelihood");
    }
    return 0;
}

}  // namespace

extern "C" {

void dl_nested_destroy(dl_nested* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    dl_dev_free({(void**)&m->sscale, (void**)&m->acc, (void**)&m->flags});
    for (void* p : {(void*)m->x, (void*)m->L, (void*)m->pi, (void*)m->logx, (void*)m->logz, (void*)m->scale, (void*)m->W, (void*)m->logw, (void*)m->mean, (void*)m->cov,
                    (void*)m->chol, (void*)m->widths, (void*)m->tmp, (void*)m->prop, (void*)m->Lp, (void*)m->pip, (void*)m->sys_ids, (void*)m->mode, (void*)m->active,
                    (void*)m->rank, (void*)m->seeds, (void*)m->first, (void*)m->status, (void*)m->iter})
        if (p) (void)hipFree(p);
    delete m;
}

int dl_nested_create(dl_nested** out, dl_ctx* ctx, int32_t nruns, int32_t nlive, const int32_t* run_ids, uint64_t seed, double offset, const double* widths) {
    if (!out || !ctx || !widths) return dl_fail("dl_nested_create: null argument");
    *out = nullptr;
    const int P = (int)dl_info(ctx, "n_params");
    if (P < 1 || P > DL_NESTED_MAX_P) return dl_fail("dl_nested_create: the sampler takes 1 .. 64 parameters, the context has " + std::to_string(P));
    if (nruns < 1) return dl_fail("dl_nested_create: nruns must be >= 1");
    if (nlive < 64 || nlive > DL_NESTED_MAX_N || nlive % 64) return dl_fail("dl_nested_create: nlive must be a multiple of 64 between 64 and 8192");
    if (!std::isfinite(offset)) return dl_fail("dl_nested_create: the offset must be finite");
    std::vector<int32_t> ids(nruns);
    for (int k = 0; k < nruns; ++k) {
        ids[k] = run_ids ? run_ids[k] : k;
        if (ids[k] < 0) return dl_fail("dl_nested_create: run ids must be non-negative");
    }
    for (int i = 0; i < P; ++i)
        if (!(widths[i] > 0.) || !std::isfinite(widths[i])) return dl_fail("dl_nested_create: the priors' widths must be positive and finite");
    dl_nested* m = new dl_nested();
    m->ctx = ctx; m->device = (int)dl_info(ctx, "device"); m->K = nruns; m->N = nlive; m->P = P; m->seed = seed; m->offset = offset; m->ids = ids;
    auto bail = [&](const std::string& msg) { dl_nested_destroy(m); return dl_fail(msg); };
    if (hipSetDevice(m->device) != hipSuccess) return bail("dl_nested_create: hipSetDevice failed");
    // (the arrays over the replaced points are sized for the largest ndelete, nlive / 2; Lp, pip and status for the nlive rows of dl_nested_set_live)
    const size_t K = nruns, N = nlive, p = P, M = N / 2;
    const bool ok = dl_dev_alloc(&m->x, K * N * p) && dl_dev_alloc(&m->L, K * N) && dl_dev_alloc(&m->pi, K * N) && dl_dev_alloc(&m->logx, K) &&
                    dl_dev_alloc(&m->logz, K) && dl_dev_alloc(&m->scale, K) && dl_dev_alloc(&m->W, K * N) && dl_dev_alloc(&m->logw, K * M) &&
                    dl_dev_alloc(&m->mean, K * p) && dl_dev_alloc(&m->cov, K * p * p) && dl_dev_alloc(&m->chol, K * p * p) && dl_dev_alloc(&m->widths, p) &&
                    dl_dev_alloc(&m->tmp, (size_t)DL_NESTED_NT * K) && dl_dev_alloc(&m->prop, K * M * p) && dl_dev_alloc(&m->Lp, K * N) &&
                    dl_dev_alloc(&m->pip, K * N) && dl_dev_alloc(&m->sys_ids, K) && dl_dev_alloc(&m->mode, K) && dl_dev_alloc(&m->active, K) &&
                    dl_dev_alloc(&m->rank, K * N) && dl_dev_alloc(&m->seeds, K * M) && dl_dev_alloc(&m->first, K) && dl_dev_alloc(&m->status, K * N) &&
                    dl_dev_alloc(&m->iter, K);
    if (!ok) return bail("dl_nested_create: device allocation failed");
    if (!(hipMemcpy(m->sys_ids, ids.data(), K * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess &&
          hipMemcpy(m->widths, widths, p * sizeof(double), hipMemcpyHostToDevice) == hipSuccess && hipDeviceSynchronize() == hipSuccess))
        return bail("dl_nested_create: initialisation of the device arrays failed");
    *out = m;
    return 0;
}

int dl_nested_set_hyper(dl_nested* m, int32_t ndelete, int32_t n_steps, double target_acceptance, double dlogz, double scale, void* hip_stream) {
    if (!m) return dl_fail("dl_nested_set_hyper: null sampler");
    if (ndelete < 1 || ndelete > m->N / 2) return dl_fail("dl_nested_set_hyper: ndelete must lie in 1 .. nlive / 2");
    if (n_steps < 1 || n_steps > DL_NESTED_MAX_STEPS) return dl_fail("dl_nested_set_hyper: n_steps must lie in 1 .. 1024");
    if (!(target_acceptance > 0.) || !(target_acceptance < 1.)) return dl_fail("dl_nested_set_hyper: target_acceptance must lie in (0, 1)");
    if (!(dlogz > 0.) || !(dlogz < 1.)) return dl_fail("dl_nested_set_hyper: dlogz must lie in (0, 1)");
    if (!(scale >= 1e-3) || !(scale <= 1e3)) return dl_fail("dl_nested_set_hyper: scale must lie in 1e-3 .. 1e3");
    hipStream_t stream = (hipStream_t)hip_stream;
    DL_HIP_CHECK(hipSetDevice(m->device));
    const size_t K = m->K, M = m->N / 2;
    if (n_steps != m->n_steps) {
        DL_HIP_CHECK(hipDeviceSynchronize());      // kernels of earlier calls may still use the buffers about to be freed
        dl_dev_free({(void**)&m->sscale, (void**)&m->acc, (void**)&m->flags});
        m->n_steps = 0;
        if (!(dl_dev_alloc(&m->sscale, K * n_steps) && dl_dev_alloc(&m->acc, K * n_steps) && dl_dev_alloc(&m->flags, K * n_steps * M)))
            return dl_fail("dl_nested_set_hyper: device allocation failed");
        DL_HIP_CHECK(hipDeviceSynchronize());
        m->n_steps = n_steps;
    }
    std::vector<double> s(K, scale);
    DL_HIP_CHECK(hipMemcpyAsync(m->scale, s.data(), K * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));   // the host buffer is pageable
    m->M = ndelete; m->target_acceptance = target_acceptance; m->dlogz = dlogz;
    m->have_hyper = true;
    return 0;
}

int dl_nested_set_live(dl_nested* m, const double* coords, void* hip_stream) {
    if (!m || !coords) return dl_fail("dl_nested_set_live: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t K = m->K, N = m->N, P = m->P;
    for (size_t e = 0; e < K * N * P; ++e)
        if (!std::isfinite(coords[e])) return dl_fail("dl_nested_set_live: the live points must be finite");
    m->have_state = false;
    DL_HIP_CHECK(hipSetDevice(m->device));
    DL_HIP_CHECK(hipMemcpyAsync(m->x, coords, K * N * P * sizeof(double), hipMemcpyHostToDevice, stream));
    if (dl_eval_batch(m->ctx, m->x, (int64_t)(K * N), m->L, m->pi, nullptr, m->status, nullptr, stream)) return 1;
    std::vector<double> L(K * N), pi(K * N), logz(K, -HUGE_VAL);
    std::vector<int32_t> status(K * N), mode(K, DL_NESTED_CLIMB);
    DL_HIP_CHECK(hipMemcpyAsync(L.data(), m->L, K * N * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipMemcpyAsync(pi.data(), m->pi, K * N * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipMemcpyAsync(status.data(), m->status, K * N * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    m->evaluations += (int64_t)(K * N);
    for (size_t e = 0; e < K * N; ++e)
        if (status[e] != 0) L[e] = -HUGE_VAL;
    if (dl_nested_check_live("dl_nested_set_live", m, nullptr, L.data(), pi.data())) return 1;
    DL_HIP_CHECK(hipMemsetAsync(m->logx, 0, K * sizeof(double), stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->logz, logz.data(), K * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->mode, mode.data(), K * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemsetAsync(m->iter, 0, K * sizeof(long long), stream));
    DL_HIP_CHECK(hipMemsetAsync(m->rank, 0, K * N * sizeof(int32_t), stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    m->iterations = 0;
    m->have_state = true;
    return 0;
}

int dl_nested_set_state(dl_nested* m, const double* coords, const double* loglike, const double* logprior, const double* logx, const double* logz, const int64_t* counters,
                        const double* scale, const int32_t* modes, void* hip_stream) {
    if (!m || !coords || !loglike || !logprior || !logx || !logz || !counters || !scale || !modes) return dl_fail("dl_nested_set_state: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t K = m->K, N = m->N, P = m->P;
    std::vector<long long> it(K);
    for (size_t k = 0; k < K; ++k) {
        if (!(logx[k] <= 0.) || !std::isfinite(logx[k])) return dl_fail("dl_nested_set_state: logx must be finite and not above 0");
        if (std::isnan(logz[k]) || logz[k] == HUGE_VAL) return dl_fail("dl_nested_set_state: logz must be finite or -inf");
        if (counters[k] < 0) return dl_fail("dl_nested_set_state: negative iteration counter");
        if (!(scale[k] >= 1e-3) || !(scale[k] <= 1e3)) return dl_fail("dl_nested_set_state: scale must lie in 1e-3 .. 1e3");
        if (modes[k] != DL_NESTED_REST && modes[k] != DL_NESTED_CLIMB) return dl_fail("dl_nested_set_state: a mode is 0 (at rest) or 1 (climbing)");
        it[k] = counters[k];
    }
    if (dl_nested_check_live("dl_nested_set_state", m, coords, loglike, logprior)) return 1;
    DL_HIP_CHECK(hipSetDevice(m->device));
    DL_HIP_CHECK(hipMemcpyAsync(m->x, coords, K * N * P * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->L, loglike, K * N * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->pi, logprior, K * N * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->logx, logx, K * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->logz, logz, K * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->iter, it.data(), K * sizeof(long long), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->scale, scale, K * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemcpyAsync(m->mode, modes, K * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipMemsetAsync(m->rank, 0, K * N * sizeof(int32_t), stream));
    // the workspaces of the context sized for the rows of a sweep before dl_nested_run (which does not allocate): one evaluation of the live points, results unused
    if (dl_eval_batch(m->ctx, m->x, (int64_t)(K * N), m->Lp, m->pip, nullptr, m->status, nullptr, stream)) return 1;
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    m->evaluations += (int64_t)(K * N);
    m->have_state = true;
    return 0;
}

int dl_nested_get_state(dl_nested* m, double* coords, double* loglike, double* logprior, double* logx, double* logz, int64_t* counters, double* scale, int32_t* modes,
                        void* hip_stream) {
    if (!m) return dl_fail("dl_nested_get_state: null sampler");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t K = m->K, N = m->N, P = m->P;
    DL_HIP_CHECK(hipSetDevice(m->device));
    if (coords) DL_HIP_CHECK(hipMemcpyAsync(coords, m->x, K * N * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (loglike) DL_HIP_CHECK(hipMemcpyAsync(loglike, m->L, K * N * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (logprior) DL_HIP_CHECK(hipMemcpyAsync(logprior, m->pi, K * N * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (logx) DL_HIP_CHECK(hipMemcpyAsync(logx, m->logx, K * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (logz) DL_HIP_CHECK(hipMemcpyAsync(logz, m->logz, K * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (counters) DL_HIP_CHECK(hipMemcpyAsync(counters, m->iter, K * sizeof(long long), hipMemcpyDeviceToHost, stream));
    if (scale) DL_HIP_CHECK(hipMemcpyAsync(scale, m->scale, K * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (modes) DL_HIP_CHECK(hipMemcpyAsync(modes, m->mode, K * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int dl_nested_get_decisions(dl_nested* m, int32_t* ranks, int32_t* seeds, uint8_t* accepts, double* mean, double* covariance, void* hip_stream) {
    if (!m) return dl_fail("dl_nested_get_decisions: null sampler");
    if (!m->have_hyper) return dl_fail("dl_nested_get_decisions: no hyper-parameters (dl_nested_set_hyper)");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t K = m->K, N = m->N, P = m->P, M = m->M;
    DL_HIP_CHECK(hipSetDevice(m->device));
    if (ranks) DL_HIP_CHECK(hipMemcpyAsync(ranks, m->rank, K * N * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (seeds) DL_HIP_CHECK(hipMemcpyAsync(seeds, m->seeds, K * M * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (accepts) DL_HIP_CHECK(hipMemcpyAsync(accepts, m->flags, K * m->n_steps * M, hipMemcpyDeviceToHost, stream));
    if (mean) DL_HIP_CHECK(hipMemcpyAsync(mean, m->mean, K * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (covariance) DL_HIP_CHECK(hipMemcpyAsync(covariance, m->cov, K * P * P * sizeof(double), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int dl_nested_run(dl_nested* m, int64_t niterations, int32_t quota, double* history_dev, double* coords_dev, double* loglike_dev, double* logprior_dev, double* logweight_dev,
                  int32_t* count_dev, int32_t* mode_dev, void* hip_stream) {
    if (!m) return dl_fail("dl_nested_run: null sampler");
    if (niterations < 0 || quota < 1) return dl_fail("dl_nested_run: invalid argument");
    if (!history_dev || !coords_dev || !loglike_dev || !logprior_dev || !logweight_dev || !count_dev || !mode_dev) return dl_fail("dl_nested_run: the record buffers are required");
    if (!m->have_hyper) return dl_fail("dl_nested_run: no hyper-parameters (dl_nested_set_hyper)");
    if (!m->have_state) return dl_fail("dl_nested_run: no live points (dl_nested_set_live or dl_nested_set_state)");
    if (!niterations) return 0;
    hipStream_t stream = (hipStream_t)hip_stream;
    DL_HIP_CHECK(hipSetDevice(m->device));
    DlNestedArgs a = dl_nested_args(m);
    a.hist = history_dev; a.out_coords = coords_dev; a.out_L = loglike_dev; a.out_pi = logprior_dev; a.out_logw = logweight_dev; a.out_count = count_dev; a.out_mode = mode_dev;
    a.quota = quota;
    const int K = m->K, P = m->P;
    const int64_t rows = (int64_t)K * m->M;
    const unsigned pgrid = (unsigned)((rows + DL_NESTED_WAVES - 1) / DL_NESTED_WAVES);
    for (int64_t it = 0; it < niterations; ++it) {
        hipLaunchKernelGGL(dl_nested_rank_kernel, dim3(K), dim3(DL_NESTED_THREADS), 0, stream, a);
        hipLaunchKernelGGL(dl_nested_moments_kernel, dim3(K, P), dim3(64 * DL_SMC_MOMENT_WAVES), 0, stream, a);
        hipLaunchKernelGGL(dl_nested_cholesky_kernel, dim3(K), dim3(64), 0, stream, a);
        hipLaunchKernelGGL(dl_nested_seed_kernel, dim3(pgrid), dim3(64 * DL_NESTED_WAVES), 0, stream, a);
        for (int j = 0; j < m->n_steps; ++j) {
            hipLaunchKernelGGL(dl_nested_propose_kernel, dim3(pgrid), dim3(64 * DL_NESTED_WAVES), 0, stream, a, j);
            if (dl_eval_batch(m->ctx, m->prop, rows, m->Lp, m->pip, nullptr, m->status, nullptr, stream)) return 1;
            hipLaunchKernelGGL(dl_nested_accept_kernel, dim3(pgrid), dim3(64 * DL_NESTED_WAVES), 0, stream, a, j);
        }
        hipLaunchKernelGGL(dl_nested_finish_kernel, dim3(K), dim3(DL_NESTED_THREADS), 0, stream, a);
        m->evaluations += rows * m->n_steps;
    }
    DL_HIP_CHECK(hipGetLastError());
    m->iterations += niterations;
    return 0;
}

int64_t dl_nested_info(const dl_nested* m, const char* key) {
    if (!m || !key) return -1;
    const std::string k(key);
    if (k == "nruns") return m->K;
    if (k == "nlive") return m->N;
    if (k == "n_params") return m->P;
    if (k == "ndelete") return m->M;
    if (k == "iterations") return m->iterations;
    if (k == "evaluations") return m->evaluations;
    if (k == "n_steps") return m->n_steps;
    return -1;
}

}  // extern "C"
