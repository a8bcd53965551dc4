// dl_ensemble_data.hip -- many device-resident ensembles, one per data vector of a data batch (include/desilike_amd.h, dl_ensemble_data_*): "sample every mock".
//
// E independent affine-invariant ensembles (dl_ensemble.hip: Goodman & Weare 2010 stretch move, two half-ensemble updates per iteration) of nw walkers x P parameters,
// ensemble e bound to data vector data_index[e] of the context's data batch (dl_data_set / dl_data_set_solved) and keyed by its own 64-bit Philox key, advance in
// lockstep.  A half-step of ALL ensembles is one enqueued sequence with no host synchronisation:
//
//     [step kernel, grid = E workgroups: accept the pending half | draw the split | stretch proposals]
//        ->  dl_eval_logposterior_data(ctx, prop [E half, P], index [E half], newlp)    (paired: row b against data vector index[b]; rows of ensemble e are e half .. (e + 1) half - 1)
//        ->  next step kernel
//
// so that the evaluation sees E nw / 2 rows where a single mock ensemble of a few dozen walkers gives it a handful.  The draws of ensemble e are those of a single
// dl_ensemble with the same key (dl_ens_draw.h: one definition): its chain is the chain of samplers.py EnsembleStretchMove with CounterRNG(key_e) on the
// log-posterior given data vector data_index[e], bit for bit (tests/test_gpu_mock_ensemble.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/desilike_amd.h"
#include "dl_kernels.h"
#include "dl_sampler_dev.h"   // dl_fail, DL_HIP_CHECK, dl_dev_alloc, dl_dev_free
#include "dl_ens_draw.h"

namespace {

#define DL_ENSD_THREADS 256   // one workgroup per ensemble: mock ensembles are a few dozen walkers (one slot per thread in either phase up to 256 walkers; loops beyond)

struct DlEnsDataArgs {
    double* coords;              // [E, nw, P]
    double* logp;                // [E, nw]
    long long* nacc;             // [E, nw]
    double* prop;                // [E half, P] proposals of the pending half-step, then of the new one
    double* factors;             // [E half] (P - 1) log z
    const double* newlp;         // [E half] log-posteriors of the pending proposals, each against its ensemble's data vector
    double* chain;               // record target of this launch: [E, nw, P] or null
    double* chain_logp;          // [E, nw] or null
    const uint64_t* keys;        // [E]
    int32_t nw, P;
    double a, offset;
    long long it_acc, it_prop;   // iteration of the half-step to accept / to propose (shared by all ensembles)
    int32_t half_acc, half_prop; // 0 / 1, or -1: nothing to accept / propose
};

// what dl_ens_draw_accept / dl_ens_draw_move read: the two half-steps of this launch with the splits of THIS ensemble
struct DlEnsDataDraw {
    DlEnsSplit split_acc, split_prop;
    long long it_acc, it_prop;
    int32_t half_acc, half_prop, P;
    uint32_t k0, k1;
    double a;
};

// LDS bytes of a workgroup: positions, log-posteriors, pending proposals (one double of slack in front: see the staging)
size_t dl_ensd_shared_bytes(int nw, int P) {
    const size_t half = (size_t)(nw / 2);
    return ((size_t)nw * P + nw + ((half * P + 3) & ~(size_t)1)) * 8 + 16;
}

// Workgroup e: the step of dl_ensemble_step_lds_kernel on ensemble e.  Everything the launch reads of the ensemble -- positions, log-posteriors, the pending
// proposals -- is requested at the top as LDS-DMA, the key's two splits and the draws and logarithms of both phases are computed in the shadow of that round trip
// (accept draws on the first wavefront, move draws half a workgroup away: another SIMD), and the phases after the barrier touch LDS only and end in fire-and-forget
// stores.  The log-posteriors of the pending proposals come finished from the paired data-batch call: NaN -> -inf, + offset here (the conventions of dl_ensemble).
__global__ __launch_bounds__(DL_ENSD_THREADS) void dl_ensemble_data_step_kernel(const DlEnsDataArgs s) {
#pragma clang fp contract(off)   // the NumPy driver rounds after every operation: no fused multiply-adds here
    extern __shared__ __attribute__((aligned(16))) double dl_ensd_lds[];
    const int tid = threadIdx.x, nthr = DL_ENSD_THREADS, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int e = blockIdx.x, nw = s.nw, half = nw / 2, P = s.P;
    const bool accepting = s.half_acc >= 0, proposing = s.half_prop >= 0;
    double* g_coords = s.coords + (size_t)e * nw * P;       // (nw is even: 16-byte aligned, as is g_logp)
    double* g_logp = s.logp + (size_t)e * nw;
    double* g_prop = s.prop + (size_t)e * half * P;
    double* g_factors = s.factors + (size_t)e * half;
    const double* g_newlp = s.newlp + (size_t)e * half;
    long long* g_nacc = s.nacc + (size_t)e * nw;
    // half P may be odd (9 proposals of 7 parameters): the proposals of an odd ensemble then start 8 bytes off the 16-byte chunks of the LDS-DMA -- staged from one
    // double earlier (the last value of ensemble e - 1: inside the array) into one double earlier in LDS
    const int skew = (int)(((size_t)e * half * P) & 1);
    double* coords = dl_ensd_lds;                            // [nw, P]
    double* logp = coords + (size_t)nw * P;                  // [nw]
    double* prop = logp + nw + skew;                         // [half, P] pending proposals (the new ones go straight to global memory)
    const double inf = __builtin_huge_val();
    dl_ens_stage(coords, g_coords, nw * P, 0, wave, lane, nthr);
    dl_ens_stage(logp, g_logp, nw, 0, wave, lane, nthr);
    double lp0 = 0., f0 = 0.;
    if (accepting) {
        dl_ens_stage(prop - skew, g_prop - skew, half * P + skew, 0, wave, lane, nthr);
        if (tid < half) { lp0 = g_newlp[tid]; f0 = g_factors[tid]; }
    }
    __builtin_amdgcn_sched_barrier(0);
    // in the shadow of the round trip: this ensemble's key, the splits of the two iterations, the draws of this thread's first slot of either phase
    const uint64_t key = *(const __attribute__((address_space(4))) uint64_t*)(s.keys + e);   // (a scalar load: a vector load would make the draws wait for the staging requests in front of it)
    DlEnsDataDraw d{};
    d.it_acc = s.it_acc; d.it_prop = s.it_prop; d.half_acc = s.half_acc; d.half_prop = s.half_prop; d.P = P; d.a = s.a;
    d.k0 = (uint32_t)key; d.k1 = (uint32_t)(key >> 32);
    if (proposing) d.split_prop = dl_ens_split(s.it_prop, nw, d.k0, d.k1);
    if (accepting) d.split_acc = (proposing && s.it_acc == s.it_prop) ? d.split_prop : dl_ens_split(s.it_acc, nw, d.k0, d.k1);
    const int jp0 = (tid + nthr / 2) % nthr;      // the move phase starts half a workgroup away from the accept phase
    int i0 = 0, is0 = 0, ic0 = 0;
    double logu0 = 0., zz0 = 0., fac0 = 0.;
    if (accepting && tid < half) dl_ens_draw_accept(d, tid, half, i0, logu0);
    if (proposing && jp0 < half) dl_ens_draw_move(d, jp0, half, is0, ic0, zz0, fac0);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    if (accepting) {
        // accept / reject the pending proposals (emcee moves/red_blue.py: lnpdiff = factors + new_log_prob - log_prob; accepted = log(u) < lnpdiff)
        for (int j = tid; j < half; j += nthr) {
            int i = i0;
            double logu = logu0, lp = lp0, fj = f0;
            if (j != tid) { dl_ens_draw_accept(d, j, half, i, logu); fj = g_factors[j]; lp = g_newlp[j]; }
            if (lp != lp) lp = -inf;                     // NaN results count as -inf (samplers/base.py:187-189)
            lp = lp + s.offset;
            const double lnpdiff = (fj + lp) - logp[i];
            if (logu < lnpdiff) {
                for (int p = 0; p < P; ++p) { const double v = prop[(size_t)j * P + p]; coords[(size_t)i * P + p] = v; g_coords[(size_t)i * P + p] = v; }
                logp[i] = lp; g_logp[i] = lp;
                (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(g_nacc) + i, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // no return value: nothing waits
            }
        }
        __syncthreads();
    }
    if (s.chain != nullptr) {
        double* chain = s.chain + (size_t)e * nw * P;
        for (int q = tid; q < nw * P; q += nthr) chain[q] = coords[q];
        if (s.chain_logp != nullptr)
            for (int q = tid; q < nw; q += nthr) s.chain_logp[(size_t)e * nw + q] = logp[q];
    }
    if (!proposing) return;
    for (int j = jp0; j < half; j += nthr) {
        int is = is0, ic = ic0;
        double zz = zz0, fac = fac0;
        if (j != jp0) dl_ens_draw_move(d, j, half, is, ic, zz, fac);
        for (int p = 0; p < P; ++p) {
            const double c = coords[(size_t)ic * P + p], x = coords[(size_t)is * P + p];
            g_prop[(size_t)j * P + p] = c - (c - x) * zz;      // q = c - (c - s) z
        }
        g_factors[j] = fac;
    }
}

// log-posteriors of starting positions as the paired call wrote them -> the ensembles' convention: NaN -> -inf, + offset
__global__ void dl_ensemble_data_start_kernel(double* logp, long long n, double offset) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    double lp = logp[q];
    if (lp != lp) lp = -__builtin_huge_val();
    logp[q] = lp + offset;
}

}  // namespace

struct dl_ensemble_data {
    dl_ctx* ctx = nullptr;
    int device = 0, E = 0, nw = 0, P = 0, max_index = 0;
    size_t shm = 0;
    double a = 2., offset = 0.;
    long long iteration = 0;      // updates of every ensemble done since creation (the counter of the random number generators)
    bool have_logp = false;
    double *coords = nullptr, *logp = nullptr, *prop = nullptr, *factors = nullptr, *newlp = nullptr;
    long long* nacc = nullptr;
    uint64_t* keys = nullptr;         // [E]
    int32_t* index_half = nullptr;    // [E half]: data vector of every proposal row of a half-step
    int32_t* index_all = nullptr;     // [E nw]: data vector of every walker (log-posteriors of a start given without them)
};

extern "C" {

void dl_ensemble_data_destroy(dl_ensemble_data* ens) {
    if (!ens) return;
    (void)hipSetDevice(ens->device);
    dl_dev_free({(void**)&ens->coords, (void**)&ens->logp, (void**)&ens->prop, (void**)&ens->factors, (void**)&ens->newlp, (void**)&ens->nacc, (void**)&ens->keys,
                 (void**)&ens->index_half, (void**)&ens->index_all});
    delete ens;
}

int dl_ensemble_data_create(dl_ensemble_data** out, dl_ctx* ctx, int32_t n_ensembles, const int32_t* data_index, const uint64_t* seeds, int32_t nwalkers, double a, double offset) {
    if (!out || !ctx || !data_index || !seeds) return dl_fail("dl_ensemble_data_create: null argument");
    *out = nullptr;
    // every refusal comes before the first device call
    const int P = (int)dl_info(ctx, "n_params"), M = (int)dl_info(ctx, "n_data_batch");
    if (M <= 0) return dl_fail("dl_ensemble_data_create: the context has no data batch (dl_data_set / dl_data_set_solved)");
    if (n_ensembles < 1) return dl_fail("dl_ensemble_data_create: the number of ensembles must be >= 1");
    if (nwalkers < 2 || nwalkers % 2 || nwalkers > 8192) return dl_fail("dl_ensemble_data_create: nwalkers must be even, in [2, 8192]");
    if (!(a > 1.)) return dl_fail("dl_ensemble_data_create: stretch parameter a must be > 1");
    int max_index = 0;
    for (int e = 0; e < n_ensembles; ++e) {
        if (data_index[e] < 0 || data_index[e] >= M)
            return dl_fail("dl_ensemble_data_create: data index " + std::to_string(data_index[e]) + " of ensemble " + std::to_string(e) + " lies outside [0, " + std::to_string(M) + ")");
        max_index = std::max(max_index, (int)data_index[e]);
    }
    const size_t shm = dl_ensd_shared_bytes(nwalkers, P);
    if (shm > DL_ENS_LDS_BUDGET)
        return dl_fail("dl_ensemble_data_create: " + std::to_string(nwalkers) + " walkers x " + std::to_string(P) + " parameters need " + std::to_string(shm) + " bytes of LDS per ensemble, beyond the " +
                       std::to_string(DL_ENS_LDS_BUDGET) + " of a workgroup: run an ensemble of this size per data vector with dl_ensemble");
    if ((size_t)n_ensembles * nwalkers * P >= ((size_t)1 << 31)) return dl_fail("dl_ensemble_data_create: n_ensembles x nwalkers x n_params must stay below 2^31");
    dl_ensemble_data* ens = new dl_ensemble_data();
    ens->ctx = ctx; ens->E = n_ensembles; ens->nw = nwalkers; ens->P = P; ens->a = a; ens->offset = offset; ens->max_index = max_index; ens->shm = shm;
    ens->device = (int)dl_info(ctx, "device");
    const size_t E = (size_t)n_ensembles, half = (size_t)nwalkers / 2;
    auto bail = [&](const std::string& msg) { dl_ensemble_data_destroy(ens); return dl_fail(msg); };
    if (hipSetDevice(ens->device) != hipSuccess) return bail("dl_ensemble_data_create: hipSetDevice failed");
    if (!dl_dev_alloc(&ens->coords, E * nwalkers * P) || !dl_dev_alloc(&ens->logp, E * nwalkers) || !dl_dev_alloc(&ens->prop, E * half * P) || !dl_dev_alloc(&ens->factors, E * half) ||
        !dl_dev_alloc(&ens->newlp, E * half) || !dl_dev_alloc(&ens->nacc, E * nwalkers) || !dl_dev_alloc(&ens->keys, E) || !dl_dev_alloc(&ens->index_half, E * half) ||
        !dl_dev_alloc(&ens->index_all, E * nwalkers))
        return bail("dl_ensemble_data_create: device allocation failed");
    // the expanded index arrays, built once: rows e half .. (e + 1) half - 1 of a half-step belong to ensemble e
    std::vector<int32_t> index_half(E * half), index_all(E * nwalkers);
    for (size_t e = 0; e < E; ++e) {
        for (size_t j = 0; j < half; ++j) index_half[e * half + j] = data_index[e];
        for (size_t w = 0; w < (size_t)nwalkers; ++w) index_all[e * nwalkers + w] = data_index[e];
    }
    if (hipMemcpy(ens->keys, seeds, E * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ens->index_half, index_half.data(), index_half.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ens->index_all, index_all.data(), index_all.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
        return bail("dl_ensemble_data_create: hipMemcpy failed");
    if (shm > 48 * 1024 && hipFuncSetAttribute((const void*)dl_ensemble_data_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess)
        return bail("dl_ensemble_data_create: hipFuncSetAttribute failed");
    if (hipDeviceSynchronize() != hipSuccess) return bail("dl_ensemble_data_create: hipDeviceSynchronize failed");   // (null-stream memsets vs the caller's non-blocking streams)
    *out = ens;
    return 0;
}

int dl_ensemble_data_set_state(dl_ensemble_data* ens, const double* coords, const double* logposterior, void* hip_stream) {
    if (!ens || !coords) return dl_fail("dl_ensemble_data_set_state: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    DL_HIP_CHECK(hipSetDevice(ens->device));
    const size_t n = (size_t)ens->E * ens->nw;
    DL_HIP_CHECK(hipMemcpyAsync(ens->coords, coords, n * ens->P * sizeof(double), hipMemcpyHostToDevice, stream));
    if (logposterior) DL_HIP_CHECK(hipMemcpyAsync(ens->logp, logposterior, n * sizeof(double), hipMemcpyHostToDevice, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));   // the host buffers may be pageable
    ens->have_logp = logposterior != nullptr;
    return 0;
}

int dl_ensemble_data_run(dl_ensemble_data* ens, int64_t niterations, int32_t thin_by, double* chain_dev, double* chain_logp_dev, void* hip_stream) {
    if (!ens) return dl_fail("dl_ensemble_data_run: null ensemble");
    if (niterations < 0 || thin_by < 1) return dl_fail("dl_ensemble_data_run: invalid argument");
    // dl_data_set replaces the batch in place: the indices were checked against the batch of the creation
    const int M = (int)dl_info(ens->ctx, "n_data_batch");
    if (ens->max_index >= M)
        return dl_fail("dl_ensemble_data_run: the context's data batch now holds " + std::to_string(M) + " data vectors, the ensembles' indices reach " + std::to_string(ens->max_index) +
                       ": create the ensembles again after dl_data_set");
    hipStream_t stream = (hipStream_t)hip_stream;
    DL_HIP_CHECK(hipSetDevice(ens->device));
    const int E = ens->E, nw = ens->nw, P = ens->P, half = nw / 2;
    const size_t n_all = (size_t)E * nw;
    if (!ens->have_logp) {
        // log-posteriors of the starting positions: every walker against its ensemble's data vector, one paired call
        if (dl_eval_logposterior_data(ens->ctx, ens->coords, (int64_t)n_all, ens->index_all, ens->logp, nullptr, stream)) return 1;
        hipLaunchKernelGGL(dl_ensemble_data_start_kernel, dim3((unsigned)((n_all + 255) / 256)), dim3(256), 0, stream, ens->logp, (long long)n_all, ens->offset);
        ens->have_logp = true;
    }
    if (niterations == 0) return 0;
    DlEnsDataArgs s;
    std::memset(&s, 0, sizeof(s));
    s.coords = ens->coords; s.logp = ens->logp; s.nacc = ens->nacc; s.prop = ens->prop; s.factors = ens->factors; s.newlp = ens->newlp; s.keys = ens->keys;
    s.nw = nw; s.P = P; s.a = ens->a; s.offset = ens->offset;
    s.half_acc = -1;
    const long long it0 = ens->iteration;
    // the launch that proposes half-step (it, h) also accepts the half-step before it; the accept of half-step 1 completes an iteration: recorded there
    auto set_record = [&]() {
        s.chain = nullptr; s.chain_logp = nullptr;
        if (s.half_acc != 1 || !chain_dev) return;
        const long long done = s.it_acc - it0 + 1;
        if (done % thin_by) return;
        const size_t row = (size_t)(done / thin_by - 1);
        s.chain = chain_dev + row * n_all * P;
        s.chain_logp = chain_logp_dev ? chain_logp_dev + row * n_all : nullptr;
    };
    for (long long it = it0; it < it0 + niterations; ++it)
        for (int h = 0; h < 2; ++h) {
            s.it_prop = it; s.half_prop = h;
            set_record();
            hipLaunchKernelGGL(dl_ensemble_data_step_kernel, dim3(E), dim3(DL_ENSD_THREADS), ens->shm, stream, s);
            if (dl_eval_logposterior_data(ens->ctx, ens->prop, (int64_t)E * half, ens->index_half, ens->newlp, nullptr, stream)) return 1;
            s.it_acc = it; s.half_acc = h;
        }
    s.half_prop = -1;
    set_record();
    hipLaunchKernelGGL(dl_ensemble_data_step_kernel, dim3(E), dim3(DL_ENSD_THREADS), ens->shm, stream, s);
    DL_HIP_CHECK(hipGetLastError());
    ens->iteration += niterations;
    return 0;
}

int dl_ensemble_data_get_state(dl_ensemble_data* ens, double* coords, double* logposterior, int64_t* naccepted, void* hip_stream) {
    if (!ens) return dl_fail("dl_ensemble_data_get_state: null ensemble");
    hipStream_t stream = (hipStream_t)hip_stream;
    DL_HIP_CHECK(hipSetDevice(ens->device));
    const size_t n = (size_t)ens->E * ens->nw;
    if (coords) DL_HIP_CHECK(hipMemcpyAsync(coords, ens->coords, n * ens->P * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (logposterior) DL_HIP_CHECK(hipMemcpyAsync(logposterior, ens->logp, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (naccepted) DL_HIP_CHECK(hipMemcpyAsync(naccepted, ens->nacc, n * sizeof(long long), hipMemcpyDeviceToHost, stream));
    DL_HIP_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int dl_ensemble_data_set_counter(dl_ensemble_data* ens, int64_t iteration, const int64_t* naccepted, void* hip_stream) {
    if (!ens) return dl_fail("dl_ensemble_data_set_counter: null ensemble");
    if (iteration < 0) return dl_fail("dl_ensemble_data_set_counter: negative iteration");
    hipStream_t stream = (hipStream_t)hip_stream;
    DL_HIP_CHECK(hipSetDevice(ens->device));
    if (naccepted) {
        DL_HIP_CHECK(hipMemcpyAsync(ens->nacc, naccepted, (size_t)ens->E * ens->nw * sizeof(long long), hipMemcpyHostToDevice, stream));
        DL_HIP_CHECK(hipStreamSynchronize(stream));   // the host buffer may be pageable
    }
    ens->iteration = iteration;
    return 0;
}

int64_t dl_ensemble_data_info(const dl_ensemble_data* ens, const char* key) {
    if (!ens || !key) return -1;
    std::string k(key);
    if (k == "n_ensembles") return ens->E;
    if (k == "nwalkers") return ens->nw;
    if (k == "n_params") return ens->P;
    if (k == "iteration") return ens->iteration;
    if (k == "lds_bytes") return (int64_t)ens->shm;
    return -1;
}

}  // extern "C"
