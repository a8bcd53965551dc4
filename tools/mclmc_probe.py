"""MCLMC on the cfg2 likelihood (analytic gradient) at 256 / 1024 / 4096 chains; prints ONE JSON line.

Per chain count:
  * us per integrator step of the device engine (dl_mclmc_run of N steps between two device events, after a warm-up), the gradient alone (as many calls of
    dl_eval_logposterior_grad on the same rows as the steps took, between two events), and their difference: what the MCLMC stage kernel adds to the gradient calls;
  * the adapted step size and L, the fraction of steps undone at a prior bound;
  * ESS per second of every parameter (samples / integrated autocorrelation time, the autocorrelation averaged over the chains; seconds: wall time of the sampling
    batch, warm-up excluded) for MCLMCSampler and, on the same box in the same process, NUTSSampler.
    python tools/mclmc_probe.py [chains ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch

from bench_configs import make_cfg2
from desilike_amd.samplers import MCLMCSampler, NUTSSampler
from nuts_probe import ess_per_second, timed_run

WARMUP, SAMPLES, THIN, NSTEPS, NUTS_WARMUP, NUTS_SAMPLES = 600, 400, 5, 200, 200, 200


def step_timings(sampler):
    """(us per MCLMC step, us of its gradient calls) by device events."""
    mclmc, ctx = sampler._engine.mclmc, sampler.likelihood._get_posterior_context()[0]
    C, P, ngrad = mclmc.nchains, mclmc.n_params, mclmc.info('gradients_per_step')
    quota = 20 + NSTEPS                                  # no chain reaches its quota: every step is a full step
    big = mclmc.buffers(quota)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    mclmc.run(20, quota, big)
    start.record(); mclmc.run(NSTEPS, quota, big); stop.record(); torch.cuda.synchronize()
    t_step = start.elapsed_time(stop) * 1e3 / NSTEPS
    q = torch.as_tensor(sampler._state[0][:C], device='cuda:{:d}'.format(ctx.device)).contiguous()
    lp, grad = torch.empty(C, dtype=torch.float64, device=q.device), torch.empty((C, P), dtype=torch.float64, device=q.device)
    for _ in range(20): ctx.eval_logposterior_grad(q, lp, grad)
    start.record()
    for _ in range(NSTEPS * ngrad): ctx.eval_logposterior_grad(q, lp, grad)
    stop.record(); torch.cuda.synchronize()
    return t_step, start.elapsed_time(stop) * 1e3 / NSTEPS, ngrad


def main(counts):
    results = {}
    for nchains in counts:
        g, like = make_cfg2()
        names = like.varied_params.names()
        mclmc = MCLMCSampler(like, chains=nchains, seed=1, adaptation={'niterations': WARMUP}, gradient='analytic')
        mclmc.run(check_every=THIN, max_iterations=THIN, thin_by=THIN)            # warm-up (+ one record)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chains = mclmc.run(check_every=SAMPLES * THIN, max_iterations=SAMPLES * THIN, thin_by=THIN)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        chains = [{name: chain[name][1:] for name in names} for chain in chains]
        t_step, t_grad, ngrad = step_timings(mclmc)
        row = {'us_per_step': t_step, 'us_gradient': t_grad, 'gradients_per_step': ngrad, 'us_mclmc_kernel': t_step - t_grad,
               'mclmc_kernel_over_gradient': (t_step - t_grad) / t_grad, 'step_size': mclmc.hyp['step_size'], 'L': mclmc.hyp['L'],
               'undone_fraction': float(mclmc._store[2][..., 1].mean()), 'steps_per_record': THIN,
               'mclmc_ess_per_s': dict(zip(names, ess_per_second(chains, names, seconds)))}
        nuts = NUTSSampler(make_cfg2()[1], chains=nchains, seed=1, adaptation={'niterations': NUTS_WARMUP}, gradient='analytic')
        nuts.run(check_every=1, max_iterations=1)
        chains, seconds = timed_run(nuts, NUTS_SAMPLES)
        row['nuts_ess_per_s'] = dict(zip(names, ess_per_second(chains, names, seconds)))
        results[str(nchains)] = row
    print(json.dumps({'probe': 'mclmc', 'config': 'cfg2', 'warmup': WARMUP, 'records': SAMPLES, 'results': results}))


if __name__ == '__main__':
    main([int(a) for a in sys.argv[1:]] or [256, 1024, 4096])
