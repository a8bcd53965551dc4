"""NUTS on the cfg2 likelihood (analytic gradient) at 256 / 1024 / 4096 chains; prints ONE JSON line.

Per chain count:
  * us per leapfrog step of the device engine (dl_nuts_run of N steps between two device events), the gradient alone (N calls of dl_eval_logposterior_grad on the
    same rows between two events), and their difference: what the NUTS step kernel adds to the gradient call;
  * mean tree depth and leapfrog steps per trajectory after warm-up;
  * ESS per second of every parameter (samples / integrated autocorrelation time, the autocorrelation averaged over the chains; seconds: wall time of the sampling batch, warm-up
    excluded) for NUTSSampler, HMCSampler at its defaults (60 leapfrog steps, adapted step size and mass matrix) and HMCSampler with the trajectory length NUTS
    chose (num_integration_steps = mean leapfrog steps per NUTS trajectory).
    python tools/nuts_probe.py [chains ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from bench_configs import make_cfg2
from desilike_amd.samplers import NUTSSampler, HMCSampler
from desilike_amd.diagnostics import integrated_autocorrelation_time

WARMUP, SAMPLES, NSTEPS = 200, 200, 200


def ess_per_second(chains, names, seconds):
    ess = []
    for name in names:
        x = np.array([chain[name] for chain in chains])               # [nchains, n]
        tau = float(integrated_autocorrelation_time(x))               # (autocorrelation averaged over the chains)
        ess.append(x.size / max(tau, 1.))
    return [e / seconds for e in ess]


def timed_run(sampler, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    chains = sampler.run(check_every=n, max_iterations=n)
    torch.cuda.synchronize()
    return chains, time.perf_counter() - t0


def step_timings(sampler):
    """(us per NUTS step, us per gradient call) by device events."""
    engine = sampler._engine
    nuts, ctx = engine.nuts, sampler.likelihood._get_posterior_context()[0]
    C, P = nuts.nchains, nuts.n_params
    quota = 256                                         # > the 20 + NSTEPS trajectories a chain can end here: no chain stops, every step is a full step
    big = nuts.buffers(quota)                           # (record buffers hold `quota` records per chain)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nuts.run(20, quota, big)
    start.record(); nuts.run(NSTEPS, quota, big); stop.record(); torch.cuda.synchronize()
    t_step = start.elapsed_time(stop) * 1e3 / NSTEPS
    q = torch.as_tensor(sampler._state[0][:C], device='cuda:{:d}'.format(ctx.device)).contiguous()
    lp, grad = torch.empty(C, dtype=torch.float64, device=q.device), torch.empty((C, P), dtype=torch.float64, device=q.device)
    for _ in range(20): ctx.eval_logposterior_grad(q, lp, grad)
    start.record()
    for _ in range(NSTEPS): ctx.eval_logposterior_grad(q, lp, grad)
    stop.record(); torch.cuda.synchronize()
    t_grad = start.elapsed_time(stop) * 1e3 / NSTEPS
    return t_step, t_grad


def main(counts):
    results = {}
    for nchains in counts:
        g, like = make_cfg2()
        names = like.varied_params.names()
        nuts = NUTSSampler(like, chains=nchains, seed=1, adaptation={'niterations': WARMUP}, gradient='analytic')
        nuts.run(check_every=1, max_iterations=1)                  # warm-up (+ one iteration)
        chains, seconds = timed_run(nuts, SAMPLES)
        info = nuts._store[2][1:]
        t_step, t_grad = step_timings(nuts)
        leapfrog = float(info[..., 1].mean())
        row = {'us_per_step': t_step, 'us_gradient': t_grad, 'us_nuts_kernel': t_step - t_grad, 'nuts_kernel_over_gradient': (t_step - t_grad) / t_grad,
               'mean_tree_depth': float(info[..., 0].mean()), 'leapfrog_per_trajectory': leapfrog, 'divergent_fraction': float((info[..., 2] > 0).mean()), 'energy_divergences': int((info[..., 2] == 1).sum()),
               'nuts_ess_per_s': dict(zip(names, ess_per_second(chains, names, seconds)))}
        for label, steps in (('hmc_default', 60), ('hmc_nuts_length', max(1, int(round(leapfrog))))):
            hmc = HMCSampler(make_cfg2()[1], chains=nchains, seed=1, num_integration_steps=steps, adaptation={'niterations': WARMUP}, gradient='analytic')
            hmc.run(check_every=1, max_iterations=1)
            chains, seconds = timed_run(hmc, SAMPLES)
            row[label + '_ess_per_s'] = dict(zip(names, ess_per_second(chains, names, seconds)))
            row[label + '_steps'] = steps
        results[str(nchains)] = row
    print(json.dumps({'probe': 'nuts', 'config': 'cfg2', 'warmup': WARMUP, 'samples': SAMPLES, 'results': results}))


if __name__ == '__main__':
    main([int(a) for a in sys.argv[1:]] or [256, 1024, 4096])
