"""Tempered SMC on the cfg2 likelihood at K x N = 1024 / 4096 / 16384 particle rows (N = 1024 particles per system), n_steps = 12; prints ONE JSON line.

Per row count:
  * us per temperature iteration of the device engine (dl_smc_run of ONE iteration between two device events, after a warm-up; median of 20 iterations; also apart: the iterations in which a system still climbs, and the sweeps at beta = 1), the same
    twelve dl_eval_batch calls alone on the same rows in the same process (median of 20), and their difference: what the SMC kernels add to the evaluations;
  * evaluations per second during the mutation.
For cfg2 (chains = 8): the temperature levels to beta = 1, the evaluations to beta = 1 and logz_std at N = 1024 and N = 4096.
    python tools/smc_probe.py [--timings-only] [rows ...]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from bench_configs import make_cfg2
from desilike_amd.smc import SMCSampler, _DeviceSMC

N, N_STEPS, WARMUP, TIMED = 1024, 12, 5, 20


def iteration_timings(rows):
    like = make_cfg2()[1]
    K = rows // N
    sampler = SMCSampler(like, nparticles=N, chains=K, seed=1, n_steps=N_STEPS)
    ctx, offset = like._get_posterior_context()
    engine = _DeviceSMC(ctx, offset, K, N, sampler.widths, seed=1)
    engine.set_hyper(0.5, N_STEPS, 0.234)
    engine.set_particles(np.stack([param.prior.sample(size=(K, N), random_state=np.random.RandomState(i)) for i, param in enumerate(like.varied_params)], axis=-1))
    quota = WARMUP + TIMED
    buffers = engine.buffers(quota)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    engine.run(WARMUP, quota, buffers)
    torch.cuda.synchronize()
    t_iter = []
    for _ in range(TIMED):
        start.record(); engine.run(1, quota, buffers); stop.record(); torch.cuda.synchronize()
        t_iter.append(start.elapsed_time(stop) * 1e3)
    history = engine.records(buffers)[0]
    device = 'cuda:{:d}'.format(ctx.device)
    x = torch.as_tensor(engine.get_state()[0].reshape(-1, ctx.n_params), device=device).contiguous()
    L, pi, status = torch.empty(len(x), dtype=torch.float64, device=device), torch.empty(len(x), dtype=torch.float64, device=device), torch.empty(len(x), dtype=torch.int32, device=device)
    for _ in range(WARMUP * N_STEPS): ctx.eval_batch(x, loglike=L, logprior=pi, status=status)
    torch.cuda.synchronize()
    t_eval = []
    for _ in range(TIMED):
        start.record()
        for _ in range(N_STEPS): ctx.eval_batch(x, loglike=L, logprior=pi, status=status)
        stop.record(); torch.cuda.synchronize()
        t_eval.append(start.elapsed_time(stop) * 1e3)
    # an iteration in which a system still climbs runs the temper, moments, Cholesky and resample kernels in full; at beta = 1 they return at once
    before = np.concatenate([np.zeros((K, 1)), history[:, :-1, 0]], axis=1)[:, WARMUP:].min(axis=0)
    split = {name: float(np.median(np.array(t_iter)[mask])) if mask.any() else None for name, mask in [('us_per_climbing_iteration', before < 1.), ('us_per_sweep_iteration', before >= 1.)]}
    t_iter, t_eval = float(np.median(t_iter)), float(np.median(t_eval))
    return {**split, 'systems': K, 'particles': N, 'us_per_iteration': t_iter, 'us_evaluations': t_eval, 'us_smc_kernels': t_iter - t_eval, 'smc_kernels_over_evaluations': (t_iter - t_eval) / t_eval,
            'evaluations_per_s': rows * N_STEPS / (t_iter * 1e-6), 'beta_after': history[:, -1, 0].tolist()}


def evidence(nparticles):
    sampler = SMCSampler(make_cfg2()[1], nparticles=nparticles, chains=8, seed=1, n_steps=N_STEPS)
    sampler.run(max_iterations=1)
    levels = sampler.nlevels
    return {'levels': levels.tolist(), 'evaluations_to_beta_1_per_system': int(nparticles * (1 + N_STEPS * levels.max())), 'logz': sampler.logz.tolist(), 'logz_mean': sampler.logz_mean,
            'logz_std': sampler.logz_std, 'sqrt_T_over_N': float(np.sqrt(levels.max() / nparticles))}


def main(rows, with_evidence=True):
    results = {str(r): iteration_timings(r) for r in rows}
    print(json.dumps({'probe': 'smc', 'config': 'cfg2', 'n_steps': N_STEPS, 'results': results, 'evidence': {str(n): evidence(n) for n in (1024, 4096)} if with_evidence else None}))


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--timings-only']       # --timings-only: without the evidence runs (a kernel trace of the timed shapes alone)
    main([int(a) for a in args] or [1024, 4096, 16384], with_evidence=len(args) == len(sys.argv[1:]))
