"""Nested sampling on the cfg2 likelihood at K x M = 256 / 1024 / 4096 replaced rows per sweep (N = 1024 live points per run, ndelete = 256), n_steps = 24; prints ONE JSON line.

Per row count:
  * us per iteration of the device engine (dl_nested_run of ONE iteration between two device events, after a warm-up; median of 20 iterations), the same 24
    dl_eval_batch calls alone on the same number of rows in the same process (median of 20), and their difference: what the nested kernels add to the evaluations;
  * evaluations per second during the mutation.
For cfg2 (chains = 4): the iterations to rest, the evaluations, logz with its error and scatter at N = 1024.
    python tools/nested_probe.py [--timings-only] [rows ...]
Every GPU step of a session belongs under its own time limit (timeout -k 10 300 python tools/nested_probe.py 256, one row count per call)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from bench_configs import make_cfg2
from desilike_amd.nested import NestedSampler, _DeviceNested

N, M, N_STEPS, WARMUP, TIMED = 1024, 256, 24, 5, 20


def iteration_timings(rows):
    like = make_cfg2()[1]
    K = rows // M
    sampler = NestedSampler(like, nlive=N, chains=K, ndelete=M, seed=1, n_steps=N_STEPS)
    ctx, offset = like._get_posterior_context()
    engine = _DeviceNested(ctx, offset, K, N, sampler.widths, seed=1)
    engine.set_hyper(M, N_STEPS, 0.234, 1e-6)        # (no run rests while it is timed)
    engine.set_live(np.stack([param.prior.sample(size=(K, N), random_state=np.random.RandomState(i)) for i, param in enumerate(like.varied_params)], axis=-1))
    quota = WARMUP + TIMED
    buffers = engine.buffers(quota)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    engine.run(WARMUP, quota, buffers)
    torch.cuda.synchronize()
    t_iter = []
    for _ in range(TIMED):
        start.record(); engine.run(1, quota, buffers); stop.record(); torch.cuda.synchronize()
        t_iter.append(start.elapsed_time(stop) * 1e3)
    assert np.all(engine.counts(buffers) == quota)
    device = 'cuda:{:d}'.format(ctx.device)
    x = torch.as_tensor(engine.get_state()[0][:, :M].reshape(-1, ctx.n_params), device=device).contiguous()
    L, pi, status = torch.empty(len(x), dtype=torch.float64, device=device), torch.empty(len(x), dtype=torch.float64, device=device), torch.empty(len(x), dtype=torch.int32, device=device)
    for _ in range(WARMUP * N_STEPS): ctx.eval_batch(x, loglike=L, logprior=pi, status=status)
    torch.cuda.synchronize()
    t_eval = []
    for _ in range(TIMED):
        start.record()
        for _ in range(N_STEPS): ctx.eval_batch(x, loglike=L, logprior=pi, status=status)
        stop.record(); torch.cuda.synchronize()
        t_eval.append(start.elapsed_time(stop) * 1e3)
    t_iter, t_eval = float(np.median(t_iter)), float(np.median(t_eval))
    return {'runs': K, 'nlive': N, 'ndelete': M, 'us_per_iteration': t_iter, 'us_evaluations': t_eval, 'us_nested_kernels': t_iter - t_eval,
            'nested_kernels_over_evaluations': (t_iter - t_eval) / t_eval, 'evaluations_per_s': rows * N_STEPS / (t_iter * 1e-6)}


def evidence():
    sampler = NestedSampler(make_cfg2()[1], nlive=N, chains=4, seed=1, n_steps=N_STEPS)
    sampler.run()
    return {'iterations': sampler.niterations.tolist(), 'evaluations': sampler.nevaluations, 'logz': sampler.logz.tolist(), 'logz_err': sampler.logz_err.tolist(),
            'information': sampler.information.tolist(), 'logz_mean': sampler.logz_mean, 'logz_std': sampler.logz_std}


def main(rows, with_evidence=True):
    results = {str(r): iteration_timings(r) for r in rows}
    print(json.dumps({'probe': 'nested', 'config': 'cfg2', 'n_steps': N_STEPS, 'results': results, 'evidence': evidence() if with_evidence else None}))


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--timings-only']       # --timings-only: without the evidence run (a kernel trace of the timed shapes alone)
    main([int(a) for a in args] or [256, 1024, 4096], with_evidence=len(args) == len(sys.argv[1:]))
