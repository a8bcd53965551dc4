"""Analytic gradient of the emulated configs[2] likelihood (make_cfg3_full, marg) at 4096 points: us per call of dl_eval_logposterior, dl_eval_logposterior_grad and
the 2 P + 1 = 21-row central-difference batch (one dl_eval_logposterior call on 21 x 4096 rows), between device events after a warm-up; with --nuts also NUTSSampler ESS
per second of every parameter (256 chains, 150 warm-up iterations, 150 samples; samples / integrated autocorrelation time over the wall time of the sampling batch)
with the analytic and with the finite-difference gradient.  Prints ONE JSON line.
    python tools/emu_grad_probe.py [points] [repeats] [--nuts]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from bench_configs import make_cfg3_full


def timed(fn, repeats):
    for _ in range(3): fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(repeats): fn()
    stop.record()
    torch.cuda.synchronize()
    return 1e3 * start.elapsed_time(stop) / repeats


def nuts_ess(gradient, nchains=256, warmup=150, samples=150):
    import time
    from desilike_amd.samplers import NUTSSampler
    from desilike_amd.diagnostics import integrated_autocorrelation_time
    g, like, pt, theory, solved = make_cfg3_full(marg=True)
    s = NUTSSampler(like, chains=nchains, seed=11, gradient=gradient, adaptation={'niterations': warmup})
    s.run(check_every=warmup, max_iterations=warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    chains = s.run(check_every=samples, max_iterations=samples)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    ess = []
    for name in s.varied_params.names():
        x = np.array([chain[name][-samples:] for chain in chains])
        ess.append(x.size / max(float(integrated_autocorrelation_time(x)), 1.) / seconds)
    return dict(seconds=seconds, ess_per_s_min=min(ess), ess_per_s_max=max(ess), acceptance=float(np.mean(s.acceptance_rate)))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    B = int(args[0]) if len(args) > 0 else 4096
    repeats = int(args[1]) if len(args) > 1 else 20
    g, like, pt, theory, solved = make_cfg3_full(marg=True)
    ctx = like._get_context()
    dev = 'cuda:{:d}'.format(ctx.device)
    rng = np.random.RandomState(3)
    theta = np.column_stack([np.clip(p.ref.sample(size=B, random_state=rng), *p.prior.limits) for p in like.varied_params])
    P = theta.shape[1]
    t = torch.as_tensor(theta, device=dev).contiguous()
    lp, grad = torch.empty(B, dtype=torch.float64, device=dev), torch.empty((B, P), dtype=torch.float64, device=dev)
    stencil = torch.as_tensor(np.repeat(theta, 2 * P + 1, axis=0), device=dev).contiguous()
    lps = torch.empty(stencil.shape[0], dtype=torch.float64, device=dev)
    out = dict(points=B, n_params=P)
    out['eval_us'] = timed(lambda: ctx.eval_logposterior(t, lp), repeats)
    out['grad_us'] = timed(lambda: ctx.eval_logposterior_grad(t, lp, grad), repeats)
    out['finite_us'] = timed(lambda: ctx.eval_logposterior(stencil, lps), max(2, repeats // 4))
    out['grad_over_eval'] = out['grad_us'] / out['eval_us']
    out['finite_over_eval'] = out['finite_us'] / out['eval_us']
    if '--nuts' in sys.argv:
        for gradient in ('analytic', 'finite'): out['nuts_' + gradient] = nuts_ess(gradient)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
