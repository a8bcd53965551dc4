"""Measurement of the wiggle-split template path (csrc/dl_wigglesplit.h) on one GPU, one session:

    python tools/wigglesplit_probe.py [--repeats 30]

* the theory launches of the 'kaiser' fixture's observable (``dl_eval_theory``: template kernel + theory kernel) at 1024 and 4096 points beside the SAME observable on the
  ShapeFit template (theory kernel alone): events, after warm-up, median of ``--repeats`` (>= 20) launches; their difference is the template kernel's time per launch;
* whole-step evaluations per second of the fixture's likelihood (``dl_eval_batch``) beside the same likelihood on the ShapeFit template -- the nearest existing path, for
  context: not a pass mark;
* the template kernel's floating-point operation count per point (from the phase counts below) and the fraction of the fp64 vector peak it reaches.

Prints one JSON line.  The fixture's ``ref_seconds_per_eval`` (the reference's time per likelihood call, measured through the stub on a CPU) is copied into it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

FP64_VECTOR_PEAK = 78.6e12     # MI355X, FLOP/s (public specification)
EXP_FLOPS = 25                 # fp64 operations of one exp / log in the device library (order of magnitude; counted apart below)


def flop_count(n_i, n_q, n_t):
    """(arithmetic, transcendental calls) per point, from the phases of dl_wigglesplit.h: an FMA is two operations."""
    knots = n_i * (2 * 3 * 2 + 6)                      # two cubics (3 FMA each), abscissa, clamp, sum
    fir = n_i * 57 * 2                                 # 57-tap convolution
    evaluate = (n_q + n_t) * (2 * 4 + 3 + 2 + 2)       # cubic from (value, moment) pairs, the dm term, the weight
    calls = 3 * n_i + n_q + n_t                        # two exp and one log10 per inner knot, one exp per node / template knot
    return knots + fir + evaluate, calls


def median_us(fn, repeats, stream):
    import torch
    for _ in range(5): fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream); fn(); stop.record(stream)
        stop.synchronize()
        times.append(1e3 * start.elapsed_time(stop))
    return float(np.median(times))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--repeats', type=int, default=30)
    args = parser.parse_args()
    assert args.repeats >= 20
    import torch
    import wigglesplit_utils as wsu
    from desilike_amd._lib import Context
    g, cfg = wsu.load_fixture('kaiser')
    shapefit = {key: value for key, value in cfg.items() if '.ws_' not in key and key != 'obs0.in.qbao'}
    shapefit['obs0.template'] = np.array([1], dtype='i4')     # the same observable on the ShapeFit template: dm acts through its own factor, qbao not at all
    contexts = {'wigglesplit': Context(cfg, device=0), 'shapefit': Context(shapefit, device=0)}
    device = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(device)
    n_i, n_q, n_t = len(cfg['obs0.ws_k']), 2048, len(cfg['obs0.k_t'])
    flops, calls = flop_count(n_i, n_q, n_t)
    out = dict(n_inner=n_i, n_nodes=n_q, n_knots=n_t, flops_per_point=flops, transcendental_calls_per_point=calls, ref_seconds_per_eval=float(g['ref_seconds_per_eval'][0]))
    rng = np.random.RandomState(3)
    for B in (1024, 4096):
        theta = torch.as_tensor(g['theta'][rng.randint(0, 48, size=B)], device=device).contiguous()
        for name, ctx in contexts.items():
            n_ell, n_kin = ctx.info('n_ell_obs0'), ctx.info('n_kin_obs0')
            power = torch.empty((B, n_ell, n_kin), dtype=torch.float64, device=device)
            loglike, logprior = torch.empty(B, dtype=torch.float64, device=device), torch.empty(B, dtype=torch.float64, device=device)
            status = torch.empty(B, dtype=torch.int32, device=device)
            out['theory_us_{}_{:d}'.format(name, B)] = median_us(lambda: ctx.eval_theory(theta, power), args.repeats, stream)
            step = median_us(lambda: ctx.eval_batch(theta, loglike=loglike, logprior=logprior, status=status), args.repeats, stream)
            out['step_us_{}_{:d}'.format(name, B)] = step
            out['evals_per_s_{}_{:d}'.format(name, B)] = B / (1e-6 * step)
        kernel = out['theory_us_wigglesplit_{:d}'.format(B)] - out['theory_us_shapefit_{:d}'.format(B)]
        out['template_kernel_us_{:d}'.format(B)] = kernel
        out['template_kernel_flops_fraction_{:d}'.format(B)] = B * (flops + EXP_FLOPS * calls) / (1e-6 * kernel) / FP64_VECTOR_PEAK
    print(json.dumps(out))


if __name__ == '__main__':
    main()
