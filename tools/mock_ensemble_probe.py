"""Time "a posterior per mock" both ways on the cfg2 likelihood (ShapeFit + Kaiser + window, 6 varied parameters):
    python tools/mock_ensemble_probe.py [--ensembles 64] [--nwalkers 32] [--iterations 200] [--repeats 3] [--route-b-mocks 64]

route A: ONE MockEmceeSampler on likelihood.data_batch(mocks): E ensembles in lockstep (dl_ensemble_data_*), one step kernel and one paired evaluation per half-step.
route B: what exists without it: E per-mock likelihoods (mock m as their own data), each through its own device-resident EmceeSampler(nwalkers), run one after another.
         The route is a loop over mocks: with more than --route-b-mocks mocks that many are created and timed and the figure is scaled to E ("route_b_scaled").
Both are warmed up (contexts, ensembles, buffers), then timed alternately --repeats times with a host clock around runs that end in a synchronisation (the chain's copy to
the host); the medians are reported.  Creation (data batch / per-mock contexts and ensembles) is excluded from both and stated separately.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--ensembles', type=int, default=64)
    parser.add_argument('--nwalkers', type=int, default=32)
    parser.add_argument('--iterations', type=int, default=200)
    parser.add_argument('--repeats', type=int, default=3)
    parser.add_argument('--route-b-mocks', type=int, default=64)
    args = parser.parse_args()
    warnings.simplefilter('ignore')
    import torch
    from bench_configs import make_cfg2
    from desilike_amd import MockEmceeSampler
    from desilike_amd.samplers import EmceeSampler
    E, nw, T = args.ensembles, args.nwalkers, args.iterations
    like = make_cfg2()[1]
    like.initialize()
    flatdata = np.concatenate(like._flatdata_list())
    mocks = flatdata + 0.05 * np.abs(flatdata) * np.random.RandomState(5).standard_normal((E, flatdata.size))

    t0 = time.perf_counter()
    batch = like.data_batch(mocks)
    sampler = MockEmceeSampler(batch, nwalkers=nw, seed=1)
    sampler.run(10)
    create_a = time.perf_counter() - t0

    nb = min(E, args.route_b_mocks)
    t0 = time.perf_counter()
    singles = [EmceeSampler(make_cfg2(data=mocks[m])[1], nwalkers=nw, seed=1 + m) for m in range(nb)]
    for single in singles: single.run(niterations=10)
    create_b = time.perf_counter() - t0
    torch.cuda.synchronize()

    times_a, times_b = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        sampler.run(T)
        times_a.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for single in singles: single.run(niterations=T)
        times_b.append((time.perf_counter() - t0) * E / nb)
    a, b = 1e6 * float(np.median(times_a)) / T, 1e6 * float(np.median(times_b)) / T
    print(json.dumps(dict(ensembles=E, nwalkers=nw, iterations=T, rows_per_half_step=E * nw // 2, route_a_us_per_update=a, route_b_us_per_update=b, ratio_b_over_a=b / a,
                          route_a_all_us=[1e6 * t / T for t in times_a], route_b_all_us=[1e6 * t / T for t in times_b], route_b_mocks_timed=nb, route_b_scaled=nb < E,
                          create_a_s=create_a, create_b_s=create_b * E / nb, acceptance_a=float(sampler.acceptance_fraction.mean()),
                          acceptance_b=float(np.mean([single.acceptance_fraction.mean() for single in singles])))))


if __name__ == '__main__':
    main()
