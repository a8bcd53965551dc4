"""GPU: the device-resident nested sampler (dl_nested_*, desilike_amd/nested.py _DeviceNested) against the NumPy statement of the same stage machine (_HostNested)
fed by the context's own dl_eval_batch, its largest tile, its evidence against a quadrature and against SMCSampler, its posterior, its repeatability, state and errors."""

import numpy as np
import pytest

from test_gpu_smc import _like, _quadrature, _terms
from test_host_api import make_cfg2
from test_nested import F, _assert_above

pytestmark = pytest.mark.gpu

SEED = 5


def _engines(config, K, N, M, n_steps=4, seed=SEED, host=True, dlogz=0.01):
    """(_DeviceNested, _HostNested) on the same live points drawn from the priors."""
    from desilike_amd.nested import NestedSampler, _DeviceNested, _HostNested
    like = _like(config)
    sampler = NestedSampler(like, nlive=N, chains=K, ndelete=M, seed=seed)
    ctx, offset = like._get_posterior_context()
    start = np.stack([param.prior.sample(size=(K, N), random_state=np.random.RandomState(100 + i)) for i, param in enumerate(like.varied_params)], axis=-1)
    engines = [_DeviceNested(ctx, offset, K, N, sampler.widths, seed=seed)]
    if host: engines.append(_HostNested(_terms(ctx), K, N, len(like.varied_params), sampler.widths, seed=seed, offset=offset))
    for engine in engines:
        engine.set_hyper(M, n_steps, 0.234, dlogz)
        engine.set_live(start)
    return engines + [like, offset]


def _close(a, b):
    assert np.allclose(a, b, rtol=1e-10, atol=1e-8), float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


# ---- 5. the device equals the host statement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config,K,N,M', [('cfg2', 2, 256, 64), ('cfg2', 3, 64, 1), ('cfg2', 1, 320, 24), ('cfg5', 2, 256, 128), ('two', 2, 256, 64), ('five', 2, 128, 32)])
def test_device_equals_the_host_statement(config, K, N, M):
    """Iteration by iteration, for 12 iterations or to rest: the same ranks, seeds and accept flags; the history, the moments, the dead records and the state to rtol
    1e-10 / atol 1e-8.  FIRST: the smallest margin of the host run's decisions is >= 1e-9 (seed 5 for every case; measured on the MI355X: 2.3e-5 .. 7.9e-3 over the six
    cases, 117 .. 12019 decisions each, no run at rest within the 12 iterations)."""
    from desilike_amd.nested import REST
    dev, host, like, offset = _engines(config, K, N, M)
    quota = 12
    hb, steps = host.buffers(quota), []
    while len(steps) < quota and np.any(host.modes(hb) != REST):
        host.run(1, quota, hb)
        steps.append([np.array(a) for a in host.get_decisions()])
    n = len(steps)
    print(config, K, N, M, 'iterations', n, 'decisions', host.ndecisions, 'smallest margin', host.min_margin)
    assert host.min_margin >= 1e-9
    db = dev.buffers(quota)
    for it, (ranks, seeds, flags, mean, cov) in enumerate(steps):
        dev.run(1, quota, db)
        dranks, dseeds, dflags, dmean, dcov = dev.get_decisions()
        assert np.array_equal(dranks, ranks), 'ranks differ in iteration {:d}'.format(it)
        assert np.array_equal(dseeds, seeds), 'seeds differ in iteration {:d}'.format(it)
        assert np.array_equal(dflags, flags), 'accept flags differ in iteration {:d}'.format(it)
        _close(dmean, mean); _close(dcov, cov)
    counts = host.counts(hb)
    assert np.array_equal(dev.counts(db), counts) and np.array_equal(dev.modes(db), host.modes(hb)) and counts.max() == n
    for d, h in zip(dev.records(db), host.records(hb)):
        for k in range(K): _close(d[k, :counts[k]], h[k, :counts[k]])
    for a, b in zip(dev.get_state(), host.get_state()): _close(a, b)
    history = dev.records(db)[0]
    assert np.all(np.isfinite(history[0, :counts[0]])) and np.all(np.diff(history[0, :counts[0], 2]) >= 0.) and (offset != 0.) == (config == 'cfg5')
    assert dev.evaluations == host.evaluations == K * (N + M * 4 * n)


# ---- 6. the largest tile ---------------------------------------------------------------------------------------------------------------------------------------
def test_largest_tile():
    """K = 1, N = 8192 (the full sort, 139840 bytes of LDS), M = 2048 (two prefix sums per thread), n_steps = 2, three iterations, twice: the invariants of the stage
    machine and the same bits."""
    from desilike_amd.nested import closing
    N, M, runs = 8192, 2048, []
    for _ in range(2):
        dev = _engines('cfg2', 1, N, M, n_steps=2, host=False)[0]
        buffers, decisions = dev.buffers(3), []
        for it in range(3):
            before = dev.get_state()[1][0]
            dev.run(1, 3, buffers)
            ranks, seeds = dev.get_decisions()[:2]
            assert np.array_equal(ranks[0], np.lexsort((np.arange(N), before)))
            assert np.all(np.isin(seeds[0], ranks[0, M:]))
            _assert_above(dev.get_state(), dev.records(buffers), it)
            decisions.append((ranks, seeds))
        runs.append((dev.records(buffers), dev.get_state(), decisions))
    (history, coords, dL, dpi, dlogw), state, decisions = runs[0]
    shrink = np.sum(1. / (N - np.arange(M)))
    assert np.allclose(history[0, :, 0], -np.arange(1, 4) * shrink, rtol=1e-12, atol=0.) and np.allclose(state[3], -3. * shrink, rtol=1e-12, atol=0.)
    assert np.all(np.diff(history[0, :, 2]) >= 0.) and np.all(np.diff(dL[0].ravel()) >= 0.) and np.all(np.diff(history[0, :, 1]) > 0.)
    closed = closing(dL[0], dlogw[0], state[1][0], state[3][0])
    assert abs(np.exp(closed['logweight']).sum() - 1.) <= 1e-12
    assert np.all((history[0, :, 3] > 0.) & (history[0, :, 3] < 1.)) and np.all(state[5] == 3)
    for a, b in zip(runs[0][0], runs[1][0]): assert np.array_equal(a, b)
    for a, b in zip(state, runs[1][1]): assert np.array_equal(a, b)
    for (r0, s0), (r1, s1) in zip(decisions, runs[1][2]): assert np.array_equal(r0, r1) and np.array_equal(s0, s1)


# ---- 7. evidence against a quadrature ----------------------------------------------------------------------------------------------------------------------------
def _information(like, nodes):
    """(log Z, H) of the two-parameter likelihood on the grid of ``_quadrature`` (its box of +- 8 Fisher widths about the posterior's maximum, Gauss-Legendre): H =
    the posterior mean of the log-likelihood - log Z, the Kullback-Leibler divergence of the posterior from the normalised priors."""
    ctx, offset = like._get_posterior_context()
    params = like.varied_params
    f = lambda x: ctx.eval_logposterior_host(np.atleast_2d(x))[0] + offset
    x = np.array([param.value for param in params], dtype='f8')
    h = np.array([param.proposal for param in params]) * 0.1
    for _ in range(6):          # Newton steps on central differences
        e = np.diag(h)
        stencil = np.array([x] + [x + e[i] for i in range(2)] + [x - e[i] for i in range(2)] + [x + e[0] + e[1], x - e[0] - e[1], x + e[0] - e[1], x - e[0] + e[1]])
        v = f(stencil)
        grad = np.array([(v[1] - v[3]) / (2. * h[0]), (v[2] - v[4]) / (2. * h[1])])
        cross = (v[5] + v[6] - v[7] - v[8]) / (4. * h[0] * h[1])
        hess = np.array([[(v[1] + v[3] - 2. * v[0]) / h[0]**2, cross], [cross, (v[2] + v[4] - 2. * v[0]) / h[1]**2]])
        x = x - np.linalg.solve(hess, grad)
    width = np.sqrt(np.diag(np.linalg.inv(-hess)))
    lo = np.array([max(x[i] - 8. * width[i], params[i].prior.limits[0]) for i in range(2)])
    hi = np.array([min(x[i] + 8. * width[i], params[i].prior.limits[1]) for i in range(2)])
    t, w = np.polynomial.legendre.leggauss(nodes)
    axes = [0.5 * (hi[i] - lo[i]) * t + 0.5 * (hi[i] + lo[i]) for i in range(2)]
    grid = np.array([[a, b] for a in axes[0] for b in axes[1]])
    loglike, logprior = _terms(ctx)(grid)
    norm = sum(float(param.prior.logpdf(x[i], remove_zerolag=False) - param.prior.logpdf(x[i])) for i, param in enumerate(params))
    lp = (loglike + offset + logprior + norm).reshape(nodes, nodes)
    top = lp.max()
    p = np.einsum('i,j,ij->ij', w, w, np.exp(lp - top)) * 0.25 * np.prod(hi - lo)
    logz = top + np.log(p.sum())
    return logz, float(np.sum(p / p.sum() * (loglike + offset).reshape(nodes, nodes)) - logz)


def _assert_evidence(sampler, exact, H):
    K, N = sampler.nchains, sampler.nlive
    unit = np.sqrt(H / N)
    print('{:d} runs: logz_mean {:.4f} yardstick {:.4f} logz_std {:.4f} sqrt(H / N) {:.4f} logz_err {:.4f} .. {:.4f} H {:.3f} .. {:.3f} yardstick {:.3f} iterations {:d} .. {:d} '
          'evaluations {:d}'.format(K, sampler.logz_mean, exact, sampler.logz_std, unit, sampler.logz_err.min(), sampler.logz_err.max(), sampler.information.min(),
                                    sampler.information.max(), H, sampler.niterations.min(), sampler.niterations.max(), sampler.nevaluations))
    assert abs(sampler.logz_mean - exact) <= 4. * F * unit / np.sqrt(K)
    assert sampler.logz_std <= 2. * F * unit
    assert np.all(np.abs(sampler.logz_err / unit - 1.) <= 0.25)


def test_evidence_against_quadrature():
    """The two-parameter cfg2 likelihood (b1, sn0): NestedSampler(chains=8, nlive=1024), then chains=64, against the 2-D Gauss-Legendre quadrature of exp(loglike) prior
    of tests/test_gpu_smc.py (-15.052629); H from the same grid (14.046; 64 against 128 nodes: 7e-15); the conditions of tests/test_nested.py with its measured f.
    Measured on the MI355X (68 - 70 iterations): 8 runs logz_mean -15.120, scatter 0.208 = 1.78 sqrt(H / N), logz_err 0.117 .. 0.119; 64 runs -15.035, 0.141 = 1.20 sqrt(H / N)."""
    from desilike_amd.samplers import NestedSampler
    like = _like('two')
    exact = _quadrature(like, 128)
    logz, H = _information(like, 128)
    coarse = _information(like, 64)
    print('quadrature', exact, 'on the grid of H', logz, 'H', H, 'at 64 nodes', coarse)
    assert abs(logz - exact) <= 1e-9 and abs(coarse[1] - H) <= 1e-6 and H > 0.
    sampler = NestedSampler(like, nlive=1024, chains=8, seed=4)
    assert sampler.device_resident and sampler.n_steps == 8 and sampler.ndelete == 256
    sampler.run()
    _assert_evidence(sampler, exact, H)
    many = NestedSampler(_like('two'), nlive=1024, chains=64, seed=4)
    many.run()
    _assert_evidence(many, exact, H)


# ---- 8. cfg2 against SMC, and the posterior ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cfg2_run():
    from desilike_amd.samplers import NestedSampler
    like = make_cfg2()[1]
    sampler = NestedSampler(like, nlive=1024, chains=4, seed=2)
    assert sampler.device_resident and sampler.n_steps == 24 and sampler.ndelete == 256
    sampler.run()
    return like, sampler


def test_evidence_against_smc(cfg2_run):
    """cfg2 (P = 6): the log of the mean Z of NestedSampler(chains=4, nlive=1024) within 4 combined standard errors of that of SMCSampler(chains=8, nparticles=1024)
    (-17.726 in DESIGN.md 6g), the standard error of each from the scatter over its own runs.  Measured on the MI355X: -17.728 (scatter 0.243 over 4 runs, 77 - 79
    iterations) against -17.726 (0.161 over 8 systems), combined standard error 0.134."""
    from desilike_amd.samplers import SMCSampler
    like, sampler = cfg2_run
    smc = SMCSampler(make_cfg2()[1], nparticles=1024, chains=8, seed=1)
    smc.run(max_iterations=1)
    se = np.sqrt(sampler.logz_std**2 / 4. + smc.logz_std**2 / 8.)
    print('nested logz', sampler.logz, 'logz_mean', sampler.logz_mean, 'logz_std', sampler.logz_std, 'logz_err', sampler.logz_err, 'H', sampler.information, 'iterations',
          sampler.niterations, 'evaluations', sampler.nevaluations, '| smc logz_mean', smc.logz_mean, 'logz_std', smc.logz_std, 'evaluations', smc.nevaluations, '| combined se', se)
    assert abs(sampler.logz_mean - smc.logz_mean) <= 4. * se


def test_nested_posterior_on_the_device(cfg2_run):
    """cfg2: the aweight-weighted means and standard deviations against EmceeSampler (the run and the bounds of test_smc_posterior_on_the_device)."""
    from desilike_amd.samplers import EmceeSampler
    like, sampler = cfg2_run
    names = like.varied_params.names()
    chains = sampler.chains
    x = np.column_stack([np.concatenate([chain[name] for chain in chains]) for name in names])
    w = np.concatenate([chain['aweight'] for chain in chains]) / len(chains)
    assert all(np.all(np.isfinite(chain['logposterior'])) for chain in chains) and abs(w.sum() - 1.) <= 1e-12
    for i, param in enumerate(like.varied_params): assert np.all((x[:, i] > param.prior.limits[0]) & (x[:, i] < param.prior.limits[1]))
    mean = w @ x
    std = np.sqrt(w @ (x - mean)**2)
    ens = EmceeSampler(make_cfg2()[1], nwalkers=64, seed=3)
    chain = ens.run(niterations=1500)
    y = np.column_stack([chain[name][500:].ravel() for name in names])
    print('mean shift / sigma', (mean - y.mean(axis=0)) / y.std(axis=0), 'std ratio', std / y.std(axis=0), 'effective count', 1. / np.sum(w**2))
    assert np.all(np.abs(mean - y.mean(axis=0)) < 0.3 * y.std(axis=0)), (mean, y.mean(axis=0), y.std(axis=0))
    assert np.allclose(std, y.std(axis=0), rtol=0.25)
    draw = sampler.samples(4096, random_state=np.random.RandomState(0))
    assert np.all(np.abs(np.array([draw[name].mean() for name in names]) - y.mean(axis=0)) < 0.3 * y.std(axis=0))


# ---- 9. repeatability and state ----------------------------------------------------------------------------------------------------------------------------------
def test_repeatability_chunking_and_state():
    from desilike_amd.nested import run_batch
    runs = []
    for chunk in (None, None, 3):
        dev = _engines('cfg2', 2, 128, 32, host=False)[0]
        runs.append(run_batch(dev, 12, chunk=chunk) + tuple(dev.get_state()))
    counts = runs[0][5]
    assert np.all(counts == 12)
    for other in runs[1:]:
        for a, b in zip(runs[0], other): assert np.array_equal(a, b)
    # a get_state / set_state round trip continues bit for bit
    first = _engines('cfg2', 2, 128, 32, host=False)[0]
    head = run_batch(first, 5)
    second = _engines('cfg2', 2, 128, 32, host=False)[0]
    state = first.get_state()
    second.set_state(*state)
    for a, b in zip(state, second.get_state()): assert np.array_equal(a, b)
    tail = run_batch(second, 7)
    for i in range(5): assert np.array_equal(np.concatenate([head[i], tail[i]], axis=1), runs[0][i])
    for a, b in zip(second.get_state(), runs[0][7:]): assert np.array_equal(a, b)
    # a run at rest does nothing and records nothing
    state = list(second.get_state())
    state[7] = np.array([0, 1], dtype='i4')
    second.set_state(*state)
    after = run_batch(second, 2)
    assert np.array_equal(after[5], [0, 2]) and np.array_equal(after[6][:1], [0])
    for a, b in zip(state, second.get_state()): assert np.array_equal(a[0], b[0])


def test_state_round_trip_and_errors():
    from desilike_amd._lib import DeviceNested, LibraryError
    like = make_cfg2()[1]
    ctx = like._get_context()
    P, widths = ctx.n_params, np.ones(ctx.n_params)
    nested = DeviceNested(ctx, 2, 64, widths, seed=3)
    assert [nested.info(key) for key in ['nruns', 'nlive', 'n_params', 'iterations', 'evaluations']] == [2, 64, P, 0, 0]
    start = np.stack([param.prior.sample(size=(2, 64), random_state=np.random.RandomState(i)) for i, param in enumerate(like.varied_params)], axis=-1)
    with pytest.raises(LibraryError, match='hyper'): nested.get_decisions()
    nested.set_hyper(16, 2, 0.234, 0.01)
    with pytest.raises(LibraryError, match='live points'): nested.run(1, 1, nested.buffers(1))
    nested.set_live(start)
    coords, L, pi, logx, logz, counters, scale, modes = nested.get_state()
    assert np.array_equal(coords, start) and np.all(np.isfinite(L)) and np.all(np.isfinite(pi)) and np.all(logx == 0.) and np.all(logz == -np.inf) and np.all(counters == 0)
    assert np.all(scale == 1.) and np.all(modes == 1) and nested.info('evaluations') == 128 and nested.info('ndelete') == 16
    outside = start.copy(); outside[1, 7, 0] = 5.
    with pytest.raises(LibraryError, match='live point 7 of run 1'): nested.set_live(outside)
    with pytest.raises(LibraryError, match='live points'): nested.run(1, 1, nested.buffers(1))          # (a refused set_live leaves no state behind)
    bad = start.copy(); bad[0, 0, 0] = np.nan
    with pytest.raises(LibraryError, match='finite'): nested.set_live(bad)
    for ndelete in (0, 33):
        with pytest.raises(LibraryError, match='ndelete'): nested.set_hyper(ndelete, 2, 0.234, 0.01)
    with pytest.raises(LibraryError, match='n_steps'): nested.set_hyper(16, 0, 0.234, 0.01)
    with pytest.raises(LibraryError, match='target_acceptance'): nested.set_hyper(16, 2, 1., 0.01)
    for dlogz in (0., 1.):
        with pytest.raises(LibraryError, match='dlogz'): nested.set_hyper(16, 2, 0.234, dlogz)
    with pytest.raises(LibraryError, match='multiple of 64'): DeviceNested(ctx, 2, 100, widths)
    with pytest.raises(LibraryError, match='multiple of 64'): DeviceNested(ctx, 2, 16384, widths)
    with pytest.raises(LibraryError, match='nruns'): DeviceNested(ctx, 0, 64, widths)
    with pytest.raises(LibraryError, match='widths'): DeviceNested(ctx, 2, 64, np.zeros(P))
    with pytest.raises(LibraryError, match='logx'): nested.set_state(coords, L, pi, logx + 1., logz, counters, scale, modes)
    broken = L.copy(); broken[1, 3] = -np.inf
    with pytest.raises(LibraryError, match='live point 3 of run 1 has no finite log-likelihood'): nested.set_state(coords, broken, pi, logx, logz, counters, scale, modes)
    with pytest.raises(LibraryError, match='mode'): nested.set_state(coords, L, pi, logx, logz, counters, scale, [2, 1])
    nested.set_state(coords, L, pi, [-0.25, -1.], [-3., -np.inf], [5, 6], [0.5, 2.], [0, 1])
    again = nested.get_state()
    assert np.array_equal(again[3], [-0.25, -1.]) and np.array_equal(again[4], [-3., -np.inf]) and np.array_equal(again[5], [5, 6]) and np.array_equal(again[6], [0.5, 2.])
    assert np.array_equal(again[0], coords) and np.array_equal(again[1], L) and np.array_equal(again[7], [0, 1])
