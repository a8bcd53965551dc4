"""GPU: the device-resident tempered sequential Monte Carlo sampler (dl_smc_*, desilike_amd/smc.py _DeviceSMC) against the NumPy statement of the same stage machine
(_HostSMC) fed by the context's own dl_eval_batch, its largest tile, its evidence against a quadrature, its posterior, its repeatability, state and errors."""

import numpy as np
import pytest

from test_host_api import make_cfg2, make_cfg5

pytestmark = pytest.mark.gpu


def _like(config):
    if config == 'cfg5':             # *.sn0 marginalised: the constant of the marginalisation travels as the offset; two observables
        like = make_cfg5()[1]
        like.all_params = {'*.sn0': {'derived': '.marg'}}
        return like
    like = make_cfg2()[1]
    fixed = {'cfg2': [], 'two': ['qpar', 'qper', 'dm', 'df'], 'five': ['dm']}[config]      # 'two': P = 2, lanes 2 .. 63 idle; 'five': an odd P
    if fixed: like.all_params = {name: {'fixed': True} for name in fixed}
    return like


def _terms(ctx):
    """f(x [B, P]) -> (loglike, logprior) through the context's dl_eval_batch; a row whose status is not 0 has no likelihood (what the device engine does with it)."""
    import torch

    def f(x):
        device = 'cuda:{:d}'.format(ctx.device)
        t = torch.as_tensor(np.ascontiguousarray(x), device=device)
        L, pi = torch.empty(len(x), dtype=torch.float64, device=device), torch.empty(len(x), dtype=torch.float64, device=device)
        status = torch.empty(len(x), dtype=torch.int32, device=device)
        ctx.eval_batch(t, loglike=L, logprior=pi, status=status)
        L, pi, status = L.cpu().numpy(), pi.cpu().numpy(), status.cpu().numpy()
        L[status != 0] = -np.inf
        return L, pi

    return f


def _engines(config, K, N, n_steps=4, seed=5, host=True):
    """(_DeviceSMC, _HostSMC) on the same particles drawn from the priors."""
    from desilike_amd.smc import SMCSampler, _DeviceSMC, _HostSMC
    like = _like(config)
    sampler = SMCSampler(like, nparticles=N, chains=K, seed=seed)
    ctx, offset = like._get_posterior_context()
    start = np.stack([param.prior.sample(size=(K, N), random_state=np.random.RandomState(100 + i)) for i, param in enumerate(like.varied_params)], axis=-1)
    engines = [_DeviceSMC(ctx, offset, K, N, sampler.widths, seed=seed)]
    if host: engines.append(_HostSMC(_terms(ctx), K, N, len(like.varied_params), sampler.widths, seed=seed, offset=offset))
    for engine in engines:
        engine.set_hyper(0.5, n_steps, 0.234)
        engine.set_particles(start)
    return engines + [like, offset]


def _close(a, b):
    assert np.allclose(a, b, rtol=1e-10, atol=1e-8), float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


# ---- 5. the device equals the host statement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config,K,N', [('cfg2', 2, 256), ('cfg2', 3, 64), ('cfg2', 1, 320), ('cfg5', 2, 256), ('two', 2, 256), ('five', 2, 128)])
def test_device_equals_the_host_statement(config, K, N):
    """Iteration by iteration until every system has done two sweeps at beta = 1: the same ancestors and accept flags; beta, logZ, ESS, acceptance, scale, the moments
    and the particles to rtol 1e-10 / atol 1e-8.  FIRST: the smallest margin of the host run's decisions is >= 1e-9 (seed 5 for every case)."""
    dev, host, like, offset = _engines(config, K, N)
    quota = 80
    hb, steps = host.buffers(quota), []
    while host.counts(hb)[:, 1].min() < 2:
        assert len(steps) < quota, 'beta = 1 not reached'
        host.run(1, quota, hb)
        steps.append([np.array(a) for a in host.get_decisions()])
    print(config, K, N, 'iterations', len(steps), 'decisions', host.ndecisions, 'smallest margin', host.min_margin)
    assert host.min_margin >= 1e-9
    db = dev.buffers(quota)
    for it, (anc, flags, mean, cov) in enumerate(steps):
        dev.run(1, quota, db)
        danc, dflags, dmean, dcov = dev.get_decisions()
        assert np.array_equal(danc, anc), 'ancestors differ in iteration {:d}'.format(it)
        assert np.array_equal(dflags, flags), 'accept flags differ in iteration {:d}'.format(it)
        tempered = np.any(anc != np.arange(N), axis=1)
        _close(dmean[tempered], mean[tempered]); _close(dcov[tempered], cov[tempered])
    (hd, cd, ld), (hh, ch, lh) = dev.records(db), host.records(hb)
    counts = host.counts(hb)
    assert np.array_equal(dev.counts(db), counts) and np.all(counts[:, 0] == len(steps)) and np.all(counts[:, 1] >= 2)
    n = len(steps)
    assert np.array_equal(hd[:, :n, 0] == 1., hh[:, :n, 0] == 1.) and np.all(hd[:, n - 1, 0] == 1.)
    _close(hd[:, :n], hh[:, :n])
    for k in range(K): _close(cd[k, :counts[k, 1]], ch[k, :counts[k, 1]]); _close(ld[k, :counts[k, 1]], lh[k, :counts[k, 1]])
    for a, b in zip(dev.get_state(), host.get_state()): _close(a, b)
    assert np.all(np.isfinite(ld[0, :counts[0, 1]])) and (offset != 0.) == (config == 'cfg5')
    assert dev.evaluations == host.evaluations == K * N * (1 + 4 * n)


# ---- 6. the largest tile ---------------------------------------------------------------------------------------------------------------------------------------
def test_largest_tile():
    """K = 1, N = 16384 (the scan's 16-per-thread path, 128 KB of L in LDS), three iterations, twice: the invariants of the stage machine and the same bits."""
    from desilike_amd import smc
    N, runs = 16384, []
    for _ in range(2):
        dev = _engines('cfg2', 1, N, n_steps=2, host=False)[0]
        buffers, before, anc = dev.buffers(3), [], []
        for it in range(3):
            before.append(dev.get_state())
            dev.run(1, 3, buffers)
            anc.append(dev.get_decisions()[0])
        runs.append((dev.records(buffers)[0], dev.get_state(), anc, before))
    history, state, anc, before = runs[0]
    beta = history[0, :, 0]
    assert np.all(np.diff(np.concatenate([[0.], beta])) > 0.) and beta[-1] < 1.
    assert np.allclose(history[0, :, 2], 0.5 * N, rtol=1e-9, atol=0.)
    for it in range(3):      # floor(N W) or ceil(N W) copies of every particle, W from the log-likelihoods before the iteration
        L, b = before[it][1][0], before[it][3][0]
        level = smc.temper(L, b, 0.5)
        assert np.isclose(level['beta'], beta[it], rtol=1e-10)
        W = smc.weights(L, level['lmax'], level['delta'], level['sumw'])
        copies = np.bincount(anc[it][0], minlength=N)
        assert copies.sum() == N and np.all((copies == np.floor(N * W)) | (copies == np.ceil(N * W)))
    assert np.array_equal(history, runs[1][0])
    for a, b in zip(state, runs[1][1]): assert np.array_equal(a, b)
    for a, b in zip(anc, runs[1][2]): assert np.array_equal(a, b)


# ---- 7. evidence against a quadrature ----------------------------------------------------------------------------------------------------------------------------
def _quadrature(like, nodes):
    """log of the integral of exp(loglike) prior over a box of +- 8 Fisher widths about the posterior's maximum clipped to the priors: Gauss-Legendre, ``nodes`` per axis,
    through eval_logposterior_host."""
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
    lp = f(grid).reshape(nodes, nodes)
    top = lp.max()
    # the library's log-priors have their maximum removed (the reference's convention): the evidence is taken under the NORMALISED priors the particles are drawn from
    norm = sum(float(param.prior.logpdf(x[i], remove_zerolag=False) - param.prior.logpdf(x[i])) for i, param in enumerate(params))
    return top + np.log(np.einsum('i,j,ij->', w, w, np.exp(lp - top)) * 0.25 * np.prod(hi - lo)) + norm


def test_evidence_against_quadrature():
    """The two-parameter cfg2 likelihood (b1, sn0): SMCSampler(chains=8, nparticles=1024) against the 2-D Gauss-Legendre quadrature of exp(loglike) prior (-15.052629;
    64 against 128 nodes per axis: 7e-15).  Measured on the MI355X over seeds 1 .. 12 (T = 15 levels each): logz_mean within -0.9 .. 1.8 standard errors of the quadrature;
    the 96 systems pooled: log of the mean Z^ 0.029 above it (standard error 0.02), scatter of logz 0.200 = 1.66 sqrt(T / N), inside the bound 0.242.  The scatter of
    EIGHT systems estimates that to +- 27 %: it was 0.143 .. 0.284 over the twelve seeds and above the bound for three of them (1, 9, 12); seed 4 (0.195) is the one nearest
    to the pooled value."""
    from desilike_amd.samplers import SMCSampler
    like = _like('two')
    exact, coarse = _quadrature(like, 128), _quadrature(like, 64)
    assert abs(exact - coarse) <= 1e-6, (exact, coarse)
    sampler = SMCSampler(like, nparticles=1024, chains=8, seed=4)
    assert sampler.device_resident and sampler.n_steps == 4
    sampler.run(max_iterations=1)
    K, N, T = 8, 1024, int(sampler.nlevels.max())
    print('logz_mean', sampler.logz_mean, 'logz_std', sampler.logz_std, 'T', T, 'quadrature', exact, 'bound', 2. * np.sqrt(T / N), 'evaluations', sampler.nevaluations)
    assert sampler.logz_std <= 2. * np.sqrt(T / N)
    assert abs(sampler.logz_mean - exact) <= 4. * sampler.logz_std / np.sqrt(K)
    # eight systems estimate the scatter to +- 27 %; 64 systems estimate it to +- 9 %: the same two conditions there, so that the sampler cannot pass by the choice of a seed
    many = SMCSampler(_like('two'), nparticles=1024, chains=64, seed=4)
    many.run(max_iterations=1)
    T = int(many.nlevels.max())
    print('64 systems: logz_mean', many.logz_mean, 'logz_std', many.logz_std, 'T', T, 'bound', 2. * np.sqrt(T / N))
    assert many.logz_std <= 2. * np.sqrt(T / N)
    assert abs(many.logz_mean - exact) <= 4. * many.logz_std / np.sqrt(64)


# ---- 8. posterior --------------------------------------------------------------------------------------------------------------------------------------------
def test_smc_posterior_on_the_device():
    """cfg2: the beta = 1 particles of SMCSampler(chains=4, nparticles=1024) against EmceeSampler (the run and the bounds of test_mclmc_posterior_on_the_device)."""
    from desilike_amd.samplers import SMCSampler, EmceeSampler
    like = make_cfg2()[1]
    names = like.varied_params.names()
    sampler = SMCSampler(like, nparticles=1024, chains=4, seed=2)
    assert sampler.device_resident and sampler.n_steps == 12
    chains = sampler.run(max_iterations=4)
    x = np.column_stack([np.concatenate([chain[name].ravel() for chain in chains]) for name in names])
    assert all(np.all(np.isfinite(chain['logposterior'])) for chain in chains)
    for i, param in enumerate(like.varied_params): assert np.all((x[:, i] > param.prior.limits[0]) & (x[:, i] < param.prior.limits[1]))
    ens = EmceeSampler(make_cfg2()[1], nwalkers=64, seed=3)
    chain = ens.run(niterations=1500)
    y = np.column_stack([chain[name][500:].ravel() for name in names])
    print('mean shift / sigma', (x.mean(axis=0) - y.mean(axis=0)) / y.std(axis=0), 'std ratio', x.std(axis=0) / y.std(axis=0), 'levels', sampler.nlevels, 'logz', sampler.logz,
          'evaluations', sampler.nevaluations)
    assert np.all(np.abs(x.mean(axis=0) - y.mean(axis=0)) < 0.3 * y.std(axis=0)), (x.mean(axis=0), y.mean(axis=0), y.std(axis=0))
    assert np.allclose(x.std(axis=0), y.std(axis=0), rtol=0.25)


# ---- 9. repeatability and state ----------------------------------------------------------------------------------------------------------------------------------
def test_repeatability_chunking_and_state():
    from desilike_amd.smc import run_batch
    runs = []
    for chunk in (None, None, 3):
        dev = _engines('cfg2', 2, 128, host=False)[0]
        runs.append(run_batch(dev, 12, chunk=chunk) + tuple(dev.get_state()))
    history, coords, logp, counts = runs[0][:4]
    assert np.all(counts[:, 0] == 12)
    for other in runs[1:]:
        assert np.array_equal(history, other[0])
        for k in range(2):       # (records beyond the count are not written)
            assert np.array_equal(coords[k, :counts[k, 1]], other[1][k, :counts[k, 1]]) and np.array_equal(logp[k, :counts[k, 1]], other[2][k, :counts[k, 1]])
        for a, b in zip(runs[0][3:], other[3:]): assert np.array_equal(a, b)
    # a get_state / set_state round trip continues bit for bit
    first = _engines('cfg2', 2, 128, host=False)[0]
    head = run_batch(first, 5)
    second = _engines('cfg2', 2, 128, host=False)[0]
    state = first.get_state()
    second.set_state(*state)
    for a, b in zip(state, second.get_state()): assert np.array_equal(a, b)
    tail = run_batch(second, 7)
    assert np.array_equal(np.concatenate([head[0], tail[0]], axis=1), history)
    for a, b in zip(second.get_state(), runs[0][4:]): assert np.array_equal(a, b)


def test_state_round_trip_and_errors():
    from desilike_amd._lib import DeviceSMC, LibraryError
    like = make_cfg2()[1]
    ctx = like._get_context()
    P, widths = ctx.n_params, np.ones(ctx.n_params)
    smc = DeviceSMC(ctx, 2, 64, widths, seed=3)
    assert [smc.info(key) for key in ['nsystems', 'nparticles', 'n_params', 'iterations', 'evaluations']] == [2, 64, P, 0, 0]
    start = np.stack([param.prior.sample(size=(2, 64), random_state=np.random.RandomState(i)) for i, param in enumerate(like.varied_params)], axis=-1)
    with pytest.raises(LibraryError, match='hyper'): smc.run(1, 1, smc.buffers(1))
    smc.set_hyper(0.5, 2, 0.234)
    with pytest.raises(LibraryError, match='particles'): smc.run(1, 1, smc.buffers(1))
    smc.set_particles(start)
    coords, L, pi, beta, logz, counters, scale, factor = smc.get_state()
    assert np.array_equal(coords, start) and np.all(np.isfinite(pi)) and np.all(beta == 0.) and np.all(logz == 0.) and np.all(counters == 0) and np.all(scale == 1.)
    assert smc.info('evaluations') == 128
    outside = start.copy(); outside[1, 7, 0] = 5.
    with pytest.raises(LibraryError, match='particle 7 of system 1 lies outside the prior'): smc.set_particles(outside)
    bad = start.copy(); bad[0, 0, 0] = np.nan
    with pytest.raises(LibraryError, match='finite'): smc.set_particles(bad)
    for fraction in (0., 1., 1.5):
        with pytest.raises(LibraryError, match='ess_fraction'): smc.set_hyper(fraction, 2, 0.234)
    with pytest.raises(LibraryError, match='n_steps'): smc.set_hyper(0.5, 0, 0.234)
    with pytest.raises(LibraryError, match='target_acceptance'): smc.set_hyper(0.5, 2, 1.)
    with pytest.raises(LibraryError, match='multiple of 64'): DeviceSMC(ctx, 2, 100, widths)
    with pytest.raises(LibraryError, match='multiple of 64'): DeviceSMC(ctx, 2, 32768, widths)
    with pytest.raises(LibraryError, match='nsystems'): DeviceSMC(ctx, 0, 64, widths)
    with pytest.raises(LibraryError, match='widths'): DeviceSMC(ctx, 2, 64, np.zeros(P))
    with pytest.raises(LibraryError, match='beta'): smc.set_state(coords, L, pi, beta + 2., logz, counters, scale, factor)
    smc.set_state(coords, L, pi, [0.25, 1.], [-3., -4.], [5, 6], [0.5, 2.], factor + np.eye(P))
    again = smc.get_state()
    assert np.array_equal(again[3], [0.25, 1.]) and np.array_equal(again[4], [-3., -4.]) and np.array_equal(again[5], [5, 6]) and np.array_equal(again[6], [0.5, 2.])
    assert np.array_equal(again[0], coords) and np.array_equal(again[1], L) and np.array_equal(again[7], factor + np.eye(P))
