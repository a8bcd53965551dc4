"""GPU (-m gpu): the BAO phase-shift template (reference: power_template.py:442-496) through the BAO kernel's phase-shift instantiations (csrc/dl_kernels.hip:
``dl_bao_kernel<MODEL, true>``) -- against fixtures captured from the reference (tests/golden/make_phaseshift_fixture.py; contexts created from the reference-side keys),
through the call surface of the mirror classes, at the workgroup sizes of ``dl_bao_threads`` (64 / 128 / 192 and 64 / 128 / 256 threads per point), with the broadband terms marginalised, and what ``dl_create`` refuses."""
import numpy as np
import pytest

import phaseshift_oracle as pso
import phaseshift_utils as psu

pytestmark = pytest.mark.gpu


def check_rows(ctx, g, theta, rows=slice(None)):
    """The bounds of tests/test_gpu_bao.py::test_bao_c_abi_vs_reference on the fixture rows ``rows`` of the batch ``theta``."""
    loglike, logprior, status, flat = ctx.eval_batch_host(theta, return_flattheory=True)
    ref_flat, ref_ll, ref_lp = g['flattheory'][rows], g['loglikelihood'][rows], g['logprior'][rows]
    n = len(ref_ll)
    print('batch {:d}: max |dlogL| / max(1, |logL|) {:.2e}, max |dflat| / max|flat| {:.2e}, max |dlogprior| {:.2e}'.format(len(theta), (np.abs(loglike[:n] - ref_ll) / np.maximum(1., np.abs(ref_ll))).max(),
          np.abs(flat[:n] - ref_flat).max() / np.abs(g['flattheory']).max(), np.abs(logprior[:n] - ref_lp).max()))
    assert (status[:n] == 0).all()
    assert np.allclose(flat[:n], ref_flat, rtol=1e-10, atol=1e-12 * np.abs(g['flattheory']).max())
    assert (np.abs(loglike[:n] - ref_ll) <= 1e-10 * np.maximum(1., np.abs(ref_ll))).all(), np.abs(loglike[:n] - ref_ll).max()
    assert np.allclose(logprior[:n], ref_lp, rtol=1e-13, atol=1e-13)
    return loglike


@pytest.mark.parametrize('name', psu.FIXTURES)
def test_phaseshift_c_abi_vs_reference(name):
    from desilike_amd._lib import Context
    g, cfg = psu.load_fixture(name)
    ctx = Context(cfg, device=0)
    power = np.hstack([ctx.eval_theory_host(g['theta'], iobs=iobs).reshape(len(g['theta']), -1) for iobs in range(int(cfg['n_obs'][0]))])
    print('{}: wiggle power, max error / tolerance {:.2e}'.format(name, (np.abs(power - g['wiggle_power']) / (1e-11 * np.abs(g['wiggle_power']) + 1e-12 * np.abs(g['wiggle_power']).max())).max()))
    assert np.allclose(power, g['wiggle_power'], rtol=1e-11, atol=1e-12 * np.abs(g['wiggle_power']).max())
    check_rows(ctx, g, g['theta'])


@pytest.mark.parametrize('name', ['pk', 'xi'])
def test_phaseshift_call_surface_vs_reference(name):
    from desilike_amd import vmap
    g, like = psu.make_likelihood(name)
    names = [str(n) for n in g['names']]
    assert like.varied_params.names() == names
    (logpost, derived), errors = vmap(like, errors='return', return_derived=True)({pname: g['theta'][:, i] for i, pname in enumerate(names)})
    assert errors == {}
    print('{}: call surface, max |dlogposterior| / max(1, |logposterior|) {:.2e}'.format(name, (np.abs(logpost - g['logposterior']) / np.maximum(1., np.abs(g['logposterior']))).max()))
    assert (np.abs(logpost - g['logposterior']) <= 1e-10 * np.maximum(1., np.abs(g['logposterior']))).all()


def test_phaseshift_sampler_smoke():
    """Ten updates of an ensemble over a likelihood with baoshift varied."""
    from desilike_amd.samplers import EmceeSampler
    g, like = psu.make_likelihood('pk')
    sampler = EmceeSampler(like, nwalkers=40, seed=42)
    chain = sampler.run(niterations=10)
    values = np.asarray(chain['baoshift'])
    assert values.shape[0] == 10 and np.isfinite(np.asarray(chain['logposterior'])).all()
    assert (values >= -8.).all() and (values <= 10.).all() and np.ptp(values[-1]) > 0.


@pytest.mark.parametrize('name', ['pk', 'xi'])
def test_phaseshift_three_workgroup_sizes(name):
    """Batches of 64, 2048 and 4096 points: the three workgroup sizes of dl_bao_threads -- 64 threads per point from 4096 points, 128 from 2048, and below the wavenumbers
    rounded up to whole waves: 192 for the 168 of 'pk', 256 for the 300 of 'xi'.  Rows 0-47 are the fixture's and meet ALL the bounds of the first test at every size, the
    per-point theory at 1e-11 included; the rest are seeded draws with baoshift over its whole prior; every 128th row against the oracle."""
    from desilike_amd._lib import Context
    g, cfg = psu.load_fixture(name)
    names = [str(n) for n in g['names']]
    assert len(cfg['obs0.kin']) == {'pk': 168, 'xi': 300}[name]
    rng = np.random.RandomState(91)
    sampled = np.isfinite(g['prior_limits']).all(axis=1)                        # (the broadband terms have no limits: drawn like the fixture's)
    lo, hi = g['theta'][:, sampled].min(axis=0), g['theta'][:, sampled].max(axis=0)
    theta = g['theta'][rng.randint(0, 48, size=4096)]
    theta[:, sampled] = rng.uniform(lo, hi, size=(4096, sampled.sum()))
    theta[:, names.index('baoshift')] = rng.uniform(-8., 10., size=4096)
    theta[:48] = g['theta']
    ctx = Context(cfg, device=0)
    ref = g['wiggle_power']
    oracle, worst = {}, 0.
    for size in (64, 2048, 4096):
        power = ctx.eval_theory_host(theta[:size], iobs=0).reshape(size, -1)
        print('{}, batch {:d}: wiggle power of rows 0-47, max error / tolerance {:.2e}'.format(name, size, (np.abs(power[:48] - ref) / (1e-11 * np.abs(ref) + 1e-12 * np.abs(ref).max())).max()))
        assert np.allclose(power[:48], ref, rtol=1e-11, atol=1e-12 * np.abs(ref).max())
        assert np.isfinite(power).all()
        loglike = check_rows(ctx, g, theta[:size])
        assert np.isfinite(loglike).all()
        for i in range(0, size, 128):
            if i not in oracle: oracle[i] = pso.loglikelihood(cfg, theta[i])
            worst = max(worst, abs(loglike[i] - oracle[i]) / max(1., abs(oracle[i])))
            assert abs(loglike[i] - oracle[i]) <= 1e-10 * max(1., abs(oracle[i])), (size, i, loglike[i], oracle[i])
    print('{}: every 128th row against the oracle, {:d} rows: max relative error on logL {:.2e}'.format(name, len(oracle), worst))


def test_phaseshift_marginalised_broadband():
    """The 'xi' pipeline with its al* parameters '.marg' (built as tests/test_gpu_bao.py does for cfg4): the first 16 points against the oracle's solve."""
    from oracle import np_oracle as orc
    g, cfg = psu.load_fixture('xi')
    names = [str(n) for n in g['names']]
    _, like = psu.make_likelihood('xi')
    like.initialize()
    theory = like.observables[0].wmatrix.theory
    for param in theory.init.params.select(basename='al*'):
        param.update(derived='.marg')
    like._invalidate()
    nbb = len(like.solved_params)
    assert nbb == 10 and len(like.varied_params) == len(names) - nbb
    vnames = like.varied_params.names()
    assert 'baoshift' in vnames
    sub = g['theta'][:16][:, [names.index(n) for n in vnames]]
    ll, lp, st, solved = like._get_context().eval_batch_host(sub, return_solved=True)
    assert (st == 0).all()
    fold = theory._fold()
    T = fold[:, -nbb:].T                                                   # d(flattheory) / d(al): constant, whatever the wiggles
    c = pso.observable_keys(cfg)
    s = np.linspace(22.5, 167.5, 30)
    worst = 0.
    for i in range(16):
        full = np.array([dict(zip(vnames, sub[i])).get(n, 0.) for n in names])
        flat = np.ravel(orc.get_corr(pso.wiggle_power(c, full), c['kin'], s, (0, 2)))      # (the oracle's own Hankel transform, as tests/test_gpu_bao.py)
        sol = orc.solve_marginalized(flat - c['flatdata'], T, like.precision, x0=np.zeros(nbb), prior_loc=np.zeros(nbb), prior_scale=np.full(nbb, np.inf), marg_mask=np.ones(nbb, dtype='?'))
        worst = max(worst, abs(ll[i] - sol['loglikelihood']) / max(1., abs(sol['loglikelihood'])))
        assert abs(ll[i] - sol['loglikelihood']) <= 1e-10 * max(1., abs(sol['loglikelihood'])), (i, ll[i], sol['loglikelihood'])
    print('marginalised broadband, 16 points: max relative error on logL {:.2e}'.format(worst))


def test_phaseshift_refusals():
    """dl_create refuses template knots that are not uniform, an inner grid that is not uniform and the kind on another theory -- with the library's error, and contexts can be
    created and used afterwards."""
    from desilike_amd._lib import Context, LibraryError
    g, cfg = psu.load_fixture('pk')
    kt = cfg['obs0.k_t'].copy(); kt[1000] *= 1. + 1e-9
    kw = cfg['obs0.ps_k'].copy(); kw[500:] *= 1.001
    for changes, word in [({'obs0.k_t': kt}, 'uniform'), ({'obs0.ps_k': kw}, 'uniform'), ({'obs0.theory': np.array([0], dtype='i4')}, 'BAO wiggle theories only')]:
        with pytest.raises(LibraryError, match=word):
            Context(dict(cfg, **changes), device=0)
    ctx = Context(cfg, device=0)
    check_rows(ctx, g, g['theta'][:4], rows=slice(0, 4))
    # a NaN baoshift is flagged like any NaN parameter (DL_STATUS_NAN_INPUT) and its multipoles are NaN, as under the reference's np.clip
    theta = g['theta'][:4].copy()
    theta[2, [str(n) for n in g['names']].index('baoshift')] = np.nan
    status = ctx.eval_batch_host(theta)[2]
    assert tuple(status) == (0, 0, 3, 0)
    power = ctx.eval_theory_host(theta, iobs=0)
    assert np.isnan(power[2]).all() and np.isfinite(power[[0, 1, 3]]).all()
