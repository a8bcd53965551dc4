"""GPU (-m gpu): the wiggle-split template (reference: power_template.py:1150-1214) through its template kernel (csrc/dl_kernels.hip: ``dl_ws_template_kernel``, phases of
csrc/dl_wigglesplit.h) and the theory kernels that copy its rows -- against fixtures captured from the reference (tests/golden/make_wigglesplit_fixture.py; contexts created
from the reference-side keys only), through the call surface of the mirror classes, at the batch sizes where the theory launch changes form, with rows far outside the
priors and NaN rows, and what ``dl_create`` refuses.  No entry point exposes the template rows: the per-observable theory rows are held to 1e-11 instead."""
import numpy as np
import pytest

import wigglesplit_oracle as wso
import wigglesplit_utils as wsu

pytestmark = pytest.mark.gpu


def check_rows(ctx, g, theta, rows=slice(None)):
    """flattheory and logL at 1e-10, logprior at 1e-13, on the fixture rows ``rows`` of the batch ``theta``."""
    loglike, logprior, status, flat = ctx.eval_batch_host(theta, return_flattheory=True)
    ref_flat, ref_ll, ref_lp = g['flattheory'][rows], g['loglikelihood'][rows], g['logprior'][rows]
    n = len(ref_ll)
    print('batch {:d}: max |dlogL| / max(1, |logL|) {:.2e}, max |dflat| / max|flat| {:.2e}, max |dlogprior| {:.2e}'.format(len(theta), (np.abs(loglike[:n] - ref_ll) / np.maximum(1., np.abs(ref_ll))).max(),
          np.abs(flat[:n] - ref_flat).max() / np.abs(g['flattheory']).max(), np.abs(logprior[:n] - ref_lp).max()))
    assert (status[:n] == 0).all()
    assert np.allclose(flat[:n], ref_flat, rtol=1e-10, atol=1e-12 * np.abs(g['flattheory']).max())
    assert (np.abs(loglike[:n] - ref_ll) <= 1e-10 * np.maximum(1., np.abs(ref_ll))).all(), np.abs(loglike[:n] - ref_ll).max()
    assert np.allclose(logprior[:n], ref_lp, rtol=1e-13, atol=1e-13)
    return loglike, flat


@pytest.mark.parametrize('name', wsu.FIXTURES)
def test_wigglesplit_c_abi_vs_reference(name):
    """All 48 rows; 'two': both tracers and the correlation function from ONE template evaluation per point (dl_create finds their tables and inputs equal)."""
    from desilike_amd._lib import Context
    g, cfg = wsu.load_fixture(name)
    ctx = Context(cfg, device=0)
    assert ctx.info('ws_ld') == len(cfg['obs0.k_t'])          # one block of the template scratch, whatever the number of observables: one evaluation per point
    for iobs in range(int(cfg['n_obs'][0])):
        power = ctx.eval_theory_host(g['theta'], iobs=iobs).reshape(len(g['theta']), -1)
        ref = g['theory_obs{:d}'.format(iobs)]
        print('{} observable {:d}: theory rows, max error / tolerance {:.2e}'.format(name, iobs, wsu.close(power, ref)))
        assert wsu.close(power, ref) <= 1.
    check_rows(ctx, g, g['theta'])


@pytest.mark.parametrize('name', ['kaiser', 'tophat_eft'])
def test_wigglesplit_batch_sizes(name):
    """Batches of 1, 3, 48 and 300 points: a single workgroup, a ragged batch, and a batch past the 256-workgroup switch from the wide form of the theory kernel ('kaiser';
    'tophat_eft' has counter terms and takes the general form throughout).  Rows are resampled from the fixture; rows 0-47 are the fixture's, meet its bounds and are
    bit-identical across the sizes; every 16th row against the oracle."""
    from desilike_amd._lib import Context
    g, cfg = wsu.load_fixture(name)
    rng = np.random.RandomState(97)
    theta = g['theta'][rng.randint(0, 48, size=300)].copy()
    for col in range(theta.shape[1]): theta[:, col] = theta[rng.permutation(300), col]     # (columns shuffled apart: new points inside the fixture's ranges)
    theta[:48] = g['theta']
    ctx = Context(cfg, device=0)
    first, oracle, worst = {}, {}, 0.
    for size in (1, 3, 48, 300):
        n = min(size, 48)
        power = ctx.eval_theory_host(theta[:size], iobs=0).reshape(size, -1)
        assert wsu.close(power[:n], g['theory_obs0'][:n]) <= 1. and np.isfinite(power).all()
        loglike, flat = check_rows(ctx, g, theta[:size], rows=slice(0, n))
        for i in range(n):
            if i not in first: first[i] = (power[i].copy(), flat[i].copy(), loglike[i])
            assert np.array_equal(power[i], first[i][0]) and np.array_equal(flat[i], first[i][1]) and loglike[i] == first[i][2], (size, i)
        for i in range(0, size, 16):
            if i not in oracle: oracle[i] = wso.loglikelihood(cfg, theta[i])
            worst = max(worst, abs(loglike[i] - oracle[i]) / max(1., abs(oracle[i])))
            assert abs(loglike[i] - oracle[i]) <= 1e-10 * max(1., abs(oracle[i])), (size, i, loglike[i], oracle[i])
    print('{}: every 16th row against the oracle, {:d} rows: max relative error on logL {:.2e}'.format(name, len(oracle), worst))


def test_wigglesplit_call_surface_vs_reference():
    from desilike_amd import vmap
    for name in ['kaiser', 'tophat_eft']:
        g, like = wsu.make_likelihood(name)
        names = [str(n) for n in g['names']]
        assert like.varied_params.names() == names
        (logpost, derived), errors = vmap(like, errors='return', return_derived=True)({pname: g['theta'][:, i] for i, pname in enumerate(names)})
        assert errors == {}
        print('{}: call surface, max |dlogposterior| / max(1, |logposterior|) {:.2e}'.format(name, (np.abs(logpost - g['logposterior']) / np.maximum(1., np.abs(g['logposterior']))).max()))
        assert (np.abs(logpost - g['logposterior']) <= 1e-10 * np.maximum(1., np.abs(g['logposterior']))).all()


def test_wigglesplit_marginalised_sn0():
    """``sn0`` analytically marginalised ('.marg'): 16 rows against the oracle's solve on the oracle's own theory vector."""
    from oracle import np_oracle as orc
    g, cfg = wsu.load_fixture('kaiser')
    names = [str(n) for n in g['names']]
    _, like = wsu.make_likelihood('kaiser', marg=True)
    like.initialize()
    vnames = like.varied_params.names()
    assert len(like.solved_params) == 1 and vnames == [n for n in names if n != 'sn0']
    sub = g['theta'][:16][:, [names.index(n) for n in vnames]]
    ll, lp, st, solved = like._get_context().eval_batch_host(sub, return_solved=True)
    assert (st == 0).all()
    c = wso.observable_keys(cfg)
    W, bias = wso.window(c)
    nkin = len(c['kin'])
    T = (W[:, :nkin].sum(axis=1) / float(c['nd'][0]))[None, :]            # d(flattheory) / d(sn0): the monopole's columns over nd (full_shape.py:549)
    worst = 0.
    for i in range(16):
        full = g['theta'][i].copy(); full[names.index('sn0')] = 0.
        flat = wso.flattheory(cfg, full)[0]
        sol = orc.solve_marginalized(flat - c['flatdata'], T, like.precision, x0=np.zeros(1), prior_loc=np.zeros(1), prior_scale=np.full(1, 2.), marg_mask=np.ones(1, dtype='?'))
        worst = max(worst, abs(ll[i] - sol['loglikelihood']) / max(1., abs(sol['loglikelihood'])))
        assert abs(ll[i] - sol['loglikelihood']) <= 1e-10 * max(1., abs(sol['loglikelihood'])), (i, ll[i], sol['loglikelihood'])
    print('marginalised sn0, 16 points: max relative error on logL {:.2e}'.format(worst))


def test_wigglesplit_sampler():
    """Ten updates of a 40-walker ensemble (the general route: the in-kernel-proposal form declines this template): the chain is finite, inside the priors and moving, and a
    second run repeats it bit for bit."""
    from desilike_amd.samplers import EmceeSampler
    chains = []
    for attempt in range(2):
        g, like = wsu.make_likelihood('kaiser')
        chain = EmceeSampler(like, nwalkers=40, seed=42).run(niterations=10)
        chains.append({name: np.asarray(chain[name]).copy() for name in ['qbao', 'qap', 'df', 'dm', 'logposterior']})
    first = chains[0]
    assert first['qbao'].shape[0] == 10 and np.isfinite(first['logposterior']).all()
    for name, (lo, hi) in [('qbao', (0.8, 1.2)), ('qap', (0.8, 1.2)), ('df', (0., 2.)), ('dm', (-3., 3.))]:
        assert (first[name] >= lo).all() and (first[name] <= hi).all() and np.ptp(first[name][-1]) > 0.
    assert (first['qbao'][-1] != first['qbao'][0]).any()
    for name in first: assert np.array_equal(first[name], chains[1][name]), name


def test_wigglesplit_far_and_nan_rows():
    """qbao = 0.3 and 5.0 (far outside the prior: the shifted abscissa is clamped to the fiducial table): logprior -inf; a NaN qbao: status 3 (DL_STATUS_NAN_INPUT) and NaN
    multipoles.  The neighbouring rows are bit-identical to a batch without them."""
    from desilike_amd._lib import Context
    g, cfg = wsu.load_fixture('kaiser')
    iq = [str(n) for n in g['names']].index('qbao')
    theta = g['theta'][:8].copy()
    theta[2, iq], theta[4, iq], theta[6, iq] = 0.3, 5., np.nan
    ctx = Context(cfg, device=0)
    clean = ctx.eval_batch_host(g['theta'][:8], return_flattheory=True)
    clean_power = ctx.eval_theory_host(g['theta'][:8], iobs=0)
    loglike, logprior, status, flat = ctx.eval_batch_host(theta, return_flattheory=True)
    power = ctx.eval_theory_host(theta, iobs=0)
    assert logprior[2] == -np.inf and logprior[4] == -np.inf
    assert status[6] == 3 and np.isnan(power[6]).all()
    good = [0, 1, 3, 5, 7]
    assert (status[good] == 0).all()
    assert np.array_equal(loglike[good], clean[0][good]) and np.array_equal(flat[good], clean[3][good]) and np.array_equal(power[good], clean_power[good])
    check_rows(ctx, g, g['theta'][:8], rows=slice(0, 8))


REFUSALS = {
    'not_uniform': (lambda cfg: {'obs0.ws_k': np.concatenate([cfg['obs0.ws_k'][:900], cfg['obs0.ws_k'][900:] * 1.001])}, 'must be uniform in log k'),
    'too_few_knots': (lambda cfg: {'obs0.ws_k': cfg['obs0.ws_k'][::16], 'obs0.ws_pknow': cfg['obs0.ws_pknow'][::16]}, 'at least 128 knots'),
    'quadrature_node_outside': (lambda cfg: {'obs0.ws_k': cfg['obs0.ws_k'][:-600], 'obs0.ws_pknow': cfg['obs0.ws_pknow'][:-600]}, 'quadrature'),
    'template_knot_outside': (lambda cfg: {'obs0.k_t': np.geomspace(1e-5, 1., len(cfg['obs0.k_t']))}, 'template knot'),
    'qbao_leaves_fiducial': (lambda cfg: {key: cfg[key][100:] for key in ['obs0.ws_kfid', 'obs0.ws_pk_tt_fid', 'obs0.ws_pknow_tt_fid']}, 'outside the fiducial table'),
    'other_theory': (lambda cfg: {'obs0.theory': np.array([2], dtype='i4'), 'obs0.pknow_dd_fid': cfg['obs0.pk_dd_fid']}, 'Kaiser / EFT-like Kaiser / Simple theories only'),
}


@pytest.mark.parametrize('case', sorted(REFUSALS))
def test_wigglesplit_refusals(case):
    """dl_create refuses, with the library's message, and a good context is created and checked afterwards."""
    from desilike_amd._lib import Context, LibraryError
    g, cfg = wsu.load_fixture('kaiser')
    changes, word = REFUSALS[case]
    with pytest.raises(LibraryError, match=word):
        Context(dict(cfg, **changes(cfg)), device=0)
    check_rows(Context(cfg, device=0), g, g['theta'][:4], rows=slice(0, 4))


def test_wigglesplit_fisher():
    """The analytic Fisher (and gradient) is outside its scope for this template, as for the turn-over template: NotImplementedError; 'auto' falls back to the finite
    differences, which work."""
    import torch
    from desilike_amd.fisher import Fisher
    g, like = wsu.make_likelihood('kaiser')
    like.initialize()
    ctx = like._get_context()
    centers = g['theta'][6:8]
    assert ctx.eval_fisher_analytic(torch.as_tensor(centers, device=torch.device('cuda', ctx.device)).contiguous()) is None
    with pytest.raises(NotImplementedError, match='Kaiser'):
        Fisher(like, method='analytic').evaluate(centers)
    auto, finite = Fisher(like, method='auto').evaluate(centers), Fisher(like, method='finite').evaluate(centers)
    assert all(np.array_equal(a, b) for a, b in zip(auto, finite)) and all(np.isfinite(a).all() for a in finite)
    hessian = finite[2][0]
    assert (np.diag(hessian) < 0.).all()            # every parameter, qbao and dm included, is constrained
