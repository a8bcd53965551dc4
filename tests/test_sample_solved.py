"""CPU (-m "not gpu"): posterior draws of analytically solved parameters -- the lane function of the draw kernel (csrc/dl_sample_solved.h) built for the host against the
NumPy restatement of the reference's Chain.sample_solved (tests/solved_oracle.py), the draw addressing, the distribution of the draws, the same source under the
sanitizers, and the Python surface (desilike_amd.sample_solved) on a stub context."""
import os
import subprocess
import warnings

import numpy as np
import pytest

import solved_oracle as so

SEED = 42


def _corrections(hessian_l, xhat, prec, is_marg, index0, size, seed=SEED):
    """Draws and corrections of the host build: with loglike = logprior = 0 the corrected values ARE the corrections."""
    return so.emulate(hessian_l, xhat, prec, is_marg, 0., 0., 0, index0, size, seed)


@pytest.mark.parametrize('gaussian', [False, True])
@pytest.mark.parametrize('pattern', ['marg', 'mixed', 'best'])
@pytest.mark.parametrize('ns', [1, 2, 5, 10, 16])
def test_host_build_vs_oracle(ns, pattern, gaussian):
    """Draws: |C^T (x - x^) - z| <= 100 cond(A) eps per component, C NumPy's Cholesky factor of A (the backward error of a triangular solve is a few ns eps |C| |v|, and
    |C| |v| <= cond(A)^1/2 |z|; the inputs are chosen such that the bound is below 1e-9).  Corrections: 1e-12 relative to the oracle's."""
    rng = np.random.RandomState(100 * ns + 10 * ['marg', 'mixed', 'best'].index(pattern) + gaussian)
    B, size, index0 = 3, 4, 1000
    hessian_l, xhat, prec, is_marg = so.random_case(rng, B, ns, pattern, gaussian)
    x, dll, dlp, status = _corrections(hessian_l, xhat, prec, is_marg, index0, size)
    assert (status == 0).all()
    z = so.gauss(SEED, index0 + np.arange(B), np.arange(size), ns)
    for b in range(B):
        C, bound = so.draw_bound(hessian_l[b], prec)
        assert bound < 1e-9, 'the inputs are at fault: cond(A) = {:.3g}'.format(bound / 100. / so.EPS)
        resid = np.abs((x[b] - xhat[b]).dot(C) - z[b])          # row d: C^T (x_d - x^) - z_d
        assert resid.max() <= bound, (resid.max(), bound)
        xo, dll_o, dlp_o = so.sample_solved(xhat[b], hessian_l[b], prec, is_marg, z[b])
        np.testing.assert_allclose(x[b], xo, rtol=0., atol=2. * bound * np.abs(np.linalg.inv(C)).sum())   # (x - x_oracle = C^-T (residuals of the two); twice: the oracle's own)
        np.testing.assert_allclose(dll[b], dll_o, rtol=1e-12, atol=0.)
        np.testing.assert_allclose(dlp[b], dlp_o, rtol=1e-12, atol=0.)
        if not gaussian: assert (dlp[b] == 0.).all()
    # the marginalised values are passed through: corrected = value + correction
    x2, ll2, lp2, _ = so.emulate(hessian_l, xhat, prec, is_marg, -12.5, 0.75, 0, index0, size, SEED)
    assert np.array_equal(x2, x)
    np.testing.assert_allclose(ll2, -12.5 + dll, rtol=1e-15)
    np.testing.assert_allclose(lp2, 0.75 + dlp, rtol=1e-15)


@pytest.mark.parametrize('ns', [1, 2, 5, 10, 16])
def test_non_positive_pivot_and_bad_status(ns):
    """A row whose A has a non-positive pivot and a row with a non-zero evaluation status get NaN draws and corrections; the first is reported as status 2
    (DL_STATUS_NONFINITE), the second keeps its status; the rows beside them are bit-identical to a run without bad rows."""
    rng = np.random.RandomState(7 + ns)
    hessian_l, xhat, prec, is_marg = so.random_case(rng, 5, ns, 'mixed', True)
    good = so.emulate(hessian_l, xhat, prec, is_marg, -3., 0.5, 0, 20, 2, SEED)
    bad_h = hessian_l.copy()
    bad_h[1, ns - 1, ns - 1] = prec[ns - 1] + 1.         # A[ns-1, ns-1] = -1: the last pivot is negative
    bad_h[2, 0, 0] = np.nan
    status_in = np.array([0, 0, 0, 3, 0], dtype='i4')
    x, ll, lp, status = so.emulate(bad_h, xhat, prec, is_marg, -3., 0.5, status_in, 20, 2, SEED)
    assert status.tolist() == [0, 2, 2, 3, 0]
    for b in (1, 2, 3):
        assert np.isnan(x[b]).all() and np.isnan(ll[b]).all() and np.isnan(lp[b]).all()
    for b in (0, 4):
        assert np.array_equal(x[b], good[0][b]) and np.array_equal(ll[b], good[1][b]) and np.array_equal(lp[b], good[2][b])


def test_addressing():
    """A draw is a pure function of (seed, global point index, draw index, component): 130 points in one piece = 64 + 66 with index0, draw d of size 3 = draw d of
    size 1 .. 3, bit for bit; two seeds differ; the index is 64 bits wide."""
    rng = np.random.RandomState(3)
    ns, B = 5, 130
    hessian_l, xhat, prec, is_marg = so.random_case(rng, B, ns, 'mixed', True)
    loglike, logprior = rng.standard_normal(B), rng.standard_normal(B)
    whole = so.emulate(hessian_l, xhat, prec, is_marg, loglike, logprior, 0, 0, 3, SEED)
    first = so.emulate(hessian_l[:64], xhat[:64], prec, is_marg, loglike[:64], logprior[:64], 0, 0, 3, SEED)
    second = so.emulate(hessian_l[64:], xhat[64:], prec, is_marg, loglike[64:], logprior[64:], 0, 64, 3, SEED)
    for w, a, b in zip(whole, first, second):
        assert np.array_equal(w, np.concatenate([a, b]))
    for size in (1, 2, 3):
        part = so.emulate(hessian_l, xhat, prec, is_marg, loglike, logprior, 0, 0, size, SEED)
        for w, p in zip(whole[:3], part[:3]):
            assert np.array_equal(w[:, :size], p)
    other = so.emulate(hessian_l, xhat, prec, is_marg, loglike, logprior, 0, 0, 3, SEED + 1)
    assert not np.isclose(other[0], whole[0]).any()
    shifted = so.emulate(hessian_l, xhat, prec, is_marg, loglike, logprior, 0, 1, 3, SEED)
    assert not np.isclose(shifted[0], whole[0]).any()
    # indices across 2^32: the high word enters the counter (mirror and host build agree; index 2^32 is not index 0)
    index0 = (1 << 32) - 2
    x = so.emulate(hessian_l[:4], xhat[:4], prec, is_marg, 0., 0., 0, index0, 1, SEED)[0]
    z = so.gauss(SEED, index0 + np.arange(4), [0], ns)
    for b in range(4):
        C, bound = so.draw_bound(hessian_l[b], prec)
        assert np.abs((x[b] - xhat[b]).dot(C) - z[b]).max() <= bound
    assert not np.isclose(z[2], so.gauss(SEED, [0], [0], ns)[0]).any()


def test_distribution():
    """One point, ns = 5, n = 16 384 draws (seed 42): every component of the mean within 5 standard errors (Sigma_ii / n)^1/2 of x^; every entry of the sample covariance
    within 5 ((Sigma_ii Sigma_jj + Sigma_ij^2) / n)^1/2 of Sigma = A^-1 (the standard deviation of a sample covariance entry of a Gaussian).  Derived bounds; the seed is
    fixed, so the test is deterministic."""
    rng = np.random.RandomState(11)
    ns, n = 5, 16384
    hessian_l, xhat, prec, is_marg = so.random_case(rng, 1, ns, 'mixed', True)
    x = _corrections(hessian_l, xhat, prec, is_marg, 0, n)[0][0]
    sigma = np.linalg.inv(-hessian_l[0] + np.diag(prec))
    diag = np.diag(sigma)
    assert (np.abs(x.mean(axis=0) - xhat[0]) <= 5. * np.sqrt(diag / n)).all()
    cov = np.cov(x, rowvar=False)
    assert (np.abs(cov - sigma) <= 5. * np.sqrt((np.outer(diag, diag) + sigma**2) / n)).all()
    # the draws of one point are distinct, and so are those of its neighbour in the chain
    assert len(np.unique(x[:, 0])) == n


def test_under_sanitizers():
    """The same source as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer: every size 1 .. 16, three marginalisation patterns, a row with a
    non-positive pivot and a row with a bad status; exit status 0, no report.  (Host code only: nothing sanitized is loaded into this process.)"""
    program = so.build_standalone()
    result = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert result.returncode == 0, (result.stdout[-2000:], result.stderr[-2000:])
    assert 'Sanitizer' not in result.stderr and 'runtime error' not in result.stderr, result.stderr[-2000:]
    assert 'draw addressing agree' in result.stdout


def test_entry_declared_and_null_context():
    """The header declares dl_sample_solved, the library exports it, a null context is an error and not a crash."""
    from desilike_amd import _lib
    lib = _lib.load()
    assert 'dl_sample_solved' in _lib.SYMBOLS
    assert lib.dl_sample_solved(None, None, 1, 0, 1, 42, None, None, None, None, None) == 1
    header = open(os.path.join(so.HERE, '..', 'include', 'desilike_amd.h')).read()
    assert 'int  dl_sample_solved(dl_ctx* ctx' in header


# ---- Python surface on a stub context ----------------------------------------------------------------------------------------------------------
class _StubContext(object):
    """What desilike_amd.sample_solved needs of a Context, from the host build: x^ and H_L are fixed functions of theta."""

    def __init__(self, ns, n_params):
        rng = np.random.RandomState(5)
        self.n_solved, self.n_params = ns, n_params
        self.T = rng.standard_normal((ns, ns + 4))
        self.slope = rng.standard_normal((n_params, ns))
        self.prec = np.where(np.arange(ns) % 2 == 1, 2., 0.)
        self.is_marg = (np.arange(ns) != 0).astype('i4')
        self.calls = []

    def point(self, theta):
        theta = np.atleast_2d(theta)
        scale = 1. + 0.1 * np.tanh(theta[:, 0])
        hessian_l = -scale[:, None, None] * self.T.dot(self.T.T)
        status = np.where(np.isnan(theta).any(axis=1), 3, 0).astype('i4')
        return hessian_l, theta.dot(self.slope), -0.5 * (theta**2).sum(axis=1), -0.1 * np.abs(theta).sum(axis=1), status

    def sample_solved(self, theta, index0=0, size=1, seed=42):
        self.calls.append((len(theta), index0))
        hessian_l, xhat, loglike, logprior, status = self.point(theta)
        return so.emulate(hessian_l, xhat, self.prec, self.is_marg, loglike, logprior, status, index0, size, seed)


class _StubLikelihood(object):
    _param_loglikelihood, _param_logprior = 'loglikelihood', 'logprior'

    def __init__(self, ns=3):
        from desilike_amd import Parameter
        self.varied_params = [Parameter('a', value=0., prior=dict(limits=(-5., 5.))), Parameter('b', value=0., prior=dict(limits=(-5., 5.)))]
        self.solved_params = [Parameter('s{:d}'.format(i), value=0., derived='.best' if i == 0 else '.marg', prior=dict(dist='norm', loc=0., scale=2.**-0.5) if i % 2 else None,
                                        fixed=False) for i in range(ns)]
        self.ctx = _StubContext(ns, 2)

    def _get_context(self):
        return self.ctx


def _chain(shape, seed=0):
    rng = np.random.RandomState(seed)
    return {'a': rng.uniform(-1., 1., shape), 'b': rng.uniform(-1., 1., shape), 'logposterior': rng.standard_normal(shape)}


def test_python_surface_shapes_and_values(monkeypatch):
    import desilike_amd
    from desilike_amd import Samples, solved
    like = _StubLikelihood()
    chain = _chain((6, 4))
    chain['fweight'] = np.arange(24).reshape(6, 4) + 1
    chain['aweight'] = np.linspace(0.1, 1., 24).reshape(6, 4)
    chain['logweight'] = np.log(chain['aweight'])
    size = 3
    new = desilike_amd.sample_solved(like, chain, size=size, seed=7)
    assert isinstance(new, Samples)
    assert set(new) == {'a', 'b', 'logposterior', 'fweight', 'aweight', 'logweight', 's0', 's1', 's2', 'loglikelihood', 'logprior'}
    for name, value in new.items():
        assert value.shape == (6, 4 * size), name
    for name in ['a', 'b', 'fweight', 'aweight', 'logweight']:          # chain.py:244-245: repeated along the last axis, weights unchanged
        assert np.array_equal(new[name], np.repeat(chain[name], size, axis=1)), name
    theta = np.column_stack([chain['a'].ravel(), chain['b'].ravel()])
    hessian_l, xhat, loglike, logprior, status = like.ctx.point(theta)
    x, ll, lp, _ = so.emulate(hessian_l, xhat, like.ctx.prec, like.ctx.is_marg, loglike, logprior, status, 0, size, 7)
    for i in range(3):
        assert np.array_equal(new['s{:d}'.format(i)], x[..., i].reshape(6, 4 * size))
    assert np.array_equal(new['loglikelihood'], ll.reshape(6, 4 * size)) and np.array_equal(new['logprior'], lp.reshape(6, 4 * size))
    assert np.array_equal(new['logposterior'], new['loglikelihood'] + new['logprior'])
    # against the oracle at one point: x = x^ + C^-T z and the corrections of chain.py:251-262
    z = so.gauss(7, [17], np.arange(size), 3)[0]
    xo, dll, dlp = so.sample_solved(xhat[17], hessian_l[17], like.ctx.prec, like.ctx.is_marg, z)
    row, col = divmod(17, 4)
    got = np.column_stack([new['s{:d}'.format(i)][row, col * size:(col + 1) * size] for i in range(3)])
    np.testing.assert_allclose(got, xo, rtol=0., atol=1e-12)
    np.testing.assert_allclose(new['loglikelihood'][row, col * size:(col + 1) * size], loglike[17] + dll, rtol=1e-12)
    np.testing.assert_allclose(new['logprior'][row, col * size:(col + 1) * size], logprior[17] + dlp, rtol=1e-12)
    # the method of Samples; how the function cuts its calls changes nothing
    monkeypatch.setattr(solved, 'CHUNK', 7)
    like.ctx.calls = []
    again = Samples(chain).sample_solved(like, size=size, seed=7)
    assert like.ctx.calls == [(7, 0), (7, 7), (7, 14), (3, 21)]
    for name in new:
        assert np.array_equal(new[name], again[name]), name


def test_python_surface_inputs(tmp_path):
    """Every container the samplers hand out: a chain dictionary [n] or [niterations, nwalkers], ``sampler.chains`` (a list; global indices run on from one chain to the
    next), a sampler, a ChainFile; the result survives a ChainFile round trip; size = 0 raises; bad rows are counted in a warning."""
    import desilike_amd
    from desilike_amd.io import ChainFile
    like = _StubLikelihood()
    chains = [_chain((5,), seed=1), None, _chain((8,), seed=2)]
    out = desilike_amd.sample_solved(like, chains, size=2, seed=3)
    assert isinstance(out, list) and len(out) == 2 and out[0]['s0'].shape == (10,) and out[1]['s0'].shape == (16,)
    joined = {name: np.concatenate([chains[0][name], chains[2][name]]) for name in chains[0]}
    whole = desilike_amd.sample_solved(like, joined, size=2, seed=3)
    for name in whole:
        assert np.array_equal(whole[name], np.concatenate([out[0][name], out[1][name]])), name

    class Sampler(object):
        pass

    sampler = Sampler()
    sampler.chains = chains
    for a, b in zip(out, desilike_amd.sample_solved(like, sampler, size=2, seed=3)):
        assert all(np.array_equal(a[name], b[name]) for name in a)
    # ChainFile in, ChainFile out; round trip through .npz
    params = {param.name: param for param in like.varied_params + like.solved_params}
    source = ChainFile(dict(chains[2], fweight=np.arange(8) + 1), params=params)
    new = desilike_amd.sample_solved(like, source, size=2, seed=3)
    assert isinstance(new, ChainFile) and new.shape == (16,)
    assert np.array_equal(new.arrays['fweight'], np.repeat(np.arange(8) + 1, 2))
    for param in like.solved_params:
        assert new.params[param.name].derived is False and not new.params[param.name].solved      # ordinary columns now (chain.py:250)
    fn = os.path.join(str(tmp_path), 'chain.npz')
    new.save(fn)
    back = ChainFile.load(fn)
    assert list(back.arrays) == list(new.arrays) and back.derivs == {}
    for name in new.arrays:
        assert np.array_equal(back.arrays[name], new.arrays[name]), name
    assert back.params['s1'].derived is False and back.params['s1'].prior.dist == 'norm'
    assert np.isclose(back.mean('s0'), np.average(new.arrays['s0'], weights=new.arrays['fweight']))
    # a Samples result goes into a ChainFile with the parameters named by the caller
    ChainFile(whole, params=params).save(fn)
    assert np.array_equal(ChainFile.load(fn).arrays['s2'], whole['s2'])
    # size = 0 (and below) raises
    for size in (0, -1):
        with pytest.raises(ValueError):
            desilike_amd.sample_solved(like, chains[0], size=size)
    with pytest.raises(ValueError):
        desilike_amd.sample_solved(like, {'a': np.zeros(3)}, size=1)      # a sampled parameter is missing
    # bad rows keep NaN and are counted
    bad = _chain((6,), seed=4)
    bad['a'][2] = np.nan
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        new = desilike_amd.sample_solved(like, bad, size=2)
    assert len(caught) == 1 and '1 chain points' in str(caught[0].message)
    assert np.isnan(new['s1'][4:6]).all() and np.isnan(new['logposterior'][4:6]).all() and np.isfinite(new['s1'][:4]).all() and np.isfinite(new['s1'][6:]).all()
