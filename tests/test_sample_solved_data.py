"""CPU (-m "not gpu"): posterior draws of the solved parameters of a data batch (csrc/dl_sample_solved_data.h; ``dl_sample_solved_data``, ``DataBatch.sample_solved``,
``desilike_amd.sample_solved(data_batch, ...)``, ``MockEmceeSampler.sample_solved``).

1. The per-pair draw the device compiles, built with g++ as a program of its own (tests/csrc/emulate_sample_solved_data.cpp), plain and under ASan + UBSan, on the cases of
   tests/marg_counts_cases.py against the data vectors of tests/data_batch_marg_utils.py, compared with the NumPy restatement of the reference's Chain.sample_solved
   (tests/solved_oracle.py) fed with the float64 oracle's solution.  YARDSTICK FIRST: for every compared (row, data vector, mask, prior) the float64 oracle is asserted to
   lie within 1/8 of the tolerance of the extended-precision reference tests/marg_reference.py, and chi2(x0) <= 1e4 (tests/test_data_batch_marg.py explains the condition).
   The program itself checks that the padded size NSP = 16 gives the bits of the size the launcher picks.
2. Draw addressing, distribution, pivot and bad index on the same program.
3. The Python surface on stub contexts: no device."""
import os
import subprocess
import warnings

import numpy as np
import pytest

from oracle import np_oracle as orc
import marg_reference as mr
import marg_counts_cases as mc
import data_batch_marg_utils as dbm
import sample_solved_data_utils as ssd
import solved_oracle as so
from test_marg_reference import worst

SEED, M_PROGRAM, SIZE, INDEX0 = 42, 3, 4, 1000
TOL = 1e-10            # the project's bound, relative to max(1, |.|), on loglike and logprior of a draw
ROWS = [0, 3, 7]       # rows of a case the draw arithmetic is compared on


def _masks(ns):
    return [('marg', np.ones(ns, dtype='?')), ('mixed', np.arange(ns) % 2 == 0), ('best', np.zeros(ns, dtype='?'))]


def _oracle(key, row, m, scale, mask):
    """(float64 oracle, its distance to the extended-precision reference, chi2(x0)) of (row, data vector m) of the case."""
    case = dbm.get_case(key)
    ref = mr.marg_from_gram(dbm.gram(key, row, m), case.x0, case.prior_loc, scale, mask)
    sol = orc.solve_marginalized(case.delta[row] + case.flatdata - dbm.mocks(key)[m], case.T[row], case.precision, case.x0, case.prior_loc, scale, mask)
    return sol, worst(sol, ref), ref['chi2_x0']


@pytest.mark.parametrize('gaussian', [False, True], ids=['flat', 'gaussian'])
@pytest.mark.parametrize('ns', [1, 2, 5, 10, 16])
def test_program_vs_oracle(ns, gaussian, tmp_path):
    """x^, ll, lps of the program against the float64 oracle (solved values rtol 1e-8, atol 1e-10; values TOL); every draw: |C^T (x - x^) - z| <= 100 cond(A) eps per
    component with NumPy's factor of A (tests/test_sample_solved.py), loglike and logprior against oracle value + correction of chain.py:251-262 to TOL max(1, |.|).
    x^, H_L = -H, prec and the mask that feed the oracle's draw are those of dl_dbm_point_host / dl_dbm_pair of the same case.  Gaussian: the priors of the case (a mix of
    Gaussian and flat parameters); flat: every prior flat."""
    key = (57, ns)
    case = dbm.get_case(key)
    scale = case.prior_scale if gaussian else np.full(ns, np.inf)
    if gaussian: assert np.isfinite(scale).any() or ns == 1
    prec = np.where(np.isinf(scale), 0., 1. / scale**2)
    programs = [ssd.build_program(), ssd.build_program(sanitize=True)]
    z = so.gauss(SEED, INDEX0 + np.arange(mc.NROWS), np.arange(SIZE), ns)
    errs = np.zeros(5)
    for name, mask in _masks(ns):
        runs = [ssd.run_program(program, key, M_PROGRAM, mask, str(tmp_path / 'input.f64'), size=SIZE, index0=INDEX0, seed=SEED, prec=prec, lp=-1.25) for program in programs]
        # (-O2 and -O1 builds: the shared functions leave nothing to contraction; the host factorisation is plain C++ and may differ in the last bits)
        for field in ('loglike', 'logprior', 'x'):
            assert np.allclose(runs[0][1][field], runs[1][1][field], rtol=1e-12, atol=1e-12), (key, name, field)
        pairs, draws = runs[0]
        for i in ROWS:
            for m in range(M_PROGRAM):
                sol, err, chi2 = _oracle(key, i, m, scale, mask)
                assert chi2 <= 1e4, (key, i, m, chi2)                                       # input condition (a)
                assert err <= TOL / 8., (key, name, i, m, 'the float64 oracle is no yardstick here', err)
                p = pairs[i][m]
                assert p['status'] == 0
                assert np.allclose(p['xhat'], sol['x'], rtol=1e-8, atol=1e-10), (key, name, i, m)
                assert np.allclose(-p['H'], sol['likelihood_hessian'], rtol=1e-10, atol=1e-10 * np.abs(p['H']).max()), (key, name, i, m)
                e = [abs(p['ll'] - sol['loglikelihood']) / max(1., abs(sol['loglikelihood'])), abs(p['lps'] - sol['logprior_solved']) / max(1., abs(sol['logprior_solved']))]
                assert max(e) <= TOL, (key, name, i, m, e)
                C, bound = so.draw_bound(-p['H'], prec)
                resid = np.abs((draws['x'][i, m] - p['xhat']).dot(C) - z[i]).max()
                assert resid <= bound, (key, name, i, m, resid, bound)
                xo, dll, dlp = so.sample_solved(p['xhat'], -p['H'], prec, mask, z[i])
                want_ll, want_lp = sol['loglikelihood'] + dll, (-1.25 + sol['logprior_solved']) + dlp
                e += [(np.abs(draws['loglike'][i, m] - want_ll) / np.maximum(1., np.abs(want_ll))).max(), (np.abs(draws['logprior'][i, m] - want_lp) / np.maximum(1., np.abs(want_lp))).max()]
                assert max(e[2:]) <= TOL, (key, name, i, m, e)
                if bound < 1e-9:      # well conditioned: the draws themselves against the oracle's (tests/test_sample_solved.py)
                    np.testing.assert_allclose(draws['x'][i, m], xo, rtol=0., atol=2. * bound * np.abs(np.linalg.inv(C)).sum())
                if not gaussian: assert np.array_equal(draws['logprior'][i, m], np.full(SIZE, -1.25 + p['lps']))
                errs = np.maximum(errs, e + [resid / bound])
    print('\nn57-ns{:d} {}: x^ ll {:.1e} lps {:.1e}; draws: loglike {:.1e} logprior {:.1e} (bound {:.0e}), residual / bound {:.1e}'.format(ns, 'gaussian' if gaussian else 'flat',
                                                                                                                                   errs[0], errs[1], errs[2], errs[3], TOL, errs[4]))


def test_addressing(tmp_path):
    """Draw d of point i is a pure function of (seed, index0 + row, d, component): unchanged under ``size``, under index0 splits of the rows and under the data index
    (v = x - x^ of the same point against two data vectors: the same z, the same factor); another seed or another global index gives other draws."""
    key, ns = (57, 5), 5
    program, path = ssd.build_program(), str(tmp_path / 'input.f64')
    mask = np.arange(ns) % 2 == 0
    pairs, whole = ssd.run_program(program, key, M_PROGRAM, mask, path, size=5, index0=40, seed=SEED)
    for size in (1, 2, 4):
        part = ssd.run_program(program, key, M_PROGRAM, mask, path, size=size, index0=40, seed=SEED)[1]
        for field in whole:
            assert np.array_equal(whole[field][:, :, :size], part[field]), (field, size)
    first = ssd.run_program(program, key, M_PROGRAM, mask, path, size=5, index0=40, seed=SEED, rows=range(3))[1]
    second = ssd.run_program(program, key, M_PROGRAM, mask, path, size=5, index0=43, seed=SEED, rows=range(3, mc.NROWS))[1]
    for field in whole:
        assert np.array_equal(whole[field], np.concatenate([first[field], second[field]])), field
    # the data index does not enter the draw: z = C^T (x - x^) is the same against every data vector
    z = so.gauss(SEED, 40 + np.arange(mc.NROWS), np.arange(5), ns)
    prec = ssd.dbm.program_input(key, M_PROGRAM)[1]
    for i in range(mc.NROWS):
        C, bound = so.draw_bound(-pairs[i][0]['H'], prec)
        v = [whole['x'][i, m] - pairs[i][m]['xhat'] for m in range(M_PROGRAM)]
        for m in range(M_PROGRAM):
            assert np.abs(v[m].dot(C) - z[i]).max() <= bound
            assert np.allclose(v[m], v[0], rtol=1e-9, atol=1e-12 * np.abs(v[0]).max())      # (x^ differs between the data vectors: x - x^ rounds differently)
        assert not np.isclose(pairs[i][0]['xhat'], pairs[i][1]['xhat']).all()
    other = ssd.run_program(program, key, M_PROGRAM, mask, path, size=5, index0=40, seed=SEED + 1)[1]
    shifted = ssd.run_program(program, key, M_PROGRAM, mask, path, size=5, index0=41, seed=SEED)[1]
    assert not np.isclose(other['x'], whole['x']).any() and not np.isclose(shifted['x'], whole['x']).any()
    # indices across 2^32: the high word enters the counter
    index0 = (1 << 32) - 2
    pairs, far = ssd.run_program(program, key, 1, mask, path, size=1, index0=index0, seed=SEED, rows=range(4))
    z = so.gauss(SEED, index0 + np.arange(4), [0], ns)
    for i in range(4):
        C, bound = so.draw_bound(-pairs[i][0]['H'], prec)
        assert np.abs((far['x'][i, 0] - pairs[i][0]['xhat']).dot(C) - z[i]).max() <= bound


def test_distribution(tmp_path):
    """One pair of case n57-ns5, n = 16 384 draws (seed 42): the bounds of tests/test_sample_solved.py::test_distribution -- every component of the mean within 5 standard
    errors of x^, every entry of the sample covariance within 5 ((Sigma_ii Sigma_jj + Sigma_ij^2) / n)^1/2 of Sigma = A^-1."""
    key, ns, n = (57, 5), 5, 16384
    mask = np.arange(ns) % 2 == 0
    pairs, draws = ssd.run_program(ssd.build_program(), key, 2, mask, str(tmp_path / 'input.f64'), size=n, index0=0, seed=SEED, rows=[2], m_range=(1, 2))
    x, p = draws['x'][0, 0], pairs[0][0]
    prec = ssd.dbm.program_input(key, 2)[1]
    sigma = np.linalg.inv(p['H'] + np.diag(prec))
    diag = np.diag(sigma)
    assert (np.abs(x.mean(axis=0) - p['xhat']) <= 5. * np.sqrt(diag / n)).all()
    cov = np.cov(x, rowvar=False)
    assert (np.abs(cov - sigma) <= 5. * np.sqrt((np.outer(diag, diag) + sigma**2) / n)).all()
    assert len(np.unique(x[:, 0])) == n


@pytest.mark.parametrize('ns', [1, 5, 16])
def test_pivot_and_bad_index(ns, tmp_path):
    """A data index of -1 and of M: NaN and status 3 (DL_STATUS_NAN_INPUT), the pairs between them bit-identical to a run without bad indices.  A pivot that is not
    positive (a negative prior precision on the last parameter): NaN and status 2 (DL_STATUS_NONFINITE) for every pair.  A log-prior of -inf: status 1."""
    key, M = (57, ns), 2
    mask = np.ones(ns, dtype='?')
    for program in (ssd.build_program(), ssd.build_program(sanitize=True)):
        path = str(tmp_path / 'input.f64')
        good_pairs, good = ssd.run_program(program, key, M, mask, path, size=2, index0=7, seed=SEED)
        pairs, draws = ssd.run_program(program, key, M, mask, path, size=2, index0=7, seed=SEED, m_range=(-1, M + 1))
        for i in range(mc.NROWS):
            assert [pairs[i][j]['status'] for j in range(M + 2)] == [3] + [0] * M + [3]
        for field in draws:
            assert np.isnan(draws[field][:, [0, M + 1]]).all() and np.array_equal(draws[field][:, 1:M + 1], good[field]), field
        prec = np.array(ssd.dbm.program_input(key, M)[1])
        prec[-1] = -1e30
        pairs, draws = ssd.run_program(program, key, M, mask, path, size=2, index0=7, seed=SEED, prec=prec)
        assert all(pairs[i][m]['status'] == 2 for i in range(mc.NROWS) for m in range(M))
        assert all(np.isnan(draws[field]).all() for field in draws)
        pairs, draws = ssd.run_program(program, key, M, mask, path, size=2, index0=7, seed=SEED, lp=-np.inf)
        assert all(pairs[i][m]['status'] == 1 for i in range(mc.NROWS) for m in range(M)) and all(np.isnan(draws[field]).all() for field in draws)


def test_under_sanitizers(tmp_path):
    """The stand-alone build under AddressSanitizer + UndefinedBehaviorSanitizer runs clean on every compiled size, padded (n_s = 9, 13) or not, with one draw more than a
    wavefront holds and an odd number of components (the unused half of the last Box-Muller pair).  Host code only: nothing sanitized is loaded into this process."""
    program = ssd.build_program(sanitize=True)
    for ns in (1, 2, 3, 4, 5, 6, 8, 9, 12, 13, 16):
        mask = np.arange(ns) % 3 != 1
        pairs, draws = ssd.run_program(program, (57, ns), 2, mask, str(tmp_path / 'input.f64'), size=65, index0=3, seed=SEED, rows=[0, 1], m_range=(-1, 3))
        assert np.isfinite(draws['x'][:, 1:3]).all() and np.isnan(draws['x'][:, [0, 3]]).all()
    out = subprocess.run([program, os.path.join(str(tmp_path), 'missing')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 2 and 'Sanitizer' not in out.stderr


def test_entry_declared_and_null_context():
    """The header declares dl_sample_solved_data, the library exports it, a null context is an error and not a crash."""
    from desilike_amd import _lib
    lib = _lib.load()
    assert 'dl_sample_solved_data' in _lib.SYMBOLS
    assert lib.dl_sample_solved_data(None, None, 1, None, 0, 1, 42, None, None, None, None, None) == 1
    header = open(os.path.join(ssd.HERE, '..', 'include', 'desilike_amd.h')).read()
    assert 'int  dl_sample_solved_data(dl_ctx* ctx' in header


# ---- Python surface on stub contexts ------------------------------------------------------------------------------------------------------------
class _StubBatchContext(object):
    """What ``DataBatch.sample_solved`` needs of a Context: x^, H_L and the values are fixed functions of theta and of the data index; the draws are those of the
    host build of dl_sample_solved.h (tests/solved_oracle.py::emulate), which shares its draw addressing with the data-batch kernel."""

    def __init__(self, ns, n_params):
        rng = np.random.RandomState(5)
        self.n_solved, self.n_params = ns, n_params
        self.T = rng.standard_normal((ns, ns + 4))
        self.slope = rng.standard_normal((n_params, ns))
        self.prec = np.where(np.arange(ns) % 2 == 1, 2., 0.)
        self.is_marg = (np.arange(ns) != 0).astype('i4')
        self.calls = []

    def point(self, theta, index):
        theta = np.atleast_2d(theta)
        scale = 1. + 0.1 * np.tanh(theta[:, 0])
        hessian_l = -scale[:, None, None] * self.T.dot(self.T.T)
        status = np.where(np.isnan(theta).any(axis=1), 3, 0).astype('i4')
        return hessian_l, theta.dot(self.slope) + 0.25 * index[:, None], -0.5 * (theta**2).sum(axis=1) - index, -0.1 * np.abs(theta).sum(axis=1), status

    def sample_solved_data(self, theta, index, index0=0, size=1, seed=42):
        assert index.dtype == np.int32 and index.shape == (len(theta),)
        self.calls.append((len(theta), index0, index.tolist()))
        hessian_l, xhat, loglike, logprior, status = self.point(theta, index)
        return so.emulate(hessian_l, xhat, self.prec, self.is_marg, loglike, logprior, status, index0, size, seed)


class _StubLikelihood(object):
    _param_loglikelihood, _param_logprior = 'loglikelihood', 'logprior'

    def __init__(self, ns=3):
        from desilike_amd import Parameter
        self.varied_params = [Parameter('a', value=0., prior=dict(limits=(-5., 5.))), Parameter('b', value=0., prior=dict(limits=(-5., 5.)))]
        self.solved_params = [Parameter('s{:d}'.format(i), value=0., derived='.best' if i == 0 else '.marg', prior=dict(dist='norm', loc=0., scale=2.**-0.5) if i % 2 else None,
                                        fixed=False) for i in range(ns)]


def _stub_batch(M=4, solve='point', ns=3):
    from desilike_amd.likelihoods.base import DataBatch
    batch = DataBatch.__new__(DataBatch)
    batch.likelihood, batch.flatdata, batch.offset, batch.solve = _StubLikelihood(ns), np.zeros((M, 7)), 0., solve
    batch.context = _StubBatchContext(ns, 2)
    return batch


def _chain(shape, seed=0):
    rng = np.random.RandomState(seed)
    return {'a': rng.uniform(-1., 1., shape), 'b': rng.uniform(-1., 1., shape), 'logposterior': rng.standard_normal(shape)}


def _expected(batch, theta, index, index0, size, seed):
    hessian_l, xhat, loglike, logprior, status = batch.context.point(theta, np.asarray(index))
    return so.emulate(hessian_l, xhat, batch.context.prec, batch.context.is_marg, loglike, logprior, status, index0, size, seed)


def test_python_errors_before_any_device_call(monkeypatch):
    import desilike_amd
    from desilike_amd import _lib

    def no_device(*args, **kwargs):
        raise AssertionError('device call')

    # Context.sample_solved_data: argument errors are raised before the library or the device is touched
    monkeypatch.setattr(_lib, 'load', no_device)
    ctx = _lib.Context.__new__(_lib.Context)
    ctx.n_solved, ctx.n_params, ctx.device, ctx.expand = 3, 2, 0, None

    class NoLib(object):
        def __getattr__(self, name): raise AssertionError('device call')

    ctx._lib = NoLib()
    theta, index = np.zeros((3, 2)), np.zeros(3, dtype='i4')
    with pytest.raises(ValueError, match='size must be at least 1'):
        ctx.sample_solved_data(theta, index, size=0)
    with pytest.raises(ValueError, match='index0 must not be negative'):
        ctx.sample_solved_data(theta, index, index0=-1)
    for bad in (np.zeros(2, dtype='i4'), np.zeros((3, 1), dtype='i4'), np.zeros(3, dtype='i8'), np.zeros(3)):
        with pytest.raises(ValueError, match='index must be'):
            ctx.sample_solved_data(theta, bad)
    ctx.n_solved = 0
    with pytest.raises(ValueError, match='no analytically solved'):
        ctx.sample_solved_data(theta, index)
    # DataBatch.sample_solved
    batch = _stub_batch(solve='constant')
    values = np.zeros((3, 2))
    with pytest.raises(ValueError, match="solve='point'"):
        batch.sample_solved(values, index)
    with pytest.raises(ValueError, match="solve='point'"):
        desilike_amd.sample_solved(batch, _chain((5,)), index=0)
    batch = _stub_batch()
    for kwargs, match in [(dict(size=0), 'size must be'), (dict(index0=-1), 'index0 must not')]:
        with pytest.raises(ValueError, match=match):
            batch.sample_solved(values, index, **kwargs)
    for bad in (None, np.zeros(2, dtype='i4'), np.zeros(3), np.array([0, 1, 4]), np.array([-1, 0, 0])):
        with pytest.raises(ValueError, match='index must'):
            batch.sample_solved(values, bad)
    with pytest.raises(ValueError, match='values must have shape'):
        batch.sample_solved(np.zeros((3, 3)), index)
    # desilike_amd.sample_solved with a data batch
    with pytest.raises(ValueError, match='index is required'):
        desilike_amd.sample_solved(batch, _chain((5,)))
    for bad in ([0, 1], 4, -1, 0.5):
        with pytest.raises(ValueError, match='index must'):
            desilike_amd.sample_solved(batch, _chain((5,)), index=bad)
    for bad in (0, [0], [0, 1, 2], [0, 4], [0., 1.]):
        with pytest.raises(ValueError, match='index must'):
            desilike_amd.sample_solved(batch, [_chain((5,)), _chain((4,))], index=bad)
    with pytest.raises(ValueError, match='size must be'):
        desilike_amd.sample_solved(batch, _chain((5,)), size=0, index=0)
    with pytest.raises(ValueError, match='data batch'):
        desilike_amd.sample_solved(_StubLikelihood(), _chain((5,)), index=0)      # index without a data batch
    assert batch.context.calls == []


def test_python_function_with_data_batch(monkeypatch, tmp_path):
    """Shapes, repeated columns, weights, dropped derivative columns, the global index over the chains of a list, chunking, ChainFile in and out, the NaN warning."""
    import desilike_amd
    from desilike_amd import Samples, solved
    from desilike_amd.io import ChainFile
    batch = _stub_batch()
    chain, size = _chain((6, 4)), 3
    chain['fweight'] = np.arange(24).reshape(6, 4) + 1
    chain['aweight'] = np.linspace(0.1, 1., 24).reshape(6, 4)
    chain['loglikelihood.s1.s2'] = np.ones((6, 4))
    new = desilike_amd.sample_solved(batch, chain, size=size, seed=7, index=2)
    assert isinstance(new, Samples)
    assert set(new) == {'a', 'b', 'logposterior', 'fweight', 'aweight', 's0', 's1', 's2', 'loglikelihood', 'logprior'}
    for name, value in new.items():
        assert value.shape == (6, 4 * size), name
    for name in ['a', 'b', 'fweight', 'aweight']:
        assert np.array_equal(new[name], np.repeat(chain[name], size, axis=1)), name
    theta = np.column_stack([chain['a'].ravel(), chain['b'].ravel()])
    x, ll, lp, _ = _expected(batch, theta, np.full(24, 2), 0, size, 7)
    for i in range(3):
        assert np.array_equal(new['s{:d}'.format(i)], x[..., i].reshape(6, 4 * size))
    assert np.array_equal(new['loglikelihood'], ll.reshape(6, 4 * size)) and np.array_equal(new['logprior'], lp.reshape(6, 4 * size))
    assert np.array_equal(new['logposterior'], new['loglikelihood'] + new['logprior'])
    assert batch.context.calls == [(24, 0, [2] * 24)]
    # a list: one data vector per chain, None entries dropped with theirs, the global index runs on; chunks cut across chains
    chains = [_chain((5,), seed=1), None, _chain((8,), seed=2)]
    monkeypatch.setattr(solved, 'CHUNK', 7)
    batch.context.calls = []
    out = desilike_amd.sample_solved(batch, chains, size=2, seed=3, index=[1, 0, 3])
    assert [call[:2] for call in batch.context.calls] == [(7, 0), (6, 7)] and batch.context.calls[0][2] == [1] * 5 + [3] * 2
    assert isinstance(out, list) and len(out) == 2 and out[0]['s0'].shape == (10,) and out[1]['s0'].shape == (16,)
    theta = np.concatenate([np.column_stack([c['a'], c['b']]) for c in (chains[0], chains[2])])
    x = _expected(batch, theta, np.array([1] * 5 + [3] * 8), 0, 2, 3)[0]
    assert np.array_equal(np.concatenate([out[0]['s1'], out[1]['s1']]), x[..., 1].ravel())

    class Sampler(object):
        pass

    sampler = Sampler()
    sampler.chains = chains
    for a, b in zip(out, desilike_amd.sample_solved(batch, sampler, size=2, seed=3, index=[1, 0, 3])):
        assert all(np.array_equal(a[name], b[name]) for name in a)
    # ChainFile in, ChainFile out; round trip through .npz
    like = batch.likelihood
    params = {param.name: param for param in like.varied_params + like.solved_params}
    source = ChainFile(dict(chains[2], fweight=np.arange(8) + 1), params=params)
    new = desilike_amd.sample_solved(batch, source, size=2, seed=3, index=np.int64(3))
    assert isinstance(new, ChainFile) and new.shape == (16,)
    assert np.array_equal(new.arrays['fweight'], np.repeat(np.arange(8) + 1, 2))
    for param in like.solved_params:
        assert new.params[param.name].derived is False and not new.params[param.name].solved
    fn = os.path.join(str(tmp_path), 'chain.npz')
    new.save(fn)
    back = ChainFile.load(fn)
    assert list(back.arrays) == list(new.arrays) and all(np.array_equal(back.arrays[name], new.arrays[name]) for name in new.arrays)
    # bad rows keep NaN and are counted
    bad = _chain((6,), seed=4)
    bad['a'][2] = np.nan
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        new = desilike_amd.sample_solved(batch, bad, size=2, index=1)
    assert len(caught) == 1 and '1 chain points' in str(caught[0].message)
    assert np.isnan(new['s1'][4:6]).all() and np.isnan(new['logposterior'][4:6]).all() and np.isfinite(new['s1'][:4]).all() and np.isfinite(new['s1'][6:]).all()


def test_mock_sampler_layout(monkeypatch):
    """``MockEmceeSampler.sample_solved`` on recorded chains (no engine, no device): the nested list, [n - burnin, nwalkers * size] per chain, repeated columns, the global
    index in the order i, k, then the chain's own flattening, each chain against ``mocks[i]``, chunked calls that do not follow the mocks; ``data_batch=`` checks."""
    from desilike_amd import MockEmceeSampler, Samples, solved
    batch = _stub_batch(M=6)
    mocks, nchains, nwalkers, n = [4, 1, 4], 2, 6, 5
    sampler = MockEmceeSampler.__new__(MockEmceeSampler)
    sampler.data_batch, sampler.mocks, sampler.nchains, sampler.nwalkers = batch, np.array(mocks), nchains, nwalkers
    sampler.varied_params = batch.likelihood.varied_params
    sampler.index = np.repeat(sampler.mocks, nchains)
    rng = np.random.RandomState(9)
    coords, logp = rng.uniform(-1., 1., (n, len(mocks) * nchains, nwalkers, 2)), rng.standard_normal((n, len(mocks) * nchains, nwalkers))
    sampler._records = [(coords, logp)]
    monkeypatch.setattr(solved, 'CHUNK', 50)
    size, burnin = 2, 1
    new = sampler.sample_solved(size=size, seed=11, burnin=burnin)
    npoints = (n - burnin) * nwalkers
    assert [call[:2] for call in batch.context.calls] == [(50, 0), (50, 50), (44, 100)]      # 6 chains of 24 points in calls of 50
    assert len(new) == len(mocks) and all(len(row) == nchains for row in new)
    thetas, index = [], []
    for i in range(len(mocks)):
        for k in range(nchains):
            assert isinstance(new[i][k], Samples)
            thetas.append(coords[burnin:, i * nchains + k].reshape(-1, 2))
            index += [mocks[i]] * npoints
    x, ll, lp, _ = _expected(batch, np.concatenate(thetas), np.array(index), 0, size, 11)
    for i in range(len(mocks)):
        for k in range(nchains):
            e = i * nchains + k
            chain, sl = new[i][k], slice(e * npoints, (e + 1) * npoints)
            assert set(chain) == {'a', 'b', 'logposterior', 'loglikelihood', 'logprior', 's0', 's1', 's2'}
            for name in chain: assert chain[name].shape == (n - burnin, nwalkers * size), name
            assert np.array_equal(chain['a'], np.repeat(coords[burnin:, e, :, 0], size, axis=1)) and np.array_equal(chain['b'], np.repeat(coords[burnin:, e, :, 1], size, axis=1))
            for s in range(3): assert np.array_equal(chain['s{:d}'.format(s)], x[sl, :, s].reshape(n - burnin, nwalkers * size))
            assert np.array_equal(chain['loglikelihood'], ll[sl].reshape(n - burnin, -1)) and np.array_equal(chain['logposterior'], chain['loglikelihood'] + chain['logprior'])
    # the two chains of mocks[0] and those of mocks[2] sample the same data vector at different global indices: different draws
    assert not np.isclose(new[0][0]['s1'], new[0][1]['s1']).any()
    # a sampler that ran on a 'constant' batch: refused with the advice, accepted with a 'point' batch over the same data
    constant = _stub_batch(M=6, solve='constant')
    constant.likelihood = batch.likelihood
    sampler.data_batch = constant
    with pytest.raises(ValueError, match="solve='point'"):
        sampler.sample_solved()
    other = sampler.sample_solved(size=size, seed=11, burnin=burnin, data_batch=batch)
    assert all(np.array_equal(other[i][k][name], new[i][k][name]) for i in range(len(mocks)) for k in range(nchains) for name in new[i][k])
    with pytest.raises(ValueError, match='data vectors of the likelihood'):
        sampler.sample_solved(data_batch=_stub_batch(M=5))
    with pytest.raises(ValueError, match='data vectors of the likelihood'):
        sampler.sample_solved(data_batch=_stub_batch(M=6))      # another likelihood
    with pytest.raises(ValueError, match="solve='point'"):
        sampler.sample_solved(data_batch=constant)
    with pytest.raises(ValueError, match='size must be'):
        sampler.sample_solved(size=0, data_batch=batch)
