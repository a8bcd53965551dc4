"""GPU (-m gpu): the data batch -- ``dl_data_set``, ``dl_eval_logposterior_data`` (cross and paired), ``dl_eval_fisher_data``, ``likelihood.data_batch`` and
``GaussNewtonProfiler.maximize_batch`` (csrc/dl_data_batch.h).

Reference of every value: the project's single-data path -- a context created from the same configuration with ``obs<i>.flatdata`` replaced by data vector m, evaluated
with ``dl_eval_logposterior`` / ``dl_eval_fisher`` (tests/data_batch_utils.py::reference, computed once per configuration).  Tolerance: 1e-10 max(1, |logL|) on values;
gradients and Hessians: the bound tests/test_fisher.py applies to ``dl_eval_fisher`` (rtol 1e-8, atol 1e-8 of the largest entry; offset rtol 1e-10).
Every 16th pair of the largest call is also checked against oracle/np_oracle.py: its Gaussian log-likelihood d P d of (flattheory - data vector m) and its log-prior, with
the flattheory of the point from the oracle itself where it evaluates the configuration from the fixture (the Kaiser full-shape ones: cfg1, cfg2) and from
``dl_eval_batch`` elsewhere (emulated, BAO and reference-side key sets: their theory is checked against the reference in their own tests; the data enter behind it).
Data vectors: flatdata + 0.05 |flatdata| z, z seeded standard normal."""
import ctypes

import numpy as np
import pytest

from data_batch_utils import get_case, reference, MMAX, BMAX

pytestmark = pytest.mark.gpu

CASES = ['cfg1_kaiser_nowindow',    # the smallest n
         'cfg2_shapefit_window',    # n = 120, N_pad = 128
         'boundary_two_tracers',    # block-diagonal precision, aligned row ranges, two 128-column blocks of N_pad
         'boundary_cfg3',           # the emulated feature path, no solved parameters
         'cfg4_bao_xi']


def _tol(ref):
    return 1e-10 * np.maximum(1., np.abs(ref))


def _context(case, flatdata=None):
    from desilike_amd._lib import Context
    return Context(case.spec if flatdata is None else case.spec_with_data(flatdata), device=0)


@pytest.mark.parametrize('name', CASES)
def test_cross_against_single_data_contexts(name):
    """M in {1, 3, 17, 65} (one vector, a ragged tile, one past a 16-wide and a 64-wide tile) x B in {1, 3, 300}."""
    from oracle import np_oracle as orc
    case, mocks, theta, ref, flattheory = reference(name)
    ctx = _context(case)
    worst = 0.
    for M in [1, 3, 17, MMAX]:
        assert ctx.set_data_batch(mocks[:M]) == M and ctx.n_data_batch == M
        for B in [1, 3, BMAX]:
            out, status = ctx.eval_logposterior_data_host(theta[:B])
            assert out.shape == (B, M) and (status == 0).all()
            err = np.abs(out - ref[:B, :M]) / _tol(ref[:B, :M])
            worst = max(worst, err.max())
            assert (err <= 1.).all(), (M, B, err.max())
    print('{}: worst |cross - single-data| = {:.2e} of the tolerance, |logL| up to {:.3e}'.format(name, worst, np.abs(ref).max()))
    # every 16th pair of the largest call against the oracle
    pairs = np.arange(0, BMAX * MMAX, 16)
    logprior = case.oracle_logprior(theta)
    oracle_ft = {}
    worst = 0.
    for k in pairs:
        b, m = divmod(int(k), MMAX)
        if b not in oracle_ft:
            ft = case.oracle_flattheory(theta[b])
            oracle_ft[b] = flattheory[b] if ft is None else ft
        value = orc.gaussian_loglikelihood(oracle_ft[b], mocks[m], case.precision)[0] + logprior[b]
        err = abs(out[b, m] - value) / max(1., abs(value)) / 1e-10
        worst = max(worst, err)
        assert err <= 1., (b, m, out[b, m], value)
    print('{}: worst |cross - oracle| over {:d} pairs = {:.2e} of the tolerance'.format(name, len(pairs), worst))
    ctx.close()


@pytest.mark.parametrize('name', CASES)
def test_paired_is_cross_bit_for_bit(name):
    """Random indices with repeats and with vectors that are never used: paired[b] == cross[b, index[b]], the same bits; and the reference at 1e-10."""
    case, mocks, theta, ref, _ = reference(name)
    ctx = _context(case)
    M = 17
    ctx.set_data_batch(mocks[:M])
    index = np.random.RandomState(3).choice([0, 2, 3, 5, 8, 13, 16], size=BMAX).astype('i4')      # (ten of the seventeen vectors are never used)
    assert len(np.unique(index)) < BMAX
    cross, _ = ctx.eval_logposterior_data_host(theta)
    paired, status = ctx.eval_logposterior_data_host(theta, index=index)
    assert paired.shape == (BMAX,) and (status == 0).all()
    assert np.array_equal(paired, cross[np.arange(BMAX), index])
    assert (np.abs(paired - ref[np.arange(BMAX), index]) <= _tol(paired)).all()
    for B in [1, 3]:      # a partial workgroup
        assert np.array_equal(ctx.eval_logposterior_data_host(theta[:B], index=index[:B])[0], paired[:B])
    ctx.close()


@pytest.mark.parametrize('name', ['cfg2_shapefit_window', 'boundary_two_tracers', 'boundary_cfg3'])
def test_own_data_vector(name):
    """A batch whose vector 0 is the context's own flatdata agrees with dl_eval_logposterior of that context."""
    case, mocks, theta, _, _ = reference(name)
    ctx = _context(case)
    ctx.set_data_batch(np.vstack([case.flatdata, mocks[:2]]))
    own, status = ctx.eval_logposterior_host(theta)
    cross, _ = ctx.eval_logposterior_data_host(theta)
    assert (status == 0).all() and (np.abs(cross[:, 0] - own) <= _tol(own)).all(), np.abs(cross[:, 0] - own).max()
    ctx.close()


def test_stacked_emulator_rows():
    """The stacked emulator layout (two launches: network chains, then the feature GEMMs) writes the un-biased rows the data-batch finalize reads: cross and paired against
    single-data contexts."""
    case = get_case('boundary_cfg3_stacked')
    mocks, theta = case.mocks(3), case.points(40)
    ctx = _context(case)
    ctx.set_data_batch(mocks)
    cross, status = ctx.eval_logposterior_data_host(theta)
    assert (status == 0).all()
    for m in range(3):
        single = _context(case, mocks[m])
        ref, status = single.eval_logposterior_host(theta)
        single.close()
        assert (status == 0).all() and (np.abs(cross[:, m] - ref) <= _tol(ref)).all(), (m, (np.abs(cross[:, m] - ref) / _tol(ref)).max())
    index = (np.arange(40) % 3).astype('i4')
    assert np.array_equal(ctx.eval_logposterior_data_host(theta, index=index)[0], cross[np.arange(40), index])
    ctx.close()


def test_kaiser_xi_cubic_context():
    """The correlation-function configuration with cubic interpolation of the Hankel transform (tests/golden/kaiser_xi_cubic.npz; it has no observable transform:
    the batch is accepted) against single-data contexts."""
    from test_gpu_kaiser_xi import make_kaiser_xi
    from desilike_amd._lib import Context
    g, like = make_kaiser_xi('kaiser_xi_cubic')
    like.initialize()
    flatdata = np.concatenate(like._flatdata_list())
    mocks = flatdata + 0.05 * np.abs(flatdata) * np.random.RandomState(5).standard_normal((3, flatdata.size))
    theta = np.asarray(g['theta'][:8], dtype='f8')
    spec = like._spec({}, like._flatdata_list(), like.precision)
    ctx = Context(spec, device=0)
    ctx.set_data_batch(mocks)
    cross, _ = ctx.eval_logposterior_data_host(theta)
    for m in range(3):
        single = Context(like._spec({}, [mocks[m]], like.precision), device=0)
        ref = single.eval_logposterior_host(theta)[0]
        ok = np.isfinite(ref)
        assert ok.sum() >= 4 and np.array_equal(np.isfinite(cross[:, m]), ok)
        assert (np.abs(cross[ok, m] - ref[ok]) <= _tol(ref[ok])).all()
        single.close()
    ctx.close()


def test_bad_rows():
    """A NaN theta row: -inf for every m, DL_STATUS_NAN_INPUT; an out-of-prior row: -inf, DL_STATUS_OUT_OF_PRIOR; a bad index: NaN, DL_STATUS_NAN_INPUT."""
    case, mocks, theta, ref, _ = reference('cfg2_shapefit_window')
    ctx = _context(case)
    M = 5
    ctx.set_data_batch(mocks[:M])
    rows = theta[:40].copy()
    rows[7, 2] = np.nan
    rows[33, 0] = case.priors[0, 2] + 1.      # above the upper limit of parameter 0
    assert np.isfinite(case.priors[0, 2])
    good = np.ones(40, dtype='?'); good[[7, 33]] = False
    cross, status = ctx.eval_logposterior_data_host(rows)
    assert np.isneginf(cross[7]).all() and status[7] == 3
    assert np.isneginf(cross[33]).all() and status[33] == 1
    assert (status[good] == 0).all() and (np.abs(cross[good] - ref[:40, :M][good]) <= _tol(ref[:40, :M][good])).all()
    index = (np.arange(40) % M).astype('i4')
    index[4], index[5] = -1, M
    paired, status = ctx.eval_logposterior_data_host(rows, index=index)
    assert np.isnan(paired[[4, 5]]).all() and (status[[4, 5]] == 3).all()
    assert np.isneginf(paired[[7, 33]]).all() and status[7] == 3 and status[33] == 1
    good[[4, 5]] = False
    assert np.array_equal(paired[good], cross[np.arange(40), np.clip(index, 0, M - 1)][good]) and (status[good] == 0).all()
    ctx.close()


def test_data_set_behaviour():
    """Refusals, replacement, M = 0, and the bits of the existing entry points before and after a dl_data_set on the same context."""
    import torch
    from desilike_amd import LibraryError
    from desilike_amd._lib import Context
    from test_gpu_variants import build
    from test_gpu_boundary import load_fixture
    case, mocks, theta, ref, _ = reference('cfg2_shapefit_window')
    dp = ctypes.POINTER(ctypes.c_double)
    # an observable transform
    like = build(template='shapefit', transform='cubic')[0]
    like.initialize()
    tctx = like._get_context()
    with pytest.raises(LibraryError, match='transform'):
        tctx.set_data_batch(np.ones((2, tctx.n_data)))
    assert tctx.n_data_batch == 0
    # analytically solved parameters
    sctx = Context(load_fixture('two_tracers_marg')[1], device=0)
    assert sctx.n_solved > 0
    with pytest.raises(LibraryError, match='solved'):
        sctx.set_data_batch(np.ones((2, sctx.n_data)))
    sctx.close()
    ctx = _context(case)
    with pytest.raises(LibraryError, match='no data batch'):
        ctx.eval_logposterior_data_host(theta[:4])
    # the existing entry points before ...
    device = torch.device('cuda', 0)
    centers = torch.as_tensor(theta[:6], device=device).contiguous()
    steps = torch.full((6, theta.shape[1], 2), 1e-3, dtype=torch.float64, device=device)

    def existing():
        out = [ctx.eval_logposterior_host(theta)[0], ctx.eval_logposterior_host(theta[:5])[0]] + list(ctx.eval_batch_host(theta[:64], return_flattheory=True))
        out += [t.cpu().numpy() for t in ctx.eval_fisher(centers, steps)]
        torch.cuda.synchronize()
        return out

    before = existing()
    ctx.set_data_batch(mocks[:17])
    # NaN / infinite data reach the library only past the Python check: refused there too, the batch held before stays
    bad = np.array(mocks[:3]); bad[1, 5] = np.nan
    with pytest.raises(ValueError, match='NaN or infinite'):
        ctx.set_data_batch(bad)
    assert ctx._lib.dl_data_set(ctx._handle, bad.ctypes.data_as(dp), 3) == 1 and b'NaN or infinite' in ctx._lib.dl_last_error(ctx._handle)
    bad[1, 5] = np.inf
    assert ctx._lib.dl_data_set(ctx._handle, bad.ctypes.data_as(dp), 3) == 1
    assert ctx._lib.dl_data_set(ctx._handle, bad.ctypes.data_as(dp), -1) == 1 and ctx._lib.dl_data_set(ctx._handle, bad.ctypes.data_as(dp), 65537) == 1
    assert ctx.n_data_batch == 17
    first = ctx.eval_logposterior_data_host(theta[:9])[0]
    assert (np.abs(first - ref[:9, :17]) <= _tol(first)).all()
    # ... a second call replaces the batch ...
    ctx.set_data_batch(mocks[20:23])
    second = ctx.eval_logposterior_data_host(theta[:9])[0]
    assert second.shape == (9, 3) and (np.abs(second - ref[:9, 20:23]) <= _tol(second)).all()
    # ... and after: the same bits
    after = existing()
    assert len(before) == len(after) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
    # M = 0 frees it
    assert ctx.set_data_batch(None) == 0 and ctx.n_data_batch == 0
    with pytest.raises(LibraryError, match='no data batch'):
        ctx.eval_logposterior_data_host(theta[:4])
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, existing()))
    ctx.close()


@pytest.mark.parametrize('name', ['cfg2_shapefit_window', 'boundary_two_tracers', 'boundary_cfg3'])
def test_fisher_data(name):
    """dl_eval_fisher_data against dl_eval_fisher on the per-mock contexts, 3 centres x 5 mocks; the Hessian does not depend on the index, bitwise."""
    import torch
    case, mocks, theta, _, _ = reference(name)
    device = torch.device('cuda', 0)
    nc, nm, P = 3, 5, theta.shape[1]
    centers = np.ascontiguousarray(np.repeat(theta[:nc], nm, axis=0))          # row c nm + m: centre c against mock m
    index = np.tile(np.arange(nm, dtype='i4'), nc)
    width = np.where(np.isfinite(case.priors[:, 2] - case.priors[:, 1]), case.priors[:, 2] - case.priors[:, 1], 1.)
    steps = np.ascontiguousarray(np.broadcast_to((1e-3 * width)[None, :, None], (nc * nm, P, 2)))
    ctx = _context(case)
    ctx.set_data_batch(mocks[:nm])
    hessian, gradient, offset = (t.cpu().numpy() for t in ctx.eval_fisher_data(torch.as_tensor(centers, device=device), torch.as_tensor(steps, device=device),
                                                                                torch.as_tensor(index, device=device)))
    worst = np.zeros(3)
    for m in range(nm):
        single = _context(case, mocks[m])
        rh, rg, ro = (t.cpu().numpy() for t in single.eval_fisher(torch.as_tensor(theta[:nc], device=device).contiguous(), torch.as_tensor(steps[:nc], device=device).contiguous()))
        single.close()
        rows = np.arange(nc) * nm + m
        assert np.allclose(offset[rows], ro, rtol=1e-10, atol=1e-9)
        for c, row in enumerate(rows):
            assert np.allclose(gradient[row], rg[c], rtol=1e-8, atol=1e-8 * np.abs(rg[c]).max()), (m, c)
            assert np.allclose(hessian[row], rh[c], rtol=1e-8, atol=1e-8 * np.abs(rh[c]).max()), (m, c)
            worst = np.maximum(worst, [abs(offset[row] / ro[c] - 1.), np.abs(gradient[row] - rg[c]).max() / np.abs(rg[c]).max(), np.abs(hessian[row] - rh[c]).max() / np.abs(rh[c]).max()])
    print('{}: worst relative differences to dl_eval_fisher: offset {:.2e}, gradient {:.2e}, hessian {:.2e}'.format(name, *worst))
    for c in range(nc):
        for m in range(1, nm):
            assert np.array_equal(hessian[c * nm + m], hessian[c * nm])
    # an index outside the table: NaN offset and gradient, the Hessian as for the others
    index[2] = nm
    hessian2, gradient2, offset2 = (t.cpu().numpy() for t in ctx.eval_fisher_data(torch.as_tensor(centers, device=device), torch.as_tensor(steps, device=device),
                                                                                   torch.as_tensor(index, device=device)))
    assert np.isnan(offset2[2]) and np.isnan(gradient2[2]).all() and np.array_equal(hessian2[2], hessian[2])
    keep = np.arange(nc * nm) != 2
    assert np.array_equal(offset2[keep], offset[keep]) and np.array_equal(gradient2[keep], gradient[keep])
    ctx.close()


# ---- Python ---------------------------------------------------------------------------------------------------------------------------
def _marg_likelihood(data=None):
    """The likelihood of tests/golden/marg_sn0_grid.npz (tests/test_gpu_marg.py::make_marg_likelihood): sn0 '.marg' with a Gaussian prior, a constant derivative row."""
    from golden_utils import load_golden
    from desilike_amd.theories.galaxy_clustering import ShapeFitPowerSpectrumTemplate, KaiserTracerPowerSpectrumMultipoles
    from desilike_amd.observables.galaxy_clustering import TracerPowerSpectrumMultipolesObservable
    from desilike_amd.likelihoods import ObservablesGaussianLikelihood
    g = load_golden('marg_sn0_grid')
    theory = KaiserTracerPowerSpectrumMultipoles(template=ShapeFitPowerSpectrumTemplate(z=0.5))
    theory.init.params['sn0'].update(prior=dict(dist='norm', loc=0.2, scale=1.5), derived='.marg')
    obs = TracerPowerSpectrumMultipolesObservable(data=g['obs0']['flatdata'] if data is None else data, kedges=np.linspace(0., 0.2, 41), ells=(0, 2, 4), wmatrix={'resolution': 10},
                                                  theory=theory, shotnoise=1e4)
    return g, ObservablesGaussianLikelihood(observables=[obs], covariance=g['covariance'])


def _marg_mocks(like, M):
    flatdata = np.concatenate(like._flatdata_list())
    return flatdata + 0.05 * np.abs(flatdata) * np.random.RandomState(5).standard_normal((M, flatdata.size))


def test_likelihood_data_batch_marginalised():
    """likelihood.data_batch with a constant-rows '.marg' sn0 against per-mock likelihood instances (what their samplers consume: evaluate_logposterior)."""
    import torch
    g, like = _marg_likelihood()
    like.initialize()
    assert like._solved_are_constant()
    M, B = 4, 24
    mocks = _marg_mocks(like, M)
    names = like.varied_params.names()
    rnames = [str(n) for n in g['names']]
    values = np.ascontiguousarray(np.asarray(g['theta'], dtype='f8')[:B][:, [rnames.index(name) for name in names]])
    batch = like.data_batch(mocks)
    assert batch.size == M and batch.context.n_solved == 0 and batch.offset != 0.
    cross = batch.logposterior(values)
    index = np.arange(len(values)) % M
    paired = batch.logposterior(values, index)
    assert cross.shape == (len(values), M) and np.array_equal(paired, cross[np.arange(len(values)), index])
    worst = 0.
    for m in range(M):
        ref = _marg_likelihood(data=mocks[m])[1].evaluate_logposterior(torch.as_tensor(values, device='cuda:0')).cpu().numpy()
        ok = np.isfinite(ref)
        assert ok.sum() >= len(values) // 2 and np.array_equal(np.isfinite(cross[:, m]), ok)
        err = np.abs(cross[ok, m] - ref[ok]) / _tol(ref[ok])
        worst = max(worst, err.max())
        assert (err <= 1.).all(), (m, err.max())
    print('marginalised sn0: worst |data_batch - per-mock likelihood| = {:.2e} of the tolerance'.format(worst))
    with pytest.raises(ValueError):
        batch.logposterior(values, index=np.full(len(values), M))


def test_point_dependent_solved_rows_raise():
    from test_gpu_sample_solved import _eft_likelihood
    like = _eft_likelihood()
    like.initialize()
    with pytest.raises(NotImplementedError, match='maximize_batch'):
        like.data_batch(np.concatenate(like._flatdata_list())[None, :])


def test_maximize_batch_against_maximize():
    """maximize_batch against maximize on per-mock likelihoods from the same starts: log-posterior at the maximum to 1e-8, best fits to 1e-5 of their errors (both runs
    do the same arithmetic up to rounding; Gauss-Newton converges quadratically past xtol = 1e-7 sigma).
    Measured (MI355X; printed below, recorded in DESIGN.md section 6l): both differences are 0.0 -- row 0 of the Fisher stencil adds the mock's whitened bias in the
    order the per-mock context adds its own, so the two runs are the same arithmetic."""
    import warnings
    from desilike_amd.profilers import GaussNewtonProfiler
    g, like = _marg_likelihood()
    like.initialize()
    M, nstarts = 3, 2
    mocks = _marg_mocks(like, M)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        profiler = GaussNewtonProfiler(like, seed=11)
        start = profiler._get_start_points(nstarts)
        profiles = profiler.maximize_batch(mocks, start=start)
        with pytest.raises(NotImplementedError):
            GaussNewtonProfiler(like, seed=11, derivatives='analytic').maximize_batch(mocks, start=start)
    assert len(profiles) == M
    names = [param.name for param in profiler.params]
    assert 'sn0' in names      # the solved parameter is varied
    worst_f, worst_x = 0., 0.
    for m in range(M):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ref = GaussNewtonProfiler(_marg_likelihood(data=mocks[m])[1], seed=11).maximize(start=start)
        assert all(profiles[m].attrs['converged']) and all(ref.attrs['converged'])
        df = np.abs(profiles[m].bestfit['logposterior'] - ref.bestfit['logposterior']).max()
        dx = max(np.abs((profiles[m].bestfit[name] - ref.bestfit[name]) / ref.error[name]).max() for name in names)
        worst_f, worst_x = max(worst_f, df), max(worst_x, dx)
        assert df <= 1e-8, (m, df)
        assert dx <= 1e-5, (m, dx)
        assert np.allclose(profiles[m].start['b1'], start[:, names.index('b1')])
    print('maximize_batch against maximize: log-posterior at the maximum differs by at most {:.2e}, best fits by at most {:.2e} of their errors'.format(worst_f, worst_x))
