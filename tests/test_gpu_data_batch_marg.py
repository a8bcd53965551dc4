"""GPU (-m gpu): the data batch of contexts with analytically solved parameters -- ``dl_data_set_solved``, ``dl_eval_logposterior_data`` on such a context,
``dl_eval_solved_data`` (csrc/dl_data_batch_marg.h), ``likelihood.data_batch(data, solve='point')``.

Cases of tests/marg_counts_cases.py (data vectors: tests/data_batch_marg_utils.py::mocks, the recipe of the cases' own data; their input conditions are asserted on the CPU
by tests/test_data_batch_marg.py).  Two yardsticks, neither of them the code under test:
  1. the extended-precision reference tests/marg_reference.py on the NROWS rows of a case against data vectors 0, M // 2, M - 1: log-posterior (with the oracle's log-prior of the
     sampled parameters) to 1e-10 max(1, |.|), solved values of dl_eval_solved_data to rtol 1e-8, atol 1e-10;
  2. every other pair against per-mock contexts -- the same configuration with its data replaced, evaluated with dl_eval_logposterior -- to 1e-10 max(1, |.|), equal sets of
     finite entries.
Bits: paired == cross; the same (row, data vector) at every M; the same pair in two batches B with an equal split count of the window GEMM (1e-12 max(1, |.|) otherwise)."""
import ctypes
import functools

import numpy as np
import pytest

import marg_counts_cases as mc
import data_batch_marg_utils as dbm
from test_gpu_marg_counts import tiled_splits, split_point, batch, _singular_residual

pytestmark = pytest.mark.gpu

DL_ST_OUT_OF_PRIOR, DL_ST_NONFINITE, DL_ST_NAN_INPUT = 1, 2, 3


def _tol(ref):
    return 1e-10 * np.maximum(1., np.abs(ref))


def with_data(spec, sizes, flatdata):
    blocks = np.split(np.asarray(flatdata, dtype='f8'), np.cumsum(sizes)[:-1])
    return dict(spec, observables=[dict(obs, flatdata=block.copy()) for obs, block in zip(spec['observables'], blocks)])


def per_mock(spec, sizes, mocks, theta):
    """[B, M] log-posteriors and [B] statuses (of data vector 0) of the project's single-data path: one context per data vector."""
    from desilike_amd._lib import Context
    ref, status0 = np.empty((len(theta), len(mocks))), None
    for m, mock in enumerate(mocks):
        ctx = Context(with_data(spec, sizes, mock), device=0)
        ref[:, m], status = ctx.eval_logposterior_host(theta)
        if m == 0: status0 = status
        ctx.close()
    return ref, status0


def check_case(key, spec_of, sizes_B, extra_B=()):
    """``spec_of(mask)`` -> (spec, observable sizes, likelihood).  Returns the largest errors against the two yardsticks."""
    from desilike_amd._lib import Context
    case = dbm.get_case(key)
    mocks = dbm.mocks(key)
    logprior_varied = case.logprior_varied(case.theta)
    rng = np.random.RandomState(case.n + case.n_s)
    Ms = dbm.data_sizes(key)
    worst = np.zeros(3)
    for name, mask in dbm.gpu_patterns(case.n_s):
        spec, sizes, like = spec_of(mask)
        ctx = Context(spec, device=0)
        assert ctx.n_solved == case.n_s and ctx.n_data == case.n
        R, N_pad, K_pad = 1 + getattr(case, 'n_var', 0), ctx.info('N_pad'), ctx.info('K_pad')
        Bs = list(sizes_B) + [B(R, N_pad, K_pad) for B in extra_B]
        filler = np.column_stack([np.clip(param.ref.sample(size=max(Bs), random_state=rng), *param.prior.limits) for param in like.varied_params])
        Bref = max(sizes_B)
        theta_ref = batch(case, Bref, filler)
        ref, status_ref = per_mock(spec, sizes, mocks[:max(Ms)], theta_ref)
        cross = {}
        for M in Ms:
            assert ctx.set_data_batch(mocks[:M], solved=True) == M and ctx.n_data_batch == M
            for B in Bs:
                theta = batch(case, B, filler)
                out, status = ctx.eval_logposterior_data_host(theta)
                assert out.shape == (B, M)
                cross[B, M] = out
                nb = min(B, Bref)
                assert np.array_equal(status[:nb], status_ref[:nb]), (key, name, M, B)
                # yardstick 2: every pair against the per-mock contexts
                assert np.array_equal(np.isfinite(out[:nb]), np.isfinite(ref[:nb, :M])), (key, name, M, B)
                ok = np.isfinite(ref[:nb, :M])
                err = np.where(ok, np.abs(np.where(ok, out[:nb] - ref[:nb, :M], 0.)) / _tol(ref[:nb, :M]), 0.)
                worst[0] = max(worst[0], err.max())
                assert (err <= 1.).all(), (key, name, M, B, 'per-mock contexts', err.max())
                # yardstick 1: the extended-precision reference on the case's rows
                nrows = min(B, mc.NROWS)
                index = np.zeros(B, dtype='i4')
                for m in dbm.reference_mocks(M):
                    index[:] = m
                    paired, pstatus, solved = ctx.eval_solved_data_host(theta, index)
                    assert np.array_equal(paired, out[:, m]) and np.array_equal(pstatus, status), (key, name, M, B, m, 'paired != cross')
                    assert np.array_equal(ctx.eval_logposterior_data_host(theta, index=index)[0], paired)
                    for i in range(nrows):
                        r = dbm.reference(key, i, m, mask)
                        lpost = r['loglikelihood'] + logprior_varied[i] + r['logprior_solved']
                        e = abs(out[i, m] - lpost) / max(1., abs(lpost))
                        worst[1] = max(worst[1], e)
                        worst[2] = max(worst[2], (np.abs(solved[i] - r['x']) / (1e-10 + 1e-8 * np.abs(r['x']))).max())
                        assert status[i] == 0
                        assert e <= 1e-10, (key, name, M, B, i, m, 'reference', out[i, m], lpost, e)
                        assert np.allclose(solved[i], r['x'], rtol=1e-8, atol=1e-10), (key, name, M, B, i, m, solved[i], r['x'])
            # paired == cross with a mixed index
            B = Bref
            index = (np.arange(B) % M).astype('i4')
            paired = ctx.eval_logposterior_data_host(batch(case, B, filler), index=index)[0]
            assert np.array_equal(paired, cross[B, M][np.arange(B), index]), (key, name, M)
        # the same (row, data vector) at every M: the same bits
        for B in Bs:
            for M in Ms:
                assert np.array_equal(cross[B, M], cross[B, max(Ms)][:, :M]), (key, name, B, M, 'bits across M')
        # ... and across B: bit for bit at an equal split count, 1e-12 max(1, |.|) otherwise (the rules of compare_batches)
        splits = {B: (tiled_splits(B * R, N_pad, K_pad) if len(key) == 2 else 1) for B in Bs}
        M = max(Ms)
        for a in Bs:
            for b in Bs:
                if b <= a: continue
                nrows = a      # (every batch is a prefix of the case's rows followed by the same filler rows)
                qa, qb = cross[a, M][:nrows], cross[b, M][:nrows]
                if splits[a] == splits[b]: assert np.array_equal(qa, qb), (key, name, a, b, splits[a])
                else: assert (np.abs(qa - qb) <= 1e-12 * np.maximum(1., np.abs(qb))).all(), (key, name, a, b, splits[a], splits[b], np.abs(qa - qb).max())
        ctx.close()
    return worst


@functools.lru_cache(maxsize=2)
def _residual_spec(key):
    case = dbm.get_case(key)
    like = case.likelihood(np.ones(case.n_s, dtype='?'))
    like.initialize()
    assert like.solved_params.names() == case.solved and like.varied_params.names() == case.names
    return like, like._spec({}, like._flatdata_list(), like._precision_input)


@pytest.mark.parametrize('key', dbm.RESIDUAL_CASES, ids=[dbm.case_id(key) for key in dbm.RESIDUAL_CASES])
def test_residual_route(key):
    like, spec = _residual_spec(key)
    sizes = [np.size(obs['flatdata']) for obs in spec['observables']]

    def spec_of(mask):      # the masks through marg.kind in the spec, as tests/test_gpu_marg_counts.py
        return dict(spec, marg=dict(spec['marg'], kind=mask.astype('i4'))), sizes, like

    # (57, 5): also one batch on each side of the point where the window GEMM is no longer split
    extra = [lambda R, N_pad, K_pad: split_point(R, N_pad, K_pad) - 1, split_point] if key == (57, 5) else []
    worst = check_case(key, spec_of, [1, 3, 65], extra)
    print('\nresidual {}: M {}: max |cross - per-mock contexts| {:.2e} tol, |cross - reference| {:.1e}, solved {:.3f} tol'.format(dbm.case_id(key), dbm.data_sizes(key), *worst))


@pytest.mark.parametrize('key', dbm.GRAM_CASES, ids=[dbm.case_id(key) for key in dbm.GRAM_CASES])
def test_feature_routes(key):
    case = dbm.get_case(key)

    def spec_of(mask):      # the flags through the Python layer
        like = case.likelihood(mask)
        like.initialize()
        assert like.solved_params.names() == case.solved and like.varied_params.names() == case.names
        return like._spec({}, [case.flatdata], like._precision_input), [case.n], like

    worst = check_case(key, spec_of, [1, 65, 200])
    print('\nfeature route {}: M {}: max |cross - per-mock contexts| {:.2e} tol, |cross - reference| {:.1e}, solved {:.3f} tol'.format(dbm.case_id(key), dbm.data_sizes(key), *worst))


def test_stacked_layout():
    """The benchmarked shape (stacked emulator layout, 5 marginalised parameters) against per-mock contexts: M = 3, B = 65."""
    from desilike_amd._lib import Context
    import data_batch_utils as dbu
    case = dbu.get_case('boundary_cfg3_stacked_bench')
    ctx = Context(case.spec, device=0)
    assert ctx.n_solved == 5
    n = case.flatdata.size
    covariance = np.linalg.inv(case.precision if case.precision.ndim == 2 else np.diag(case.precision))
    mocks = case.flatdata + np.random.RandomState(dbm.MOCK_SEED).multivariate_normal(np.zeros(n), covariance, size=3)
    theta = case.points(65)
    ref = np.empty((65, 3))
    for m in range(3):
        rctx = Context(case.spec_with_data(mocks[m]), device=0)
        ref[:, m], status_ref = rctx.eval_logposterior_host(theta)
        rctx.close()
    assert ctx.set_data_batch(mocks, solved=True) == 3
    out, status = ctx.eval_logposterior_data_host(theta)
    assert np.array_equal(np.isfinite(out), np.isfinite(ref)) and np.isfinite(ref).sum() >= ref.size // 2
    ok = np.isfinite(ref)
    err = np.abs(out[ok] - ref[ok]) / _tol(ref[ok])
    print('\nstacked layout: worst |cross - per-mock contexts| = {:.2e} of the tolerance, |logposterior| up to {:.3e}'.format(err.max(), np.abs(ref[ok]).max()))
    assert (err <= 1.).all(), err.max()
    index = (np.arange(65) % 3).astype('i4')
    paired, pstatus, solved = ctx.eval_solved_data_host(theta, index)
    assert np.array_equal(paired, out[np.arange(65), index]) and solved.shape == (65, 5) and np.isfinite(solved[np.isfinite(paired)]).all()
    ctx.close()


def _mvn_mocks(like, covariance, M):
    flatdata = np.concatenate(like._flatdata_list())
    return flatdata + np.random.RandomState(dbm.MOCK_SEED).multivariate_normal(np.zeros(flatdata.size), covariance, size=M)


def test_python_layer_point_dependent_rows():
    """``_eft_likelihood()`` (two counter terms '.marg', sn0_2 '.best') with solve='point' against per-mock likelihood instances; the default call still raises."""
    import torch
    from golden_utils import load_golden
    import test_gpu_sample_solved as tss
    like = tss._eft_likelihood()
    like.initialize()
    g = load_golden('cfg2_shapefit_window_dense')
    M, B = 3, 24
    mocks = _mvn_mocks(like, g['covariance'], M)
    with pytest.raises(NotImplementedError, match='maximize_batch'):
        like.data_batch(mocks)
    rng = np.random.RandomState(3)
    values = np.column_stack([np.clip(param.ref.sample(size=B, random_state=rng), *param.prior.limits) for param in like.varied_params])
    dbatch = like.data_batch(mocks, solve='point')
    assert dbatch.size == M and dbatch.context.n_solved == 3 and dbatch.offset == 0.
    cross = dbatch.logposterior(values)
    index = np.arange(B) % M
    paired, solved = dbatch.logposterior(values, index), dbatch.solved(values, index)
    assert cross.shape == (B, M) and np.array_equal(paired, cross[np.arange(B), index]) and solved.shape == (B, 3)
    worst = np.zeros(2)
    for m in range(M):
        other = _with_data(tss._eft_likelihood, mocks[m])
        ref = other.evaluate_logposterior(torch.as_tensor(values, device='cuda:0')).cpu().numpy()
        ref_solved = other._get_context().eval_batch_derived_host(values)[3]
        assert np.array_equal(np.isfinite(cross[:, m]), np.isfinite(ref)) and np.isfinite(ref).all()
        err = np.abs(cross[:, m] - ref) / _tol(ref)
        worst[0] = max(worst[0], err.max())
        assert (err <= 1.).all(), (m, err.max())
        rows = index == m
        worst[1] = max(worst[1], (np.abs(solved[rows] - ref_solved[rows]) / (1e-10 + 1e-8 * np.abs(ref_solved[rows]))).max())
        assert np.allclose(solved[rows], ref_solved[rows], rtol=1e-8, atol=1e-10), m
    print('\nsolve=\'point\' vs per-mock likelihoods: log-posterior {:.2e} tol, solved {:.3f} tol'.format(*worst))


def _with_data(make, data):
    """The likelihood of ``make()`` with the data of its (single) observable replaced."""
    like = make()
    obs = like.init['observables']
    obs = obs[0] if isinstance(obs, (list, tuple)) else obs
    obs.init.update(data=np.array(data))
    return like


def test_python_layer_constant_rows_both_routes():
    """The constant-row likelihood of tests/golden/marg_sn0_grid.npz through solve='constant' (marginalised precision) and solve='point': the same values."""
    from test_gpu_data_batch import _marg_likelihood
    g, like = _marg_likelihood()
    like.initialize()
    assert like._solved_are_constant()
    M, B = 4, 24
    mocks = _mvn_mocks(like, g['covariance'], M)
    names, rnames = like.varied_params.names(), [str(n) for n in g['names']]
    values = np.ascontiguousarray(np.asarray(g['theta'], dtype='f8')[:B][:, [rnames.index(name) for name in names]])
    B = len(values)
    constant, point = like.data_batch(mocks), like.data_batch(mocks, solve='point')
    assert constant.solve == 'constant' and constant.context.n_solved == 0 and point.context.n_solved == 1
    a, b = constant.logposterior(values), point.logposterior(values)
    assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.isfinite(a).sum() >= a.size // 2
    ok = np.isfinite(a)
    err = np.abs(a[ok] - b[ok]) / _tol(a[ok])
    print('\nconstant rows: worst |solve=constant - solve=point| = {:.2e} of the tolerance, |logposterior| up to {:.3e}'.format(err.max(), np.abs(a[ok]).max()))
    assert (err <= 1.).all(), err.max()
    with pytest.raises(ValueError, match="solve='point'"):
        constant.solved(values, np.zeros(B, dtype='i4'))
    assert point.solved(values, np.zeros(B, dtype='i4')).shape == (B, 1)


def test_bad_rows_and_indices():
    """A NaN row and a row outside the prior: -inf for every data vector, the status set; paired indices outside [0, M): NaN and DL_STATUS_NAN_INPUT."""
    from desilike_amd._lib import Context
    key = (57, 5)
    case, (like, spec) = dbm.get_case(key), _residual_spec(key)
    ctx = Context(spec, device=0)
    M = 3
    ctx.set_data_batch(dbm.mocks(key)[:M], solved=True)
    theta = np.array(case.theta)
    theta[2, 1] = np.nan
    limits = like.varied_params[0].prior.limits
    assert np.isfinite(limits[1])
    theta[5, 0] = limits[1] + 1.
    good = np.array([0, 1, 3, 4, 6, 7])
    clean = ctx.eval_logposterior_data_host(case.theta)[0]
    out, status = ctx.eval_logposterior_data_host(theta)
    assert np.isneginf(out[2]).all() and status[2] == DL_ST_NAN_INPUT
    assert np.isneginf(out[5]).all() and status[5] == DL_ST_OUT_OF_PRIOR
    assert np.array_equal(out[good], clean[good]) and (status[good] == 0).all() and np.isfinite(out[good]).all()
    index = np.array([0, M, 1, -1, 2, 0, 65536, 1], dtype='i4')
    paired, pstatus, solved = ctx.eval_solved_data_host(case.theta, index)
    bad = (index < 0) | (index >= M)
    assert np.isnan(paired[bad]).all() and (pstatus[bad] == DL_ST_NAN_INPUT).all() and np.isnan(solved[bad]).all()
    assert np.array_equal(paired[~bad], clean[np.flatnonzero(~bad), index[~bad]]) and (pstatus[~bad] == 0).all() and np.isfinite(solved[~bad]).all()
    assert np.array_equal(ctx.eval_logposterior_data_host(case.theta, index=index)[0], paired, equal_nan=True)
    ctx.close()


def test_singular_system():
    """A flat-prior solved parameter with an exactly zero derivative row (tests/test_gpu_marg_counts.py::_singular_residual): -inf and DL_ST_NONFINITE for every row and
    every data vector, nothing else happens."""
    from desilike_amd._lib import Context
    like = _singular_residual()
    like.initialize()
    like._get_context()
    ctx = Context(like._context_specs[()], device=0)
    assert ctx.n_solved == 1
    mocks = _mvn_mocks(like, like.covariance, 3)
    ctx.set_data_batch(mocks, solved=True)
    rng = np.random.RandomState(2)
    theta = np.column_stack([np.clip(param.ref.sample(size=67, random_state=rng), *param.prior.limits) for param in like.varied_params])
    out, status = ctx.eval_logposterior_data_host(theta)
    assert out.shape == (67, 3) and np.isneginf(out).all() and (status == DL_ST_NONFINITE).all()
    paired, pstatus, solved = ctx.eval_solved_data_host(theta, (np.arange(67) % 3).astype('i4'))
    assert np.isneginf(paired).all() and (pstatus == DL_ST_NONFINITE).all()
    ctx.close()


def test_data_set_solved_behaviour():
    """Refusals, replacement, M = 0; the bits of the existing entry points before and after a batch is set on the same solved context; dl_data_set still refuses it."""
    import torch
    from desilike_amd import LibraryError
    from desilike_amd._lib import Context
    from golden_utils import load_golden, spec_from_golden
    from test_gpu_variants import build
    key = (57, 5)
    case, (like, spec) = dbm.get_case(key), _residual_spec(key)
    mocks = dbm.mocks(key)
    dp = ctypes.POINTER(ctypes.c_double)
    # an observable transform is still refused
    tlike = build(template='shapefit', transform='cubic')[0]
    tlike.initialize()
    tctx = tlike._get_context()
    with pytest.raises(LibraryError, match='transform'):
        tctx.set_data_batch(np.ones((2, tctx.n_data)), solved=True)
    assert tctx.n_data_batch == 0
    # a context without solved parameters: exactly dl_data_set
    g = load_golden('cfg2_shapefit_window')
    pctx = Context(spec_from_golden(g), device=0)
    pmocks = np.concatenate([np.ravel(obs['flatdata']) for obs in spec_from_golden(g)['observables']])[None, :] * np.array([[1.01], [0.99]])
    ptheta = np.asarray(g['theta'], dtype='f8')[:9]
    pctx.set_data_batch(pmocks)
    plain = pctx.eval_logposterior_data_host(ptheta)
    pctx.set_data_batch(pmocks, solved=True)
    again = pctx.eval_logposterior_data_host(ptheta)
    assert np.array_equal(plain[0], again[0]) and np.array_equal(plain[1], again[1])
    with pytest.raises(LibraryError, match='no analytically solved'):
        pctx.eval_solved_data_host(ptheta, np.zeros(9, dtype='i4'))
    pctx.close()
    ctx = Context(spec, device=0)
    with pytest.raises(LibraryError, match='no data batch'):
        ctx.eval_logposterior_data_host(case.theta)
    with pytest.raises(LibraryError, match='no data batch'):
        ctx.eval_solved_data_host(case.theta, np.zeros(mc.NROWS, dtype='i4'))

    def existing():
        out = list(ctx.eval_logposterior_host(case.theta)) + list(ctx.eval_batch_derived_host(case.theta))
        out += [t.cpu().numpy() for t in ctx.sample_solved(torch.as_tensor(case.theta, device='cuda:0'), index0=3, size=2, seed=7)]
        torch.cuda.synchronize()
        return out

    before = existing()
    with pytest.raises(LibraryError, match='solved'):
        ctx.set_data_batch(mocks[:2])                  # dl_data_set keeps refusing the context
    assert ctx.n_data_batch == 0
    assert ctx.set_data_batch(mocks[:17], solved=True) == 17
    first = ctx.eval_logposterior_data_host(case.theta)[0]
    # NaN / infinite data and counts out of range reach the library only past the Python checks: refused there too, the batch held before stays
    bad = np.array(mocks[:3]); bad[1, 5] = np.inf
    with pytest.raises(ValueError, match='NaN or infinite'):
        ctx.set_data_batch(bad, solved=True)
    assert ctx._lib.dl_data_set_solved(ctx._handle, bad.ctypes.data_as(dp), 3) == 1 and b'NaN or infinite' in ctx._lib.dl_last_error(ctx._handle)
    assert ctx._lib.dl_data_set_solved(ctx._handle, bad.ctypes.data_as(dp), -1) == 1
    assert ctx._lib.dl_data_set_solved(ctx._handle, bad.ctypes.data_as(dp), 65537) == 1
    assert ctx._lib.dl_data_set_solved(ctx._handle, None, 2) == 1
    assert ctx._lib.dl_data_set(ctx._handle, bad.ctypes.data_as(dp), 3) == 1
    assert ctx.n_data_batch == 17 and np.array_equal(ctx.eval_logposterior_data_host(case.theta)[0], first)
    # replacement, then M = 0
    assert ctx.set_data_batch(mocks[3:5], solved=True) == 2 and ctx.n_data_batch == 2
    assert np.array_equal(ctx.eval_logposterior_data_host(case.theta)[0], first[:, 3:5])
    after = existing()
    assert len(before) == len(after) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
    assert ctx.set_data_batch(None, solved=True) == 0 and ctx.n_data_batch == 0
    with pytest.raises(LibraryError, match='no data batch'):
        ctx.eval_logposterior_data_host(case.theta)
    ctx.close()
