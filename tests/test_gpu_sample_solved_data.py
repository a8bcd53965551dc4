"""GPU (-m gpu): posterior draws of the solved parameters of a data batch -- ``dl_sample_solved_data`` (csrc/dl_sample_solved_data.h), ``DataBatch.sample_solved``,
``desilike_amd.sample_solved(data_batch, ...)``, ``MockEmceeSampler.sample_solved``.

Cases of tests/marg_counts_cases.py with the data vectors of tests/data_batch_marg_utils.py (rows of ONE seeded draw around the cases' own data: chi2(x0) stays small; the
input conditions are asserted on the CPU by tests/test_data_batch_marg.py and tests/test_sample_solved_data.py).  Yardsticks, none of them the code under test:
  1. the context with NOTHING marginalised (the solved parameters varied: tests/test_gpu_sample_solved.py::_full_context) given the same batch with dl_data_set and
     evaluated with the paired call at (theta, draw): loglike + logprior of every draw to 1e-10 max(1, |.|);
  2. per-mock contexts and dl_sample_solved with the same seed and index0: draws to rtol 1e-8, atol 1e-10, loglike and logprior SEPARATELY to 1e-10 max(1, |.|);
  3. the Python mirror of the draw addressing: |C^T (x - x^) - z| <= 100 cond(A) eps with x^ of dl_eval_solved_data and NumPy's factor of the per-mock context's H_L.
x0 + dx of the draw path cannot be observed on its own without a change of the ABI (every output carries v; no seed gives v = 0): its bitwise equality with
dl_eval_solved_data rests on the shared row phase and dl_dbm_pair_finish, and is bounded here by yardstick 3."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import marg_counts_cases as mc
import data_batch_marg_utils as dbm
import solved_oracle as so
from test_gpu_marg_counts import tiled_splits, batch, _singular_residual
from test_gpu_data_batch_marg import with_data, _residual_spec, _mvn_mocks

pytestmark = pytest.mark.gpu

SEED = 42
DL_ST_OUT_OF_PRIOR, DL_ST_NONFINITE, DL_ST_NAN_INPUT = 1, 2, 3
REF_MOCKS = 3      # per-mock contexts per case


def _rel(got, ref):
    return np.abs(got - ref) / np.maximum(1., np.abs(ref))


def _identity(full, theta, index, x, loglike, logprior):
    """Worst |loglike + logprior - full log-posterior at (theta, x) given data vector index| / max(1, |.|) over the draws."""
    size, ns = x.shape[1], x.shape[2]
    points = np.concatenate([np.repeat(theta, size, axis=0), x.reshape(-1, ns)], axis=1)
    ref, status = full.eval_logposterior_data_host(points, index=np.repeat(index, size).astype('i4'))
    assert (status == 0).all() and np.isfinite(ref).all()
    return _rel((loglike + logprior).ravel(), ref).max()


def _check(ctx, full, per_mock_spec, mocks, theta, M, size, index0, label, worst, prec):
    """One (context, M, B, size): identity on a mixed index; per-mock contexts and the mean on REF_MOCKS data vectors.  ``prec``: prior precisions of the solved
    parameters.  ``worst``: running maxima [identity, draws / tol, loglike, logprior, mean residual / bound] and the number of points the mean was checked on."""
    from desilike_amd._lib import Context
    B, ns = len(theta), ctx.n_solved
    assert ctx.set_data_batch(mocks[:M], solved=True) == M
    assert full.set_data_batch(mocks[:M]) == M
    index = ((np.arange(B) * 7 + 3) % M).astype('i4')
    x, loglike, logprior, status = ctx.sample_solved_data(theta, index, index0=index0, size=size, seed=SEED)
    assert x.shape == (B, size, ns) and loglike.shape == logprior.shape == (B, size) and status.shape == (B,)
    ok = status == 0      # (filler rows drawn from the ref distributions may fail; the rows of the case must not)
    assert ok[:mc.NROWS].all() and ok.sum() >= (B + 1) // 2 and np.isfinite(x[ok]).all() and np.isnan(x[~ok]).all(), (label, status)
    worst[0] = max(worst[0], _identity(full, theta[ok], index[ok], x[ok], loglike[ok], logprior[ok]))
    assert worst[0] <= 1e-10, (label, 'full-posterior identity', worst[0])
    z = so.gauss(SEED, index0 + np.arange(B), np.arange(size), ns)
    for m in sorted({0, M // 2, M - 1})[:REF_MOCKS]:
        index = np.full(B, m, dtype='i4')
        x, loglike, logprior, status = ctx.sample_solved_data(theta, index, index0=index0, size=size, seed=SEED)
        xhat = ctx.eval_solved_data_host(theta, index)[2]
        rctx = Context(per_mock_spec(mocks[m]), device=0)
        rx, rll, rlp, rstatus = rctx.sample_solved(theta, index0=index0, size=size, seed=SEED)
        hessian = rctx.eval_batch_derived_host(theta)[4]
        rctx.close()
        ok = status == 0
        assert np.array_equal(status, rstatus) and ok[:mc.NROWS].all() and ok.sum() >= (B + 1) // 2, (label, m, status, rstatus)
        assert np.isnan(x[~ok]).all() and np.isnan(loglike[~ok]).all() and np.isnan(logprior[~ok]).all()
        x, loglike, logprior, xhat, hessian, rx, rll, rlp, zm = x[ok], loglike[ok], logprior[ok], xhat[ok], hessian[ok], rx[ok], rll[ok], rlp[ok], z[ok]
        worst[1] = max(worst[1], (np.abs(x - rx) / (1e-10 + 1e-8 * np.abs(rx))).max())
        worst[2], worst[3] = max(worst[2], _rel(loglike, rll).max()), max(worst[3], _rel(logprior, rlp).max())
        assert np.allclose(x, rx, rtol=1e-8, atol=1e-10), (label, m, 'draws vs per-mock context', worst[1])
        assert worst[2] <= 1e-10 and worst[3] <= 1e-10, (label, m, 'loglike / logprior vs per-mock context', worst[2], worst[3])
        for b in range(len(x)):      # the mean: C^T (x - x^) against the mirror's z, where cond(A) meets the condition of tests/test_gpu_sample_solved.py::test_draws_vs_oracle
            C, bound = so.draw_bound(hessian[b], prec)
            if not bound < 1e-9: continue
            resid = np.abs((x[b] - xhat[b]).dot(C) - zm[b]).max()
            worst[4] = max(worst[4], resid / bound)
            worst[5] += 1
            assert resid <= bound, (label, m, b, resid, bound)


def _prior_precision(prior_scale):
    return np.where(np.isinf(prior_scale), 0., 1. / np.asarray(prior_scale, dtype='f8')**2)


# cases whose cond(A) meets the condition of the mean check (bound below 1e-9) on their own rows: the check must reach points there
MEAN_CHECKED = [(57, 1), (57, 4), (20, 3)]


def _report(label, worst):
    print('\n{}: identity {:.2e}; vs per-mock contexts: draws {:.3f} tol, loglike {:.2e}, logprior {:.2e}; mean residual {:.2e} of the bound on {:d} points'.format(
        label, worst[0], worst[1], worst[2], worst[3], worst[4], int(worst[5])))


RESIDUAL_CASES = [(57, n_s) for n_s in (1, 4, 5, 8, 9, 13, 16)] + [(20, 3), (512, 16)]


@pytest.mark.parametrize('key', RESIDUAL_CASES, ids=[dbm.case_id(key) for key in RESIDUAL_CASES])
def test_residual_route(key):
    """Masks all / none / half; (M, B, size) = (33, 65, 3), (1, 3, 65), (33, 1, 130), (1, 65, 1), (33, 3, 64): every B, M and size of the sweep, either side of one and
    two trips of the lane loop.  (512, 16): one mask, one shape."""
    from desilike_amd._lib import Context
    import test_gpu_sample_solved as tss
    case, (like, spec) = dbm.get_case(key), _residual_spec(key)
    sizes = [np.size(obs['flatdata']) for obs in spec['observables']]
    mocks = dbm.mocks(key)
    full = tss._full_context(like)
    rng = np.random.RandomState(case.n + case.n_s)
    filler = np.column_stack([np.clip(param.ref.sample(size=65, random_state=rng), *param.prior.limits) for param in like.varied_params])
    shapes = [(33, 65, 3), (1, 3, 65), (33, 1, 130), (1, 65, 1), (33, 3, 64)]
    patterns = dbm.gpu_patterns(case.n_s)
    if key[0] == 512: shapes, patterns = [(3, 3, 3)], patterns[:1]
    worst = np.zeros(6)
    for ip, (name, mask) in enumerate(patterns):
        mspec = dict(spec, marg=dict(spec['marg'], kind=mask.astype('i4')))
        ctx = Context(mspec, device=0)
        for M, B, size in (shapes if ip == 0 else shapes[:2]):
            _check(ctx, full, lambda mock: with_data(mspec, sizes, mock), mocks, batch(case, B, filler), M, size, 11 * B, (key, name, M, B, size), worst,
                   _prior_precision(case.prior_scale))
        ctx.close()
    full.close()
    _report('residual ' + dbm.case_id(key), worst)
    if key in MEAN_CHECKED:
        assert worst[5] >= mc.NROWS, 'the inputs are at fault: the mean check reached {:d} points'.format(int(worst[5]))


def test_mlp_emulated():
    """The emulated feature route (Gram epilogue off for data batches: residual rows from the feature GEMM), 5 solved parameters, mask half."""
    from desilike_amd._lib import Context
    key = ('mlp', 'physical', 5)
    case = dbm.get_case(key)
    name, mask = dbm.gpu_patterns(case.n_s)[-1]
    like = case.likelihood(mask)
    like.initialize()
    spec = like._spec({}, [case.flatdata], like._precision_input)
    ctx, full = Context(spec, device=0), Context(like._spec({}, [case.flatdata], like._precision_input, vary_solved=True), device=0)
    rng = np.random.RandomState(4)
    filler = np.column_stack([np.clip(param.ref.sample(size=65, random_state=rng), *param.prior.limits) for param in like.varied_params])
    filler = case.theta[0] + (filler - case.theta[0]) / 20.      # (near the cases' rows: tests/marg_counts_cases.py::GramCase)
    worst = np.zeros(6)
    for M, B, size in [(33, 65, 3), (3, 3, 65)]:
        _check(ctx, full, lambda mock: with_data(spec, [case.n], mock), dbm.mocks(key), batch(case, B, filler), M, size, 5, (key, name, M, B, size), worst,
               _prior_precision(case.prior_scale))
    # index0 splits of one chain (one slab whatever B on this route): bit for bit
    assert ctx.set_data_batch(dbm.mocks(key)[:33], solved=True) == 33
    theta, index = batch(case, 65, filler), (np.arange(65) % 33).astype('i4')
    whole = ctx.sample_solved_data(theta, index, index0=9, size=2, seed=SEED)
    parts = [ctx.sample_solved_data(theta[lo:hi], index[lo:hi], index0=9 + lo, size=2, seed=SEED) for lo, hi in [(0, 20), (20, 65)]]
    assert (whole[3] == 0).sum() >= 33
    for w, a, b in zip(whole, *parts):
        assert np.array_equal(w, np.concatenate([a, b]), equal_nan=True)      # (filler rows that fail carry NaN in both)
    ctx.close(); full.close()
    _report('mlp-physical-ns5', worst)


def test_stacked_layout():
    """The benchmarked shape (stacked emulator layout, 5 marginalised parameters): identity against the reference-side keys with the solved parameters varied, and
    per-mock contexts; M = 3, B = 65, size = 2."""
    from desilike_amd._lib import Context
    import data_batch_utils as dbu
    import test_gpu_sample_solved as tss
    case = dbu.get_case('boundary_cfg3_stacked_bench')
    ctx, full = Context(case.spec, device=0), Context(tss._vary_solved_keys(case.spec), device=0)
    assert ctx.n_solved == 5
    n = case.flatdata.size
    covariance = np.linalg.inv(case.precision if case.precision.ndim == 2 else np.diag(case.precision))
    mocks = case.flatdata + np.random.RandomState(dbm.MOCK_SEED).multivariate_normal(np.zeros(n), covariance, size=3)
    theta = case.points(65)
    worst = np.zeros(6)
    _check(ctx, full, case.spec_with_data, mocks, theta, 3, 2, 100, 'stacked', worst, np.reshape(case.spec['marg.prior'], (-1, 2))[:, 1].astype('f8'))
    ctx.close(); full.close()
    _report('stacked layout', worst)


@functools.lru_cache(maxsize=None)
def _ctx57():
    """(context with a batch of 33, case, likelihood, filler rows) of case n57-ns5, mask all."""
    from desilike_amd._lib import Context
    key = (57, 5)
    case, (like, spec) = dbm.get_case(key), _residual_spec(key)
    ctx = Context(spec, device=0)
    ctx.set_data_batch(dbm.mocks(key)[:33], solved=True)
    rng = np.random.RandomState(8)
    filler = np.column_stack([np.clip(param.ref.sample(size=130, random_state=rng), *param.prior.limits) for param in like.varied_params])
    return ctx, case, like, filler


def _same(a, b, rows=slice(None), draws=slice(None)):
    return all(np.array_equal(p[rows][:, draws] if p.ndim > 1 else p[rows], q, equal_nan=True) for p, q in zip(a, b))


def test_bits():
    """The same (point, data vector, global index): across M, across B at an equal split-K count, draw d across ``size``, across index0 splits of one chain, in two calls
    in a row; two rows with the same point and data vector at different global indices differ."""
    from desilike_amd._lib import Context
    ctx, case, like, filler = _ctx57()
    key = (57, 5)
    R, N_pad, K_pad = 1 + case.n_var, ctx.info('N_pad'), ctx.info('K_pad')
    B = 65
    theta, index = batch(case, B, filler), (np.arange(B) % 33).astype('i4')
    whole = ctx.sample_solved_data(theta, index, index0=50, size=130, seed=SEED)
    assert (whole[3][:mc.NROWS] == 0).all() and (whole[3] == 0).sum() >= 33 and np.isfinite(whole[0][whole[3] == 0]).all()
    assert _same(whole, ctx.sample_solved_data(theta, index, index0=50, size=130, seed=SEED))
    for size in (1, 3, 64, 65):
        assert _same(whole[:3], ctx.sample_solved_data(theta, index, index0=50, size=size, seed=SEED)[:3], draws=slice(0, size)), size
    # across M: data vector 0 of a batch of 1 and of 33
    zero = np.zeros(B, dtype='i4')
    m33 = ctx.sample_solved_data(theta, zero, index0=50, size=3, seed=SEED)
    one = Context(_residual_spec(key)[1], device=0)
    one.set_data_batch(dbm.mocks(key)[:1], solved=True)
    assert _same(m33, one.sample_solved_data(theta, zero, index0=50, size=3, seed=SEED))
    one.close()
    # across B and across index0 splits, at an equal split count of the window GEMM
    splits = {b: tiled_splits(b * R, N_pad, K_pad) for b in range(1, B + 1)}
    equal = [b for b in (1, 3) if splits[b] == splits[B]]
    for b in equal:
        assert _same(whole, ctx.sample_solved_data(theta[:b], index[:b], index0=50, size=130, seed=SEED), rows=slice(0, b))
    cuts = [c for c in range(1, B) if splits[c] == splits[B - c] == splits[B]]
    print('\nbits: split counts B = 1, 3, 65: {}, {}, {}; compared across B: {}; index0 cuts with equal counts: {:d}'.format(splits[1], splits[3], splits[B], equal, len(cuts)))
    assert equal and cuts, 'the inputs are at fault: no batch / no cut of the chain has the split count of B = {:d} ({})'.format(B, splits[B])
    for c in cuts[:1] + cuts[-1:]:
        first, second = ctx.sample_solved_data(theta[:c], index[:c], index0=50, size=3, seed=SEED), ctx.sample_solved_data(theta[c:], index[c:], index0=50 + c, size=3, seed=SEED)
        assert all(np.array_equal(w[:, :3] if w.ndim > 1 else w, np.concatenate([a, b])) for w, a, b in zip(whole, first, second)), c
    # unequal counts: 1e-12 max(1, |.|) on the values (the rule of tests/test_gpu_data_batch_marg.py), draws to the solved-value tolerance
    for b in (1, 3):
        if b in equal: continue
        part = ctx.sample_solved_data(theta[:b], index[:b], index0=50, size=130, seed=SEED)
        assert np.allclose(part[0], whole[0][:b], rtol=1e-8, atol=1e-10) and (_rel(part[1], whole[1][:b]) <= 1e-12).all() and (_rel(part[2], whole[2][:b]) <= 1e-12).all()
    # the same point and data vector at two global indices: the same x^, other draws
    twice = ctx.sample_solved_data(np.ascontiguousarray(theta[[4, 4]]), np.array([2, 2], dtype='i4'), index0=0, size=3, seed=SEED)
    assert not np.isclose(twice[0][0], twice[0][1]).any() and not np.isclose(twice[1][0], twice[1][1]).any()


def test_status():
    """An index of -1 and of M, a NaN row, a row outside the prior: NaN outputs and the status; the rows beside them untouched.  The singular system: DL_STATUS_NONFINITE."""
    from desilike_amd._lib import Context
    ctx, case, like, filler = _ctx57()
    M = 33
    clean_index = (np.arange(mc.NROWS) % M).astype('i4')
    clean = ctx.sample_solved_data(case.theta, clean_index, index0=0, size=65, seed=SEED)
    assert (clean[3] == 0).all()
    theta, index = np.array(case.theta), clean_index.copy()
    theta[2, 1] = np.nan
    limits = like.varied_params[0].prior.limits
    assert np.isfinite(limits[1])
    theta[5, 0] = limits[1] + 1.
    index[0], index[7] = -1, M
    x, loglike, logprior, status = ctx.sample_solved_data(theta, index, index0=0, size=65, seed=SEED)
    assert status.tolist() == [DL_ST_NAN_INPUT, 0, DL_ST_NAN_INPUT, 0, 0, DL_ST_OUT_OF_PRIOR, 0, DL_ST_NAN_INPUT]
    good = [1, 3, 4, 6]
    for row in (0, 2, 5, 7):
        assert np.isnan(x[row]).all() and np.isnan(loglike[row]).all() and np.isnan(logprior[row]).all()
    assert np.array_equal(x[good], clean[0][good]) and np.array_equal(loglike[good], clean[1][good]) and np.array_equal(logprior[good], clean[2][good])
    slike = _singular_residual()
    slike.initialize()
    slike._get_context()
    sctx = Context(slike._context_specs[()], device=0)
    sctx.set_data_batch(_mvn_mocks(slike, slike.covariance, 3), solved=True)
    rng = np.random.RandomState(2)
    stheta = np.column_stack([np.clip(param.ref.sample(size=67, random_state=rng), *param.prior.limits) for param in slike.varied_params])
    x, loglike, logprior, status = sctx.sample_solved_data(stheta, (np.arange(67) % 3).astype('i4'), size=2)
    assert (status == DL_ST_NONFINITE).all() and np.isnan(x).all() and np.isnan(loglike).all() and np.isnan(logprior).all()
    sctx.close()


def test_refusals_through_the_c_abi():
    """No batch, a context without solved parameters, size = 0, index0 < 0, null pointers: 1 with a message, nothing written; B = 0: 0."""
    import torch
    from desilike_amd._lib import Context
    from golden_utils import load_golden, spec_from_golden
    ctx, case, like, filler = _ctx57()
    vp = ctypes.c_void_p
    B, ns = mc.NROWS, ctx.n_solved
    theta = torch.as_tensor(case.theta, dtype=torch.float64, device='cuda:0').contiguous()
    index = torch.zeros(B, dtype=torch.int32, device='cuda:0')
    out = torch.full((B, 1, ns), 7., dtype=torch.float64, device='cuda:0')

    def call(context, size=1, index0=0, th=theta, idx=index, o=out, nrows=B):
        rc = context._lib.dl_sample_solved_data(context._handle, None if th is None else vp(th.data_ptr()), nrows, None if idx is None else vp(idx.data_ptr()), index0, size, SEED,
                                                None if o is None else vp(o.data_ptr()), vp(out.data_ptr()), vp(out.data_ptr()), None, None)
        torch.cuda.synchronize()
        return rc, context._lib.dl_last_error(context._handle).decode()

    fresh = Context(_residual_spec((57, 5))[1], device=0)
    rc, message = call(fresh)
    assert rc == 1 and 'no data batch' in message
    fresh.close()
    g = load_golden('cfg2_shapefit_window')
    plain = Context(spec_from_golden(g), device=0)
    plain.set_data_batch(np.concatenate([np.ravel(obs['flatdata']) for obs in spec_from_golden(g)['observables']])[None, :])
    ptheta = torch.as_tensor(np.asarray(g['theta'], dtype='f8')[:B], dtype=torch.float64, device='cuda:0').contiguous()
    rc, message = call(plain, th=ptheta)
    assert rc == 1 and 'no analytically solved' in message
    plain.close()
    for kwargs, word in [(dict(size=0), 'size must be at least 1'), (dict(size=-3), 'size must be at least 1'), (dict(index0=-1), 'index0 must not be negative'),
                         (dict(idx=None), 'null data index or output'), (dict(o=None), 'null data index or output'), (dict(nrows=-1), 'invalid batch')]:
        rc, message = call(ctx, **kwargs)
        assert rc == 1 and word in message, (kwargs, rc, message)
    assert call(ctx, nrows=0)[0] == 0 and call(ctx, nrows=0, idx=None, o=None, th=None)[0] == 0
    assert (out.cpu().numpy() == 7.).all()
    assert call(ctx)[0] == 0 and np.isfinite(out.cpu().numpy()).all()


def test_existing_entry_points_keep_their_bits():
    """dl_eval_logposterior_data, dl_eval_solved_data, dl_sample_solved (and dl_eval_logposterior, dl_eval_batch_derived) before and after dl_sample_solved_data calls on the
    same context: shared workspaces, the same bits."""
    ctx, case, like, filler = _ctx57()
    theta, index = batch(case, 65, filler), (np.arange(65) % 33).astype('i4')

    def existing():
        out = list(ctx.eval_logposterior_data_host(theta)) + list(ctx.eval_logposterior_data_host(theta, index=index)) + list(ctx.eval_solved_data_host(theta, index))
        out += list(ctx.sample_solved(theta, index0=3, size=2, seed=7)) + list(ctx.eval_logposterior_host(theta)) + list(ctx.eval_batch_derived_host(theta))
        return out

    before = existing()
    draws = ctx.sample_solved_data(theta, index, index0=3, size=65, seed=7)
    ctx.sample_solved_data(theta[:3], index[:3], index0=0, size=1, seed=1)
    after = existing()
    assert len(before) == len(after) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
    assert _same(draws, ctx.sample_solved_data(theta, index, index0=3, size=65, seed=7))
    # the Python layer: DataBatch.sample_solved is the context's call
    from desilike_amd.likelihoods.base import DataBatch
    dbatch = DataBatch.__new__(DataBatch)
    dbatch.likelihood, dbatch.flatdata, dbatch.offset, dbatch.context, dbatch.solve = like, dbm.mocks((57, 5))[:33], 0., ctx, 'point'
    assert _same(draws, dbatch.sample_solved(theta, index.astype('i8'), index0=3, size=65, seed=7))


def test_end_to_end():
    """MockEmceeSampler on a solve='point' batch (3 mocks x 2 chains, 14 walkers), then .sample_solved(size=2): shapes and the full-posterior identity on 32 sampled rows
    per mock; the same sampler on a solve='constant' batch with data_batch= a 'point' batch; examples/sample_mocks_solved.py."""
    import desilike_amd
    from desilike_amd import MockEmceeSampler, Samples
    from golden_utils import load_golden
    import test_gpu_sample_solved as tss
    from test_gpu_data_batch import _marg_likelihood
    like = tss._eft_likelihood()
    like.initialize()
    mocks = _mvn_mocks(like, load_golden('cfg2_shapefit_window_dense')['covariance'], 3)
    dbatch = like.data_batch(mocks, solve='point')
    sampler = MockEmceeSampler(dbatch, nwalkers=14, chains=2, seed=6)
    sampler.run(5)
    new = sampler.sample_solved(size=2, seed=SEED, burnin=1)
    full = tss._full_context(like)
    full.set_data_batch(mocks + dbatch.shift)
    names = like.varied_params.names() + like.solved_params.names()
    worst = 0.
    for i in range(3):
        for k in range(2):
            chain = new[i][k]
            assert isinstance(chain, Samples)
            for name in names + ['loglikelihood', 'logprior', 'logposterior']: assert chain[name].shape == (4, 28), name
            assert np.array_equal(chain[names[0]], np.repeat(sampler.chains[i][k][names[0]][1:], 2, axis=1))
        points = np.concatenate([np.column_stack([np.ravel(new[i][k][name]) for name in names]) for k in range(2)])
        got = np.concatenate([np.ravel(new[i][k]['logposterior']) for k in range(2)])
        rows = np.linspace(0, len(got) - 1, 32).astype(int)
        ref = full.eval_logposterior_data_host(points[rows], index=np.full(32, i, dtype='i4'))[0]
        assert np.isfinite(ref).all()
        worst = max(worst, _rel(got[rows], ref).max())
    print('\nend to end: max |sample_solved - full posterior| / max(1, |.|) = {:.3e} on 32 rows per mock'.format(worst))
    assert worst <= 1e-10
    # the function on the flattened chains is the method
    flat = desilike_amd.sample_solved(dbatch, [{name: value[1:] for name, value in chain.items()} for row in sampler.chains for chain in row], size=2, seed=SEED,
                                      index=np.repeat(np.arange(3), 2))
    assert all(np.array_equal(flat[2 * i + k][name], new[i][k][name]) for i in range(3) for k in range(2) for name in new[i][k])
    full.close()
    # a sampler on a 'constant' batch, the draws from a 'point' batch over the same data
    g, clike = _marg_likelihood()
    clike.initialize()
    cmocks = _mvn_mocks(clike, g['covariance'], 3)
    constant, point = clike.data_batch(cmocks), clike.data_batch(cmocks, solve='point')
    csampler = MockEmceeSampler(constant, nwalkers=14, chains=2, seed=2)
    assert constant.solve == 'constant' and point.solve == 'point'
    csampler.run(4)
    with pytest.raises(ValueError, match="solve='point'"):
        csampler.sample_solved()
    cnew = csampler.sample_solved(size=2, data_batch=point)
    solved = clike.solved_params.names()
    assert len(cnew) == 3 and len(cnew[0]) == 2 and all(cnew[i][k][name].shape == (4, 28) and np.isfinite(cnew[i][k][name]).all() for i in range(3) for k in range(2) for name in solved + ['logposterior'])
    # the example runs
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    out = subprocess.run([sys.executable, os.path.join(root, 'examples', 'sample_mocks_solved.py'), '3'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'sn0' in out.stdout
