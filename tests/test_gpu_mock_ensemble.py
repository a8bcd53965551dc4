"""GPU (-m gpu): many device-resident ensembles, one per data vector of a data batch (``dl_ensemble_data_*``, ``MockEmceeSampler``) against the NumPy engine
``_HostMockEnsembles`` on the same ``DataBatch`` -- coordinates, log-posteriors and accepted counts with ``np.array_equal`` -- and against the routes that existed before:
``DataBatch.logposterior`` re-evaluated and a per-mock likelihood's ``EmceeSampler.logposterior``."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'examples'))
from test_host_api import make_cfg2   # noqa: E402
from test_gpu_sampler import make_cfg5   # noqa: E402

pytestmark = pytest.mark.gpu


def _tol(ref):
    """tests/test_gpu_data_batch.py's bound against other arithmetic of the same value."""
    return 1e-10 * np.maximum(1., np.abs(ref))


def _mocks(like, M, seed=5):
    """``flatdata + 0.05 |flatdata| z``, z seeded standard normal (data_batch_utils.Case.mocks)."""
    like.initialize()
    flatdata = np.concatenate(like._flatdata_list())
    return flatdata + 0.05 * np.abs(flatdata) * np.random.RandomState(seed).standard_normal((M, flatdata.size))


@functools.lru_cache(maxsize=None)
def _cfg2_batch():
    like = make_cfg2()[1]
    mocks = _mocks(like, 6)
    return like, mocks, like.data_batch(mocks)


def _pair(batch, **kwargs):
    """The device-resident sampler and the host one with the same keys and the same start."""
    from desilike_amd import MockEmceeSampler
    return MockEmceeSampler(batch, **kwargs), MockEmceeSampler(batch, device_resident=False, **kwargs)


def _same(dev, host):
    (dc, dl), (hc, hl) = dev._arrays(), host._arrays()
    assert dc.shape == hc.shape and dl.shape == hl.shape
    assert np.array_equal(dc, hc), 'coordinates differ from update {}'.format(np.argwhere((dc != hc).any(axis=(1, 2, 3, 4))).ravel()[:3])
    assert np.array_equal(dl, hl)
    assert np.array_equal(dev._accepted, host._accepted) and dev._iterations == host._iterations
    assert dev._accepted.sum() > 0 and np.isfinite(dl).all()


@pytest.mark.parametrize('mocks,chains,nwalkers,niterations,thin_by', [
    ([3], 1, 14, 8, 1),                              # the smallest legal ensemble; 7 proposals per half-step
    ([0, 1, 5], 1, 18, 6, 1),                        # 9 proposals per half-step (cfg2 varies 6 parameters: the odd count of doubles per block is test_marginalised_constant_offset's)
    ([1, 4, 2], 1, 18, 3, 2),                        # ... thinned
    ([4, 0, 4, 2, 2], 1, 22, 6, 1),                  # repeats, unsorted, data vectors 1, 3, 5 unused
    ([2, 5], 2, 14, 6, 1),                           # two chains per mock
    (list(np.arange(70) % 6), 1, 14, 4, 1)])         # more ensembles than lanes in a wavefront; 490 rows per half-step
def test_shapes_against_host_engine(mocks, chains, nwalkers, niterations, thin_by):
    like, _, batch = _cfg2_batch()
    dev, host = _pair(batch, nwalkers=nwalkers, chains=chains, mocks=mocks, seed=11)
    dev.run(niterations, thin_by=thin_by); host.run(niterations, thin_by=thin_by)
    assert dev._engine.device_resident and not host._engine.device_resident
    _same(dev, host)
    chains_ = dev.chains
    assert len(chains_) == len(mocks) and len(chains_[0]) == chains and chains_[0][0]['logposterior'].shape == (niterations, nwalkers)
    assert dev.acceptance_fraction.shape == (len(mocks), chains, nwalkers)
    assert dev._iterations == niterations * thin_by


def test_two_tracers():
    """cfg5, E = 4, 30 walkers: 15 proposals per ensemble and half-step."""
    like = make_cfg5()[1]
    batch = like.data_batch(_mocks(like, 3))
    dev, host = _pair(batch, nwalkers=30, mocks=[2, 0, 1, 0], seed=4)
    dev.run(6); host.run(6)
    _same(dev, host)


def test_independence_of_the_other_ensembles():
    """The same mocks in two orders with the same key and start per mock: every mock's chain is the same bits."""
    from desilike_amd import MockEmceeSampler
    like, _, batch = _cfg2_batch()
    nwalkers, ndim = 18, len(like.varied_params)
    keys = {0: 101, 1: (7 << 33) + 3, 2: 0xABCDEF0123456789}
    first = MockEmceeSampler(batch, nwalkers=nwalkers, mocks=[0, 1, 2], counter_seeds=[[keys[m]] for m in [0, 1, 2]], seed=2)
    first.run(6)
    start = first._arrays()[0][0]                      # [3, 1, nwalkers, ndim]: the ensembles after one update, a start with finite log-posteriors
    order = [2, 0, 1]
    a = MockEmceeSampler(batch, nwalkers=nwalkers, mocks=[0, 1, 2], counter_seeds=[[keys[m]] for m in [0, 1, 2]])
    b = MockEmceeSampler(batch, nwalkers=nwalkers, mocks=order, counter_seeds=[[keys[m]] for m in order])
    a.run(6, start=start); b.run(6, start=start[order])
    (ac, al), (bc, bl) = a._arrays(), b._arrays()
    assert ac.shape == (6, 3, 1, nwalkers, ndim)
    for position, m in enumerate(order):
        assert np.array_equal(bc[:, position], ac[:, m]) and np.array_equal(bl[:, position], al[:, m])
        assert np.array_equal(b.acceptance_fraction[position], a.acceptance_fraction[m])
    assert not np.array_equal(ac[:, 0], ac[:, 1])


def test_continuation_and_state_round_trip():
    from desilike_amd import MockEmceeSampler
    from desilike_amd._lib import DeviceEnsembleData
    import torch
    like, _, batch = _cfg2_batch()
    kw = dict(nwalkers=18, mocks=[5, 1, 1], seed=8)
    whole, parts = MockEmceeSampler(batch, **kw), MockEmceeSampler(batch, **kw)
    whole.run(8)
    parts.run(4)
    state = parts._engine.get_state()
    parts.run(4)
    assert np.array_equal(whole._arrays()[0], parts._arrays()[0]) and np.array_equal(whole._arrays()[1], parts._arrays()[1])
    assert np.array_equal(whole._accepted, parts._accepted) and parts._iterations == 8
    # the state after 4 updates into a fresh handle
    fresh = DeviceEnsembleData(batch.context, parts.index, parts._draw_keys(), 18, offset=batch.offset)
    fresh.set_state(state[0], state[1])
    fresh.set_counter(4, naccepted=state[2])
    coords = torch.empty((4, 3, 18, fresh.n_params), dtype=torch.float64, device='cuda:0')
    logp = torch.empty((4, 3, 18), dtype=torch.float64, device='cuda:0')
    fresh.run(4, chain=coords, chain_logp=logp)
    final = fresh.get_state()
    assert np.array_equal(coords.cpu().numpy(), whole._records[0][0][4:]) and np.array_equal(logp.cpu().numpy(), whole._records[0][1][4:])
    assert np.array_equal(final[2], whole._accepted) and np.array_equal(final[0], whole._records[0][0][-1]) and fresh.info('iteration') == 8
    # a start given without log-posteriors is evaluated on the device, every walker against its ensemble's data vector
    other = DeviceEnsembleData(batch.context, parts.index, parts._draw_keys(), 18, offset=batch.offset)
    other.set_state(state[0])
    other.run(0)
    err = np.abs(other.get_state()[1] - state[1]) / _tol(state[1])
    assert (err <= 1.).all(), err.max()
    fresh.close(); other.close()


def _reevaluated(sampler, batch):
    """Worst |recorded log-posterior - DataBatch.logposterior(point, index)| in units of the bound (the batch sizes differ: E nwalkers / 2 rows against all records)."""
    coords, logp = sampler._arrays()
    index = np.broadcast_to(sampler.mocks[None, :, None, None], logp.shape)
    again = batch.logposterior(coords.reshape(-1, coords.shape[-1]), index.ravel())
    err = np.abs(again - logp.ravel()) / _tol(again)
    assert np.isfinite(again).all()
    return err.max()


def test_marginalised_constant_offset():
    """solve='constant' on the likelihood of test_likelihood_data_batch_marginalised: the marginalised-precision context and a non-zero offset."""
    from test_gpu_data_batch import _marg_likelihood, _marg_mocks
    g, like = _marg_likelihood()
    like.initialize()
    batch = like.data_batch(_marg_mocks(like, 4))
    assert batch.offset != 0. and batch.context.n_solved == 0
    # 5 varied parameters x 7 proposals: an odd count of doubles per proposal block -- the blocks of ensembles 1 and 3 start 8 bytes off the 16-byte chunks of the staging
    assert len(like.varied_params) == 5
    dev, host = _pair(batch, nwalkers=14, mocks=[3, 0, 2, 0], seed=5)
    dev.run(6); host.run(6)
    _same(dev, host)
    worst = _reevaluated(dev, batch)
    print('\nsolve=constant: worst |chain - data_batch.logposterior| = {:.2e} of the bound'.format(worst))
    assert worst <= 1.


def test_marginalised_per_point():
    """solve='point' on the likelihood of tests/test_gpu_data_batch_marg.py (two counter terms '.marg', sn0_2 '.best'): solved per point and per mock by the paired call."""
    from golden_utils import load_golden
    import test_gpu_sample_solved as tss
    from test_gpu_data_batch_marg import _mvn_mocks
    like = tss._eft_likelihood()
    like.initialize()
    batch = like.data_batch(_mvn_mocks(like, load_golden('cfg2_shapefit_window_dense')['covariance'], 3), solve='point')
    assert batch.context.n_solved == 3 and batch.offset == 0.
    dev, host = _pair(batch, mocks=[1, 2, 0], seed=6)
    dev.run(6); host.run(6)
    _same(dev, host)
    worst = _reevaluated(dev, batch)
    print('\nsolve=point: worst |chain - data_batch.logposterior| = {:.2e} of the bound'.format(worst))
    assert worst <= 1.


def test_against_per_mock_likelihood():
    """The route of before: a likelihood with mock m as its own data, through EmceeSampler.logposterior (direct differences against the chi2 GEMM)."""
    from desilike_amd import MockEmceeSampler
    from desilike_amd.samplers import EmceeSampler
    like, mocks, batch = _cfg2_batch()
    m = 4
    sampler = MockEmceeSampler(batch, nwalkers=18, mocks=[1, m], seed=9)
    sampler.run(6)
    coords, logp = sampler._arrays()
    ref = EmceeSampler(make_cfg2(data=mocks[m])[1], nwalkers=18).logposterior(coords[:, 1].reshape(-1, coords.shape[-1]))
    err = np.abs(logp[:, 1].ravel() - ref) / _tol(ref)
    print('\nper-mock likelihood: worst difference {:.2e} of the bound, |logposterior| up to {:.1f}'.format(err.max(), np.abs(ref).max()))
    assert np.isfinite(ref).all() and (err <= 1.).all(), err.max()


def test_priors_hold():
    """A wide start: many proposals land outside the priors; every recorded point is inside its prior box with a finite log-posterior."""
    like, _, batch = _cfg2_batch()
    from desilike_amd import MockEmceeSampler
    sampler = MockEmceeSampler(batch, nwalkers=18, mocks=[0, 3, 5], seed=3, ref_scale=4.)
    sampler.run(30)
    for row in sampler.chains:
        for chain in row:
            assert np.isfinite(chain['logposterior']).all()
            for param in like.varied_params:
                lo, hi = param.prior.limits
                assert (chain[param.name] >= lo).all() and (chain[param.name] <= hi).all()
    assert 0.1 < sampler.acceptance_fraction.mean() < 0.9, sampler.acceptance_fraction.mean()
    samples = sampler.to_samples(1, burnin=10)
    assert samples['logposterior'].shape == (20 * 18,) and set(samples) == set(like.varied_params.names()) | {'logposterior'}


def test_refusals_of_the_c_abi(tmp_path):
    """dl_ensemble_data_create returns 1 with a message and a null handle (every refusal comes before the first device call of the function)."""
    from desilike_amd import _lib, MockEmceeSampler
    like, mocks, batch = _cfg2_batch()
    lib = _lib.load()
    ctx = batch.context
    M, P = ctx.n_data_batch, ctx.n_params
    assert M == 6

    def create(context, index, nwalkers, a=2.):
        index = np.ascontiguousarray(index, dtype='i4')
        seeds = np.arange(1, index.size + 1, dtype=np.uint64)
        handle = ctypes.c_void_p()
        rc = lib.dl_ensemble_data_create(ctypes.byref(handle), context._handle, index.size, index.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                         seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), nwalkers, a, 0.)
        return rc, handle, lib.dl_last_error(None).decode()

    plain = like._get_posterior_context()[0]
    assert plain.n_data_batch == 0
    nwalkers_big = 2000
    assert (3 * nwalkers_big * P // 2 + nwalkers_big) * 8 > 144 * 1024 and nwalkers_big <= 8192
    for context, index, nwalkers, a, word in [(plain, [0], 14, 2., 'no data batch'), (ctx, [0, M], 14, 2., 'outside'), (ctx, [0, -1], 14, 2., 'outside'), (ctx, [0], 15, 2., 'even'),
                                             (ctx, [0], 0, 2., 'even'), (ctx, [0], 14, 1., 'a must be'), (ctx, [0], nwalkers_big, 2., 'LDS')]:
        rc, handle, message = create(context, index, nwalkers, a)
        assert rc == 1 and not handle.value and word in message, (rc, handle.value, message)
    with pytest.raises(_lib.LibraryError, match='LDS'):
        _lib.DeviceEnsembleData(ctx, [0], [1], nwalkers_big)
    rc, handle, message = create(ctx, [0, M - 1], 14)
    assert rc == 0 and handle.value, message
    lib.dl_ensemble_data_destroy(handle)
    # a batch replaced by a shorter one: the ensembles' indices no longer fit, the run refuses
    own = like.data_batch(mocks)
    sampler = MockEmceeSampler(own, nwalkers=14, mocks=[5], seed=1)
    sampler.run(2)
    own.context.set_data_batch(mocks[:3] + own.shift)
    with pytest.raises(_lib.LibraryError, match='create the ensembles again'):
        sampler._engine.ens.run(1)
    # files: one per (mock, chain)
    two = MockEmceeSampler(batch, nwalkers=14, chains=2, mocks=[2, 0], seed=1)
    two.run(12)
    names = two.save(str(tmp_path / 'mock_*.npy'))
    from desilike_amd.io import ChainFile
    assert len(names) == 4 and all(os.path.isfile(name) for name in names)
    loaded = ChainFile.load(names[3])
    assert loaded.attrs['mock'] == 0 and loaded.attrs['chain'] == 1 and np.array_equal(np.asarray(loaded.arrays['logposterior']), two.chains[1][1]['logposterior'])
    assert two.gelman_rubin(burnin=2).shape == (2,)


def test_sample_mocks_example():
    import sample_mocks
    out = sample_mocks.main(nmocks=4, niterations=200)
    truth = np.array([out['truth'][name] for name in out['names']])
    assert out['mean'].shape == (4, len(truth)) and np.isfinite(out['mean']).all() and (out['std'] > 0.).all()
    assert out['gelman_rubin'].shape == (4,) and np.isfinite(out['gelman_rubin']).all()
    assert 0.1 < out['sampler'].acceptance_fraction.mean() < 0.9
