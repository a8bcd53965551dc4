"""CPU (-m "not gpu"): the NumPy engine of MockEmceeSampler (``_HostMockEnsembles``: E ensembles in lockstep, one batched call per half-step) against one
``EnsembleStretchMove`` with ``CounterRNG(key_e)`` per ensemble, and the argument checks of MockEmceeSampler that run before any device call."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_host_engine_is_one_stretch_move_per_ensemble():
    """Toy Gaussians: ensemble e on centre mu[index[e]], index [2, 0, 2] over 3 centres; chains, log-probabilities and accepted counts bit for bit those of the single
    ensembles; every half-step is ONE call of E * nwalkers / 2 rows, rows e * half .. (e + 1) * half - 1 those of ensemble e."""
    from desilike_amd.mock_sampler import _HostMockEnsembles
    from desilike_amd.samplers import EnsembleStretchMove, CounterRNG
    E, ndim, nwalkers, niterations = 3, 3, 8, 6
    mu = np.array([[0., 1., 2.], [-3., 0.5, 4.], [2.5, -1., 0.]])
    index, keys = [2, 0, 2], [11, (1 << 40) + 5, 0xFEDCBA9876543210]
    calls = []

    def f(values, idx):
        calls.append((values.shape, np.array(idx)))
        return -0.5 * ((values - mu[idx])**2).sum(axis=-1)

    start = mu[index][:, None, :] + np.random.RandomState(3).standard_normal((E, nwalkers, ndim))
    engine = _HostMockEnsembles(f, index, keys, nwalkers, ndim)
    engine.set_state(start)
    assert calls[0][0] == (E * nwalkers, ndim) and np.array_equal(calls[0][1], np.repeat(index, nwalkers))
    coords, logp = engine.run(niterations)
    assert coords.shape == (niterations, E, nwalkers, ndim) and logp.shape == (niterations, E, nwalkers)
    assert len(calls) == 1 + 2 * niterations
    for shape, idx in calls[1:]:
        assert shape == (E * nwalkers // 2, ndim) and np.array_equal(idx, np.repeat(index, nwalkers // 2))
    assert engine.iteration == niterations
    for e in range(E):
        single = EnsembleStretchMove(nwalkers, ndim, lambda values, e=e: -0.5 * ((values - mu[index[e]])**2).sum(axis=-1), rng=CounterRNG(keys[e]))
        x, lp = start[e].copy(), -0.5 * ((start[e] - mu[index[e]])**2).sum(axis=-1)
        for it in range(niterations):
            x, lp = single.step(x, lp)
            assert np.array_equal(x, coords[it, e]) and np.array_equal(lp, logp[it, e]), (e, it)
        assert np.array_equal(single.naccepted, engine.naccepted[e]) and single.naccepted.sum() > 0
    # the two ensembles on centre 2 are different chains (their keys differ)
    assert not np.array_equal(coords[-1, 0] - start[0], coords[-1, 2] - start[2])


def test_host_engine_thinning_and_continuation():
    from desilike_amd.mock_sampler import _HostMockEnsembles
    mu = np.array([[0., 1.], [3., -1.]])
    f = lambda values, idx: -0.5 * ((values - mu[idx])**2).sum(axis=-1)      # noqa: E731
    start = np.random.RandomState(1).standard_normal((2, 6, 2))
    a, b = _HostMockEnsembles(f, [1, 0], [5, 6], 6, 2), _HostMockEnsembles(f, [1, 0], [5, 6], 6, 2)
    a.set_state(start); b.set_state(start)
    ca, la = a.run(8)
    cb, lb = b.run(2, thin_by=2)
    cb2, lb2 = b.run(2, thin_by=2)
    assert np.array_equal(ca[1::2], np.concatenate([cb, cb2])) and np.array_equal(la[1::2], np.concatenate([lb, lb2]))
    # a fresh engine given (state, counters) continues the chain
    c = _HostMockEnsembles(f, [1, 0], [5, 6], 6, 2)
    c.set_state(ca[3], la[3], iteration=4, naccepted=None)
    assert np.array_equal(c.run(4)[0], ca[4:])
    # NaN log-probabilities count as -inf: such proposals are never accepted
    d = _HostMockEnsembles(lambda values, idx: np.where(values[:, 0] > 0.5, np.nan, f(values, idx)), [1, 0], [5, 6], 6, 2)
    d.set_state(np.minimum(start, 0.4))
    assert (d.run(6)[0][..., 0] <= 0.5).all()


def test_argument_checks_functions():
    from desilike_amd import mock_sampler as ms
    assert ms.default_nwalkers(7) == 18 and ms.default_nwalkers(1) == 4
    assert ms.check_nwalkers(14, 7) == 14
    for nwalkers in [15, 12, 0]:      # odd; < 2 * ndim
        with pytest.raises(ValueError, match='nwalkers'):
            ms.check_nwalkers(nwalkers, 7)
    assert np.array_equal(ms.check_mocks(None, 4), [0, 1, 2, 3]) and np.array_equal(ms.check_mocks([3, 0, 3], 4), [3, 0, 3])
    for mocks in [[0, 4], [-1], [], [0.5]]:
        with pytest.raises(ValueError, match='mocks'):
            ms.check_mocks(mocks, 4)
    assert ms.check_counter_seeds(None, 2, 3) is None
    assert ms.check_counter_seeds([[1, 2, 3], [4, 5, (1 << 64) + 7]], 2, 3) == [[1, 2, 3], [4, 5, 7]]
    assert ms.check_counter_seeds([1, 2], 2, 1) == [[1], [2]]
    for seeds in [[1, 2, 3], [[1, 2], [3, 4]], [[1, 2, 3]]]:
        with pytest.raises(ValueError, match='counter seed'):
            ms.check_counter_seeds(seeds, 2, 3)
    # keys below and above 2^63 in one list keep every bit on their way to the device
    from desilike_amd._lib import _seeds
    keys = [5, (1 << 63) + 12345, (1 << 40) + 3]
    assert _seeds(keys).dtype == np.uint64 and [int(key) for key in _seeds(keys)] == keys and [int(key) for key in _seeds(np.array(keys, dtype=np.uint64))] == keys
    ms.check_gelman_rubin(2)
    with pytest.raises(ValueError, match='chains >= 2'):
        ms.check_gelman_rubin(1)


def test_argument_checks_of_the_sampler():
    """The constructor makes no device call: a stand-in for the DataBatch (likelihood, size, offset; no context) is enough to reach every refusal."""
    from test_host_api import make_cfg2
    from desilike_amd import MockEmceeSampler
    g, like = make_cfg2()
    ndim = len(like.varied_params)
    batch = types.SimpleNamespace(likelihood=like, size=6, offset=0., context=None)
    sampler = MockEmceeSampler(batch, chains=2, mocks=[4, 0, 4], seed=1)
    assert sampler.nwalkers == 2 * max((int(2.5 * ndim) + 1) // 2, 2) and sampler.n_ensembles == 6 and np.array_equal(sampler.index, [4, 4, 0, 0, 4, 4])
    keys = sampler._draw_keys()
    assert len(set(keys)) == 6 and keys == MockEmceeSampler(batch, chains=2, mocks=[4, 0, 4], seed=1)._draw_keys()
    with pytest.raises(ValueError, match='nwalkers'):
        MockEmceeSampler(batch, nwalkers=2 * ndim + 1)
    with pytest.raises(ValueError, match='nwalkers'):
        MockEmceeSampler(batch, nwalkers=2 * ndim - 2)
    with pytest.raises(ValueError, match='mocks'):
        MockEmceeSampler(batch, mocks=[0, 6])
    with pytest.raises(ValueError, match='counter seed'):
        MockEmceeSampler(batch, chains=2, mocks=[0, 1, 2], counter_seeds=[[1, 2], [3, 4]])
    with pytest.raises(ValueError, match='a must be'):
        MockEmceeSampler(batch, a=1.)
    with pytest.raises(ValueError, match='chains >= 2'):
        MockEmceeSampler(batch, chains=1).gelman_rubin()
    with pytest.raises(ValueError, match='no samples yet'):
        sampler.chains
