"""Sample every mock: one affine-invariant ensemble per data vector of a :class:`~desilike_amd.likelihoods.base.DataBatch`, all resident on one GPU and advancing
in lockstep (``dl_ensemble_data_*``, csrc/dl_ensemble_data.hip).

The per-mock route -- one likelihood and one :class:`~desilike_amd.samplers.EmceeSampler` per mock, run one after another -- gives the evaluation a handful of rows per
launch (half an ensemble of a few dozen walkers).  Here every half-step of ALL ensembles is one step kernel and one paired data-batch evaluation of
``E * nwalkers / 2`` rows.  Ensemble e draws from its own Philox key what a single ``dl_ensemble`` with that key draws, so its chain is the chain of
:class:`~desilike_amd.samplers.EnsembleStretchMove` with ``CounterRNG(key_e)`` on the posterior given its mock; :class:`_HostMockEnsembles` is that statement in NumPy
and the reference the device is compared against, bit for bit (tests/test_gpu_mock_ensemble.py)."""
import numpy as np

from .parameter import Samples
from .samplers import BasePosteriorSampler, CounterRNG, _chain_file_names


# ---- argument checks (no device call) ----------------------------------------------------------------------------------------------------------------------------
def default_nwalkers(ndim):
    """:class:`~desilike_amd.samplers.EmceeSampler`'s rule (samplers/emcee.py:66)."""
    return 2 * max((int(2.5 * ndim) + 1) // 2, 2)


def check_nwalkers(nwalkers, ndim):
    nwalkers = int(nwalkers)
    if nwalkers % 2 or nwalkers < 2 * ndim:
        raise ValueError('nwalkers must be even and at least 2 * ndim = {:d}, found {:d}'.format(2 * ndim, nwalkers))
    return nwalkers


def check_mocks(mocks, size):
    """``mocks`` (default: all) as integers in ``[0, size)``; repeats and any order are allowed."""
    if mocks is None: return np.arange(size, dtype='i4')
    mocks = np.atleast_1d(np.asarray(mocks))
    if mocks.ndim != 1 or not mocks.size or not np.issubdtype(mocks.dtype, np.integer):
        raise ValueError('mocks must be a list of integers, found {!r}'.format(mocks))
    if mocks.min() < 0 or mocks.max() >= size:
        raise ValueError('mocks must lie in [0, {:d}), found {}'.format(size, mocks.tolist()))
    return mocks.astype('i4')


def check_counter_seeds(counter_seeds, nmocks, nchains):
    """``counter_seeds [nmocks, nchains]`` as Python integers (64-bit keys), or ``None``."""
    if counter_seeds is None: return None
    seeds = np.asarray(counter_seeds, dtype=object)
    if nchains == 1 and seeds.shape == (nmocks,): seeds = seeds[:, None]
    if seeds.shape != (nmocks, nchains):
        raise ValueError('provide one counter seed per mock and chain: shape {}, found {}'.format((nmocks, nchains), seeds.shape))
    return [[int(seed) & 0xFFFFFFFFFFFFFFFF for seed in row] for row in seeds]


def check_gelman_rubin(nchains):
    if nchains < 2:
        raise ValueError('Gelman-Rubin compares the chains of a mock: run with chains >= 2')


# ---- engines ---------------------------------------------------------------------------------------------------------------------------------------------------
class _HostMockEnsembles(object):
    """``E`` ensembles of ``nwalkers`` walkers in NumPy, ensemble e on ``f(values, index_e)`` with ``CounterRNG(keys[e])``, advanced in lockstep: every half-step of
    all ensembles is ONE call ``f(values [E * half, ndim], index [E * half])``, rows ``e * half .. (e + 1) * half - 1`` those of ensemble e -- the batch the device
    presents to the paired data-batch evaluation.  The arithmetic of an ensemble is :meth:`~desilike_amd.samplers.EnsembleStretchMove.step`'s, operation by operation."""
    device_resident = False

    def __init__(self, f, index, keys, nwalkers, ndim, a=2.):
        self.f, self.index = f, np.asarray(index, dtype='i4').ravel()
        self.n_ensembles, self.nwalkers, self.ndim, self.a = self.index.size, check_nwalkers(nwalkers, ndim), int(ndim), float(a)
        keys = [int(key) & 0xFFFFFFFFFFFFFFFF for key in np.ravel(np.asarray(keys, dtype=object))]
        if len(keys) != self.n_ensembles: raise ValueError('provide one key per ensemble')
        self.rngs = [CounterRNG(key) for key in keys]
        self.index_half = np.repeat(self.index, self.nwalkers // 2)
        self.coords = self.logp = None
        self.iteration, self.naccepted = 0, np.zeros((self.n_ensembles, self.nwalkers), dtype='i8')

    def logposterior(self, values, index):
        out = np.array(self.f(values, index), dtype='f8')
        out[np.isnan(out)] = -np.inf      # NaN results count as -inf (samplers/base.py:187-189)
        return out

    def set_state(self, coords, logp=None, iteration=0, naccepted=None):
        shape = (self.n_ensembles, self.nwalkers, self.ndim)
        self.coords = np.array(coords, dtype='f8').reshape(shape)
        if logp is None: logp = self.logposterior(self.coords.reshape(-1, self.ndim), np.repeat(self.index, self.nwalkers))
        self.logp = np.array(logp, dtype='f8').reshape(shape[:2])
        self.iteration = int(iteration)
        self.naccepted = np.zeros(shape[:2], dtype='i8') if naccepted is None else np.array(naccepted, dtype='i8').reshape(shape[:2])

    def get_state(self):
        return self.coords.copy(), self.logp.copy(), self.naccepted.copy()

    def step(self):
        E, half = self.n_ensembles, self.nwalkers // 2
        perms = [rng.permutation(self.iteration, self.nwalkers) for rng in self.rngs]
        for ihalf in range(2):
            firsts, zzs, proposals = [], [], np.empty((E, half, self.ndim), dtype='f8')
            for e, (rng, perm) in enumerate(zip(self.rngs, perms)):
                first, second = (perm[:half], perm[half:]) if ihalf == 0 else (perm[half:], perm[:half])
                uz, partner = rng.move(self.iteration, ihalf, half)
                zz = ((self.a - 1.) * uz + 1.)**2 / self.a          # g(z) ~ 1 / sqrt(z) on [1 / a, a]
                partners = self.coords[e][second][partner]
                proposals[e] = partners - (partners - self.coords[e][first]) * zz[:, None]
                firsts.append(first); zzs.append(zz)
            new_log_prob = self.logposterior(proposals.reshape(E * half, self.ndim), self.index_half).reshape(E, half)
            for e, rng in enumerate(self.rngs):
                first, zz = firsts[e], zzs[e]
                with np.errstate(invalid='ignore', divide='ignore'):
                    lnpdiff = ((self.ndim - 1.) * np.log(zz) + new_log_prob[e]) - self.logp[e][first]
                    accepted = np.log(rng.accept(self.iteration, ihalf, half)) < lnpdiff
                idx = first[accepted]
                self.coords[e][idx], self.logp[e][idx] = proposals[e][accepted], new_log_prob[e][accepted]
                self.naccepted[e][idx] += 1
        self.iteration += 1

    def run(self, niterations, thin_by=1):
        """``niterations`` recorded updates (``niterations * thin_by`` updates): (coords [niterations, E, nwalkers, ndim], logposterior [niterations, E, nwalkers])."""
        coords, logp = [], []
        for it in range(niterations * thin_by):
            self.step()
            if (it + 1) % thin_by == 0:
                coords.append(self.coords.copy()); logp.append(self.logp.copy())
        shape = (niterations, self.n_ensembles, self.nwalkers, self.ndim)
        return np.array(coords, dtype='f8').reshape(shape), np.array(logp, dtype='f8').reshape(shape[:3])


class _DeviceMockEnsembles(object):
    """The same surface on :class:`~desilike_amd._lib.DeviceEnsembleData`: the ensembles live on the GPU, a run is enqueued whole and drained once."""
    device_resident = True

    def __init__(self, data_batch, index, keys, nwalkers, a=2.):
        from ._lib import DeviceEnsembleData
        self.ens = DeviceEnsembleData(data_batch.context, index, keys, nwalkers, a=a, offset=data_batch.offset)
        self.n_ensembles, self.nwalkers, self.ndim = self.ens.n_ensembles, self.ens.nwalkers, self.ens.n_params

    def set_state(self, coords, logp=None, iteration=0, naccepted=None):
        shape = (self.n_ensembles, self.nwalkers, self.ndim)
        self.ens.set_state(np.reshape(coords, shape), None if logp is None else np.reshape(logp, shape[:2]))
        self.ens.set_counter(iteration, naccepted=naccepted)

    def get_state(self):
        return self.ens.get_state()

    def run(self, niterations, thin_by=1):
        import torch
        device = torch.device('cuda', self.ens.device)
        shape = (niterations, self.n_ensembles, self.nwalkers, self.ndim)
        coords, logp = torch.empty(shape, dtype=torch.float64, device=device), torch.empty(shape[:3], dtype=torch.float64, device=device)
        self.ens.run(niterations * thin_by, thin_by=thin_by, chain=coords, chain_logp=logp)
        return coords.cpu().numpy(), logp.cpu().numpy()      # (the copies synchronise)

    @property
    def iteration(self):
        return self.ens.info('iteration')

    @property
    def naccepted(self):
        return self.ens.get_state()[2]


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------------------------------
class MockEmceeSampler(BasePosteriorSampler):
    """One posterior per mock: ``chains`` independent ensembles of ``nwalkers`` walkers for each selected data vector of ``data_batch``
    (``likelihood.data_batch(data)``, ``solve='constant'`` or ``'point'``), E = len(mocks) * chains ensembles advancing in lockstep on the batch's own context.

    ``mocks``: the data vectors to sample (default: all; repeats allowed).  ``counter_seeds [len(mocks), chains]``: the 64-bit key of every ensemble (default: drawn
    from the host generator seeded by ``seed``, as :class:`~desilike_amd.samplers.EmceeSampler` draws its chains' keys); an ensemble's chain depends on its key, its
    start and its mock only -- not on the other ensembles, nor on their order.  ``device_resident=False``: the NumPy engine, evaluated by ``data_batch.logposterior``.

    After :meth:`run`: ``chains[i][k]`` (dict name -> [niterations, nwalkers], ``'logposterior'`` included) of chain k of ``mocks[i]``, ``acceptance_fraction``
    [len(mocks), chains, nwalkers], :meth:`to_samples`, :meth:`gelman_rubin`, :meth:`save`.  All ensembles live on one GPU: more than one rank in the process group
    raises ``NotImplementedError``.  Resuming from files is not built."""
    name = 'mock_emcee'

    def __init__(self, data_batch, nwalkers=None, chains=1, mocks=None, a=2., seed=None, counter_seeds=None, device_resident=True, **kwargs):
        super(MockEmceeSampler, self).__init__(data_batch.likelihood, seed=seed, **kwargs)
        if self.sharding.active and self.sharding.world > 1:
            raise NotImplementedError('MockEmceeSampler keeps all ensembles of a data batch on one GPU: run one sampler per rank on its share of the mocks')
        self.data_batch = data_batch
        ndim = len(self.varied_params)
        self.nwalkers = check_nwalkers(default_nwalkers(ndim) if nwalkers is None else nwalkers, ndim)
        self.nchains = int(chains)
        if self.nchains < 1: raise ValueError('chains must be >= 1')
        self.mocks = check_mocks(mocks, data_batch.size)
        self.a = float(a)
        if not self.a > 1.: raise ValueError('stretch parameter a must be > 1')
        self.counter_seeds = check_counter_seeds(counter_seeds, len(self.mocks), self.nchains)
        self.device_resident = bool(device_resident)
        self.index = np.repeat(self.mocks, self.nchains)      # ensemble e = i * chains + k samples mock mocks[i]
        self._engine = None
        self._records = []           # per run: (coords [n, E, nwalkers, ndim], logposterior [n, E, nwalkers])
        self._iterations = 0
        self._accepted = np.zeros((len(self.index), self.nwalkers), dtype='i8')

    @property
    def n_ensembles(self):
        return len(self.index)

    def _draw_keys(self):
        if self.counter_seeds is None:
            draw = lambda: int(self.rng.randint(0, 2**32, dtype=np.uint64))      # noqa: E731
            self.counter_seeds = [[draw() | (draw() << 32) for _ in range(self.nchains)] for _ in self.mocks]
        return [key for row in self.counter_seeds for key in row]

    def logposterior(self, values, index=None):
        """Rows of ``values`` given data vector ``index[b]`` (NaN -> -inf), through the data batch."""
        out = np.array(self.data_batch.logposterior(values, index), dtype='f8')
        out[np.isnan(out)] = -np.inf
        return out

    def _get_engine(self):
        if self._engine is None:
            keys = self._draw_keys()
            if self.device_resident: self._engine = _DeviceMockEnsembles(self.data_batch, self.index, keys, self.nwalkers, a=self.a)
            else: self._engine = _HostMockEnsembles(self.data_batch.logposterior, self.index, keys, self.nwalkers, len(self.varied_params), a=self.a)
        return self._engine

    def _get_start(self, index):
        """One starting point per entry of ``index`` from the parameters' ``ref`` distributions, redrawn until its log-posterior given its own mock is finite
        (:meth:`BasePosteriorSampler._get_start` with a data vector per row)."""
        size = len(index)
        start, logposterior = np.full((size, len(self.varied_params)), np.nan), np.full(size, -np.inf)
        for _ in range(self.max_tries):
            mask = ~np.isfinite(logposterior)
            if not mask.any(): break
            for iparam, param in enumerate(self.varied_params):
                if param.ref.is_proper():
                    draw = param.ref.sample(size=int(mask.sum()), random_state=self.rng)
                    if self.ref_scale != 1.: draw = param.value + self.ref_scale * (draw - param.value)
                else:
                    draw = np.full(int(mask.sum()), param.value)
                start[mask, iparam] = draw
            logposterior[mask] = self.logposterior(start[mask], index[mask])
        if not np.isfinite(logposterior).all():
            raise ValueError('Could not find finite log posterior after {:d} tries'.format(self.max_tries))
        return start, logposterior

    def _starts(self, start):
        shape = (len(self.mocks), self.nchains, self.nwalkers, len(self.varied_params))
        index = np.repeat(self.index, self.nwalkers)
        if start is None:
            return self._get_start(index)
        start = np.array(start, dtype='f8')
        if start.shape != shape: raise ValueError('Provide start with shape {}, found {}'.format(shape, start.shape))
        start = start.reshape(-1, shape[-1])
        logposterior = self.logposterior(start, index)
        bad = ~np.isfinite(logposterior)
        if bad.any():      # a start row without a finite log-posterior given its own mock is drawn again
            start[bad], logposterior[bad] = self._get_start(index[bad])
        return start, logposterior

    def run(self, niterations=300, thin_by=1, start=None):
        """``niterations`` recorded updates of every ensemble (one in ``thin_by`` updates is kept).  ``start [len(mocks), chains, nwalkers, ndim]``: where to start
        (default at the first call: drawn from the parameters' ``ref`` distributions; later calls continue from the state of the ensembles).  Returns ``chains``."""
        engine = self._get_engine()
        if start is not None or not self._records:
            coords, logp = self._starts(start)
            engine.set_state(coords, logp, iteration=self._iterations, naccepted=self._accepted)
        coords, logp = engine.run(int(niterations), thin_by=int(thin_by))
        self._records.append((coords, logp))
        self._iterations, self._accepted = int(engine.iteration), np.array(engine.naccepted, dtype='i8')
        return self.chains

    # ---- results -------------------------------------------------------------------------------------------------------------------------------------------
    def _arrays(self):
        """(coords [n, len(mocks), chains, nwalkers, ndim], logposterior [n, len(mocks), chains, nwalkers]) of all runs so far."""
        if not self._records: raise ValueError('no samples yet: call run')
        if len(self._records) > 1:
            self._records = [(np.concatenate([rec[0] for rec in self._records]), np.concatenate([rec[1] for rec in self._records]))]
        coords, logp = self._records[0]
        shape = (coords.shape[0], len(self.mocks), self.nchains, self.nwalkers)
        return coords.reshape(shape + (coords.shape[-1],)), logp.reshape(shape)

    @property
    def chains(self):
        """``chains[i][k]``: dict name -> [niterations, nwalkers] (``'logposterior'`` included) of chain k of mock ``mocks[i]``."""
        coords, logp = self._arrays()
        out = []
        for i in range(len(self.mocks)):
            row = []
            for k in range(self.nchains):
                chain = {param.name: coords[:, i, k, :, iparam] for iparam, param in enumerate(self.varied_params)}
                chain['logposterior'] = logp[:, i, k]
                row.append(chain)
            out.append(row)
        return out

    @property
    def acceptance_fraction(self):
        """Accepted fraction per walker ``[len(mocks), chains, nwalkers]``."""
        return (self._accepted / max(self._iterations, 1)).reshape(len(self.mocks), self.nchains, self.nwalkers)

    def to_samples(self, i, burnin=0):
        """The samples of mock ``mocks[i]`` pooled over its chains and walkers, without the first ``burnin`` recorded updates: name -> [n] (``'logposterior'`` included)."""
        coords, logp = self._arrays()
        coords, logp = coords[int(burnin):, i], logp[int(burnin):, i]
        samples = Samples(coords.reshape(-1, coords.shape[-1]).T, params=self.varied_params)
        samples['logposterior'] = logp.ravel()
        return samples

    def sample_solved(self, size=1, seed=42, burnin=0, data_batch=None):
        """Posterior draws of the analytically solved parameters at every chain point, each chain against its own mock (:func:`desilike_amd.sample_solved` with a
        data batch): a nested list shaped like ``chains`` of :class:`Samples` ``[niterations - burnin, nwalkers * size]`` -- every column repeated ``size`` times along
        the last axis, the solved parameters as columns, ``loglikelihood`` / ``logprior`` / ``logposterior`` with nothing marginalised.  All chains are flattened into
        one point list with a data index per point, in the order i, k, then the chain's own flattening -- that order is the global point index of the draws -- and
        treated in chunked calls, not one call per mock.  ``data_batch``: a ``solve='point'`` batch over the same data, for a sampler that ran on a
        ``solve='constant'`` batch (default: the sampler's own batch, which must then be a ``'point'`` one)."""
        from .solved import check_point_batch, sample_solved_chains
        size, burnin = int(size), int(burnin)
        if size < 1:
            raise ValueError('sample_solved: size must be at least 1, found {:d}'.format(size))
        if data_batch is None:
            data_batch = self.data_batch
        elif data_batch.size != self.data_batch.size or data_batch.likelihood is not self.data_batch.likelihood:
            raise ValueError('sample_solved: data_batch must hold the {:d} data vectors of the likelihood this sampler ran on'.format(self.data_batch.size))
        check_point_batch(data_batch)
        flat = [{name: value[burnin:] for name, value in chain.items()} for row in self.chains for chain in row]
        new = sample_solved_chains(data_batch, flat, self.index, size=size, seed=seed)
        return [[Samples(new[i * self.nchains + k]) for k in range(self.nchains)] for i in range(len(self.mocks))]

    def gelman_rubin(self, burnin=0):
        """``[len(mocks)]``: max eigenvalue of the Gelman-Rubin statistic - 1 across the chains of every mock (:func:`desilike_amd.diagnostics.gelman_rubin`)."""
        from . import diagnostics
        check_gelman_rubin(self.nchains)
        coords = self._arrays()[0][int(burnin):]
        return np.array([diagnostics.gelman_rubin([coords[:, i, k] for k in range(self.nchains)], method='eigen', check_valid='ignore').max() - 1. for i in range(len(self.mocks))])

    def save(self, save_fn):
        """One chain file per (mock, chain) in the format of :meth:`EmceeSampler.save`: ``save_fn`` a template with ``*`` (replaced by ``i * chains + k``) or a list of
        ``len(mocks) * chains`` names."""
        names = _chain_file_names(save_fn, self.n_ensembles, distinct=True)
        chains, keys = self.chains, self._draw_keys()
        files = []
        for e, name in enumerate(names):
            i, k = divmod(e, self.nchains)
            attrs = {'sampler': self.name, 'nwalkers': self.nwalkers, 'a': self.a, 'iteration': int(self._iterations), 'naccepted': self._accepted[e].tolist(),
                     'counter_seed': int(keys[e]), 'mock': int(self.mocks[i]), 'chain': int(k)}
            files.append((name, chains[i][k], attrs))
        self._write_chains(files)
        return names
