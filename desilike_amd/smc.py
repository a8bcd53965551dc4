"""Tempered sequential Monte Carlo with log-evidence on systems of particles (adaptive tempering after Del Moral, Doucet & Jasra 2006: the skeleton of the PocoMC
the reference wraps in desilike/samplers/pocomc.py, with ``precondition=False, sample='rwm'``; its normalising flows, t-preconditioned Crank-Nicolson and persistent
reweighting are third-party arithmetic and are not reproduced).

A system is N particles drawn from the PRIOR at inverse temperature beta = 0.  An iteration chooses the next beta by bisection on the effective sample size, adds to
logZ, resamples systematically and mutates with ``n_steps`` random-walk Metropolis sweeps -- each sweep ONE likelihood batch over all particles of all systems
(csrc/dl_smc.h states the algorithm, the order of the sums and the random draws).  At beta = 1 a system keeps sweeping: its particles are the posterior sample.

* :class:`_DeviceSMC` runs the systems on the GPU (``dl_smc_*``);
* :class:`_HostSMC` is the NumPy statement of the same stage machine, with the same counter-based draws, around an injected
  ``(loglike, logprior) = f(x [B, P])``: likelihoods without a device context, and the yardstick of the device engine in the tests.  It also records the MARGIN of
  every discrete decision (``|log u - log ratio|`` of a Metropolis test, the relative distance of ``(i + u) / N`` to the nearest prefix sum of an ancestor search): two
  runs whose arithmetic differs by less than the smallest margin take the same decisions."""
import numpy as np

from .mclmc import _matvec
from .nuts import _Draws
from .samplers import CounterRNG, _DeviceEngine, _EvidenceSampler, _HostEvidenceEngine, _expression, _open_chain_files, _run_chunks

STREAM_PROPOSE, STREAM_ACCEPT, STREAM_RESAMPLE = 50, 51, 52
HISTORY_FIELDS = ('beta', 'logz', 'ess', 'acceptance', 'scale')
MAX_PARTICLES, MAX_STEPS, PIVOT = 16384, 1024, 1e-10


class _SmcDraws(_Draws):
    """The draws of csrc/dl_smc.h: Philox4x32-10 keyed by ``seed``, counter (iteration, sweep, system id, stream word)."""

    def _slots(self, it, sweep, system, words):
        words = np.asarray(words, dtype=np.uint32)
        return self._words(np.full(len(words), int(it) | (int(sweep) << 32), dtype='i8'), np.full(len(words), system), words)

    def gauss(self, it, sweep, system, N, P):
        """Standard Gaussians [N, P] of the proposals of sweep ``sweep`` (Box-Muller pairs)."""
        slots = np.arange(N, dtype=np.uint32) << np.uint32(16)
        z = np.empty((N, P + (P & 1)))
        for j in range((P + 1) // 2):
            z[:, 2 * j], z[:, 2 * j + 1] = CounterRNG.box_muller(self._slots(it, sweep, system, np.uint32(STREAM_PROPOSE | (j << 8)) | slots))
        return z[:, :P]

    def log_uniform(self, it, sweep, system, N):
        w = self._slots(it, sweep, system, np.uint32(STREAM_ACCEPT) | (np.arange(N, dtype=np.uint32) << np.uint32(16)))
        with np.errstate(divide='ignore'):
            return np.log(CounterRNG.uniform53(w[:, 0], w[:, 1]))

    def resample_uniform(self, it, system):
        w = self._slots(it, 0, system, [STREAM_RESAMPLE])
        return 1. - float(CounterRNG.uniform53(w[:, 0], w[:, 1])[0])


def _live(L):
    with np.errstate(invalid='ignore'):
        return np.abs(L) < np.inf


def temper(L, beta, ess_fraction):
    """Next level of a system at ``beta`` with log-likelihoods ``L`` [N] (dl_smc_temper): dict delta, lmax, sumw, ess, beta (the new one), dlogz."""
    L = np.asarray(L, dtype='f8')
    N, live = len(L), _live(L)
    out = dict(delta=0., lmax=-np.inf, sumw=float(N), ess=float(N), beta=float(beta), dlogz=0.)
    if not live.any() or not beta < 1.: return out
    lmax = out['lmax'] = float(L[live].max())
    d = np.where(live, L - np.where(live, lmax, 0.), 0.)

    def ess(delta):
        w = np.where(live, np.exp(delta * d), 0.)
        s1, s2 = w.sum(), (w * w).sum()
        return s1, (s1 * s1 / s2 if s2 > 0. else 0.)

    target = ess_fraction * N
    if not live.sum() > target: target = ess_fraction * live.sum()
    lo, hi = 0., 1. - beta
    delta = hi
    sumw, e = ess(hi)
    if e >= target: new = 1.
    else:
        for _ in range(64):
            mid = 0.5 * (lo + hi)
            if ess(mid)[1] > target: lo = mid
            else: hi = mid
        delta = 0.5 * (lo + hi)
        sumw, e = ess(delta)
        new = min(beta + delta, 1.)
    out.update(delta=delta, sumw=sumw, ess=e, beta=new, dlogz=np.log(sumw / N) + delta * lmax)
    return out


def weights(L, lmax, delta, sumw):
    live = _live(L)
    return np.where(live, np.exp(delta * np.where(live, L - lmax, 0.)), 0.) / sumw


def moments(x, W):
    """Mean and lower triangle of the covariance of the particles ``x`` [N, P] under the normalised weights ``W``, about the first particle (dl_smc_moment_partial)."""
    y = x - x[0]
    m = (W[:, None] * y).sum(axis=0)
    d = y - m
    return x[0] + m, np.tril((W[:, None] * d).T @ d)


def factor(cov, widths):
    """Lower Cholesky factor of ``cov`` (its lower triangle is read); a pivot that is not finite and above 1e-10 of its diagonal entry: the diagonal
    fallback (dl_smc_factor)."""
    P = len(cov)
    C = np.zeros((P, P))
    for j in range(P):
        v = cov[j:, j] - C[j:, :j] @ C[j, :j]
        if not PIVOT * cov[j, j] < v[0] < np.inf:
            diag = np.diag(cov)
            with np.errstate(invalid='ignore'):
                return np.diag(np.where((diag > 0.) & (diag < np.inf), np.sqrt(np.abs(diag)), widths))
        r = np.sqrt(v[0])
        C[j, j], C[j + 1:, j] = r, v[1:] / r
    return C


def prefix_sums(W, threads=1024, group=32):
    """Inclusive prefix sums of ``W`` in the order of dl_smc_resample_kernel: every thread its slice of ceil(N / threads) entries, one thread in ``group`` the totals
    of ``group`` threads, one thread the groups; additions only, each in the kernel's order: the same bits."""
    N = len(W)
    S = -(-N // threads)
    slices = np.cumsum(np.concatenate([W, np.zeros(threads * S - N)]).reshape(threads, S), axis=1)
    tot = np.cumsum(slices[:, -1].reshape(threads // group, group), axis=1)        # inclusive within a group
    gtot = np.concatenate([[0.], np.cumsum(tot[:, -1])[:-1]])                      # exclusive over the groups
    off = gtot[:, None] + np.concatenate([np.zeros((threads // group, 1)), tot[:, :-1]], axis=1)
    return (slices + off.reshape(threads, 1)).ravel()[:N]


def ancestors(W, u):
    """Systematic resampling: (ancestor of every slot, margin of every search) for the normalised weights ``W`` and the uniform ``u`` in (0, 1]."""
    N = len(W)
    cum = prefix_sums(W)
    t = np.minimum((np.arange(N) + u) / N, cum[-1])
    anc = np.searchsorted(cum, t, side='left')
    last = np.nonzero(W > 0.)[0][-1]       # beyond the last particle with weight nothing can be chosen: no decision above it
    upper = np.where(anc >= last, np.inf, np.abs(cum[anc] - t))
    lower = np.where(anc > 0, np.abs(t - cum[np.maximum(anc - 1, 0)]), np.inf)
    return anc, np.minimum(upper, lower) / t


def next_scale(s, a, target_acceptance):
    return float(np.clip(s * np.exp(a - target_acceptance), 1e-3, 1e3))


def _check_hyper(ess_fraction, n_steps, target_acceptance, scale):
    if not 0. < ess_fraction < 1.: raise ValueError('ess_fraction must lie in (0, 1), found {}'.format(ess_fraction))
    if not 1 <= n_steps <= MAX_STEPS: raise ValueError('n_steps must lie in 1 .. {:d}, found {}'.format(MAX_STEPS, n_steps))
    if not 0. < target_acceptance < 1.: raise ValueError('target_acceptance must lie in (0, 1), found {}'.format(target_acceptance))
    if not 1e-3 <= scale <= 1e3: raise ValueError('scale must lie in 1e-3 .. 1e3, found {}'.format(scale))


def _check_particles(nparticles):
    if nparticles % 64 or not 64 <= nparticles <= MAX_PARTICLES:
        raise ValueError('nparticles must be a multiple of 64 between 64 and {:d}, found {}'.format(MAX_PARTICLES, nparticles))


class _HostSMC(_HostEvidenceEngine):
    """NumPy statement of the device engine's stage machine (csrc/dl_smc.h, same records, same draws), around ``f(x [B, P]) -> (loglike [B], logprior [B])``."""
    _check_size = staticmethod(_check_particles)

    def __init__(self, f, nsystems, nparticles, n_params, widths, system_ids=None, seed=0, offset=0.):
        super(_HostSMC, self).__init__(f, nsystems, nparticles, n_params, widths, system_ids, offset, 'system')
        self.draws = _SmcDraws(seed)
        K, P = self.K, self.P
        self.beta, self.logz, self.scale, self.iter, self.chol = np.zeros(K), np.zeros(K), np.ones(K), np.zeros(K, dtype='i8'), np.zeros((K, P, P))

    # ---- set-up (dl_smc_set_hyper / set_particles / set_state / get_state / get_decisions) ----------------------------------------------------------------------------
    def set_hyper(self, ess_fraction, n_steps, target_acceptance, scale=1.):
        _check_hyper(ess_fraction, n_steps, target_acceptance, scale)
        self.ess_fraction, self.n_steps, self.target_acceptance = float(ess_fraction), int(n_steps), float(target_acceptance)
        self.scale[:] = scale

    def set_particles(self, coords):
        coords = np.array(coords, dtype='f8').reshape(self.K, self.N, self.P)
        if not np.all(np.isfinite(coords)): raise ValueError('the particles must be finite')
        L, pi = self._eval(coords)
        if not np.all(np.isfinite(pi)):
            k, i = np.argwhere(~np.isfinite(pi))[0]
            raise ValueError('particle {:d} of system {:d} lies outside the prior (its log-prior is not finite)'.format(i, k))
        L[~_live(L)] = -np.inf
        for k in range(self.K):
            if not _live(L[k]).any(): raise ValueError('no particle of system {:d} has a finite log-likelihood'.format(k))
        self.x, self.L, self.pi = coords, L, pi
        self.beta[:] = 0.; self.logz[:] = 0.; self.iter[:] = 0; self.chol[...] = 0.
        self.iterations = 0

    def set_state(self, coords, loglike, logprior, beta, logz, counters, scale, factor):
        K, N, P = self.K, self.N, self.P
        self.x, self.L, self.pi = np.array(coords, dtype='f8').reshape(K, N, P), np.array(loglike, dtype='f8').reshape(K, N), np.array(logprior, dtype='f8').reshape(K, N)
        self.beta, self.logz, self.scale = np.array(beta, dtype='f8').reshape(K), np.array(logz, dtype='f8').reshape(K), np.array(scale, dtype='f8').reshape(K)
        self.iter, self.chol = np.array(counters, dtype='i8').reshape(K), np.array(factor, dtype='f8').reshape(K, P, P)
        if not (np.all(self.beta >= 0.) and np.all(self.beta <= 1.)): raise ValueError('beta must lie in 0 .. 1')

    def get_state(self):
        return tuple(a.copy() for a in (self.x, self.L, self.pi, self.beta, self.logz, self.iter, self.scale, self.chol))

    # ---- an iteration -------------------------------------------------------------------------------------------------------------------------------------------
    def _iteration(self, rec):
        hist, coords, logp, count, quota = rec
        K, N, P, n = self.K, self.N, self.P, self.n_steps
        active = np.nonzero(count[:, 0] < quota)[0]
        beta0, ess = self.beta.copy(), np.full(K, float(N))
        anc = np.tile(np.arange(N), (K, 1))
        mean, cov = np.zeros((K, P)), np.zeros((K, P, P))
        if self._decisions is not None: mean, cov = self._decisions[2].copy(), self._decisions[3].copy()
        for k in active:
            level = temper(self.L[k], self.beta[k], self.ess_fraction)
            ess[k] = level['ess']
            if not level['delta'] > 0.: continue
            W = weights(self.L[k], level['lmax'], level['delta'], level['sumw'])
            self.beta[k] = level['beta']; self.logz[k] += level['dlogz']
            mean[k], cov[k] = moments(self.x[k], W)
            self.chol[k] = factor(cov[k], self.widths)
            anc[k], margins = ancestors(W, self.draws.resample_uniform(self.iter[k], self.ids[k]))
            self._margin(margins)
            self.x[k], self.L[k], self.pi[k] = self.x[k][anc[k]], self.L[k][anc[k]], self.pi[k][anc[k]]
        s, total = self.scale.copy(), np.zeros(K)
        flags = np.zeros((K, n, N), dtype=bool)
        for j in range(n):
            prop = self.x.copy()
            for k in active:
                z = self.draws.gauss(self.iter[k], j, self.ids[k], N, P)
                prop[k] = self.x[k] + (s[k] * (2.38 / np.sqrt(float(P)))) * _matvec(self.chol[k], z)
            Lp, pip = self._eval(prop)
            for k in active:
                logu = self.draws.log_uniform(self.iter[k], j, self.ids[k], N)
                ok = _live(Lp[k]) & _live(pip[k])
                with np.errstate(invalid='ignore'):
                    ratio = self.beta[k] * (np.where(ok, Lp[k], 0.) - self.L[k]) + (np.where(ok, pip[k], 0.) - self.pi[k])
                    accept = ok & (logu < ratio)
                    self._margin(np.abs(logu - ratio)[ok])
                self.x[k][accept], self.L[k][accept], self.pi[k][accept] = prop[k][accept], Lp[k][accept], pip[k][accept]
                flags[k, j] = accept
                total[k] += accept.sum()
                s[k] = next_scale(s[k], accept.sum() / N, self.target_acceptance)
        for k in active:
            hist[k, count[k, 0]] = self.beta[k], self.logz[k] + self.offset, ess[k], total[k] / (float(n) * N), s[k]
            if not beta0[k] < 1.:
                coords[k, count[k, 1]], logp[k, count[k, 1]] = self.x[k], self.L[k] + self.pi[k] + self.offset
                count[k, 1] += 1
            self.scale[k] = s[k]
            self.iter[k] += 1
            count[k, 0] += 1
        self._decisions = (anc, flags, mean, cov)

    # ---- a batch ------------------------------------------------------------------------------------------------------------------------------------------------
    def buffers(self, quota):
        K, N, P = self.K, self.N, self.P
        return (np.zeros((K, quota, 5)), np.zeros((K, quota, N, P)), np.zeros((K, quota, N)), np.zeros((K, 2), dtype='i8'))

    def run(self, niterations, quota, buffers):
        """``niterations`` iterations of every system into ``buffers`` (the semantics of dl_smc_run)."""
        if not self.n_steps: raise ValueError('no hyper-parameters (set_hyper)')
        for _ in range(int(niterations)): self._iteration(tuple(buffers) + (int(quota),))
        self.iterations += int(niterations)


class _DeviceSMC(_DeviceEngine):
    """Systems resident on the GPU (``dl_smc_*``): the calls of :class:`_HostSMC` go to the owner ``smc``."""
    _counters = ('iterations', 'evaluations')

    def __init__(self, ctx, offset, nsystems, nparticles, widths, system_ids=None, seed=0):
        from ._lib import DeviceSMC
        self.smc = self._owner = DeviceSMC(ctx, nsystems, nparticles, widths, system_ids=system_ids, seed=seed, offset=offset)
        self.K, self.N, self.P = int(nsystems), int(nparticles), self.smc.n_params


def run_batch(engine, niterations, chunk=None):
    """``niterations`` iterations of every system in chunks of at most ``chunk``: (history [K, n, 5], coords [K, n, N, P], logposterior [K, n, N], counts [K, 2]);
    rows of coords / logposterior beyond counts[k, 1] are not written."""
    buffers = _run_chunks(engine, niterations, chunk)
    return engine.records(buffers) + (engine.counts(buffers).copy(),)


class SMCSampler(_EvidenceSampler):
    """``SMCSampler(likelihood, nparticles=1024, chains=1, ess_fraction=0.5, n_steps='2 * ndim', target_acceptance=0.234, seed=None, save_fn=None, device_resident=None)``:
    adaptive tempered sequential Monte Carlo from the PRIOR to the posterior, with the Bayesian evidence.

    nparticles : particles of a system, a multiple of 64 between 64 and 16384.
    chains : number of independent systems (their scatter is the error of ``logz``), or the files written by :meth:`save` (one per system): the run is continued.
    ess_fraction : the effective sample size, as a fraction of ``nparticles``, that every temperature level keeps.
    n_steps : random-walk Metropolis sweeps per iteration (an expression of ``ndim`` or a number).
    target_acceptance : the acceptance fraction the proposal scale is steered to.

    Every varied parameter needs a PROPER prior: the particles start there.  All particles of a system live on one GPU: more than one rank in the process group raises
    ``NotImplementedError`` (run one sampler per rank with different seeds and pool their ``logz`` instead).

    After :meth:`run`: ``logz`` [chains] (the constant of a marginalised posterior context included), ``logz_mean`` = log of the mean of the unbiased estimates Z
    (logsumexp(logz) - log chains: not the mean of the logs), ``logz_std`` (the scatter of ``logz``; ``None`` for one system), ``history`` (dict of [chains, T] arrays:
    beta, logz, ess, acceptance, scale), ``nevaluations``, ``chains`` (per system name -> [sweeps, nparticles] with ``logposterior``: the layout of
    :class:`~desilike_amd.samplers.EmceeSampler`)."""
    name, _words = 'smc', ('SMCSampler', 'particles', 'system')

    def __init__(self, likelihood, nparticles=1024, chains=1, ess_fraction=0.5, n_steps='2 * ndim', target_acceptance=0.234, seed=None, save_fn=None, device_resident=None,
                 **kwargs):
        super(SMCSampler, self).__init__(likelihood, seed=seed, **kwargs)
        resume = self._setup(chains, seed, save_fn, device_resident)
        ndim, self.nparticles = len(self.varied_params), int(nparticles)
        _check_particles(self.nparticles)
        self.ess_fraction, self.n_steps, self.target_acceptance = float(ess_fraction), int(_expression(n_steps, ndim=ndim)), float(target_acceptance)
        _check_hyper(self.ess_fraction, self.n_steps, self.target_acceptance, 1.)
        self._history = np.zeros((self.nchains, 0, 5))
        self._coords = [np.zeros((0, self.nparticles, ndim)) for _ in range(self.nchains)]
        self._logp = [np.zeros((0, self.nparticles)) for _ in range(self.nchains)]
        if resume is not None: self._resume(resume)

    # ---- engine -------------------------------------------------------------------------------------------------------------------------------------------------
    def _make_engine(self):
        ids, ndim = np.arange(self.nchains), len(self.varied_params)
        if self.device_resident:
            ctx, offset = self.likelihood._get_posterior_context()
            engine = _DeviceSMC(ctx, offset, self.nchains, self.nparticles, self.widths, system_ids=ids, seed=self.counter_seed)
        else:
            engine = _HostSMC(self._host_terms, self.nchains, self.nparticles, ndim, self.widths, system_ids=ids, seed=self.counter_seed)
        engine.set_hyper(self.ess_fraction, self.n_steps, self.target_acceptance, 1.)
        if self._state is not None: engine.set_state(*self._state)
        else:
            start = np.empty((self.nchains, self.nparticles, ndim))
            for iparam, param in enumerate(self.varied_params):
                start[..., iparam] = param.prior.sample(size=(self.nchains, self.nparticles), random_state=self.rng)
            engine.set_particles(start)
            self._evaluations += engine.evaluations
        return engine

    def _advance(self, niterations):
        if self._engine is None: self._engine = self._make_engine()
        before = self._engine.evaluations
        history, coords, logp, counts = run_batch(self._engine, niterations)
        self._evaluations += self._engine.evaluations - before
        self._history = np.concatenate([self._history, history], axis=1)
        for k in range(self.nchains):
            self._coords[k] = np.concatenate([self._coords[k], coords[k, :counts[k, 1]]])
            self._logp[k] = np.concatenate([self._logp[k], logp[k, :counts[k, 1]]])
        self._state = self._engine.get_state()

    def run(self, min_iterations=0, max_iterations=10, check_every=None, check=None, max_levels=1000):
        """Climb to beta = 1 (one iteration at a time: the stop does not depend on any chunking), then sweep in batches of ``check_every`` until every system has
        recorded ``max_iterations`` sweeps at beta = 1 in all -- or, past ``min_iterations``, until ``check(sampler)`` returns True.  ``max_levels``: a climb that has not
        reached beta = 1 after that many iterations in all raises ``RuntimeError`` (a temperature step that underflows never ends).  Returns the list of chains."""
        max_iterations = int(max_iterations)
        if self._engine is None: self._engine = self._make_engine()
        self._state = self._engine.get_state()
        while np.any(self._state[3] < 1.):
            if self._history.shape[1] >= int(max_levels):
                raise RuntimeError('beta = 1 not reached after {:d} iterations (beta = {}): the temperature does not advance'.format(self._history.shape[1], self._state[3].tolist()))
            self._advance(1)
        while True:
            done = min(len(c) for c in self._coords)
            if done >= max_iterations or (check is not None and done >= min_iterations and check(self)): break
            self._advance(min(max_iterations - done, int(check_every) if check_every else max_iterations))
        if self.save_fn is not None: self.save()
        return self.chains

    # ---- outputs ------------------------------------------------------------------------------------------------------------------------------------------------
    @property
    def chains(self):
        """Per system: dict name -> [sweeps, nparticles] (incl. 'logposterior')."""
        out = []
        for coords, logp in zip(self._coords, self._logp):
            chain = {param.name: coords[..., iparam] for iparam, param in enumerate(self.varied_params)}
            chain['logposterior'] = logp
            out.append(chain)
        return out

    @property
    def history(self):
        return {name: self._history[..., i] for i, name in enumerate(HISTORY_FIELDS)}

    @property
    def nlevels(self):
        """Per system: temperature levels to beta = 1."""
        beta = self._history[..., 0]
        return np.array([int(np.argmax(b >= 1.)) + 1 if np.any(b >= 1.) else len(b) for b in beta])

    @property
    def logz(self):
        if not self._history.shape[1]: return np.full(self.nchains, np.nan)
        return self._history[:, -1, 1].copy()

    def save(self, fn=None):
        """One file per system in the reference's checkpoint format; attributes ``{'sampler': 'smc', 'seed', 'state', 'history', ...}``: the state continues the run."""
        fn = self._save_names(fn)
        if self._state is None: return
        self._write_chains((name, chain, {'sampler': self.name, 'seed': self.counter_seed, 'system': k, 'state': [np.asarray(a[k]) for a in self._state], 'history': self._history[k],
                                          'hyper': [self.ess_fraction, self.n_steps, self.target_acceptance], 'evaluations': self._evaluations})
                           for k, (chain, name) in enumerate(zip(self.chains, fn)))

    def _resume(self, sources):
        """Continue the systems saved by :meth:`save`: particles, temperatures, evidences, counters, scales, factors (and the records so far)."""
        files = _open_chain_files(sources)
        names = self.varied_params.names()
        for f in files:
            if f.attrs.get('sampler', None) != self.name or 'state' not in f.attrs: raise ValueError('not a chain file of SMCSampler')
        self._state = tuple(np.array([np.asarray(f.attrs['state'][i]) for f in files]) for i in range(8))
        if self._state[0].shape[1:] != (self.nparticles, len(names)): raise ValueError('the saved systems have {:d} particles'.format(self._state[0].shape[1]))
        self._history = np.array([np.asarray(f.attrs['history'], dtype='f8').reshape(-1, 5) for f in files])
        self._coords = [np.stack([np.asarray(f.arrays[name], dtype='f8') for name in names], axis=-1).reshape(-1, self.nparticles, len(names)) for f in files]
        self._logp = [np.asarray(f.arrays['logposterior'], dtype='f8').reshape(-1, self.nparticles) for f in files]
        self.counter_seed = int(files[0].attrs['seed'])
        self.ess_fraction, self.n_steps, self.target_acceptance = float(files[0].attrs['hyper'][0]), int(files[0].attrs['hyper'][1]), float(files[0].attrs['hyper'][2])
        self._evaluations = int(files[0].attrs.get('evaluations', 0))
