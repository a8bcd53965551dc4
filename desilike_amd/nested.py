"""Batched nested sampling with log-evidence on runs of live points (Skilling 2006; what the reference's samplers/dynesty.py, polychord.py and nautilus.py are used
for -- those wrap third-party codes whose arithmetic, ellipsoids, slices and networks are not reproduced).

A run is N live points drawn from the PRIOR.  An iteration ranks them, lets the ``ndelete`` lowest die with the weights of a shrinking prior volume, adds them to logZ,
reseeds their slots from survivors and mutates those slots with ``n_steps`` random-walk Metropolis sweeps in the prior under the hard constraint L > L* -- each sweep
ONE likelihood batch over the replaced points of all runs (csrc/dl_nested.h states the algorithm, the order of the sums and the random draws).  A run rests when the
evidence left in its live points is below ``dlogz`` of the total; the live points then close the sum at weight X / N each.

* :class:`_DeviceNested` runs the runs on the GPU (``dl_nested_*``);
* :class:`_HostNested` is the NumPy statement of the same stage machine, with the same counter-based draws, around an injected
  ``(loglike, logprior) = f(x [B, P])``: likelihoods without a device context, and the yardstick of the device engine in the tests.  It also records the MARGIN of
  every discrete decision (``|log u - (pi' - pi)|`` of a Metropolis test, ``|L' - L*| / |L*|`` of a constraint, the distance of ``u (N - M)`` to the nearest integer of
  a seed): two runs whose arithmetic differs by less than the smallest margin take the same decisions."""
import numpy as np

from .mclmc import _matvec
from .nuts import _Draws
from .samplers import CounterRNG, _DeviceEngine, _EvidenceSampler, _HostEvidenceEngine, _expression, _open_chain_files, _run_chunks
from .smc import factor, moments, next_scale, prefix_sums

STREAM_PROPOSE, STREAM_ACCEPT, STREAM_SEED = 64, 65, 66
HISTORY_FIELDS = ('logx', 'logz', 'lstar', 'acceptance', 'scale', 'logz_remaining')
MAX_LIVE, MAX_STEPS = 8192, 1024
REST, CLIMB = 0, 1


class _NestedDraws(_Draws):
    """The draws of csrc/dl_nested.h: Philox4x32-10 keyed by ``seed``, counter (iteration, sweep, run id, stream word)."""

    def _slots(self, it, sweep, run, words):
        words = np.asarray(words, dtype=np.uint32)
        return self._words(np.full(len(words), int(it) | (int(sweep) << 32), dtype='i8'), np.full(len(words), run), words)

    def gauss(self, it, sweep, run, M, P):
        """Standard Gaussians [M, P] of the proposals of sweep ``sweep`` (Box-Muller pairs)."""
        ranks = np.arange(M, dtype=np.uint32) << np.uint32(16)
        z = np.empty((M, P + (P & 1)))
        for j in range((P + 1) // 2):
            z[:, 2 * j], z[:, 2 * j + 1] = CounterRNG.box_muller(self._slots(it, sweep, run, np.uint32(STREAM_PROPOSE | (j << 8)) | ranks))
        return z[:, :P]

    def log_uniform(self, it, sweep, run, M):
        w = self._slots(it, sweep, run, np.uint32(STREAM_ACCEPT) | (np.arange(M, dtype=np.uint32) << np.uint32(16)))
        with np.errstate(divide='ignore'):
            return np.log(CounterRNG.uniform53(w[:, 0], w[:, 1]))

    def seed_uniform(self, it, run, M):
        w = self._slots(it, 0, run, np.uint32(STREAM_SEED) | (np.arange(M, dtype=np.uint32) << np.uint32(16)))
        return CounterRNG.uniform53(w[:, 0], w[:, 1])


def ranks(L):
    """Slot of every rank: the live points ordered by (L, slot) ascending (dl_nested_rank_kernel)."""
    L = np.asarray(L, dtype='f8') + 0.
    return np.lexsort((np.arange(len(L)), L))


def shrinkage(N, M):
    """(c [M], log(-expm1(-1 / (N - j))) [M]): the inclusive prefix sums of 1 / (N - j) in the order of the kernel's scan, and the log width of every shell relative to
    the volume it starts from."""
    t = 1. / (N - np.arange(M)).astype('f8')
    return prefix_sums(t), np.log(-np.expm1(-t))


def evidence(Ldead, N, logx, logz):
    """The evidence update of one iteration from the dead points' log-likelihoods in rank order (dl_nested_evidence): (log w [M], new log X, new log Z)."""
    M = len(Ldead)
    cum, width = shrinkage(N, M)
    prev = np.concatenate([[0.], cum[:-1]])
    lstar = Ldead[-1]
    term = (lstar + logx) + np.log(np.sum(np.exp((Ldead - lstar) + (width - prev))))
    return (logx - prev) + width, logx - cum[-1], float(np.logaddexp(logz, term))


def survivor_moments(x, dead):
    """Mean and lower triangle of the covariance of the survivors with equal weights, about the first survivor in slot order."""
    N = len(x)
    W = np.full(N, 1. / (N - len(dead)))
    W[dead] = 0.
    first = int(np.argmax(W > 0.))
    return moments(x[first:], W[first:])


def seed_ranks(u, N, M):
    """(rank of the survivor that seeds every dead point, the distance of u (N - M) to the nearest integer)."""
    t = u * float(N - M)
    return M + np.minimum(t.astype('i8'), N - M - 1), np.abs(t - np.rint(t))


def remaining(L, logx):
    """log Z_rem = log X + log mean exp(L) over the live points."""
    top = np.max(L)
    return (logx + top) + np.log(np.sum(np.exp(L - top)) / len(L))


def at_rest(logz, logz_remaining, dlogz):
    return bool(logz_remaining - np.logaddexp(logz, logz_remaining) < np.log(dlogz))


def closing(dead_loglike, dead_logweight, live_loglike, logx):
    """The whole weighted path of one run, the dead points then the live points at weight X / N each (the code both engines share): dict of ``logweight`` [n] (log prior
    volumes: they sum to 1), ``loglike`` [n], ``logz``, ``aweight`` [n] (normalised posterior weights), ``information`` H = sum p L - log Z and ``logz_err`` =
    sqrt(H / N)."""
    live_loglike = np.asarray(live_loglike, dtype='f8')
    N = len(live_loglike)
    logw = np.concatenate([np.asarray(dead_logweight, dtype='f8').ravel(), np.full(N, logx - np.log(N))])
    L = np.concatenate([np.asarray(dead_loglike, dtype='f8').ravel(), live_loglike])
    lp = logw + L
    top = lp.max()
    logz = top + np.log(np.sum(np.exp(lp - top)))
    p = np.exp(lp - logz)
    H = float(np.sum(p * L) - logz)
    return dict(logweight=logw, loglike=L, logz=float(logz), aweight=p / p.sum(), information=H, logz_err=float(np.sqrt(max(H, 0.) / N)))


def _check_hyper(nlive, ndelete, n_steps, target_acceptance, dlogz, scale):
    if not 1 <= ndelete <= nlive // 2: raise ValueError('ndelete must lie in 1 .. nlive / 2 = {:d}, found {}'.format(nlive // 2, ndelete))
    if not 1 <= n_steps <= MAX_STEPS: raise ValueError('n_steps must lie in 1 .. {:d}, found {}'.format(MAX_STEPS, n_steps))
    if not 0. < target_acceptance < 1.: raise ValueError('target_acceptance must lie in (0, 1), found {}'.format(target_acceptance))
    if not 0. < dlogz < 1.: raise ValueError('dlogz must lie in (0, 1), found {}'.format(dlogz))
    if not 1e-3 <= scale <= 1e3: raise ValueError('scale must lie in 1e-3 .. 1e3, found {}'.format(scale))


def _check_live(nlive):
    if nlive % 64 or not 64 <= nlive <= MAX_LIVE:
        raise ValueError('nlive must be a multiple of 64 between 64 and {:d}, found {}'.format(MAX_LIVE, nlive))


class _HostNested(_HostEvidenceEngine):
    """NumPy statement of the device engine's stage machine (csrc/dl_nested.h, same records, same draws), around ``f(x [B, P]) -> (loglike [B], logprior [B])``."""
    _check_size, _counts, _nrecords = staticmethod(_check_live), 5, 5

    def __init__(self, f, nruns, nlive, n_params, widths, run_ids=None, seed=0, offset=0.):
        super(_HostNested, self).__init__(f, nruns, nlive, n_params, widths, run_ids, offset, 'run')
        self.draws = _NestedDraws(seed)
        K = self.K
        self.logx, self.logz, self.scale, self.iter, self.mode = np.zeros(K), np.full(K, -np.inf), np.ones(K), np.zeros(K, dtype='i8'), np.full(K, CLIMB, dtype='i4')
        self.M, self._have_state = 0, False

    # ---- set-up (dl_nested_set_hyper / set_live / set_state / get_state / get_decisions) ---------------------------------------------------------------------------
    def set_hyper(self, ndelete, n_steps, target_acceptance, dlogz, scale=1.):
        _check_hyper(self.N, ndelete, n_steps, target_acceptance, dlogz, scale)
        self.M, self.n_steps, self.target_acceptance, self.dlogz = int(ndelete), int(n_steps), float(target_acceptance), float(dlogz)
        self.scale[:] = scale

    def terms(self, x):
        """(loglike, logprior) of rows x [B, P], -inf where there is no likelihood (not counted as evaluations of the runs)."""
        L, pi = self.f(np.ascontiguousarray(x))
        return np.array(L, dtype='f8'), np.array(pi, dtype='f8')

    @staticmethod
    def _check_terms(L, pi):
        if not np.all(np.isfinite(pi)):
            k, i = np.argwhere(~np.isfinite(pi))[0]
            raise ValueError('live point {:d} of run {:d} lies outside the prior (its log-prior is not finite)'.format(i, k))
        if not np.all(np.isfinite(L)):
            k, i = np.argwhere(~np.isfinite(L))[0]
            raise ValueError('live point {:d} of run {:d} has no finite log-likelihood'.format(i, k))

    def set_live(self, coords):
        coords = np.array(coords, dtype='f8').reshape(self.K, self.N, self.P)
        if not np.all(np.isfinite(coords)): raise ValueError('the live points must be finite')
        L, pi = self._eval(coords)
        self._check_terms(L, pi)
        self.x, self.L, self.pi = coords, L, pi
        self.logx[:] = 0.; self.logz[:] = -np.inf; self.iter[:] = 0; self.mode[:] = CLIMB
        self.iterations, self._have_state = 0, True

    def set_state(self, coords, loglike, logprior, logx, logz, counters, scale, modes):
        K, N, P = self.K, self.N, self.P
        x, L, pi = np.array(coords, dtype='f8').reshape(K, N, P), np.array(loglike, dtype='f8').reshape(K, N), np.array(logprior, dtype='f8').reshape(K, N)
        if not np.all(np.isfinite(x)): raise ValueError('the live points must be finite')
        self._check_terms(L, pi)
        logx, logz = np.array(logx, dtype='f8').reshape(K), np.array(logz, dtype='f8').reshape(K)
        if not (np.all(logx <= 0.) and np.all(np.isfinite(logx))): raise ValueError('logx must be finite and not above 0')
        if np.any(np.isnan(logz)) or np.any(logz == np.inf): raise ValueError('logz must be finite or -inf')
        self.x, self.L, self.pi, self.logx, self.logz = x, L, pi, logx, logz
        self.iter, self.scale, self.mode = np.array(counters, dtype='i8').reshape(K), np.array(scale, dtype='f8').reshape(K), np.array(modes, dtype='i4').reshape(K)
        self._have_state = True

    def get_state(self):
        return tuple(a.copy() for a in (self.x, self.L, self.pi, self.logx, self.logz, self.iter, self.scale, self.mode))

    # ---- an iteration -------------------------------------------------------------------------------------------------------------------------------------------
    def _iteration(self, rec):
        hist, dcoords, dL, dpi, dlogw, count, modes, quota = rec
        K, N, P, M, n = self.K, self.N, self.P, self.M, self.n_steps
        active = np.nonzero((self.mode != REST) & (count < quota))[0]
        if self._decisions is not None and self._decisions[0].shape == (K, N) and self._decisions[1].shape == (K, M) and self._decisions[2].shape == (K, n, M):
            order, seeds, flags, mean, cov = (a.copy() for a in self._decisions)
        else: order, seeds, flags, mean, cov = np.zeros((K, N), dtype='i8'), np.zeros((K, M), dtype='i8'), np.zeros((K, n, M), dtype=bool), np.zeros((K, P)), np.zeros((K, P, P))
        lstar, chol = np.zeros(K), np.zeros((K, P, P))
        for k in active:
            order[k] = ranks(self.L[k])
            dead = order[k, :M]
            lstar[k] = self.L[k, dead[-1]]
            logw, self.logx[k], self.logz[k] = evidence(self.L[k, dead], N, self.logx[k], self.logz[k])
            mean[k], cov[k] = survivor_moments(self.x[k], dead)
            chol[k] = factor(cov[k], self.widths)
            r, margins = seed_ranks(self.draws.seed_uniform(self.iter[k], self.ids[k], M), N, M)
            self._margin(margins)
            seeds[k] = order[k, r]
            slot = count[k]
            dcoords[k, slot], dL[k, slot], dpi[k, slot], dlogw[k, slot] = self.x[k, dead], self.L[k, dead], self.pi[k, dead], logw
            self.x[k, dead], self.L[k, dead], self.pi[k, dead] = self.x[k, seeds[k]], self.L[k, seeds[k]], self.pi[k, seeds[k]]
        s, total = self.scale.copy(), np.zeros(K)
        for j in range(n):
            prop = np.stack([self.x[k, order[k, :M]] for k in range(K)])          # [K, M, P]; the rows of a run that does not take part are evaluated and ignored
            for k in active:
                z = self.draws.gauss(self.iter[k], j, self.ids[k], M, P)
                prop[k] = prop[k] + (s[k] * (2.38 / np.sqrt(float(P)))) * _matvec(chol[k], z)
            Lp, pip = self._eval(prop)
            for k in active:
                dead = order[k, :M]
                logu = self.draws.log_uniform(self.iter[k], j, self.ids[k], M)
                with np.errstate(invalid='ignore'):
                    ok = (np.abs(Lp[k]) < np.inf) & (np.abs(pip[k]) < np.inf)
                    above = ok & (np.where(ok, Lp[k], 0.) > lstar[k])
                    ratio = np.where(ok, pip[k], 0.) - self.pi[k, dead]
                    accept = above & (logu < ratio)
                    self._margin(np.abs(np.where(ok, Lp[k], 0.) - lstar[k])[ok] / max(abs(lstar[k]), 1e-300))
                    self._margin(np.abs(logu - ratio)[above])
                self.x[k, dead[accept]], self.L[k, dead[accept]], self.pi[k, dead[accept]] = prop[k][accept], Lp[k][accept], pip[k][accept]
                flags[k, j] = accept
                total[k] += accept.sum()
                s[k] = next_scale(s[k], accept.sum() / M, self.target_acceptance)
        for k in active:
            rem = remaining(self.L[k], self.logx[k])
            hist[k, count[k]] = self.logx[k], self.logz[k] + self.offset, lstar[k], total[k] / (float(n) * M), s[k], rem + self.offset
            self.scale[k] = s[k]
            self.iter[k] += 1
            count[k] += 1
            self.mode[k] = REST if at_rest(self.logz[k], rem, self.dlogz) else CLIMB
        modes[:] = self.mode
        self._decisions = (order, seeds, flags, mean, cov)

    # ---- a batch ------------------------------------------------------------------------------------------------------------------------------------------------
    def buffers(self, quota):
        K, M, P = self.K, self.M, self.P
        return (np.zeros((K, quota, 6)), np.zeros((K, quota, M, P)), np.zeros((K, quota, M)), np.zeros((K, quota, M)), np.zeros((K, quota, M)), np.zeros(K, dtype='i8'),
                np.ones(K, dtype='i4'))

    def run(self, niterations, quota, buffers):
        """``niterations`` iterations of every run into ``buffers`` (the semantics of dl_nested_run)."""
        if not self.n_steps: raise ValueError('no hyper-parameters (set_hyper)')
        if not self._have_state: raise ValueError('no live points (set_live or set_state)')
        for _ in range(int(niterations)): self._iteration(tuple(buffers) + (int(quota),))
        self.iterations += int(niterations)

    def modes(self, buffers):
        return np.asarray(buffers[6])


class _DeviceNested(_DeviceEngine):
    """Runs resident on the GPU (``dl_nested_*``): the calls of :class:`_HostNested` go to the owner ``nested``."""
    _counts, _nrecords, _counters = 5, 5, ('iterations', 'evaluations')
    M = property(lambda self: self.nested.ndelete)

    def __init__(self, ctx, offset, nruns, nlive, widths, run_ids=None, seed=0):
        from ._lib import DeviceNested
        self.nested, self.ctx = DeviceNested(ctx, nruns, nlive, widths, run_ids=run_ids, seed=seed, offset=offset), ctx
        self._owner = self.nested
        self.K, self.N, self.P, self.offset = int(nruns), int(nlive), self.nested.n_params, float(offset)

    def terms(self, x):
        """(loglike, logprior) of rows x [B, P] through the context's dl_eval_batch, -inf where the status is not 0."""
        import torch
        device = 'cuda:{:d}'.format(self.ctx.device)
        t = torch.as_tensor(np.ascontiguousarray(x, dtype='f8'), device=device)
        L, pi = torch.empty(len(x), dtype=torch.float64, device=device), torch.empty(len(x), dtype=torch.float64, device=device)
        status = torch.empty(len(x), dtype=torch.int32, device=device)
        self.ctx.eval_batch(t, loglike=L, logprior=pi, status=status)
        L, pi, status = L.cpu().numpy(), pi.cpu().numpy(), status.cpu().numpy()
        L[status != 0] = -np.inf
        return L, pi

    def modes(self, buffers):
        return buffers[6].cpu().numpy()        # the one synchronisation of a chunk (the counts are read after the last)


def run_batch(engine, niterations, chunk=None):
    """At most ``niterations`` iterations of every run in chunks of at most ``chunk``, ending early once every run is at rest (the modes are read once per chunk):
    (history [K, n, 6], dead coords [K, n, M, P], dead loglike, logprior, logweight [K, n, M], counts [K], modes [K]); rows beyond counts[k] are not written."""
    buffers = _run_chunks(engine, niterations, chunk, stop=lambda buffers: not np.any(engine.modes(buffers) != REST))
    return engine.records(buffers) + (engine.counts(buffers).copy(), engine.modes(buffers).copy())


class NestedSampler(_EvidenceSampler):
    """``NestedSampler(likelihood, nlive=1024, chains=1, ndelete='nlive // 4', n_steps='4 * ndim', target_acceptance=0.234, dlogz=0.01, seed=None, save_fn=None,
    device_resident=None)``: nested sampling from the PRIOR to the posterior, with the Bayesian evidence and its error from a single run.

    nlive : live points of a run, a multiple of 64 between 64 and 8192.
    chains : number of independent runs, or the files written by :meth:`save` (one per run): the run is continued.
    ndelete : points that die per iteration, 1 .. nlive / 2 (an expression of ``nlive`` or a number).
    n_steps : constrained random-walk Metropolis sweeps over the replaced points per iteration (an expression of ``ndim`` or a number).
    target_acceptance : the acceptance fraction the proposal scale is steered to.
    dlogz : a run rests once the evidence left in its live points is below this fraction of the total.

    Every varied parameter needs a PROPER prior: the live points start there (a draw without a finite likelihood is redrawn; the accepted fraction enters ``logz``).
    All live points of a run live on one GPU: more than one rank in the process group raises ``NotImplementedError`` (run one sampler per rank with different seeds
    and pool their ``logz`` instead).

    After :meth:`run`: ``logz`` [chains] (the constant of a marginalised posterior context and log ``prior_fraction`` included), ``logz_err`` [chains] = sqrt(H / nlive),
    ``information`` [chains] (H), ``logz_mean`` = log of the mean Z, ``logz_std`` (the scatter of ``logz``; ``None`` for one run), ``history`` (dict of [chains, T]
    arrays, NaN beyond a run's last iteration), ``nevaluations``, ``chains`` (per run name -> [n] with ``logposterior``, ``loglikelihood``, ``logweight`` and ``aweight``:
    the dead points in the order of their death, then the closing live points), :meth:`samples`."""
    name, _words = 'nested', ('NestedSampler', 'live points', 'run')

    def __init__(self, likelihood, nlive=1024, chains=1, ndelete='nlive // 4', n_steps='4 * ndim', target_acceptance=0.234, dlogz=0.01, seed=None, save_fn=None,
                 device_resident=None, **kwargs):
        super(NestedSampler, self).__init__(likelihood, seed=seed, **kwargs)
        resume = self._setup(chains, seed, save_fn, device_resident)
        ndim, self.nlive, self._offset = len(self.varied_params), int(nlive), 0.
        _check_live(self.nlive)
        self.ndelete, self.n_steps = int(_expression(ndelete, nlive=self.nlive)), int(_expression(n_steps, ndim=ndim))
        self.target_acceptance, self.dlogz = float(target_acceptance), float(dlogz)
        _check_hyper(self.nlive, self.ndelete, self.n_steps, self.target_acceptance, self.dlogz, 1.)
        self._history = [np.zeros((0, 6)) for _ in range(self.nchains)]
        self._dead = [[np.zeros((0, ndim)), np.zeros(0), np.zeros(0), np.zeros(0)] for _ in range(self.nchains)]       # coords, loglike, logprior, logweight
        self.prior_fraction = np.ones(self.nchains)
        if resume is not None: self._resume(resume)

    # ---- engine -------------------------------------------------------------------------------------------------------------------------------------------------
    def _draw(self, size):
        return np.column_stack([param.prior.sample(size=size, random_state=self.rng) for param in self.varied_params])

    def _start(self, engine):
        """N points per run from the priors with a finite likelihood: the rows without one are redrawn, at most 64 times; ``prior_fraction`` = accepted / drawn."""
        K, N, ndim = self.nchains, self.nlive, len(self.varied_params)
        start, drawn = self._draw(K * N), np.full(K, N)
        L, pi = engine.terms(start)
        self._evaluations += K * N
        bad = ~(np.isfinite(L) & np.isfinite(pi))
        for _ in range(64):
            if not bad.any(): break
            fresh = self._draw(int(bad.sum()))
            L, pi = engine.terms(fresh)
            self._evaluations += len(fresh)
            drawn = drawn + bad.reshape(K, N).sum(axis=1)
            start[bad] = fresh
            bad[bad] = ~(np.isfinite(L) & np.isfinite(pi))
        if bad.any(): raise RuntimeError('no finite likelihood for {:d} live points after 64 rounds of redraws from the priors'.format(int(bad.sum())))
        start = start.reshape(K, N, ndim)
        self.prior_fraction = N / drawn.astype('f8')
        return start

    def _make_engine(self):
        ids, ndim = np.arange(self.nchains), len(self.varied_params)
        if self.device_resident:
            ctx, offset = self.likelihood._get_posterior_context()
            engine = _DeviceNested(ctx, offset, self.nchains, self.nlive, self.widths, run_ids=ids, seed=self.counter_seed)
        else:
            engine = _HostNested(self._host_terms, self.nchains, self.nlive, ndim, self.widths, run_ids=ids, seed=self.counter_seed)
        self._offset = float(engine.offset)
        engine.set_hyper(self.ndelete, self.n_steps, self.target_acceptance, self.dlogz, 1.)
        if self._state is not None: engine.set_state(*self._state)
        else:
            engine.set_live(self._start(engine))
            self._evaluations += engine.evaluations
        return engine

    def _advance(self, niterations):
        before = self._engine.evaluations
        history, coords, L, pi, logw, counts, modes = run_batch(self._engine, niterations)
        self._evaluations += self._engine.evaluations - before
        P = coords.shape[-1]
        for k in range(self.nchains):
            c = counts[k]
            self._history[k] = np.concatenate([self._history[k], history[k, :c]])
            for i, a in enumerate((coords[k, :c].reshape(-1, P), L[k, :c].ravel(), pi[k, :c].ravel(), logw[k, :c].ravel())):
                self._dead[k][i] = np.concatenate([self._dead[k][i], a])
        self._state = self._engine.get_state()

    def run(self, max_iterations=100000, check_every=16):
        """Iterate in chunks of ``check_every`` (the modes are read once per chunk; how the iterations are chunked does not change the runs) until every run is at rest.
        A run that has not come to rest after ``max_iterations`` iterations in all raises ``RuntimeError``.  Returns the list of chains."""
        max_iterations = int(max_iterations)
        if self._engine is None: self._engine = self._make_engine()
        self._state = self._engine.get_state()
        while np.any(self._state[7] != REST):
            done = int(self._state[5].max())
            if done >= max_iterations:
                raise RuntimeError('not at rest after {:d} iterations (log Z_rem - log Z = {}): raise max_iterations or dlogz'.format(
                    done, [float(h[-1, 5] - h[-1, 1]) if len(h) else None for h in self._history]))
            self._advance(min(int(check_every), max_iterations - done))
        if self.save_fn is not None: self.save()
        return self.chains

    # ---- outputs ------------------------------------------------------------------------------------------------------------------------------------------------
    def _closing(self):
        if self._state is None: return None
        return [closing(self._dead[k][1], self._dead[k][3], self._state[1][k], self._state[3][k]) for k in range(self.nchains)]

    @property
    def chains(self):
        """Per run: dict name -> [n] (incl. 'logposterior', 'loglikelihood', 'logweight', 'aweight'): the dead points, then the closing live points."""
        out, closed = [], self._closing()
        if closed is None: return out
        for k, c in enumerate(closed):
            coords = np.concatenate([self._dead[k][0], self._state[0][k]])
            logprior = np.concatenate([self._dead[k][2], self._state[2][k]])
            chain = {param.name: coords[:, iparam] for iparam, param in enumerate(self.varied_params)}
            chain['loglikelihood'] = c['loglike'] + self._offset
            chain['logposterior'] = chain['loglikelihood'] + logprior
            chain['logweight'], chain['aweight'] = c['logweight'], c['aweight']
            out.append(chain)
        return out

    def samples(self, size, random_state=None):
        """``size`` equally weighted posterior samples, the runs pooled at equal shares: systematic resampling on ``aweight``; dict name -> [size]."""
        chains = self.chains
        rng = self.rng if random_state is None else random_state
        weights = np.concatenate([chain['aweight'] for chain in chains]) / len(chains)
        cum = np.cumsum(weights)
        index = np.minimum(np.searchsorted(cum, (np.arange(size) + rng.uniform()) / size * cum[-1], side='left'), len(cum) - 1)
        return {name: np.concatenate([chain[name] for chain in chains])[index] for name in chains[0] if name not in ('aweight', 'logweight')}

    @property
    def history(self):
        T = max(len(h) for h in self._history)
        padded = np.full((self.nchains, T, 6), np.nan)
        for k, h in enumerate(self._history): padded[k, :len(h)] = h
        return {name: padded[..., i] for i, name in enumerate(HISTORY_FIELDS)}

    @property
    def niterations(self):
        return np.array([len(h) for h in self._history])

    @property
    def logz(self):
        closed = self._closing()
        if closed is None: return np.full(self.nchains, np.nan)
        return np.array([c['logz'] for c in closed]) + self._offset + np.log(self.prior_fraction)

    @property
    def logz_err(self):
        closed = self._closing()
        if closed is None: return np.full(self.nchains, np.nan)
        return np.array([c['logz_err'] for c in closed])

    @property
    def information(self):
        closed = self._closing()
        if closed is None: return np.full(self.nchains, np.nan)
        return np.array([c['information'] for c in closed])

    def save(self, fn=None):
        """One file per run in the reference's checkpoint format; attributes ``{'sampler': 'nested', 'seed', 'state', 'history', ...}``: the state continues the run."""
        fn = self._save_names(fn)
        if self._state is None: return
        self._write_chains((name, chain, {'sampler': self.name, 'seed': self.counter_seed, 'run': k, 'state': [np.asarray(a[k]) for a in self._state], 'history': self._history[k],
                                          'hyper': [self.ndelete, self.n_steps, self.target_acceptance, self.dlogz], 'evaluations': self._evaluations,
                                          'offset': self._offset, 'prior_fraction': float(self.prior_fraction[k])}) for k, (chain, name) in enumerate(zip(self.chains, fn)))

    def _resume(self, sources):
        """Continue the runs saved by :meth:`save`: live points, volumes, evidences, counters, scales, modes (and the dead points so far)."""
        files = _open_chain_files(sources)
        names = self.varied_params.names()
        for f in files:
            if f.attrs.get('sampler', None) != self.name or 'state' not in f.attrs: raise ValueError('not a chain file of NestedSampler')
        dtypes = ['f8', 'f8', 'f8', 'f8', 'f8', 'i8', 'f8', 'i4']
        self._state = tuple(np.array([np.asarray(f.attrs['state'][i]) for f in files], dtype=dtypes[i]) for i in range(8))
        if self._state[0].shape[1:] != (self.nlive, len(names)): raise ValueError('the saved runs have {:d} live points'.format(self._state[0].shape[1]))
        self._history = [np.asarray(f.attrs['history'], dtype='f8').reshape(-1, 6) for f in files]
        self._offset = float(files[0].attrs.get('offset', 0.))
        for k, f in enumerate(files):
            ndead = len(np.asarray(f.arrays['logweight'])) - self.nlive
            loglike = np.asarray(f.arrays['loglikelihood'], dtype='f8')[:ndead]
            self._dead[k] = [np.stack([np.asarray(f.arrays[name], dtype='f8') for name in names], axis=-1)[:ndead], loglike - self._offset,
                             np.asarray(f.arrays['logposterior'], dtype='f8')[:ndead] - loglike, np.asarray(f.arrays['logweight'], dtype='f8')[:ndead]]
        self.prior_fraction = np.array([float(f.attrs.get('prior_fraction', 1.)) for f in files])
        self.counter_seed = int(files[0].attrs['seed'])
        hyper = files[0].attrs['hyper']
        self.ndelete, self.n_steps, self.target_acceptance, self.dlogz = int(hyper[0]), int(hyper[1]), float(hyper[2]), float(hyper[3])
        self._evaluations = int(files[0].attrs.get('evaluations', 0))
