"""No-U-Turn sampler on batches of asynchronous chains (the reference's ``NUTSSampler``, desilike/samplers/nuts.py, wraps ``blackjax.nuts`` around ``jax.value_and_grad``
of one chain).

Multinomial NUTS (Hoffman & Gelman 2014; Betancourt 2017) with the generalised U-turn criterion and the extra checks across a join (Stan >= 2.26, blackjax); the
trajectory is built one leaf per step from a fixed-size per-chain record (csrc/dl_nuts.h states the algorithm and the random draws).  Every step advances every
chain by one leapfrog step, so a batch of chains never waits for its deepest tree:

* :class:`_DeviceNUTS` runs the chains on the GPU (``dl_nuts_*``: one gradient batch + one fused kernel per step);
* :class:`_HostNUTS` is the NumPy statement of the same step, with the same counter-based draws (:class:`~desilike_amd.samplers.CounterRNG`), around an injected
  ``(logposterior, gradient) = f(q [C, P])``: likelihoods without a device context, and the yardstick of the device engine in the tests.

Warm-up as :class:`~desilike_amd.hmc.HMCSampler`: per-chain dual averaging of the step size, the inverse mass matrix from the pooled positions of a window (Stan's
regularisation), dual averaging restarted, final step size exp(mean over chains of log eps-bar)."""
import numpy as np

from .samplers import BasePosteriorSampler, CounterRNG, _DeviceEngine, _batch_iterate, _open_chain_files, _parse_chains
from .parallel import WalkerSharding

STREAM_MOMENTUM, STREAM_DIRECTION, STREAM_SELECT = 32, 33, 34
INFO_FIELDS = ('tree_depth', 'num_integration_steps', 'divergent', 'acceptance', 'energy')


def _logaddexp(a, b):
    with np.errstate(invalid='ignore', over='ignore'):
        m = np.maximum(a, b)
        out = m + np.log1p(np.exp(-np.abs(a - b)))
    out = np.where(a == -np.inf, b, out)
    return np.where(b == -np.inf, a, out)


def _ckpt_range(n):
    """Checkpoints of leaf n (NumPyro's _leaf_idx_to_ckpt_idxs): (idx_min, idx_max)."""
    n = np.asarray(n, dtype='i8')
    mx, ones, m = np.zeros_like(n), np.zeros_like(n), n >> 1
    while np.any(m > 0):
        mx += m & 1; m = m >> 1
    m = n.copy()
    while np.any(m & 1):
        ones += m & 1; m = np.where(m & 1, m >> 1, 0)
    return mx - ones + 1, mx


class _Draws(object):
    """The draws of csrc/dl_nuts.h: Philox4x32-10 keyed by ``seed``, counter (iteration lo, iteration hi, chain id, stream word)."""

    def __init__(self, seed):
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)

    def _words(self, it, chain, stream):
        it = np.asarray(it, dtype='i8')
        counter = np.empty(it.shape + (4,), dtype=np.uint32)
        counter[..., 0], counter[..., 1] = (it & 0xFFFFFFFF).astype(np.uint32), ((it >> 32) & 0xFFFFFFFF).astype(np.uint32)
        counter[..., 2], counter[..., 3] = np.asarray(chain, dtype=np.uint32), np.asarray(stream, dtype=np.uint32)
        return CounterRNG.philox4x32(counter, np.broadcast_to(self.key, it.shape + (2,)))

    def gauss(self, it, chain, P):
        """Standard Gaussians [C, P] of the momentum of trajectory ``it`` (Box-Muller pairs)."""
        it, chain = np.asarray(it, dtype='i8'), np.asarray(chain)
        z = np.empty((len(it), P + (P & 1)))
        for j in range((P + 1) // 2):
            z[:, 2 * j], z[:, 2 * j + 1] = CounterRNG.box_muller(self._words(it, chain, np.full(len(it), STREAM_MOMENTUM | (j << 8), dtype=np.uint32)))
        return z[:, :P]

    def direction(self, it, chain, depth):
        """(direction +1 / -1, join uniform) of doubling ``depth``."""
        w = self._words(it, chain, STREAM_DIRECTION | (np.asarray(depth, dtype=np.uint32) << np.uint32(8)))
        return np.where(w[:, 0] >> np.uint32(31), 1, -1), CounterRNG.uniform53(w[:, 2], w[:, 3])

    def select(self, it, chain, depth, leaf):
        w = self._words(it, chain, STREAM_SELECT | (np.asarray(depth, dtype=np.uint32) << np.uint32(8)) | (np.asarray(leaf, dtype=np.uint32) << np.uint32(12)))
        return CounterRNG.uniform53(w[:, 0], w[:, 1])


class _HostNUTS(object):
    """NumPy statement of the device engine's step (csrc/dl_nuts.h, same record, same draws), around ``f(q [C, P]) -> (logposterior [C], gradient [C, P])``."""
    device_resident = False

    def __init__(self, f, nchains, n_params, chain_ids=None, max_num_doublings=10, divergence_threshold=1000., seed=0, offset=0.):
        self.f, self.C, self.P, self.D = f, int(nchains), int(n_params), int(max_num_doublings)
        self.chain_ids = np.arange(self.C) if chain_ids is None else np.asarray(chain_ids, dtype='i8')
        self.threshold, self.offset, self.draws = float(divergence_threshold), float(offset), _Draws(seed)
        C, P = self.C, self.P
        self.v = {name: np.zeros((C, P)) for name in ['ql', 'pl', 'gl', 'qr', 'pr', 'gr', 'qp', 'gp', 'qs', 'gs', 'qn', 'pn', 'pf', 'rho', 'rhos']}
        self.ck_rho, self.ck_sharp = np.zeros((self.D, C, P)), np.zeros((self.D, C, P))
        self.d = {name: np.zeros(C) for name in ['lpp', 'hp', 'lps', 'hs', 'h0', 'lw', 'lws', 'sacc', 'logeps', 'hbar', 'logbar', 'mu', 'dacount']}
        self.i = {name: np.zeros(C, dtype='i8') for name in ['depth', 'leaf', 'dir', 'nleaf', 'active']}
        self.iter = np.zeros(C, dtype='i8')
        self.minv, self.lmass, self.adapt, self.target, self.steps = None, None, False, 0.8, 0

    # ---- set-up (dl_nuts_set_mass / set_state / get_state / set_adaptation) -------------------------------------------------------------------------------------
    def set_mass(self, inverse_mass, step_size):
        minv = np.array(inverse_mass, dtype='f8')
        self.minv = minv
        self.lmass = np.linalg.cholesky(np.linalg.inv(minv)) if minv.ndim == 2 else None
        self.d['logeps'][:] = self.d['logbar'][:] = np.log(step_size)

    def set_state(self, coords, logposterior=None, iterations=None):
        coords = np.array(coords, dtype='f8').reshape(self.C, self.P)
        if not np.all(np.isfinite(coords)): raise ValueError('the starting positions must be finite')
        lp, g = self.f(coords)
        lp = np.asarray(lp, dtype='f8') + self.offset if logposterior is None else np.asarray(logposterior, dtype='f8')
        if not np.all(np.isfinite(lp)): raise ValueError('the log-posterior of a starting position is not finite')
        self.v['qp'][...] = coords; self.v['qn'][...] = coords; self.v['gp'][...] = g
        self.d['lpp'][:] = lp
        self.iter[:] = 0 if iterations is None else np.asarray(iterations, dtype='i8')
        self.i['active'][:] = 0

    def get_state(self):
        return self.v['qp'].copy(), self.d['lpp'].copy(), self.iter.copy(), self.d['logbar'].copy()

    def set_adaptation(self, enabled, target_acceptance=0.8, initial_step_size=1.):
        self.adapt = bool(enabled)
        if not self.adapt: return
        self.target = float(target_acceptance)
        init = np.log(initial_step_size)
        self.d['logeps'][:] = self.d['logbar'][:] = init
        self.d['mu'][:] = np.log(10.) + init
        self.d['hbar'][:] = 0.; self.d['dacount'][:] = 0.

    # ---- arithmetic ---------------------------------------------------------------------------------------------------------------------------------------------
    def _sharp(self, p):
        return p @ self.minv.T if self.minv.ndim == 2 else p * self.minv

    @staticmethod
    def _dot(a, b):
        return (a * b).sum(axis=-1)

    def _no_uturn(self, a, b, rho):
        return (self._dot(a, rho) > 0.) & (self._dot(b, rho) > 0.)

    def _launch_leaf(self, c, v, q, p, g):
        h = v * np.exp(self.d['logeps'][c])
        ph = p + (0.5 * h)[:, None] * g
        self.v['pn'][c] = ph
        self.v['qn'][c] = q + h[:, None] * self._sharp(ph)
        self.i['active'][c] = 1

    def _start(self, c):
        if not len(c): return
        it, chain = self.iter[c], self.chain_ids[c]
        z = self.draws.gauss(it, chain, self.P)
        p = z @ self.lmass.T if self.minv.ndim == 2 else z / np.sqrt(self.minv)
        h0 = -self.d['lpp'][c] + 0.5 * self._dot(p, self._sharp(p))
        q, g = self.v['qp'][c], self.v['gp'][c]
        for e in 'lr':
            self.v['q' + e][c], self.v['p' + e][c], self.v['g' + e][c] = q, p, g
        self.v['rho'][c] = p
        self.d['h0'][c] = h0; self.d['hp'][c] = h0; self.d['lw'][c] = 0.; self.d['sacc'][c] = 0.
        self.i['depth'][c] = 0; self.i['leaf'][c] = 0; self.i['nleaf'][c] = 0
        v = self.draws.direction(it, chain, np.zeros(len(c), dtype='i8'))[0]
        self.i['dir'][c] = v
        self._launch_leaf(c, v, q, p, g)

    def _finish(self, c, depth_attempted, divergent, rec):
        if not len(c): return
        coords, logp, info, count, quota, thin_by = rec
        nleaf = self.i['nleaf'][c]
        accept = self.d['sacc'][c] / nleaf
        it = self.iter[c] + 1
        r = it % thin_by == 0
        cr, slot = c[r], count[c[r]]
        coords[cr, slot], logp[cr, slot] = self.v['qp'][cr], self.d['lpp'][cr]
        info[cr, slot] = np.column_stack([np.asarray(depth_attempted)[r], nleaf[r], np.broadcast_to(divergent, len(c))[r], accept[r], self.d['hp'][cr]])
        count[cr] += 1
        if self.adapt:
            d = self.d
            n = d['dacount'][c] + 1.
            d['hbar'][c] = (1. - 1. / (n + 10.)) * d['hbar'][c] + (self.target - accept) / (n + 10.)
            d['logeps'][c] = d['mu'][c] - np.sqrt(n) / 0.05 * d['hbar'][c]
            eta = n**(-0.75)
            d['logbar'][c] = eta * d['logeps'][c] + (1. - eta) * d['logbar'][c]
            d['dacount'][c] = n
        self.iter[c] = it
        self.i['active'][c] = 0
        self._start(c[count[c] < quota])

    def _step(self, lp_new, g_new, rec):
        count, quota = rec[3], rec[4]
        V, d, I = self.v, self.d, self.i
        c = np.nonzero((count < quota) & (I['active'] == 1))[0]
        if not len(c): return
        it, chain = self.iter[c], self.chain_ids[c]
        depth, leaf, v = I['depth'][c], I['leaf'][c], I['dir'][c]
        h = v * np.exp(d['logeps'][c])
        lp = np.asarray(lp_new, dtype='f8')[c]
        lp = np.where((lp == lp) & (lp < np.inf), lp + self.offset, -np.inf)
        q, g = V['qn'][c], np.array(g_new, dtype='f8')[c]
        g[~(lp > -np.inf)[:, None] | ~(np.abs(g) < np.inf)] = 0.
        p = V['pn'][c] + (0.5 * h)[:, None] * g
        ps = self._sharp(p)
        with np.errstate(invalid='ignore', over='ignore'):
            H = -lp + 0.5 * self._dot(p, ps)
            dH = H - d['h0'][c]
            acc = np.where(dH == dH, np.where(dH > 0., np.exp(-np.where(dH > 0., dH, 0.)), 1.), 0.)
        I['nleaf'][c] += 1
        d['sacc'][c] += acc
        div = ~(dH <= self.threshold)
        self._finish(c[div], depth[div] + 1, np.where(lp[div] > -np.inf, 1, 2), rec)     # 2: the leaf left the support
        k = ~div
        c, it, chain, depth, leaf, v, lp, q, g, p, ps, H, dH = (x[k] for x in (c, it, chain, depth, leaf, v, lp, q, g, p, ps, H, dH))
        lw_leaf = -dH
        # uniform progressive sampling inside the subtree
        first = leaf == 0
        before = np.where(first[:, None], 0., V['rhos'][c])
        lws = np.where(first, lw_leaf, _logaddexp(d['lws'][c], lw_leaf))
        with np.errstate(over='ignore'):
            take = first | (self.draws.select(it, chain, depth, leaf) < np.exp(lw_leaf - lws))
        rhos = before + p
        V['pf'][c[first]] = p[first]
        V['qs'][c[take]], V['gs'][c[take]] = q[take], g[take]
        # checkpoints, U-turns of the sub-subtrees this leaf completes
        imin, imax = _ckpt_range(leaf)
        even = leaf % 2 == 0
        self.ck_rho[imax[even], c[even]], self.ck_sharp[imax[even], c[even]] = before[even], ps[even]
        turning = np.zeros(len(c), dtype=bool)
        for j in range(self.D):
            i = imax - j
            check = ~even & (i >= imin) & ~turning
            if not check.any(): continue
            ii, cc = i[check], c[check]
            turning[check] = ~self._no_uturn(self.ck_sharp[ii, cc], ps[check], rhos[check] - self.ck_rho[ii, cc])
        d['lws'][c] = lws
        d['lps'][c[take]], d['hs'][c[take]] = lp[take], H[take]
        self._finish(c[turning], depth[turning] + 1, 0, rec)
        cont = ~turning & (leaf + 1 < (1 << depth))
        cc = c[cont]
        V['rhos'][cc] = rhos[cont]
        I['leaf'][cc] = leaf[cont] + 1
        self._launch_leaf(cc, v[cont], q[cont], p[cont], g[cont])
        # joins: biased progressive sampling, U-turn of the trajectory and across the join
        k = ~turning & ~cont
        c, it, chain, depth, v, lp, q, g, p, ps, rhos, lws = (x[k] for x in (c, it, chain, depth, v, lp, q, g, p, ps, rhos, lws))
        if not len(c): return
        u_join = self.draws.direction(it, chain, depth)[1]
        lw = d['lw'][c]
        with np.errstate(over='ignore'):
            swap = u_join < np.exp(lws - lw)
        rho, pf, pl, pr = V['rho'][c], V['pf'][c], V['pl'][c], V['pr'][c]
        psf, psl, psr = self._sharp(pf), self._sharp(pl), self._sharp(pr)
        rho_new = rho + rhos
        right = v > 0
        go_r = self._no_uturn(psl, ps, rho_new) & self._no_uturn(psl, psf, rho + pf) & self._no_uturn(psr, ps, pr + rhos)
        go_l = self._no_uturn(ps, psr, rho_new) & self._no_uturn(ps, psl, rhos + pl) & self._no_uturn(psf, psr, pf + rho)
        go = np.where(right, go_r, go_l)
        V['qp'][c[swap]], V['gp'][c[swap]] = V['qs'][c[swap]], V['gs'][c[swap]]
        for e, sel in (('r', right), ('l', ~right)):
            V['q' + e][c[sel]], V['p' + e][c[sel]], V['g' + e][c[sel]] = q[sel], p[sel], g[sel]
        V['rho'][c] = rho_new
        d['lw'][c] = _logaddexp(lw, lws)
        d['lpp'][c[swap]], d['hp'][c[swap]] = d['lps'][c[swap]], d['hs'][c[swap]]
        end = ~go | (depth + 1 >= self.D)
        self._finish(c[end], depth[end] + 1, 0, rec)
        k = ~end
        c, it, chain, depth = c[k], it[k], chain[k], depth[k]
        w = self.draws.direction(it, chain, depth + 1)[0]
        I['depth'][c], I['leaf'][c], I['dir'][c] = depth + 1, 0, w
        e = w > 0
        qe = np.where(e[:, None], V['qr'][c], V['ql'][c]); pe = np.where(e[:, None], V['pr'][c], V['pl'][c]); ge = np.where(e[:, None], V['gr'][c], V['gl'][c])
        self._launch_leaf(c, w, qe, pe, ge)

    # ---- a batch ------------------------------------------------------------------------------------------------------------------------------------------------
    def buffers(self, quota):
        return (np.zeros((self.C, quota, self.P)), np.zeros((self.C, quota)), np.zeros((self.C, quota, 5)), np.zeros(self.C, dtype='i8'))

    def run(self, nsteps, quota, buffers, thin_by=1):
        """``nsteps`` leapfrog steps of every chain into ``buffers`` (the semantics of dl_nuts_run)."""
        rec = tuple(buffers) + (int(quota), int(thin_by))
        count = buffers[3]
        self._start(np.nonzero((self.i['active'] == 0) & (count < quota))[0])
        for _ in range(int(nsteps)):
            lp, g = self.f(self.v['qn'].copy())
            self._step(lp, g, rec)
        self.steps += int(nsteps)

    def counts(self, buffers):
        return np.asarray(buffers[3])

    def records(self, buffers):
        return tuple(np.asarray(b) for b in buffers[:3])


class _DeviceNUTS(_DeviceEngine):
    """Chains of this rank resident on the GPU (``dl_nuts_*``): the calls of :class:`_HostNUTS` go to the owner ``nuts``."""
    _counters = ('steps',)

    def __init__(self, ctx, offset, chain_ids, max_num_doublings, divergence_threshold, seed, gradient, fd_delta, fd_limits):
        from ._lib import DeviceNUTS
        self.nuts = self._owner = DeviceNUTS(ctx, len(chain_ids), chain_ids=chain_ids, max_num_doublings=max_num_doublings, divergence_threshold=divergence_threshold,
                                             seed=seed, offset=offset, gradient=gradient, fd_delta=fd_delta, fd_limits=fd_limits)
        self.C, self.P = len(chain_ids), self.nuts.n_params


def run_batch(engine, quota, thin_by=1, chunk=32):
    """Chunks of ``chunk`` leapfrog steps until every chain has ``quota`` records: (coords [C, quota, P], logposterior [C, quota], info [C, quota, 5])."""
    buffers = engine.buffers(quota)
    while True:
        engine.run(chunk, quota, buffers, thin_by=thin_by)
        if np.all(engine.counts(buffers) >= quota): break
    return engine.records(buffers)


class NUTSSampler(BasePosteriorSampler):
    """``NUTSSampler(likelihood, chains=64, adaptation=True, covariance=None, step_size=1e-3, max_num_doublings=10, divergence_threshold=1000,
    integrator='velocity_verlet', gradient='auto', seed=None, save_fn=None, device_resident=None)``: the arguments of the reference's sampler (samplers/nuts.py:17-121)
    and of :class:`~desilike_amd.hmc.HMCSampler`; ``run(min_iterations, max_iterations, check_every, check, thin_by, start)`` as samplers/base.py:409-502.

    adaptation : ``True`` / dict (``niterations`` default 300, ``target_acceptance_rate`` 0.8, ``is_mass_matrix_diagonal`` True, ``initial_step_size``) / ``False``.
    chains : number of chains, or the chain files written by :meth:`save` (one per chain): the saved chains are continued (last points, iteration counters,
        hyper-parameters; no new warm-up).
    covariance : initial inverse mass matrix (as HMCSampler).
    device_resident : run the chains on the GPU (``dl_nuts_*``); default: where the likelihood has a device context and no derived parameters.
    chunk : leapfrog steps enqueued between two reads of the record counts."""
    name = 'nuts'

    def __init__(self, likelihood, chains=64, adaptation=True, covariance=None, step_size=1e-3, max_num_doublings=10, divergence_threshold=1000., integrator='velocity_verlet',
                 gradient='auto', seed=None, save_fn=None, device_resident=None, chunk=32, **kwargs):
        if integrator != 'velocity_verlet':
            raise NotImplementedError('integrator {!r} is not built: NUTSSampler integrates with velocity_verlet only'.format(integrator))
        self.nchains, resume = _parse_chains(chains)
        super(NUTSSampler, self).__init__(likelihood, seed=seed, **kwargs)
        self.step_size, self.max_num_doublings, self.divergence_threshold = float(step_size), int(max_num_doublings), float(divergence_threshold)
        if not self.step_size > 0.: raise ValueError('step_size must be positive')
        if not 1 <= self.max_num_doublings <= 15: raise ValueError('max_num_doublings must be in [1, 15]')
        if not self.divergence_threshold > 0.: raise ValueError('divergence_threshold must be positive')
        if gradient not in ('auto', 'analytic', 'finite'): raise ValueError('gradient must be one of auto, analytic, finite')
        self.gradient, self.chunk = gradient, int(chunk)
        self.chain_group = self.sharding.group if self.sharding.active and self.sharding.world > 1 else None
        self.sharding = WalkerSharding(group=False)
        self.chain_rank = self.chain_group.rank if self.chain_group is not None else 0
        self.chain_world = self.chain_group.world if self.chain_group is not None else 1
        self.device_resident = bool(self._device_default() if device_resident is None else device_resident)
        self.counter_seed = self._counter_seed(seed)
        if adaptation is True: adaptation = {}
        self.adaptation = None if adaptation is False or adaptation is None else dict(adaptation)
        from .hmc import HMCSampler
        self.inverse_mass_matrix = HMCSampler._initial_covariance(self, covariance)
        self.save_fn = save_fn
        self._store = None               # (coords [n, nchains, ndim], logposterior [n, nchains], info [n, nchains, 5])
        self._state = None               # (points [nchains, ndim], log-posteriors [nchains] or None, iteration counters [nchains])
        self._engine = None
        self._adapted = self.adaptation is None
        self.diagnostics = {}
        self.hyp = None
        self.adaptation_acceptance = None
        if resume is not None: self._resume(resume)

    # ---- engines ------------------------------------------------------------------------------------------------------------------------------------------------
    def local_chains(self):
        return [ichain for ichain in range(self.nchains) if ichain % self.chain_world == self.chain_rank]

    def _fd_tables(self):
        delta = np.array([[param.delta[1], param.delta[2]] for param in self.varied_params], dtype='f8')
        limits = np.array([list(param.prior.limits) for param in self.varied_params], dtype='f8')
        return delta, limits

    def _host_value_and_grad(self, q):
        """Central differences through the sampler's log-posterior (one batch of C (2 P + 1) rows; steps as HMCSampler._value_and_grad)."""
        C, P = q.shape
        delta, limits = self._fd_tables()
        with np.errstate(invalid='ignore'):      # (a diverging leaf can sit at infinity)
            lower = np.maximum(np.minimum(delta[:, 0], q - limits[:, 0]), 0.)
            upper = np.maximum(np.minimum(delta[:, 1], limits[:, 1] - q), 0.)
        points = np.repeat(q[:, None, :], 2 * P + 1, axis=1)
        index = np.arange(P)
        points[:, 1 + 2 * index, index] -= lower
        points[:, 2 + 2 * index, index] += upper
        values = np.asarray(self.logposterior(points.reshape(-1, P)), dtype='f8').reshape(C, 2 * P + 1)
        with np.errstate(invalid='ignore', divide='ignore'):
            grad = (values[:, 2::2] - values[:, 1::2]) / (lower + upper)
        return values[:, 0], grad

    def _make_engine(self):
        local = np.array(self.local_chains(), dtype='i8')
        P = len(self.varied_params)
        if self.device_resident:
            ctx, offset = self.likelihood._get_posterior_context()
            delta, limits = self._fd_tables()
            return _DeviceNUTS(ctx, offset, local, self.max_num_doublings, self.divergence_threshold, self.counter_seed, self.gradient, delta, limits)
        if self.gradient == 'analytic': raise NotImplementedError('the host engine differentiates numerically: use gradient="auto" or "finite"')
        return _HostNUTS(self._host_value_and_grad, len(local), P, chain_ids=local, max_num_doublings=self.max_num_doublings,
                         divergence_threshold=self.divergence_threshold, seed=self.counter_seed)

    @staticmethod
    def _mass_argument(minv):
        minv = np.asarray(minv, dtype='f8')
        return np.diag(minv).copy() if np.allclose(np.diag(np.diag(minv)), minv) else minv     # a diagonal matrix is kept as its diagonal (hmc.py:_mass)

    def _gather(self, arrays):
        """Per-chain arrays of the local chains [nlocal, ...] -> [nchains, ...] on every rank (chain c lives on rank c % world)."""
        if self.chain_group is None: return arrays
        local = self.local_chains()
        nmax = (self.nchains + self.chain_world - 1) // self.chain_world
        shapes = [a.shape[1:] for a in arrays]
        sizes = [int(np.prod(s)) for s in shapes]
        block = np.zeros((nmax, sum(sizes)))
        for slot in range(len(local)):
            block[slot] = np.concatenate([np.asarray(a[slot], dtype='f8').ravel() for a in arrays])
        gathered = np.asarray(self.chain_group.allgather(block)).reshape(self.chain_world, nmax, sum(sizes))
        out = [np.empty((self.nchains,) + s) for s in shapes]
        for c in range(self.nchains):
            row, start = gathered[c % self.chain_world, c // self.chain_world], 0
            for o, s, n in zip(out, shapes, sizes):
                o[c] = row[start:start + n].reshape(s); start += n
        return [o.astype(a.dtype) for o, a in zip(out, arrays)]

    # ---- warm-up ------------------------------------------------------------------------------------------------------------------------------------------------
    def _warmup(self, engine):
        """Per-chain dual averaging; inverse mass matrix from the pooled positions of the window (all chains, every rank); dual averaging restarted; final step size
        exp(mean over chains of log eps-bar)."""
        a = self.adaptation
        niterations, target = int(a.get('niterations', 300)), float(a.get('target_acceptance_rate', 0.8))
        diagonal = bool(a.get('is_mass_matrix_diagonal', True))
        step_size = float(a.get('initial_step_size', self.step_size))
        window = (niterations // 2, niterations - max(niterations // 6, 10))
        engine.set_mass(self._mass_argument(self.inverse_mass_matrix), step_size)
        engine.set_adaptation(True, target, step_size)
        acceptance = []
        coords, _, info = run_batch(engine, window[1], chunk=self.chunk)
        coords, info = self._gather([coords, info])
        acceptance.append(info[..., 3])
        x = coords[:, window[0]:].reshape(-1, coords.shape[-1])
        if x.shape[0] > 2 * x.shape[1]:
            cov = np.atleast_2d(np.cov(x, rowvar=False, ddof=1))
            n, d = x.shape
            cov = (n / (n + 5.)) * cov + 1e-3 * (5. / (n + 5.)) * np.eye(d)       # Stan's regularisation of the estimate
            self.inverse_mass_matrix = np.diag(np.diag(cov)) if diagonal else cov
        logbar = self._gather([engine.get_state()[3][:, None]])[0][:, 0]
        step_size = float(np.exp(np.mean(logbar)))
        engine.set_mass(self._mass_argument(self.inverse_mass_matrix), step_size)
        engine.set_adaptation(True, target, step_size)
        if niterations > window[1]:
            _, _, info = run_batch(engine, niterations - window[1], chunk=self.chunk)
            acceptance.append(self._gather([info])[0][..., 3])
            logbar = self._gather([engine.get_state()[3][:, None]])[0][:, 0]
        self.step_size = float(np.exp(np.mean(logbar)))
        self.adaptation_acceptance = float(np.mean(np.concatenate(acceptance, axis=1)))
        self.hyp = {'step_size': self.step_size, 'inverse_mass_matrix': np.asarray(self.inverse_mass_matrix).copy()}
        self._adapted = True

    # ---- batches ------------------------------------------------------------------------------------------------------------------------------------------------
    def _run_batch(self, niterations, thin_by=1):
        local = self.local_chains()
        if self._engine is None:
            self._engine = self._make_engine()
            points, logp, iterations = self._state
            self._engine.set_mass(self._mass_argument(self.inverse_mass_matrix), self.step_size)
            self._engine.set_state(points[local], logposterior=None if logp is None else logp[local], iterations=iterations[local])
            if not self._adapted:
                self._warmup(self._engine)
            self._engine.set_adaptation(False)
            self._engine.set_mass(self._mass_argument(self.inverse_mass_matrix), self.step_size)
            if self.hyp is None: self.hyp = {'step_size': self.step_size, 'inverse_mass_matrix': np.asarray(self.inverse_mass_matrix).copy()}
        nrec = niterations // thin_by
        if not nrec: return
        coords, logp, info = run_batch(self._engine, nrec, thin_by=thin_by, chunk=self.chunk)
        points, lps, iterations, _ = self._engine.get_state()
        coords, logp, info, points, lps, iterations = self._gather([coords, logp, info, points, lps, iterations])
        self._state = (points, lps, iterations)
        batch = (coords.transpose(1, 0, 2), logp.T, info.transpose(1, 0, 2))
        self._store = batch if self._store is None else tuple(np.concatenate([s, b]) for s, b in zip(self._store, batch))

    def run(self, min_iterations=0, max_iterations=None, check_every=300, check=None, thin_by=1, start=None):
        """Batches of ``check_every`` trajectories of every chain until :meth:`check` passes or ``max_iterations``.  Returns the list of chains."""
        run_check = bool(check) or isinstance(check, dict)
        if max_iterations is None: max_iterations = np.iinfo('i8').max if run_check else check_every
        if start is not None:
            start = np.asarray(start, dtype='f8').reshape(self.nchains, len(self.varied_params))
            self._state, self._engine = (start, None, np.zeros(self.nchains, dtype='i8')), None
        elif self._state is None:
            self._state = self._get_start(self.nchains) + (np.zeros(self.nchains, dtype='i8'),)
        criteria = check if isinstance(check, dict) else {}

        def batch(niterations):
            self._run_batch(niterations, thin_by=thin_by)
            if self.save_fn is not None: self.save()
            return self.check(**criteria) if run_check else False

        _batch_iterate(batch, min_iterations=min_iterations, max_iterations=max_iterations, check_every=int(check_every))
        return self.chains

    # ---- outputs ------------------------------------------------------------------------------------------------------------------------------------------------
    @property
    def chains(self):
        """Per chain: dict name -> [n] (incl. 'logposterior'), or None before the first iteration."""
        if self._store is None: return [None] * self.nchains
        coords, logp, _ = self._store
        out = []
        for c in range(self.nchains):
            chain = {param.name: coords[:, c, iparam] for iparam, param in enumerate(self.varied_params)}
            chain['logposterior'] = logp[:, c]
            out.append(chain)
        return out

    def _info(self, field):
        if self._store is None: return np.zeros(self.nchains)
        return self._store[2][..., INFO_FIELDS.index(field)]

    @property
    def acceptance_rate(self):
        """Per chain: mean acceptance statistic of the recorded transitions."""
        return self._info('acceptance').mean(axis=0) if self._store is not None else np.zeros(self.nchains)

    @property
    def divergences(self):
        """Per chain: number of divergent recorded transitions (energy error or a leaf outside the support, as Stan and blackjax count them)."""
        return (self._info('divergent') > 0).sum(axis=0).astype('i8') if self._store is not None else np.zeros(self.nchains, dtype='i8')

    @property
    def energy_divergences(self):
        """Per chain: divergent recorded transitions caused by an energy error (H - H0 > divergence_threshold or NaN), not by a leaf outside the prior's support."""
        return (self._info('divergent') == 1).sum(axis=0).astype('i8') if self._store is not None else np.zeros(self.nchains, dtype='i8')

    @property
    def mean_tree_depth(self):
        return self._info('tree_depth').mean(axis=0) if self._store is not None else np.zeros(self.nchains)

    def check(self, *args, **kwargs):
        """Gelman-Rubin (eigenvalues and diagonal) across the chains, each split in ``nsplits`` (as HMCSampler.check)."""
        from .hmc import HMCSampler
        return HMCSampler.check(self, *args, **kwargs)

    def save(self, fn=None):
        """One file per chain in the reference's checkpoint format; attributes ``{'sampler': 'nuts', 'hyp': ...}`` and the chain's iteration counter ('iteration')."""
        fn = self._save_names(fn)
        if self.chain_rank != 0 or self._store is None: return
        hyp = None if self.hyp is None else {'step_size': self.hyp['step_size'], 'inverse_mass_matrix': np.asarray(self.hyp['inverse_mass_matrix']).tolist()}
        self._write_chains((name, chain, {'sampler': self.name, 'hyp': hyp, 'iteration': int(self._state[2][c]), 'seed': self.counter_seed})
                           for c, (chain, name) in enumerate(zip(self.chains, fn)))

    def _resume(self, sources):
        """Continue the chains saved by :meth:`save`: last points, iteration counters, hyper-parameters (no new warm-up)."""
        files = _open_chain_files(sources)
        names = self.varied_params.names()
        points = np.array([[np.asarray(f.arrays[name], dtype='f8').ravel()[-1] for name in names] for f in files])
        logp = np.array([np.asarray(f.arrays['logposterior'], dtype='f8').ravel()[-1] for f in files])
        iterations = np.array([int(f.attrs.get('iteration', 0)) for f in files], dtype='i8')
        hyp = files[0].attrs.get('hyp', None)
        if hyp is not None:
            self.step_size, self.inverse_mass_matrix = float(hyp['step_size']), np.asarray(hyp['inverse_mass_matrix'], dtype='f8')
            self.hyp = {'step_size': self.step_size, 'inverse_mass_matrix': self.inverse_mass_matrix.copy()}
            self._adapted = True
        if 'seed' in files[0].attrs: self.counter_seed = int(files[0].attrs['seed'])
        self._state = (points, logp, iterations)
