"""Microcanonical Langevin Monte Carlo on batches of chains (the reference's ``MCLMCSampler``, desilike/samplers/mclmc.py, wraps ``blackjax.mclmc`` around one chain;
Robnik, De Luca, Silverstein & Seljak, arXiv:2212.08549).

A chain is a position and a unit momentum; a step is a fixed sequence of exact momentum flows B and drifts A (``isokinetic_leapfrog``: one gradient per step,
``isokinetic_mclachlan``: two) followed by a partial refresh of the momentum.  There is no accept / reject, no tree and no variable trajectory length: every
gradient row of a batch is used (csrc/dl_mclmc.h states the algorithm, the rule for a step that leaves the support and the random draws).

* :class:`_DeviceMCLMC` runs the chains on the GPU (``dl_mclmc_*``: one gradient batch + one fused kernel per stage);
* :class:`_HostMCLMC` is the NumPy statement of the same stage machine, with the same counter-based draws, around an injected
  ``(logposterior, gradient) = f(q [C, P])``: likelihoods without a device context, and the yardstick of the device engine in the tests.

Coordinates: as the reference, the chains move in ``(theta - param.value) / param.proposal``; the preconditioner A acts on those, so ``L`` and ``step_size`` mean what
they mean there (the engines are given diag(proposal) A and never see the centring).  Warm-up as ``blackjax.mclmc_find_L_and_step_size``, per chain and pooled:
:meth:`MCLMCSampler._warmup`."""
import numpy as np

from .nuts import NUTSSampler, _Draws
from .samplers import CounterRNG, _DeviceEngine, _open_chain_files

STREAM_REFRESH, STREAM_INIT = 48, 49
INFO_FIELDS = ('energy_change', 'undone', 'step_size')
INTEGRATORS = {'isokinetic_leapfrog': ((0.5, 0.5), (1.,)),
               'isokinetic_mclachlan': ((0.1931833275037836, 1. - 2. * 0.1931833275037836, 0.1931833275037836), (0.5, 0.5))}      # (B coefficients, A coefficients)


class _MclmcDraws(_Draws):
    """The draws of csrc/dl_mclmc.h: Philox4x32-10 keyed by ``seed``, counter (step lo, step hi, chain id, stream | pair << 8)."""

    def gauss(self, it, chain, P, stream):
        it, chain = np.asarray(it, dtype='i8'), np.asarray(chain)
        z = np.empty((len(it), P + (P & 1)))
        for j in range((P + 1) // 2):
            z[:, 2 * j], z[:, 2 * j + 1] = CounterRNG.box_muller(self._words(it, chain, np.full(len(it), stream | (j << 8), dtype=np.uint32)))
        return z[:, :P]


def _dot(a, b):
    """Row-wise a . b, the components summed in order (the host build of csrc/dl_mclmc.h sums them so)."""
    s = np.zeros(a.shape[0])
    for j in range(a.shape[1]): s = s + a[:, j] * b[:, j]
    return s


def _matvec(A, x):
    """Rows of x times A^T, the columns accumulated in order (dl_nuts_matvec)."""
    out = np.zeros_like(x)
    for k in range(A.shape[1]): out = out + A[:, k][None, :] * x[:, k][:, None]
    return out


def _normalise(u):
    n = np.sqrt(_dot(u, u))
    ok = (n > 0.) & (n < np.inf)
    out = u.copy()
    out[ok] = u[ok] / n[ok][:, None]
    return out


class _HostMCLMC(object):
    """NumPy statement of the device engine's stage machine (csrc/dl_mclmc.h, same record, same draws), around ``f(q [C, P]) -> (logposterior [C], gradient [C, P])``."""
    device_resident = False

    def __init__(self, f, nchains, n_params, chain_ids=None, integrator='isokinetic_mclachlan', seed=0, offset=0.):
        if integrator not in INTEGRATORS: raise ValueError('integrator must be one of {}, found {!r}'.format(sorted(INTEGRATORS), integrator))
        self.f, self.C, self.P = f, int(nchains), int(n_params)
        if not 2 <= self.P <= 64: raise ValueError('the sampler takes 2 .. 64 parameters (one parameter has no isokinetic dynamics: d - 1 = 0), found {:d}'.format(self.P))
        if self.C < 1: raise ValueError('nchains must be >= 1')
        self.cb, self.ca = INTEGRATORS[integrator]
        self.chain_ids = np.arange(self.C) if chain_ids is None else np.asarray(chain_ids, dtype='i8')
        self.offset, self.draws = float(offset), _MclmcDraws(seed)
        C, P = self.C, self.P
        self.v = {name: np.zeros((C, P)) for name in ['x', 'g', 'u', 'u0', 'xn', 'sx', 'sxx']}
        self.d = {name: np.zeros(C) for name in ['lp', 'eps', 'epsmax', 'ca', 'cb', 'dk', 'sw']}
        self.i = {name: np.zeros(C, dtype='i8') for name in ['active', 'bad']}
        self.iter = np.zeros(C, dtype='i8')
        self.fac, self.L, self.adapt, self.moments, self.steps = None, 1., False, False, 0
        self.energy_var, self.trust, self.gamma = 5e-4, 1.5, 149. / 151.

    # ---- set-up (dl_mclmc_set_preconditioner / set_hyper / set_state / get_state / set_adaptation / get_moments) ---------------------------------------------------
    def set_preconditioner(self, factor):
        fac = np.array(factor, dtype='f8')
        if fac.ndim == 2: fac = np.tril(fac)
        if not (np.all(np.isfinite(fac)) and np.all((np.diag(fac) if fac.ndim == 2 else fac) > 0.)): raise ValueError('the preconditioner must be finite with a positive diagonal')
        self.fac = fac

    def set_hyper(self, step_size, L):
        if not (step_size > 0. and np.isfinite(step_size)): raise ValueError('step_size must be positive and finite')
        if not L > 0.: raise ValueError('L must be positive (+inf: no refresh)')
        self.d['eps'][:] = step_size
        self.L = float(L)

    def set_state(self, coords, momenta=None, logposterior=None, counters=None):
        coords = np.array(coords, dtype='f8').reshape(self.C, self.P)
        if not np.all(np.isfinite(coords)): raise ValueError('the starting positions must be finite')
        self.iter[:] = 0 if counters is None else np.asarray(counters, dtype='i8')
        if momenta is None:
            u = _normalise(self.draws.gauss(self.iter, self.chain_ids, self.P, STREAM_INIT))
        else:
            u = np.array(momenta, dtype='f8').reshape(self.C, self.P)
            if not np.all(np.abs(_dot(u, u) - 1.) < 1e-6): raise ValueError('the momenta must be unit vectors')
        lp, g = self.f(coords)
        lp = np.asarray(lp, dtype='f8') + self.offset if logposterior is None else np.asarray(logposterior, dtype='f8')
        if not np.all(np.isfinite(lp)): raise ValueError('the log-posterior of a starting position is not finite')
        if not np.all(np.isfinite(g)): raise ValueError('the gradient at a starting position is not finite')
        self.v['x'][...] = coords; self.v['xn'][...] = coords; self.v['g'][...] = g; self.v['u'][...] = u
        self.d['lp'][:] = lp
        self.i['active'][:] = 0; self.i['bad'][:] = 0

    def get_state(self):
        return self.v['x'].copy(), self.v['u'].copy(), self.d['lp'].copy(), self.iter.copy(), self.d['eps'].copy()

    def set_adaptation(self, step_size_on, moments_on=False, desired_energy_var=5e-4, trust_in_estimate=1.5, num_effective_samples=150.):
        if step_size_on:
            self.energy_var, self.trust = float(desired_energy_var), float(trust_in_estimate)
            self.gamma = (num_effective_samples - 1.) / (num_effective_samples + 1.)
            self.d['ca'][:] = 0.; self.d['cb'][:] = 0.; self.d['epsmax'][:] = np.inf
        if moments_on:
            self.v['sx'][...] = 0.; self.v['sxx'][...] = 0.; self.d['sw'][:] = 0.
        self.adapt, self.moments = bool(step_size_on), bool(moments_on)

    def get_moments(self):
        return self.d['sw'].copy(), self.v['sx'].copy(), self.v['sxx'].copy()

    # ---- arithmetic ---------------------------------------------------------------------------------------------------------------------------------------------
    def _apply(self, v, transpose=False):
        if self.fac.ndim == 2: return _matvec(self.fac.T if transpose else self.fac, v)
        return self.fac * v

    def _bstep(self, u, gq, h):
        """B(h) on rows: (new momenta, dK)."""
        t = self._apply(gq, transpose=True)
        n2 = _dot(t, t)
        ok = n2 > 0.
        nrm = np.sqrt(np.where(ok, n2, 1.))
        delta = h * nrm / (self.P - 1)
        eu = _dot(t, u) / nrm
        zeta, m1, m2 = np.exp(-delta), np.expm1(-delta), np.expm1(-2. * delta)
        ce = -m2 + eu * (m1 * m1)
        new = _normalise((2. * zeta)[:, None] * u + (t / nrm[:, None]) * ce[:, None])
        with np.errstate(divide='ignore', invalid='ignore'):
            dk = (self.P - 1) * (delta + np.log1p(0.5 * (1. - eu) * m2))
        return np.where(ok[:, None], new, u), np.where(ok, dk, 0.)

    def _open(self, c, x, u, g, eps):
        if not len(c): return
        self.v['u0'][c] = u
        u, dk = self._bstep(u, g, self.cb[0] * eps)
        self.v['u'][c] = u
        self.v['xn'][c] = x + (self.ca[0] * eps)[:, None] * self._apply(u)
        self.d['dk'][c] = dk
        self.i['bad'][c] = 0; self.i['active'][c] = 1

    def _stage(self, stage, open_next, lp_new, g_new, rec):
        coords, logp, info, count, quota, thin_by = rec
        V, d, I = self.v, self.d, self.i
        if stage < 0:
            rest = count >= quota
            I['active'][rest] = 0
            c = np.nonzero(~rest)[0]
            self._open(c, V['x'][c], V['u'][c], V['g'][c], d['eps'][c])
            return
        c = np.nonzero(I['active'] == 1)[0]
        if not len(c): return
        eps, bad, dk = d['eps'][c], I['bad'][c].astype(bool), d['dk'][c]
        lp = np.asarray(lp_new, dtype='f8')[c]
        g = np.array(g_new, dtype='f8')[c]
        with np.errstate(invalid='ignore'):
            inside = (lp == lp) & (np.abs(lp) < np.inf)
            lp = lp + self.offset
            bad = bad | ~inside | ~np.all(np.abs(g) < np.inf, axis=1)
        u = V['u'][c]
        good = ~bad
        if good.any():
            un, dkn = self._bstep(u[good], g[good], self.cb[stage + 1] * eps[good])
            u[good] = un; dk[good] = dk[good] + dkn
        if stage + 1 < len(self.ca):
            xn = V['x'][c]
            xn[good] = V['xn'][c][good] + (self.ca[stage + 1] * eps[good])[:, None] * self._apply(u[good])
            V['u'][c[good]] = u[good]
            V['xn'][c] = xn
            d['dk'][c] = dk; I['bad'][c] = bad
            return
        # the step is complete
        lp0 = d['lp'][c]
        with np.errstate(invalid='ignore'):
            de = dk - (lp - lp0)
            bad = bad | ~(np.abs(de) < np.inf)
        good = ~bad
        x = np.where(bad[:, None], V['x'][c], V['xn'][c])
        g = np.where(bad[:, None], V['g'][c], g)
        u = np.where(bad[:, None], -V['u0'][c], u)
        lp, de = np.where(bad, lp0, lp), np.where(bad, 0., de)
        V['x'][c], V['g'][c] = x, g
        it = self.iter[c]
        if self.L < np.inf:
            nu = np.sqrt(np.expm1(2. * eps / self.L) / self.P)
            u = _normalise(u + nu[:, None] * self.draws.gauss(it, self.chain_ids[c], self.P, STREAM_REFRESH))
        V['u'][c] = u
        eps_next = eps.copy()
        if self.adapt:
            epsmax, ca, cb = d['epsmax'][c], d['ca'][c], d['cb'][c]
            eps_next[bad] = 0.8 * eps[bad]; epsmax[bad] = eps_next[bad]
            xi = de * de / (self.P * self.energy_var) + 1e-8
            r = np.log(xi) / (6. * self.trust)
            w, e2 = np.exp(-0.5 * r * r), eps * eps
            ca[good] = (self.gamma * ca + w * (xi / (e2 * e2 * e2)))[good]
            cb[good] = (self.gamma * cb + w)[good]
            with np.errstate(divide='ignore', invalid='ignore'):
                e = (ca / cb) ** (-1. / 6.)
            take = good & (e > 0.) & (e < np.inf)
            eps_next[take] = e[take]
            cap = good & (eps_next > epsmax)
            eps_next[cap] = epsmax[cap]
            d['eps'][c], d['epsmax'][c], d['ca'][c], d['cb'][c] = eps_next, epsmax, ca, cb
        if self.moments:
            cg = c[good]
            V['sx'][cg] += eps[good][:, None] * x[good]
            V['sxx'][cg] += eps[good][:, None] * (x[good] * x[good])
            d['sw'][cg] = d['sw'][cg] + eps[good]
        r = (it + 1) % thin_by == 0
        cr, slot = c[r], count[c[r]]
        coords[cr, slot], logp[cr, slot] = x[r], lp[r]
        info[cr, slot] = np.column_stack([de[r], bad[r].astype('f8'), eps[r]])
        count[cr] += 1
        d['lp'][c] = lp
        self.iter[c] = it + 1
        nxt = (count[c] < quota) if open_next else np.zeros(len(c), dtype=bool)
        I['active'][c[~nxt]] = 0
        self._open(c[nxt], x[nxt], u[nxt], g[nxt], eps_next[nxt])

    # ---- a batch ------------------------------------------------------------------------------------------------------------------------------------------------
    def buffers(self, quota):
        return (np.zeros((self.C, quota, self.P)), np.zeros((self.C, quota)), np.zeros((self.C, quota, 3)), np.zeros(self.C, dtype='i8'))

    def run(self, nsteps, quota, buffers, thin_by=1):
        """``nsteps`` integrator steps of every chain into ``buffers`` (the semantics of dl_mclmc_run)."""
        nsteps = int(nsteps)
        if not nsteps: return
        rec = tuple(buffers) + (int(quota), int(thin_by))
        self._stage(-1, False, None, None, rec)
        for s in range(nsteps):
            for stage in range(len(self.ca)):
                lp, g = self.f(self.v['xn'].copy())
                self._stage(stage, s + 1 < nsteps, lp, g, rec)
        self.steps += nsteps

    def counts(self, buffers):
        return np.asarray(buffers[3])

    def records(self, buffers):
        return tuple(np.asarray(b) for b in buffers[:3])


class _DeviceMCLMC(_DeviceEngine):
    """Chains of this rank resident on the GPU (``dl_mclmc_*``): the calls of :class:`_HostMCLMC` go to the owner ``mclmc``."""
    _counters = ('steps',)

    def __init__(self, ctx, offset, chain_ids, integrator, seed, gradient, fd_delta, fd_limits):
        from ._lib import DeviceMCLMC
        self.mclmc = self._owner = DeviceMCLMC(ctx, len(chain_ids), chain_ids=chain_ids, integrator=integrator, seed=seed, offset=offset, gradient=gradient,
                                               fd_delta=fd_delta, fd_limits=fd_limits)
        self.C, self.P = len(chain_ids), self.mclmc.n_params


def run_batch(engine, quota, thin_by=1, chunk=64):
    """Chunks of at most ``chunk`` steps until every chain has ``quota`` records: (coords [C, quota, P], logposterior [C, quota], info [C, quota, 3])."""
    buffers = engine.buffers(quota)
    left = quota
    while left > 0:
        engine.run(min(int(chunk), left * thin_by), quota, buffers, thin_by=thin_by)
        left = quota - int(np.min(engine.counts(buffers)))
    return engine.records(buffers)


class MCLMCSampler(NUTSSampler):
    """``MCLMCSampler(likelihood, chains=64, adaptation=True, L=1., step_size=0.1, integrator='isokinetic_mclachlan', gradient='auto', seed=None, save_fn=None,
    device_resident=None, chunk=64)``: the arguments of the reference's sampler (samplers/mclmc.py:20-71) and those :class:`~desilike_amd.nuts.NUTSSampler` adds, whose
    bookkeeping of chains (ranks, files, convergence checks) this class shares; ``run(min_iterations, max_iterations, check_every, check, thin_by, start)``.

    adaptation : ``True`` / dict (the reference's keys ``niterations`` default 1000, ``frac_tune1``, ``frac_tune2``, ``frac_tune3`` 0.1 each, ``desired_energy_var`` 5e-4,
        ``trust_in_estimate`` 1.5, ``num_effective_samples`` 150, ``diagonal_preconditioning`` True; ours: ``dense_preconditioning`` False, ``initial_step_size``) /
        ``False`` (``L`` and ``step_size`` as given, no preconditioner).
    L, step_size : momentum decoherence length and step size, in the coordinates ``(theta - param.value) / param.proposal`` (then preconditioned).
    chains : number of chains, or the chain files written by :meth:`save` (one per chain): the saved chains are continued (last points, momenta, step counters,
        hyper-parameters; no new warm-up).
    chunk : steps enqueued between two reads of the record counts."""
    name = 'mclmc'

    def __init__(self, likelihood, chains=64, adaptation=True, L=1., step_size=0.1, integrator='isokinetic_mclachlan', gradient='auto', seed=None, save_fn=None,
                 device_resident=None, chunk=64, **kwargs):
        if integrator not in INTEGRATORS: raise ValueError('integrator must be one of {}, found {!r}'.format(sorted(INTEGRATORS), integrator))
        if not step_size > 0.: raise ValueError('step_size must be positive')
        if not L > 0.: raise ValueError('L must be positive')
        self._momenta = None             # [nchains, ndim] where the chains are continued
        self.mclmc_integrator, self.L, self.preconditioner = integrator, float(L), None
        super(MCLMCSampler, self).__init__(likelihood, chains=chains, adaptation=adaptation, step_size=step_size, gradient=gradient, seed=seed, save_fn=save_fn,
                                           device_resident=device_resident, chunk=chunk, **kwargs)
        P = len(self.varied_params)
        if P < 2: raise ValueError('MCLMC needs at least two varied parameters: with one, the isokinetic dynamics do not exist (d - 1 = 0)')
        if P > 64: raise ValueError('MCLMCSampler takes at most 64 varied parameters, found {:d}'.format(P))
        self.scale = np.array([param.proposal for param in self.varied_params], dtype='f8')
        if not (np.all(np.isfinite(self.scale)) and np.all(self.scale > 0.)): raise ValueError('every varied parameter needs a positive proposal scale')
        if self.preconditioner is None: self.preconditioner = np.ones(P)
        self.energy_var = None

    # ---- engines ------------------------------------------------------------------------------------------------------------------------------------------------
    def _make_engine(self):
        local = np.array(self.local_chains(), dtype='i8')
        if self.device_resident:
            ctx, offset = self.likelihood._get_posterior_context()
            delta, limits = self._fd_tables()
            return _DeviceMCLMC(ctx, offset, local, self.mclmc_integrator, self.counter_seed, self.gradient, delta, limits)
        if self.gradient == 'analytic': raise NotImplementedError('the host engine differentiates numerically: use gradient="auto" or "finite"')
        return _HostMCLMC(self._host_value_and_grad, len(local), len(self.varied_params), chain_ids=local, integrator=self.mclmc_integrator, seed=self.counter_seed)

    def _factor(self):
        """diag(proposal) A: the preconditioner in the parameters' own coordinates, as the engines take it."""
        A = np.asarray(self.preconditioner, dtype='f8')
        return self.scale * A if A.ndim == 1 else self.scale[:, None] * A

    # ---- warm-up ------------------------------------------------------------------------------------------------------------------------------------------------
    def _warmup(self, engine):
        """``blackjax.mclmc_find_L_and_step_size`` on every chain at once.  Phase 1 (``frac_tune1``): the energy-variance controller alone, from L = sqrt(d) and
        step size sqrt(d) / 4.  Phase 2 (``frac_tune2``): the controller and the moments; then the preconditioner from the variances (``diagonal_preconditioning``)
        or the covariance (``dense_preconditioning``) pooled over all chains and ranks, L = sqrt(d), and a third as many steps of the controller alone (without
        preconditioning: L = sqrt(sum of the variances)).  Step size: exp(mean over chains of log eps).  Phase 3 (``frac_tune3``): a recorded run at that step size;
        L = 0.4 eps / mean_i(1 / tau_i), tau_i the integrated autocorrelation time of whitened component i averaged over chains."""
        from .diagnostics import integrated_autocorrelation_time
        a = self.adaptation
        P = len(self.varied_params)
        niterations = int(a.get('niterations', 1000))
        n1, n2, n3 = (int(round(niterations * float(a.get(name, 0.1)))) for name in ['frac_tune1', 'frac_tune2', 'frac_tune3'])
        control = dict(desired_energy_var=float(a.get('desired_energy_var', 5e-4)), trust_in_estimate=float(a.get('trust_in_estimate', 1.5)),
                       num_effective_samples=float(a.get('num_effective_samples', 150)))
        diagonal, dense = bool(a.get('diagonal_preconditioning', True)), bool(a.get('dense_preconditioning', False))
        self.L = np.sqrt(P)
        engine.set_preconditioner(self._factor())
        engine.set_hyper(float(a.get('initial_step_size', 0.25 * np.sqrt(P))), self.L)

        def pooled_step_size():
            eps = self._gather([engine.get_state()[4][:, None]])[0][:, 0]
            return float(np.exp(np.mean(np.log(eps))))

        if n1 > 0:
            engine.set_adaptation(True, False, **control)
            run_batch(engine, n1, chunk=self.chunk)
        if n2 > 0:
            engine.set_adaptation(True, True, **control)
            coords, _, info = run_batch(engine, n2, chunk=self.chunk)
            sw, sx, sxx = self._gather([m if m.ndim > 1 else m[:, None] for m in engine.get_moments()])
            total = sw.sum()
            if total > 0.:
                mean = sx.sum(axis=0) / total
                var = (sxx.sum(axis=0) / total - mean**2) / self.scale**2
                if dense:
                    coords, info = self._gather([coords, info])
                    w = (info[..., 2] * (info[..., 1] == 0)).ravel()
                    y = (coords.reshape(-1, P) - mean) / self.scale
                    cov = (y * w[:, None]).T @ y / w.sum()
                    try:
                        self.preconditioner, self.L = np.linalg.cholesky(cov), np.sqrt(P)
                    except np.linalg.LinAlgError:
                        dense = False
                if not dense and np.all(np.isfinite(var)) and np.all(var > 0.):
                    if diagonal: self.preconditioner, self.L = np.sqrt(var), np.sqrt(P)
                    else: self.L = float(np.sqrt(var.sum()))
            engine.set_preconditioner(self._factor())
            engine.set_hyper(pooled_step_size(), self.L)
            if (dense or diagonal) and n2 // 3 > 0:
                engine.set_adaptation(True, False, **control)
                run_batch(engine, n2 // 3, chunk=self.chunk)
        if n1 > 0 or n2 > 0: self.step_size = pooled_step_size()
        engine.set_adaptation(False, False)
        engine.set_hyper(self.step_size, self.L)
        if n3 > 1:
            coords = self._gather([run_batch(engine, n3, chunk=self.chunk)[0]])[0]
            A = self._factor()
            y = coords / A if A.ndim == 1 else np.linalg.solve(A, coords.reshape(-1, P).T).T.reshape(coords.shape)
            with np.errstate(invalid='ignore', divide='ignore'):
                tau = integrated_autocorrelation_time(y)
                L = 0.4 * self.step_size / np.mean(1. / tau)
            if np.all(np.isfinite(tau)) and np.all(tau > 0.) and np.isfinite(L) and L > 0.: self.L = float(L)
        self.energy_var = control['desired_energy_var']
        self._adapted = True

    def _hyp(self):
        A = np.asarray(self.preconditioner, dtype='f8').copy()
        return {'step_size': self.step_size, 'L': self.L, 'sqrt_diag_cov' if A.ndim == 1 else 'factor': A}

    # ---- batches ------------------------------------------------------------------------------------------------------------------------------------------------
    def _run_batch(self, niterations, thin_by=1):
        local = self.local_chains()
        if self._engine is None:
            self._engine = self._make_engine()
            points, logp, counters = self._state
            self._engine.set_preconditioner(self._factor())
            self._engine.set_hyper(self.step_size, self.L)
            self._engine.set_state(points[local], momenta=None if self._momenta is None else self._momenta[local], logposterior=None if logp is None else logp[local],
                                   counters=counters[local])
            if not self._adapted:
                self._warmup(self._engine)
            self._engine.set_adaptation(False, False)
            self._engine.set_preconditioner(self._factor())
            self._engine.set_hyper(self.step_size, self.L)
            self.hyp = self._hyp()
        nrec = niterations // thin_by
        if not nrec: return
        coords, logp, info = run_batch(self._engine, nrec, thin_by=thin_by, chunk=self.chunk)
        points, momenta, lps, counters, _ = self._engine.get_state()
        coords, logp, info, points, momenta, lps, counters = self._gather([coords, logp, info, points, momenta, lps, counters])
        self._state, self._momenta = (points, lps, counters), momenta
        batch = (coords.transpose(1, 0, 2), logp.T, info.transpose(1, 0, 2))
        self._store = batch if self._store is None else tuple(np.concatenate([s, b]) for s, b in zip(self._store, batch))

    def run(self, *args, **kwargs):
        """Batches of ``check_every`` steps of every chain until :meth:`check` passes or ``max_iterations``.  Returns the list of chains."""
        if kwargs.get('start', None) is not None: self._momenta = None
        return super(MCLMCSampler, self).run(*args, **kwargs)

    # ---- outputs ------------------------------------------------------------------------------------------------------------------------------------------------
    def _info(self, field):
        if self._store is None: return np.zeros(self.nchains)
        return self._store[2][..., INFO_FIELDS.index(field)]

    @property
    def undone_steps(self):
        """Per chain: number of recorded steps that left the support and were undone."""
        return (self._info('undone') > 0).sum(axis=0).astype('i8') if self._store is not None else np.zeros(self.nchains, dtype='i8')

    @property
    def energy_change(self):
        """Energy change of every recorded step [n, nchains] (0 for an undone step)."""
        return self._info('energy_change')

    @property
    def acceptance_rate(self):
        """Per chain: fraction of the recorded steps that were kept (there is no accept / reject: a step is undone only where it leaves the support)."""
        return 1. - self._info('undone').mean(axis=0) if self._store is not None else np.zeros(self.nchains)

    divergences = undone_steps

    def _not_here(self):
        raise AttributeError('MCLMC has no tree and no energy threshold: see undone_steps and energy_change')

    energy_divergences = mean_tree_depth = property(_not_here)

    def save(self, fn=None):
        """One file per chain in the reference's checkpoint format; attributes ``{'sampler': 'mclmc', 'hyp': ...}``, the chain's step counter ('iteration') and
        its momentum."""
        fn = self._save_names(fn)
        if self.chain_rank != 0 or self._store is None: return
        hyp = None if self.hyp is None else {name: (value.tolist() if isinstance(value, np.ndarray) else value) for name, value in self.hyp.items()}
        self._write_chains((name, chain, {'sampler': self.name, 'hyp': hyp, 'integrator': self.mclmc_integrator, 'iteration': int(self._state[2][c]), 'seed': self.counter_seed,
                                          'momentum': self._momenta[c].tolist()}) for c, (chain, name) in enumerate(zip(self.chains, fn)))

    def _resume(self, sources):
        """Continue the chains saved by :meth:`save`: last points, momenta, step counters, hyper-parameters (no new warm-up)."""
        files = _open_chain_files(sources)
        names = self.varied_params.names()
        points = np.array([[np.asarray(f.arrays[name], dtype='f8').ravel()[-1] for name in names] for f in files])
        logp = np.array([np.asarray(f.arrays['logposterior'], dtype='f8').ravel()[-1] for f in files])
        counters = np.array([int(f.attrs.get('iteration', 0)) for f in files], dtype='i8')
        if all('momentum' in f.attrs for f in files): self._momenta = np.array([f.attrs['momentum'] for f in files], dtype='f8')
        hyp = files[0].attrs.get('hyp', None)
        if hyp is not None:
            self.step_size, self.L = float(hyp['step_size']), float(hyp['L'])
            self.preconditioner = np.asarray(hyp['sqrt_diag_cov'] if 'sqrt_diag_cov' in hyp else hyp['factor'], dtype='f8')
            self._adapted = True
        if 'integrator' in files[0].attrs: self.mclmc_integrator = files[0].attrs['integrator']
        if 'seed' in files[0].attrs: self.counter_seed = int(files[0].attrs['seed'])
        self._state = (points, logp, counters)
