"""Tempered sequential Monte Carlo (desilike_amd/smc.py) on the CPU: the host build of the device arithmetic (csrc/dl_smc.h via tests/csrc/emulate_smc.cpp, also as a
stand-alone program under the sanitizers) against the NumPy statement, the invariants of the stage machine, log-evidences with closed forms, errors and resume."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from emulation import SANITIZE_FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'csrc', 'emulate_smc.cpp')
DEPS = [SRC] + [os.path.join(HERE, '..', 'desilike_amd', 'csrc', name) for name in ['dl_smc.h', 'dl_nuts.h', 'dl_philox.h']]
_lib = []


def _stale(target):
    return not os.path.isfile(target) or any(os.path.getmtime(dep) > os.path.getmtime(target) for dep in DEPS)


def _emulation():
    if _lib: return _lib[0]
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, 'libdl_emulate_smc.so')
    if _stale(so): subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', so, SRC])
    lib = ctypes.CDLL(so)
    p, i32, f8 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    lib.emu_smc_temper.argtypes = [p, i32, f8, f8, p, p]
    lib.emu_smc_moments.argtypes = [p, p, i32, i32, p, p]
    lib.emu_smc_factor.argtypes = [p, p, i32, p]
    lib.emu_smc_resample.argtypes = [p, i32, ctypes.c_longlong, i32, ctypes.c_uint64, p, p, p]
    lib.emu_smc_propose.argtypes = [p, f8, p, i32, i32, ctypes.c_longlong, i32, i32, ctypes.c_uint64, p]
    lib.emu_smc_accept.argtypes = [f8, p, p, p, p, p, i32, ctypes.c_longlong, i32, i32, ctypes.c_uint64, p, p, p]
    lib.emu_smc_next_scale.argtypes, lib.emu_smc_next_scale.restype = [f8, f8, f8], f8
    _lib.append(lib)
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _close(a, b):
    a, b = np.asarray(a, dtype='f8'), np.asarray(b, dtype='f8')
    assert np.allclose(a, b, rtol=1e-10, atol=1e-8), float(np.max(np.abs(a - b)))      # (the bounds of tests/test_gpu_mclmc.py::_compare)


# ---- 1. host build of the device arithmetic ---------------------------------------------------------------------------------------------------------------------
def _particles(N, P, edge, seed=3):
    """Particles x [N, P] and log-likelihoods of a correlated Gaussian; edge 'dead': a third of the L are -inf; 'equal': those, and all live L equal; 'shared': all
    particles share the last coordinate."""
    rng = np.random.RandomState(seed + 7 * N + P)
    mix = np.eye(P) + 0.3 * np.tril(rng.standard_normal((P, P)), -1)
    x = rng.standard_normal((N, P)) @ mix.T + rng.standard_normal(P)
    if edge == 'shared': x[:, -1] = 0.25
    L = -0.5 * (rng.standard_normal((N, P))**2).sum(axis=1) * 40. / P
    if edge == 'equal': L[:] = -1.5
    if edge in ('dead', 'equal'): L[::3] = -np.inf
    return np.ascontiguousarray(x), L


@pytest.mark.parametrize('edge', ['none', 'dead', 'equal', 'shared'])
@pytest.mark.parametrize('P', [1, 2, 15, 64])
@pytest.mark.parametrize('N', [64, 320, 16384])
def test_host_build_equals_the_numpy_statement(N, P, edge):
    from desilike_amd import smc
    lib, seed, it, sys = _emulation(), 2024, 5, 3
    x, L = _particles(N, P, edge)
    beta = 0.125
    # the temperature bisection and the evidence
    out, W = np.zeros(6), np.zeros(N)
    assert lib.emu_smc_temper(_ptr(L), N, beta, 0.5, _ptr(out), _ptr(W)) == 0
    level = smc.temper(L, beta, 0.5)
    _close(out, [level[name] for name in ['delta', 'lmax', 'sumw', 'ess', 'beta', 'dlogz']])
    live = np.isfinite(L)
    if edge == 'equal': assert out[4] == 1. and level['beta'] == 1. and out[3] == live.sum() == level['ess']       # ESS(1) = the live count
    else: assert 0. < out[0] < 1. - beta and abs(out[3] - 0.5 * N) < 1e-9 * N
    Wh = smc.weights(L, level['lmax'], level['delta'], level['sumw'])
    _close(W, Wh)
    assert np.all(W[~live] == 0.) and np.all(Wh[~live] == 0.)
    # the moments and the factor with its fallbacks
    mean, cov, C, widths = np.zeros(P), np.zeros((P, P)), np.zeros((P, P)), np.linspace(2., 3., P)
    assert lib.emu_smc_moments(_ptr(x), _ptr(W), N, P, _ptr(mean), _ptr(cov)) == 0
    mh, ch = smc.moments(x, Wh)
    _close(mean, mh); _close(cov, ch)
    assert lib.emu_smc_factor(_ptr(cov), _ptr(widths), P, _ptr(C)) == 0
    Ch = smc.factor(ch, widths)
    _close(C, Ch)
    singular = edge == 'shared' or N <= P        # all particles share a coordinate; or fewer particles than dimensions: what is left of a pivot is rounding error
    if singular:      # the diagonal fallback, and the prior's width for a component without variance
        assert np.count_nonzero(C - np.diag(np.diag(C))) == 0
        if edge == 'shared': assert cov[-1, -1] == 0. and ch[-1, -1] == 0. and C[-1, -1] == widths[-1]
        keep = slice(None, -1 if edge == 'shared' else None)
        _close(np.diag(C)[keep], np.sqrt(np.diag(ch)[keep]))
    else: _close(C @ C.T, ch + np.tril(ch, -1).T)
    # the scan with the ancestor search
    cum, anc, u = np.zeros(N), np.zeros(N, dtype='i4'), np.zeros(1)
    assert lib.emu_smc_resample(_ptr(W), N, it, sys, seed, _ptr(cum), _ptr(anc), _ptr(u)) == 0
    draws = smc._SmcDraws(seed)
    uh = draws.resample_uniform(it, sys)
    assert u[0] == uh and 0. < uh <= 1.
    # decisions exact: the statement's prefix sums are taken in the kernel's order (slice, group, top), so on the same weights they are the same bits
    ah, margins = smc.ancestors(W, uh)
    assert np.array_equal(cum, smc.prefix_sums(W)) and np.array_equal(anc, ah)
    assert np.allclose(cum, np.cumsum(Wh), rtol=1e-10, atol=1e-8) and np.all(np.diff(cum) >= -4e-16) and np.all(W[anc] > 0.)      # (across two threads' slices the sums may step back by an ulp)
    awh = smc.ancestors(Wh, uh)[0]            # the statement's own weights differ from the host build's by the rounding of exp: searches with a margin above it agree
    assert np.array_equal(anc[margins > 1e-12], awh[margins > 1e-12])
    # the proposal and the Metropolis test
    prop = np.zeros((N, P))
    assert lib.emu_smc_propose(_ptr(C), 0.7, _ptr(x), N, P, it, 2, sys, seed, _ptr(prop)) == 0
    z = draws.gauss(it, 2, sys, N, P)
    _close(prop, x + (0.7 * (2.38 / np.sqrt(float(P)))) * smc._matvec(Ch, z))
    assert abs(z.mean()) < 5. / np.sqrt(N * P) and abs(z.std() - 1.) < 5. / np.sqrt(N * P)
    rng = np.random.RandomState(1)
    pi, Lp, pip = rng.standard_normal(N), L[rng.permutation(N)] + 0.3 * rng.standard_normal(N), rng.standard_normal(N)
    status = (rng.uniform(size=N) < 0.1).astype('i4')
    pip[status == 1] = -np.inf
    Lp[::11] = np.nan
    flags, logu, nacc = np.zeros(N, dtype='u1'), np.zeros(N), np.zeros(1, dtype='i4')
    assert lib.emu_smc_accept(0.4, _ptr(L), _ptr(pi), _ptr(Lp), _ptr(pip), _ptr(status), N, it, 2, sys, seed, _ptr(flags), _ptr(logu), _ptr(nacc)) == 0
    lh = draws.log_uniform(it, 2, sys, N)
    _close(logu, lh)
    ok = np.isfinite(Lp) & np.isfinite(pip) & (status == 0)
    with np.errstate(invalid='ignore'):
        ratio = 0.4 * (np.where(ok, Lp, 0.) - L) + (np.where(ok, pip, 0.) - pi)
        expected = ok & (lh < ratio)
    assert np.min(np.abs(lh - ratio)[ok]) > 1e-12 and np.array_equal(flags.astype(bool), expected) and nacc[0] == expected.sum() and 0 < nacc[0] < N
    for a in (0., 0.234, 1.): assert np.isclose(lib.emu_smc_next_scale(1.3, a, 0.234), smc.next_scale(1.3, a, 0.234), rtol=1e-14)
    assert lib.emu_smc_next_scale(999., 1., 0.234) == 1e3 and lib.emu_smc_next_scale(1.001e-3, 0., 0.234) == 1e-3


def test_host_build_under_the_sanitizers():
    """tests/csrc/emulate_smc.cpp with -DEMU_SMC_MAIN: a stand-alone program (every phase, every shape and edge input above) built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run directly."""
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, 'emulate_smc_main')
    if _stale(exe): subprocess.check_call(['g++', '-O1', '-std=c++17', '-DEMU_SMC_MAIN'] + SANITIZE_FLAGS + ['-o', exe, SRC])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert done.returncode == 0 and 'emulate_smc: ok' in done.stdout and 'runtime error' not in done.stdout and 'Sanitizer' not in done.stdout, done.stdout


# ---- 2. invariants of the stage machine --------------------------------------------------------------------------------------------------------------------------
MEAN, SIGMA = np.array([0.4, -0.2]), np.array([0.1, 0.25])


def _gauss2(x):
    """Gaussian likelihood in a uniform box [-2, 2]^2: (loglike, logprior)."""
    inside = np.all(np.abs(x) < 2., axis=1)
    return -0.5 * (((x - MEAN) / SIGMA)**2).sum(axis=1), np.where(inside, -np.log(16.), -np.inf)


def _host(K=2, N=256, seed=9, ids=None, n_steps=3):
    from desilike_amd.smc import _HostSMC
    host = _HostSMC(_gauss2, K, N, 2, [4., 4.], system_ids=ids, seed=seed)
    host.set_hyper(0.5, n_steps, 0.234)
    host.set_particles(np.random.RandomState(4).uniform(-2., 2., (K, N, 2)))
    return host


def test_invariants_of_the_host_statement():
    from desilike_amd.smc import run_batch, ancestors
    host = _host()
    history, coords, logp, counts = run_batch(host, 14)
    beta = history[..., 0]
    for k in range(2):
        T = int(np.argmax(beta[k] >= 1.)) + 1
        assert np.all(np.diff(np.concatenate([[0.], beta[k, :T]])) > 0.) and beta[k, T - 1] == 1. and np.all(beta[k, T:] == 1.)       # strictly increasing, then exactly 1
        assert np.allclose(history[k, :T - 1, 2], 0.5 * 256, rtol=1e-9, atol=0.) and np.all(history[k, T:, 2] == 256.)
        assert history[k, T - 1, 2] >= 0.5 * 256 and np.all(history[k, T:, 1] == history[k, T - 1, 1])     # logZ stays once beta = 1
        assert counts[k, 0] == 14 and counts[k, 1] == 14 - T and 3 < T < 12
        assert np.all(np.abs(coords[k, :counts[k, 1]]) < 2.) and np.all(np.isfinite(logp[k, :counts[k, 1]]))
    assert np.all((history[..., 3] > 0.05) & (history[..., 3] < 0.9)) and np.all((history[..., 4] >= 1e-3) & (history[..., 4] <= 1e3))
    assert np.isfinite(host.min_margin) and host.ndecisions > 2 * 14 * 3 * 256 // 2
    # systematic resampling: floor(N W_i) or ceil(N W_i) copies, exactly
    rng = np.random.RandomState(0)
    for N in (64, 320):
        W = rng.exponential(size=N)**3
        W[::5] = 0.
        W /= W.sum()
        for u in (1e-9, 0.3, 1.):
            copies = np.bincount(ancestors(W, u)[0], minlength=N)
            assert copies.sum() == N and np.all((copies == np.floor(N * W)) | (copies == np.ceil(N * W)))


def test_chunking_and_system_ids():
    from desilike_amd.smc import run_batch
    runs = [run_batch(_host(), 9, chunk=chunk) for chunk in (None, 4, 1)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other): assert np.array_equal(a, b)
    # a system is its id: system 1 of a pair is the one-system run with id 1; another id draws differently
    pair, single, other = _host(), _host(K=1, ids=[1]), _host(K=1, ids=[5])
    start = pair.get_state()[0]
    for engine in (single, other): engine.set_particles(start[1:])
    hp, hs, ho = run_batch(pair, 5)[0], run_batch(single, 5)[0], run_batch(other, 5)[0]
    assert np.array_equal(hp[1], hs[0]) and not np.array_equal(hs[0, :, 3], ho[0, :, 3])
    for a, b in zip(pair.get_state(), single.get_state()): assert np.array_equal(a[1:], b)
    # a state round trip continues bit for bit
    resumed = _host()
    resumed.set_state(*_host_after(4).get_state())
    assert np.array_equal(run_batch(resumed, 5)[0], runs[0][0][:, 4:])


def _host_after(niterations):
    from desilike_amd.smc import run_batch
    host = _host()
    run_batch(host, niterations)
    return host


# ---- 3. closed-form evidences ----------------------------------------------------------------------------------------------------------------------------------
class ToyLikelihood(object):
    """Minimal object with the likelihood surface the samplers use (varied_params, _param_*, _evaluate_dict) around ``loglike(x [B, P])``."""

    def __init__(self, loglike, priors):
        from desilike_amd.parameter import Parameter, ParameterCollection
        self.varied_params = ParameterCollection([Parameter('p{:d}'.format(i), prior=prior) for i, prior in enumerate(priors)])
        self.loglike = loglike
        self._param_loglikelihood, self._param_logprior = Parameter('loglikelihood', derived=True), Parameter('logprior', derived=True)

    def _evaluate_dict(self, flat, shape, errors='raise', return_derived=False):
        from desilike_amd.parameter import Samples
        x = np.column_stack([flat[param.name] for param in self.varied_params])
        loglike = self.loglike(x)
        logprior = sum(param.prior(flat[param.name]) for param in self.varied_params)
        derived = Samples()
        derived[self._param_loglikelihood], derived[self._param_logprior] = loglike.reshape(shape), logprior.reshape(shape)
        return ((loglike + logprior).reshape(shape), derived), {}


D4_MEAN, D4_SIGMA = np.array([0.5, -0.3, 0.2, 0.8]), np.array([0.3, 0.5, 0.2, 0.4])


def _loglike4(x):
    return -0.5 * (((x - D4_MEAN) / D4_SIGMA)**2).sum(axis=1) - np.log(D4_SIGMA).sum() - 2. * np.log(2. * np.pi)       # a normalised Gaussian in d = 4


def _assert_evidence(sampler, exact):
    K, N = sampler.nchains, sampler.nparticles
    T = int(sampler.nlevels.max())
    print('logz_mean {:.4f} exact {:.4f} logz_std {:.4f} bound {:.4f} T {:d} evaluations {:d}'.format(sampler.logz_mean, exact, sampler.logz_std, 2. * np.sqrt(T / N), T,
                                                                                                       sampler.nevaluations))
    # var(log Z^) ~ T (N / ESS - 1) / N = T / N at ess_fraction = 0.5: a noisy sampler cannot pass by being noisy
    assert sampler.logz_std <= 2. * np.sqrt(T / N)
    assert abs(sampler.logz_mean - exact) <= 4. * sampler.logz_std / np.sqrt(K)


def test_evidence_gaussian_with_gaussian_priors():
    """Normalised Gaussian likelihood N(x; mu, diag(sigma^2)) in d = 4 under priors N(0, 2^2): Z = prod_i N(mu_i; 0, sigma_i^2 + 4).
    Achieved here (K = 8, N = 1024, seed 1): logz_mean -6.6397 against -6.6374, logz_std 0.096 against the bound 0.140 (T = 5 levels); over seeds 1 .. 4 the deviation
    is -0.7 .. 1.0 standard errors and logz_std 0.096 .. 0.136: the sweeps of a level do not decorrelate the copies of a resampled particle completely, the scatter is
    1.4 .. 1.9 sqrt(T / N)."""
    from desilike_amd.samplers import SMCSampler
    like = ToyLikelihood(_loglike4, [dict(dist='norm', loc=0., scale=2.)] * 4)
    sampler = SMCSampler(like, nparticles=1024, chains=8, seed=1)
    assert not sampler.device_resident and sampler.n_steps == 8
    sampler.run(max_iterations=1)
    var = D4_SIGMA**2 + 4.
    _assert_evidence(sampler, float(np.sum(-0.5 * D4_MEAN**2 / var - 0.5 * np.log(2. * np.pi * var))))
    assert np.all(sampler.history['beta'][:, -1] == 1.) and sampler.nevaluations == 8 * 1024 * (1 + 8 * sampler.history['beta'].shape[1])


def test_evidence_gaussian_in_a_uniform_box():
    """The same likelihood in the box [-6, 6]^4: Z = (1 - truncation) / 12^4.  The nearest face is (6 - 0.8) / 0.4 = 13 sigma away: the truncated mass is below
    4 erfc(13 / sqrt 2) ~ 1e-37 <= 1e-12.  Achieved here (K = 8, N = 1024, seed 3): logz_mean 0.56 standard errors below -4 log 12 = -9.9396, logz_std 0.108 against
    the bound 0.165 (T = 7); over seeds 1 .. 4: -1.4 .. 2.8 standard errors, logz_std 0.108 .. 0.182."""
    from math import erfc
    from desilike_amd.samplers import SMCSampler
    assert 4. * erfc(np.min((6. - np.abs(D4_MEAN)) / D4_SIGMA) / np.sqrt(2.)) <= 1e-12
    like = ToyLikelihood(_loglike4, [dict(limits=[-6., 6.])] * 4)
    sampler = SMCSampler(like, nparticles=1024, chains=8, seed=3)
    sampler.run(max_iterations=1)
    _assert_evidence(sampler, -4. * np.log(12.))


MODES, MODE_WEIGHTS = np.array([[-3., 0.5], [3., 0.5]]), np.array([0.3, 0.7])        # sigma = 0.5: 12 sigma apart


def _loglike_mixture(x):
    terms = [np.log(w) - 0.5 * (((x - m) / 0.5)**2).sum(axis=1) - np.log(2. * np.pi * 0.25) for m, w in zip(MODES, MODE_WEIGHTS)]
    return np.logaddexp(*terms)


def test_evidence_and_shares_of_a_mixture():
    """Two Gaussians (weights 0.3 / 0.7, sigma 0.5, 12 sigma apart) in the box [-8, 8]^2: Z = 1 / 256 (the nearest face is 10 sigma away: truncation ~1e-23); the share
    of the beta = 1 particles nearer to each mode within 4 binomial standard errors at the pooled effective count K N / (2 tau), tau the integrated autocorrelation
    time of the mode indicator over the beta = 1 sweeps.  Achieved here (K = 8, N = 512, n_steps = 4, seed 3): logz_mean -5.4995 against -5.5452 (1.3 standard errors),
    logz_std 0.102 against the bound 0.177 (T = 4); share of the heavier mode 0.6914; the particles change mode rarely at beta = 1 (tau = 22 sweeps: an effective count
    of 91, 4 standard errors = 0.19)."""
    from desilike_amd.samplers import SMCSampler
    like = ToyLikelihood(_loglike_mixture, [dict(limits=[-8., 8.])] * 2)
    sampler = SMCSampler(like, nparticles=512, chains=8, seed=3, n_steps=4)
    chains = sampler.run(max_iterations=30)
    _assert_evidence(sampler, -np.log(256.))
    right = np.array([chain['p0'][-30:] > 0. for chain in chains], dtype='f8')       # [K, sweeps, N]
    share = right[:, -1].mean()
    # pooled autocorrelation of the indicator about the pooled mean (a particle that never changes mode in 30 sweeps has no variance of its own), Sokal's window
    d = right.transpose(0, 2, 1).reshape(-1, 30) - right.mean()
    acf = np.array([np.mean(d[:, :30 - t] * d[:, t:]) for t in range(30)]) / np.mean(d * d)
    taus = 2. * np.cumsum(acf) - 1.
    window = np.arange(30) >= 5. * taus
    tau = max(float(taus[np.argmax(window)] if window.any() else taus[-1]), 1.)
    neff = 8 * 512 / (2. * tau)
    print('share of the heavier mode {:.4f} tau {:.2f} effective count {:.0f}'.format(share, tau, neff))
    assert abs(share - 0.7) <= 4. * np.sqrt(0.3 * 0.7 / neff)


# ---- 4. errors and plumbing ------------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    from desilike_amd.samplers import SMCSampler
    from desilike_amd.smc import _HostSMC
    box = [dict(limits=[-6., 6.])] * 4
    with pytest.raises(ValueError, match='p1.*not proper|not proper.*p1|p1'):
        SMCSampler(ToyLikelihood(_loglike4, [dict(limits=[-6., 6.]), dict(limits=[-np.inf, 6.])] + box[:2]))
    with pytest.raises(ValueError, match='multiple of 64'): SMCSampler(ToyLikelihood(_loglike4, box), nparticles=100)
    with pytest.raises(ValueError, match='multiple of 64'): SMCSampler(ToyLikelihood(_loglike4, box), nparticles=32768)
    for bad in (0., 1., -0.2, 1.5):
        with pytest.raises(ValueError, match='ess_fraction'): SMCSampler(ToyLikelihood(_loglike4, box), ess_fraction=bad)
    with pytest.raises(ValueError, match='n_steps'): SMCSampler(ToyLikelihood(_loglike4, box), n_steps=0)
    host = _HostSMC(_gauss2, 1, 64, 2, [4., 4.])
    host.set_hyper(0.5, 2, 0.234)
    start = np.random.RandomState(0).uniform(-2., 2., (1, 64, 2))
    outside = start.copy(); outside[0, 5, 1] = 2.5
    with pytest.raises(ValueError, match='particle 5 of system 0 lies outside the prior'): host.set_particles(outside)
    dead = _HostSMC(lambda x: (np.full(len(x), -np.inf), np.zeros(len(x))), 1, 64, 2, [4., 4.])
    with pytest.raises(ValueError, match='no particle of system 0 has a finite log-likelihood'): dead.set_particles(start)
    with pytest.raises(ValueError, match='hyper'): _HostSMC(_gauss2, 1, 64, 2, [4., 4.]).run(1, 1, host.buffers(1))
    sampler = SMCSampler(ToyLikelihood(_loglike4, box), nparticles=64, seed=0)
    assert sampler.logz_std is None and np.allclose(sampler.widths, 12.)


def test_resume_through_save_fn(tmp_path):
    """A run saved at beta = 1 after 2 sweeps and continued from its files equals the uninterrupted run bit for bit."""
    from desilike_amd.samplers import SMCSampler
    box = [dict(limits=[-6., 6.])] * 4
    fn = str(tmp_path / 'smc_*.npz')
    whole = SMCSampler(ToyLikelihood(_loglike4, box), nparticles=64, chains=2, seed=5, n_steps=3)
    whole.run(max_iterations=5)
    first = SMCSampler(ToyLikelihood(_loglike4, box), nparticles=64, chains=2, seed=5, n_steps=3, save_fn=fn)
    first.run(max_iterations=2)
    second = SMCSampler(ToyLikelihood(_loglike4, box), nparticles=64, chains=[fn.replace('*', str(k)) for k in range(2)], seed=77)
    assert second.counter_seed == 5 and second.n_steps == 3
    second.run(max_iterations=5)
    for a, b in zip(whole.chains, second.chains):
        assert sorted(a) == sorted(b) and a['logposterior'].shape[1] == 64 and a['logposterior'].shape[0] >= 5
        for name in a: assert np.array_equal(a[name], b[name])
    assert np.array_equal(whole._history, second._history) and np.array_equal(whole.logz, second.logz) and whole.nevaluations == second.nevaluations
