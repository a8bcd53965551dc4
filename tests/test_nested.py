"""Batched nested sampling (desilike_amd/nested.py) on the CPU: the host build of the device arithmetic (csrc/dl_nested.h via tests/csrc/emulate_nested.cpp, also as a
stand-alone program under the sanitizers) against the NumPy statement, the invariants of the stage machine, log-evidences with closed forms, errors and resume."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from emulation import SANITIZE_FLAGS
from test_smc import D4_MEAN, D4_SIGMA, MODE_WEIGHTS, ToyLikelihood, _gauss2, _loglike4, _loglike_mixture

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'csrc', 'emulate_nested.cpp')
DEPS = [SRC] + [os.path.join(HERE, '..', 'desilike_amd', 'csrc', name) for name in ['dl_nested.h', 'dl_smc.h', 'dl_nuts.h', 'dl_philox.h']]
_lib = []


def _stale(target):
    return not os.path.isfile(target) or any(os.path.getmtime(dep) > os.path.getmtime(target) for dep in DEPS)


def _emulation():
    """The shared object pytest loads: built WITHOUT the sanitizers (only the stand-alone program below has them)."""
    if _lib: return _lib[0]
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, 'libdl_emulate_nested.so')
    if _stale(so): subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', so, SRC])
    lib = ctypes.CDLL(so)
    p, i32, f8, i64, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_longlong, ctypes.c_uint64
    lib.emu_nested_rank.argtypes = [p, i32, i32, p, p, p]
    lib.emu_nested_evidence.argtypes = [p, p, i32, i32, f8, f8, p, p, p]
    lib.emu_nested_moments.argtypes = [p, p, i32, i32, i32, p, p]
    lib.emu_nested_factor.argtypes = [p, p, i32, p]
    lib.emu_nested_seeds.argtypes = [p, i32, i32, i64, i32, u64, p, p]
    lib.emu_nested_propose.argtypes = [p, f8, p, i32, i32, i64, i32, i32, u64, p]
    lib.emu_nested_accept.argtypes = [f8, p, p, p, p, i32, i64, i32, i32, u64, p, p, p]
    lib.emu_nested_finish.argtypes = [p, i32, f8, f8, f8, p]
    lib.emu_nested_key.argtypes, lib.emu_nested_key.restype = [f8], u64
    _lib.append(lib)
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype='f8'), np.asarray(b, dtype='f8')
    assert np.allclose(a, b, rtol=tol, atol=tol), float(np.max(np.abs(a - b)))


# ---- 1. host build of the device arithmetic ---------------------------------------------------------------------------------------------------------------------
def _points(N, P, edge, seed=3):
    """Live points x [N, P] and log-likelihoods of a correlated Gaussian; edge 'equal': three values of L only (rank ties); 'shared': all points share the last
    coordinate (a singular covariance)."""
    rng = np.random.RandomState(seed + 7 * N + P)
    mix = np.eye(P) + 0.3 * np.tril(rng.standard_normal((P, P)), -1)
    x = rng.standard_normal((N, P)) @ mix.T + rng.standard_normal(P)
    if edge == 'shared': x[:, -1] = 0.25
    L = -0.5 * (rng.standard_normal((N, P))**2).sum(axis=1) * 40. / P
    if edge == 'equal': L = -1.5 - (np.arange(N) % 3).astype('f8')
    return np.ascontiguousarray(x), L


@pytest.mark.parametrize('edge', ['none', 'equal', 'shared'])
@pytest.mark.parametrize('P', [1, 2, 15, 64])
@pytest.mark.parametrize('mode', ['one', 24, 'half'])
@pytest.mark.parametrize('N', [64, 320, 8192])
def test_host_build_equals_the_numpy_statement(N, mode, P, edge):
    """N = 320 takes the padded sort, M = 24 a partial wavefront and a partial workgroup of the propose and accept kernels, P = 15 the odd Box-Muller tail; equal L
    makes rank ties, a shared coordinate a singular covariance, a proposal with L' exactly L* is rejected.  Ranks, seeds and flags equal, values to 1e-12."""
    from desilike_amd import nested
    lib, seed, it, run = _emulation(), 2024, 5, 3
    M = {'one': 1, 24: 24, 'half': N // 2}[mode]
    x, L = _points(N, P, edge)
    # the sort, the survivors' weights and the first survivor
    rank, W, first = np.zeros(N, dtype='i4'), np.zeros(N), np.zeros(1, dtype='i4')
    assert lib.emu_nested_rank(_ptr(L), N, M, _ptr(rank), _ptr(W), _ptr(first)) == 0
    order = nested.ranks(L)
    assert np.array_equal(rank, order) and np.array_equal(np.sort(rank), np.arange(N))
    assert np.all(np.diff(L[rank]) >= 0.) and np.all((np.diff(L[rank]) > 0.) | (np.diff(rank) > 0))       # (L, slot) ascending
    if edge == 'equal': assert np.count_nonzero(np.diff(L[rank]) == 0.) == N - 3
    dead = order[:M]
    assert first[0] == np.setdiff1d(np.arange(N), dead).min() and W[dead].sum() == 0. and np.all(W[order[M:]] == 1. / (N - M))
    # the evidence with its prefix sums
    logx, logz = -0.75, -31.5
    out, cum, logw = np.zeros(3), np.zeros(M), np.zeros(M)
    assert lib.emu_nested_evidence(_ptr(L), _ptr(rank), N, M, logx, logz, _ptr(out), _ptr(cum), _ptr(logw)) == 0
    lw, lx, lz = nested.evidence(L[dead], N, logx, logz)
    assert np.array_equal(cum, nested.shrinkage(N, M)[0])          # additions and divisions only, in the kernel's order: the same bits
    _close(cum, np.cumsum(1. / (N - np.arange(M))))
    _close(logw, lw); _close(out, [L[dead[-1]], lx, lz])
    assert out[0] == L[dead[-1]]
    # log w_j = log(X_{j-1} - X_j): with the closing volume the shells fill the volume the iteration started from
    _close(np.exp(logw).sum() + np.exp(out[1]), np.exp(logx))
    _close(out[2], np.logaddexp(logz, np.log(np.sum(np.exp(logw + L[dead] - L[dead].max()))) + L[dead].max()))      # the statement of the issue, log X not factored out
    # the moments and the factor with its fallbacks
    mean, cov, C, widths = np.zeros(P), np.zeros((P, P)), np.zeros((P, P)), np.linspace(2., 3., P)
    assert lib.emu_nested_moments(_ptr(x), _ptr(W), int(first[0]), N, P, _ptr(mean), _ptr(cov)) == 0
    mh, ch = nested.survivor_moments(x, dead)
    _close(mean, mh); _close(cov, ch)
    survivors = x[order[M:]]
    assert np.allclose(mh, survivors.mean(axis=0), rtol=1e-10, atol=1e-10) and np.allclose(ch, np.tril(np.cov(survivors.T, bias=True).reshape(P, P)), rtol=1e-9, atol=1e-10)
    assert lib.emu_nested_factor(_ptr(cov), _ptr(widths), P, _ptr(C)) == 0
    Ch = nested.factor(ch, widths)
    _close(C, Ch)
    if edge == 'shared' or N - M <= P:      # the diagonal fallback, and the prior's width for a component without variance
        assert np.count_nonzero(C - np.diag(np.diag(C))) == 0
        if edge == 'shared': assert cov[-1, -1] == 0. and ch[-1, -1] == 0. and C[-1, -1] == widths[-1]
    else: _close(C @ C.T, ch + np.tril(ch, -1).T, tol=1e-10)
    # the seeds
    seeds, u = np.zeros(M, dtype='i4'), np.zeros(M)
    assert lib.emu_nested_seeds(_ptr(rank), N, M, it, run, seed, _ptr(seeds), _ptr(u)) == 0
    draws = nested._NestedDraws(seed)
    uh = draws.seed_uniform(it, run, M)
    r, margins = nested.seed_ranks(uh, N, M)
    assert np.array_equal(u, uh) and np.all((0. <= u) & (u < 1.)) and np.array_equal(seeds, order[r]) and np.all(r >= M) and np.all(r < N) and np.all(W[seeds] > 0.)
    assert np.all(margins <= 0.5) and np.array_equal(nested.seed_ranks(np.array([0., 1. - 2.**-53]), N, M)[0], [M, N - 1])
    # the proposal and the constrained test on the replaced points
    xs, prop = np.ascontiguousarray(x[seeds]), np.zeros((M, P))
    assert lib.emu_nested_propose(_ptr(C), 0.7, _ptr(xs), M, P, it, 2, run, seed, _ptr(prop)) == 0
    z = draws.gauss(it, 2, run, M, P)
    _close(prop, xs + (0.7 * (2.38 / np.sqrt(float(P)))) * nested._matvec(Ch, z))
    rng = np.random.RandomState(1)
    lstar = out[0]
    pi, pip = rng.standard_normal(M), rng.standard_normal(M)
    Lp = lstar + rng.standard_normal(M)
    Lp[::5] = lstar                                   # L' exactly L*: rejected (the constraint is strict)
    status = (rng.uniform(size=M) < 0.1).astype('i4')
    pip[status == 1] = -np.inf
    if M > 11: Lp[11::13] = np.nan
    flags, logu, nacc = np.zeros(M, dtype='u1'), np.zeros(M), np.zeros(1, dtype='i4')
    assert lib.emu_nested_accept(lstar, _ptr(pi), _ptr(Lp), _ptr(pip), _ptr(status), M, it, 2, run, seed, _ptr(flags), _ptr(logu), _ptr(nacc)) == 0
    lh = draws.log_uniform(it, 2, run, M)
    _close(logu, lh)
    ok = np.isfinite(Lp) & np.isfinite(pip) & (status == 0)
    with np.errstate(invalid='ignore'):
        expected = ok & (np.where(ok, Lp, -np.inf) > lstar) & (lh < np.where(ok, pip, 0.) - pi)
    assert np.array_equal(flags.astype(bool), expected) and nacc[0] == expected.sum() and not flags[::5].any()
    if M >= 24: assert 0 < nacc[0] < M
    # the evidence left in the live points and the rest
    fin = np.zeros(2)
    for dlogz in (0.01, 0.999999):
        assert lib.emu_nested_finish(_ptr(L), N, out[1], out[2], dlogz, _ptr(fin)) == 0
        rem = nested.remaining(L, lx)
        _close(fin[0], rem)
        assert bool(fin[1]) == nested.at_rest(lz, rem, dlogz)
    _close(fin[0], lx + np.log(np.mean(np.exp(L))))


def test_keys_keep_the_order_of_the_doubles():
    lib = _emulation()
    values = np.array([-np.inf, -1e308, -2.5, -1., -5e-324, -0., 0., 5e-324, 1., 2.5, 1e308, np.inf])
    keys = [lib.emu_nested_key(v) for v in values]
    assert keys[5] == keys[6] and np.all(np.diff(np.array(keys[:5] + keys[6:], dtype=object)) > 0) and keys[-1] < 2**64 - 1      # (-0 as +0; the padding key is above +inf)


def test_host_build_under_the_sanitizers():
    """tests/csrc/emulate_nested.cpp with -DEMU_NESTED_MAIN: a stand-alone program (every phase, every shape and edge input above) built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run directly."""
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, 'emulate_nested_main')
    if _stale(exe): subprocess.check_call(['g++', '-O1', '-std=c++17', '-DEMU_NESTED_MAIN'] + SANITIZE_FLAGS + ['-o', exe, SRC])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert done.returncode == 0 and 'emulate_nested: ok' in done.stdout and 'runtime error' not in done.stdout and 'Sanitizer' not in done.stdout, done.stdout


# ---- 2. invariants of the stage machine --------------------------------------------------------------------------------------------------------------------------
def _host(K=2, N=128, M=32, seed=9, ids=None, n_steps=3, dlogz=0.01):
    from desilike_amd.nested import _HostNested
    host = _HostNested(_gauss2, K, N, 2, [4., 4.], run_ids=ids, seed=seed)
    host.set_hyper(M, n_steps, 0.234, dlogz)
    host.set_live(np.random.RandomState(4).uniform(-2., 2., (K, N, 2)))
    return host


def _assert_above(state, records, slot):
    """Every live L is above the L* of the iteration recorded in ``slot``, strictly -- but for the unmoved copies of the last dead point: a reseeded slot whose sweeps
    were all rejected keeps the L of its seed, the pair ties, the slot index decides which of the two dies and the other stays with L = L* exactly."""
    x, L = state[0], state[1]
    history, coords = records[0], records[1]
    for k in range(len(L)):
        lstar = history[k, slot, 2]
        assert np.all(L[k] >= lstar)
        tied = L[k] == lstar
        assert np.all(x[k][tied] == coords[k, slot, -1]), 'a live point at L* that is not a copy of the last dead point'


def test_invariants_of_the_host_statement():
    from desilike_amd.nested import run_batch, closing
    K, N, M, T = 2, 128, 32, 14
    host = _host()
    buffers = host.buffers(T)
    for t in range(1, T + 1):
        host.run(1, T, buffers)
        history, L = host.records(buffers)[0], host.get_state()[1]
        assert np.all(host.counts(buffers) == t)
        _assert_above(host.get_state(), host.records(buffers), t - 1)
        assert np.allclose(host.get_state()[3], -t * np.sum(1. / (N - np.arange(M))), rtol=1e-12, atol=0.)
    history, coords, dL, dpi, dlogw = host.records(buffers)
    assert np.allclose(history[..., 0], -np.arange(1, T + 1) * np.sum(1. / (N - np.arange(M))), rtol=1e-12, atol=0.)
    assert np.all(np.diff(history[..., 2], axis=1) >= 0.) and np.all(np.diff(history[..., 1], axis=1) > 0.)        # L* does not decrease; log Z grows
    assert np.all(np.diff(dL.reshape(K, -1), axis=1) >= 0.)                                     # the dead leave in the order of their likelihood
    assert np.all((history[..., 3] > 0.02) & (history[..., 3] < 0.9)) and np.all((history[..., 4] >= 1e-3) & (history[..., 4] <= 1e3))
    assert np.all(np.abs(coords) < 2.) and np.all(dpi == -np.log(16.))
    state = host.get_state()
    for k in range(K):
        closed = closing(dL[k], dlogw[k], state[1][k], state[3][k])
        assert abs(np.exp(closed['logweight']).sum() - 1.) <= 1e-12 and abs(closed['aweight'].sum() - 1.) <= 1e-12
        assert closed['logz'] >= history[k, -1, 1] and closed['information'] > 0. and len(closed['aweight']) == T * M + N
    assert np.isfinite(host.min_margin) and host.ndecisions > K * T * M * 3 and host.evaluations == K * (N + M * 3 * T)


def test_rest_chunking_and_run_ids():
    from desilike_amd.nested import run_batch, REST
    runs = [run_batch(_host(), 60, chunk=chunk) for chunk in (None, 7, 1)]
    history, counts, modes = runs[0][0], runs[0][5], runs[0][6]
    assert np.all(modes == REST) and np.all(counts < 60) and np.all(counts > 10)
    for k in range(2):          # at rest exactly when the criterion first holds
        gap = history[k, :counts[k], 5] - np.logaddexp(history[k, :counts[k], 1], history[k, :counts[k], 5])
        assert gap[-1] < np.log(0.01) and np.all(gap[:-1] >= np.log(0.01)) and np.all(history[k, counts[k]:] == 0.)
    for other in runs[1:]:
        assert np.array_equal(other[5], counts)
        for a, b in zip(runs[0][:5], other[:5]):
            for k in range(2): assert np.array_equal(a[k, :counts[k]], b[k, :counts[k]])
    # a run at rest does nothing and records nothing
    host = _host()
    run_batch(host, 60)
    state, evaluations = host.get_state(), host.evaluations
    more = run_batch(host, 3)
    assert np.all(more[5] == 0) and all(np.array_equal(a, b) for a, b in zip(state, host.get_state()))
    # a run is its id: run 1 of a pair is the one-run engine with id 1; another id draws differently
    pair, single, other = _host(), _host(K=1, ids=[1]), _host(K=1, ids=[5])
    start = pair.get_state()[0]
    for engine in (single, other): engine.set_live(start[1:])
    hp, hs, ho = run_batch(pair, 5)[0], run_batch(single, 5)[0], run_batch(other, 5)[0]
    assert np.array_equal(hp[1], hs[0]) and not np.array_equal(hs[0, :, 3], ho[0, :, 3])
    for a, b in zip(pair.get_state(), single.get_state()): assert np.array_equal(a[1:], b)
    # a state round trip continues bit for bit
    first, resumed = _host(), _host()
    run_batch(first, 4)
    resumed.set_state(*first.get_state())
    whole = run_batch(_host(), 9)[0]
    assert np.array_equal(run_batch(resumed, 5)[0], whole[:, 4:])


# ---- 3. closed-form evidences ----------------------------------------------------------------------------------------------------------------------------------
# The inflation f of the scatter of log Z over sqrt(H / N) from imperfect mixing of the constrained random walk, measured on _HostNested at the defaults (ndelete =
# nlive / 4, n_steps = 4 ndim) over 48 runs per case (6 seeds x 8 runs, N = 256): 0.88 (Gaussian priors, d = 4), 1.07 (box, d = 4), 1.38 (mixture, d = 2); the worst,
# rounded up to the next 0.25
F = 1.5
NLIVE = 256


def _assert_evidence(sampler, exact, H):
    K, N = sampler.nchains, sampler.nlive
    unit = np.sqrt(H / N)
    print('logz_mean {:.4f} exact {:.4f} logz_std {:.4f} sqrt(H / N) {:.4f} logz_err {:.4f} .. {:.4f} H {:.3f} .. {:.3f} exact {:.3f} iterations {} evaluations {:d}'.format(
        sampler.logz_mean, exact, sampler.logz_std, unit, sampler.logz_err.min(), sampler.logz_err.max(), sampler.information.min(), sampler.information.max(), H,
        sampler.niterations.tolist(), sampler.nevaluations))
    assert abs(sampler.logz_mean - exact) <= 4. * F * unit / np.sqrt(K)
    assert sampler.logz_std <= 2. * F * unit
    assert np.all(np.abs(sampler.logz_err / unit - 1.) <= 0.25)


def _gaussian_priors():
    """Normalised Gaussian likelihood N(x; mu, diag(sigma^2)) in d = 4 under priors N(0, 2^2): Z = prod_i N(mu_i; 0, sigma_i^2 + 4); H = the Kullback-Leibler divergence of
    the Gaussian posterior N(m, v) from the prior, sum_i (v_i / 4 + m_i^2 / 4 - 1 - log(v_i / 4)) / 2."""
    var = D4_SIGMA**2 + 4.
    v = 1. / (1. / D4_SIGMA**2 + 0.25)
    m = v * D4_MEAN / D4_SIGMA**2
    return (ToyLikelihood(_loglike4, [dict(dist='norm', loc=0., scale=2.)] * 4), float(np.sum(-0.5 * D4_MEAN**2 / var - 0.5 * np.log(2. * np.pi * var))),
            float(np.sum(0.5 * (v / 4. + m**2 / 4. - 1. - np.log(v / 4.)))))


def _mixture():
    """Two Gaussians (weights 0.3 / 0.7, sigma 0.5, 12 sigma apart) in the box [-8, 8]^2: Z = 1 / 256 (the nearest face is 10 sigma away); H = log 256 - the entropy of the
    posterior, which for modes that do not overlap is log(2 pi e sigma^2) - sum w log w."""
    return (ToyLikelihood(_loglike_mixture, [dict(limits=[-8., 8.])] * 2), -np.log(256.),
            float(np.log(256.) - np.log(2. * np.pi * np.e * 0.25) + np.sum(MODE_WEIGHTS * np.log(MODE_WEIGHTS))))


def test_evidence_gaussian_with_gaussian_priors():
    """Measured (6 seeds x 8 runs, N = 256, 42 - 43 iterations): scatter 0.88 sqrt(H / N), log of the mean Z 0.039 above the closed form (1.9 standard errors of 48 runs),
    logz_err 0.98 .. 1.02 sqrt(H_exact / N)."""
    from desilike_amd.samplers import NestedSampler
    like, exact, H = _gaussian_priors()
    sampler = NestedSampler(like, nlive=NLIVE, chains=8, seed=1)
    assert not sampler.device_resident and sampler.n_steps == 16 and sampler.ndelete == 64
    chains = sampler.run()
    _assert_evidence(sampler, exact, H)
    # (rows evaluated: the start, then ndelete proposals per run and sweep in every iteration enqueued, in chunks of 16, those of a run already at rest included)
    assert np.all(sampler.prior_fraction == 1.) and sampler.nevaluations == 2 * 8 * NLIVE + 8 * 64 * 16 * 16 * -(-int(sampler.niterations.max()) // 16)
    for chain, n in zip(chains, sampler.niterations):
        assert len(chain['aweight']) == n * 64 + NLIVE and abs(chain['aweight'].sum() - 1.) <= 1e-12 and abs(np.exp(chain['logweight']).sum() - 1.) <= 1e-12
    # the weighted sample is the posterior: means within 4 standard errors at the effective count of the weights
    v = 1. / (1. / D4_SIGMA**2 + 0.25)
    m = v * D4_MEAN / D4_SIGMA**2
    w = np.concatenate([chain['aweight'] for chain in chains]) / 8.
    x = np.column_stack([np.concatenate([chain['p{:d}'.format(i)] for chain in chains]) for i in range(4)])
    neff = 1. / np.sum(w**2)
    print('posterior mean', w @ x, 'exact', m, 'effective count', neff)
    assert np.all(np.abs(w @ x - m) <= 4. * F * np.sqrt(v / neff))
    draw = sampler.samples(2000, random_state=np.random.RandomState(0))
    assert sorted(draw) == sorted(['p0', 'p1', 'p2', 'p3', 'loglikelihood', 'logposterior']) and np.all(np.abs(draw['p0'].mean() - m[0]) <= 4. * F * np.sqrt(v[0] / min(neff, 2000.)))


def test_evidence_gaussian_in_a_uniform_box():
    """The same likelihood in the box [-6, 6]^4: Z = 1 / 12^4 (truncation below 1e-12, tests/test_smc.py); H = 4 log 12 - sum_i log(2 pi e sigma_i^2) / 2.
    Measured (6 seeds x 8 runs, N = 256, 54 - 55 iterations): scatter 1.07 sqrt(H / N), log of the mean Z 0.028 above the closed form, logz_err 0.98 .. 1.03."""
    from desilike_amd.samplers import NestedSampler
    like = ToyLikelihood(_loglike4, [dict(limits=[-6., 6.])] * 4)
    sampler = NestedSampler(like, nlive=NLIVE, chains=8, seed=2)
    sampler.run()
    _assert_evidence(sampler, -4. * np.log(12.), float(4. * np.log(12.) - np.sum(0.5 * np.log(2. * np.pi * np.e * D4_SIGMA**2))))


def test_evidence_and_shares_of_a_mixture():
    """Measured (6 seeds x 8 runs, N = 256, n_steps = 8, 33 - 34 iterations): scatter 1.38 sqrt(H / N), log of the mean Z 0.009 above the closed form, logz_err 0.95 .. 1.05;
    share of the heavier mode, mean of 8 runs, 0.688 .. 0.726.  The share is Z_b / (Z_a + Z_b): the two log-evidences scatter by f sqrt(H / N) each, so the logit of the
    share by sqrt(2) f sqrt(H / N) and the mean share of K runs by 0.3 x 0.7 x sqrt(2) f sqrt(H / N) / sqrt(K); four of those are allowed.  Then the same two conditions
    once with 64 runs (the scatter of eight estimates itself to +- 27 %, of 64 to +- 9 %), so that no seed can be chosen to pass."""
    from desilike_amd.samplers import NestedSampler
    like, exact, H = _mixture()
    sampler = NestedSampler(like, nlive=NLIVE, chains=8, seed=3)
    assert sampler.n_steps == 8
    chains = sampler.run()
    _assert_evidence(sampler, exact, H)
    share = np.array([chain['aweight'][chain['p0'] > 0.].sum() for chain in chains])
    bound = 4. * 0.3 * 0.7 * np.sqrt(2.) * F * np.sqrt(H / NLIVE) / np.sqrt(8.)
    print('share of the heavier mode', share, 'mean', share.mean(), 'bound', bound)
    assert abs(share.mean() - 0.7) <= bound
    many = NestedSampler(_mixture()[0], nlive=NLIVE, chains=64, seed=3)
    many.run()
    _assert_evidence(many, exact, H)


# ---- 4. errors and plumbing ------------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    from desilike_amd.samplers import NestedSampler
    from desilike_amd.nested import _HostNested
    box = [dict(limits=[-6., 6.])] * 4
    with pytest.raises(ValueError, match='p1.*not proper|not proper.*p1|p1'):
        NestedSampler(ToyLikelihood(_loglike4, [dict(limits=[-6., 6.]), dict(limits=[-np.inf, 6.])] + box[:2]))
    with pytest.raises(ValueError, match='multiple of 64'): NestedSampler(ToyLikelihood(_loglike4, box), nlive=100)
    with pytest.raises(ValueError, match='multiple of 64'): NestedSampler(ToyLikelihood(_loglike4, box), nlive=16384)
    for bad in (0, 33):
        with pytest.raises(ValueError, match='ndelete'): NestedSampler(ToyLikelihood(_loglike4, box), nlive=64, ndelete=bad)
    for bad in (0., 1., -0.2):
        with pytest.raises(ValueError, match='dlogz'): NestedSampler(ToyLikelihood(_loglike4, box), dlogz=bad)
    with pytest.raises(ValueError, match='n_steps'): NestedSampler(ToyLikelihood(_loglike4, box), n_steps=0)
    with pytest.raises(ValueError, match='target_acceptance'): NestedSampler(ToyLikelihood(_loglike4, box), target_acceptance=1.)
    host = _HostNested(_gauss2, 1, 64, 2, [4., 4.])
    with pytest.raises(ValueError, match='hyper'): host.run(1, 1, host.buffers(1))
    host.set_hyper(16, 2, 0.234, 0.01)
    with pytest.raises(ValueError, match='live points'): host.run(1, 1, host.buffers(1))
    start = np.random.RandomState(0).uniform(-2., 2., (1, 64, 2))
    outside = start.copy(); outside[0, 5, 1] = 2.5
    with pytest.raises(ValueError, match='live point 5 of run 0 lies outside the prior'): host.set_live(outside)
    dead = _HostNested(lambda x: (np.where(np.arange(len(x)) == 7, -np.inf, 0.), np.zeros(len(x))), 1, 64, 2, [4., 4.])
    with pytest.raises(ValueError, match='live point 7 of run 0 has no finite log-likelihood'): dead.set_live(start)
    host.set_live(start)
    state = list(host.get_state())
    state[1] = state[1].copy(); state[1][0, 3] = -np.inf
    with pytest.raises(ValueError, match='live point 3 of run 0 has no finite log-likelihood'): host.set_state(*state)
    sampler = NestedSampler(ToyLikelihood(_loglike4, box), nlive=64, seed=0)
    assert sampler.logz_std is None and np.allclose(sampler.widths, 12.) and sampler.ndelete == 16 and sampler.chains == [] and np.isnan(sampler.logz[0])
    slow = NestedSampler(ToyLikelihood(_loglike4, box), nlive=64, seed=0, n_steps=2)
    with pytest.raises(RuntimeError, match='not at rest after 3 iterations'): slow.run(max_iterations=3)
    # a likelihood without a value on half of the prior: the rows are redrawn, the accepted fraction enters logz; nowhere a value: an error after 64 rounds
    half = NestedSampler(ToyLikelihood(lambda x: np.where(x[:, 0] > 0., _loglike4(x), -np.inf), box), nlive=64, chains=2, seed=4, n_steps=2)
    half._engine = half._make_engine()
    assert np.all(np.abs(half.prior_fraction - 0.5) < 4. * 0.5 / np.sqrt(64.)) and np.all(half._engine.get_state()[0][..., 0] > 0.)
    none = NestedSampler(ToyLikelihood(lambda x: np.full(len(x), -np.inf), box), nlive=64, seed=4)
    with pytest.raises(RuntimeError, match='64 rounds'): none.run()


def test_resume_through_save_fn(tmp_path):
    """A run saved after 6 iterations and continued from its files equals the uninterrupted run bit for bit."""
    from desilike_amd.samplers import NestedSampler
    box = [dict(limits=[-6., 6.])] * 4
    fn = str(tmp_path / 'nested_*.npz')
    whole = NestedSampler(ToyLikelihood(_loglike4, box), nlive=64, chains=2, seed=5, n_steps=3, dlogz=0.2)
    whole.run()
    first = NestedSampler(ToyLikelihood(_loglike4, box), nlive=64, chains=2, seed=5, n_steps=3, dlogz=0.2, save_fn=fn)
    with pytest.raises(RuntimeError, match='not at rest'): first.run(max_iterations=6, check_every=4)
    first.save()
    second = NestedSampler(ToyLikelihood(_loglike4, box), nlive=64, chains=[fn.replace('*', str(k)) for k in range(2)], seed=77)
    assert second.counter_seed == 5 and second.n_steps == 3 and second.dlogz == 0.2 and np.all(second.niterations == 6)
    second.run()
    for a, b in zip(whole.chains, second.chains):
        assert sorted(a) == sorted(b)
        for name in a: assert np.array_equal(a[name], b[name]), name
    assert all(np.array_equal(a, b) for a, b in zip(whole._history, second._history)) and np.array_equal(whole.logz, second.logz) and np.array_equal(whole.logz_err, second.logz_err)


def test_null_handles_are_errors():
    """The C ABI without a GPU: every dl_nested_* entry refuses a null handle (and says so), none crashes."""
    from desilike_amd import _lib
    lib = _lib.load()
    handle = ctypes.c_void_p()
    assert lib.dl_nested_create(ctypes.byref(handle), None, 1, 64, None, 0, 0., None) != 0 and not handle.value and b'dl_nested_create' in lib.dl_last_error(None)
    assert lib.dl_nested_set_hyper(None, 16, 2, 0.234, 0.01, 1., None) != 0 and b'dl_nested_set_hyper' in lib.dl_last_error(None)
    assert lib.dl_nested_set_live(None, None, None) != 0
    assert lib.dl_nested_set_state(None, None, None, None, None, None, None, None, None, None) != 0
    assert lib.dl_nested_get_state(None, None, None, None, None, None, None, None, None, None) != 0
    assert lib.dl_nested_get_decisions(None, None, None, None, None, None, None) != 0
    assert lib.dl_nested_run(None, 1, 1, None, None, None, None, None, None, None, None) != 0 and b'dl_nested_run' in lib.dl_last_error(None)
    assert lib.dl_nested_info(None, b'nlive') == -1
    lib.dl_nested_destroy(None)
