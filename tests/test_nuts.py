"""No-U-Turn sampler (desilike_amd/nuts.py; the reference wraps blackjax.nuts, samplers/nuts.py) on the CPU: the leaf-at-a-time engine against a recursive textbook
statement, its invariants, what it samples, the host build of the device arithmetic (csrc/dl_nuts.h via tests/csrc/emulate_nuts.cpp), counters, ranks and resume."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_samplers import ToyGaussianLikelihood

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- a recursive textbook multinomial NUTS (Betancourt 2017 appendix A; Stan's base_nuts), for fixed momentum and directions ----------------------------------
def recursive_nuts(q0, p0, grad_fn, eps, minv, directions, threshold=1000.):
    """Returns dict(leaves: positions evaluated in order, trajectory: (position, log weight) of the final trajectory's leaves in trajectory order,
    subtrees: [(log weight of the trajectory before the join, [(leaf index in trajectory, log weight)])], depth, turning, divergent, n_leapfrog)."""
    sharp = (lambda p: minv @ p) if minv.ndim == 2 else (lambda p: minv * p)
    crit = lambda a, b, rho: sharp(a) @ rho > 0. and sharp(b) @ rho > 0.
    lp0, g0 = grad_fn(q0)
    h0 = -lp0 + 0.5 * p0 @ sharp(p0)
    ctx = dict(leaves=[], n=0, divergent=False, turning=False)

    def build(state, depth, v):
        if depth == 0:
            q, p, g = state
            p = p + 0.5 * v * eps * g
            q = q + v * eps * sharp(p)
            lp, g = grad_fn(q)
            p = p + 0.5 * v * eps * g
            ctx['n'] += 1
            ctx['leaves'].append(q)
            H = -lp + 0.5 * p @ sharp(p)
            if not H - h0 <= threshold:
                ctx['divergent'] = True
                return None
            return dict(first=(q, p, g), last=(q, p, g), rho=p, leaves=[(q, h0 - H)])
        a = build(state, depth - 1, v)
        if a is None: return None
        b = build(a['last'], depth - 1, v)
        if b is None: return None
        rho = a['rho'] + b['rho']
        if not crit(a['first'][1], b['last'][1], rho):
            ctx['turning'] = True
            return None
        return dict(first=a['first'], last=b['last'], rho=rho, leaves=a['leaves'] + b['leaves'])

    left = right = (q0, p0, g0)
    rho, traj, subtrees, depth = p0, [(q0, 0.)], [], 0
    for d, v in enumerate(directions):
        depth = d + 1
        sub = build(right if v > 0 else left, d, v)
        if sub is None: break
        lw_old = np.logaddexp.reduce([w for _, w in traj])
        if v > 0:
            L = dict(first=left, last=right, rho=rho)
            R = dict(first=sub['first'], last=sub['last'], rho=sub['rho'])
            offset, traj = len(traj), traj + sub['leaves']
            leaves = [(offset + i, w) for i, (_, w) in enumerate(sub['leaves'])]
            right = sub['last']
        else:
            L = dict(first=sub['last'], last=sub['first'], rho=sub['rho'])
            R = dict(first=left, last=right, rho=rho)
            n = len(sub['leaves'])
            traj = sub['leaves'][::-1] + traj
            subtrees = [(lw, [(i + n, w) for i, w in ls]) for lw, ls in subtrees]
            leaves = [(n - 1 - i, w) for i, (_, w) in enumerate(sub['leaves'])]
            left = sub['last']
        subtrees.append((lw_old, leaves))
        rho = L['rho'] + R['rho']
        go = crit(L['first'][1], R['last'][1], rho) and crit(L['first'][1], R['first'][1], L['rho'] + R['first'][1]) and \
            crit(L['last'][1], R['last'][1], L['last'][1] + R['rho'])
        if not go:
            ctx['turning'] = True
            break
    return dict(leaves=ctx['leaves'], trajectory=traj, subtrees=subtrees, depth=depth, turning=ctx['turning'], divergent=ctx['divergent'], n_leapfrog=ctx['n'])


def selection_probabilities(result):
    """Analytic probability of every leaf of the final trajectory being the sample: uniform inside a subtree, biased progressive at every join."""
    traj = result['trajectory']
    used = {i for _, ls in result['subtrees'] for i, _ in ls}
    mass = {[i for i in range(len(traj)) if i not in used][0]: 1.}      # the start: the one index no subtree holds
    for lw_old, leaves in result['subtrees']:
        lws = np.logaddexp.reduce([w for _, w in leaves])
        accept = min(1., np.exp(lws - lw_old))
        for key in mass: mass[key] *= 1. - accept
        for i, w in leaves: mass[i] = accept * np.exp(w - lws)
    prob = np.zeros(len(traj))
    for key, value in mass.items(): prob[key] = value
    return prob


def _fixed_engine(C, P, f, minv, eps, p0, directions, max_num_doublings=10, seed=0):
    from desilike_amd.nuts import _HostNUTS
    engine = _HostNUTS(f, C, P, max_num_doublings=max_num_doublings, seed=seed)
    original = engine.draws.direction
    engine.draws.gauss = lambda it, chain, P: np.tile(p0 if minv.ndim == 1 else np.linalg.solve(np.linalg.cholesky(np.linalg.inv(minv)), p0), (len(it), 1))
    engine.draws.direction = lambda it, chain, depth: (np.asarray(directions)[np.asarray(depth)], original(it, chain, depth)[1])
    engine.set_mass(minv, eps)
    return engine


def _gaussian(mean, cov):
    prec = np.linalg.inv(cov)

    def f(q):
        x = q - mean
        return -0.5 * np.einsum('ij,jk,ik->i', x, prec, x), -x @ prec
    return f


CASES = [(np.array([0.5, -0.3]), np.array([[1., 0.8], [0.8, 1.]]), np.array([1., 1.]), 0.2, np.array([0.3, -0.4]), np.array([0.9, 0.2])),
         (np.zeros(5), np.diag([1., 2., 0.5, 1.5, 1.]) + 0.3, None, 0.25, np.array([0.5, -1., 0.2, 0.8, -0.3]), np.array([0.4, -0.8, 1.1, 0.2, -0.5]))]


@pytest.mark.parametrize('case', range(len(CASES)))
def test_trajectory_equals_the_recursive_statement(case):
    mean, cov, diag, eps, q0, p0 = CASES[case]
    P = len(mean)
    minv = diag if diag is not None else cov       # dense: the posterior covariance
    f = _gaussian(mean, cov)
    grad_fn = lambda q: tuple(x[0] for x in f(q[None, :]))
    for directions in ([1, 1, -1, 1, -1, -1, 1, 1, 1, 1], [-1, 1, 1, -1, -1, 1, -1, 1, 1, -1], [1] * 10):
        ref = recursive_nuts(q0, p0, grad_fn, eps, minv, directions)
        seen = []

        def recording(q):
            seen.append(q[0].copy())
            return f(q)

        engine = _fixed_engine(1, P, recording, minv, eps, p0, directions)
        engine.set_state(q0[None, :])
        seen.clear()
        from desilike_amd.nuts import run_batch
        _, _, info = run_batch(engine, 1, chunk=2000)
        n = int(info[0, 0, 1])
        assert n == ref['n_leapfrog'] and int(info[0, 0, 0]) == ref['depth'] and bool(info[0, 0, 2]) == ref['divergent']
        assert ref['turning'] or ref['divergent'] or ref['depth'] == 10
        assert np.allclose(np.array(seen[:n]), np.array(ref['leaves']), rtol=0, atol=1e-13)
        ends = [engine.v['ql'][0], engine.v['qr'][0]]
        assert np.allclose(ends[0], ref['trajectory'][0][0], atol=1e-13) and np.allclose(ends[1], ref['trajectory'][-1][0], atol=1e-13)
    # selected-leaf frequencies against the analytic biased-progressive probabilities
    directions = [1, -1, 1, -1, 1, 1, -1, 1, 1, 1]
    ref = recursive_nuts(q0, p0, grad_fn, eps, minv, directions)
    prob = selection_probabilities(ref)
    assert abs(prob.sum() - 1.) < 1e-12 and len(prob) >= 4
    positions = np.array([q for q, _ in ref['trajectory']])
    counts = np.zeros(len(prob))
    from desilike_amd.nuts import run_batch
    for seed in range(5):
        engine = _fixed_engine(4000, P, f, minv, eps, p0, directions, seed=seed)
        engine.set_state(np.tile(q0, (4000, 1)))
        coords = run_batch(engine, 1, chunk=2000)[0][:, 0]
        index = np.argmin(((coords[:, None, :] - positions[None]) ** 2).sum(axis=-1), axis=1)
        assert np.allclose(coords, positions[index], atol=1e-12)
        counts += np.bincount(index, minlength=len(prob))
    from scipy import stats
    keep = prob > 0
    assert counts[~keep].sum() == 0
    chi2 = ((counts[keep] - 20000 * prob[keep]) ** 2 / (20000 * prob[keep])).sum()
    assert stats.chi2.sf(chi2, keep.sum() - 1) > 1e-3, (counts, 20000 * prob)


def test_invariants():
    from desilike_amd.samplers import NUTSSampler
    like = ToyGaussianLikelihood()
    start = np.tile(like.mean, (8, 1)) + 0.05 * np.random.RandomState(0).standard_normal((8, 2))
    # a tiny step conserves the energy
    s = NUTSSampler(like, chains=8, seed=1, step_size=1e-3, max_num_doublings=5, adaptation=False, covariance=like.cov)
    s.run(check_every=5, max_iterations=5, start=start)
    assert s.acceptance_rate.min() > 0.999 and s.divergences.sum() == 0 and s.mean_tree_depth.min() == 5
    # a huge step diverges at once and keeps the start
    s = NUTSSampler(like, chains=8, seed=1, step_size=50., adaptation=False, covariance=like.cov)
    chains = s.run(check_every=1, max_iterations=1, start=start)
    assert np.all(s.divergences == 1)
    assert np.array_equal(np.column_stack([[c['a'][0], c['b'][0]] for c in chains]).T, start)
    # next to the NaN region (a > 4.9): no non-finite log-posterior is ever recorded
    near = np.tile([4.85, 0.], (8, 1))
    like_far = ToyGaussianLikelihood()
    like_far.mean = np.array([4.8, 0.])
    s = NUTSSampler(like_far, chains=8, seed=3, step_size=0.3, adaptation=False, covariance=like.cov)
    chains = s.run(check_every=30, max_iterations=30, start=near)
    assert all(np.all(np.isfinite(c['logposterior'])) and np.all(c['a'] <= 4.9) for c in chains)
    assert s.divergences.sum() > 0 and s.energy_divergences.sum() == 0          # the NaN region: leaves outside the support
    # one doubling at most
    s = NUTSSampler(like, chains=8, seed=1, step_size=0.05, max_num_doublings=1, adaptation=False, covariance=like.cov)
    s.run(check_every=20, max_iterations=20, start=start)
    assert s._store[2][..., 0].max() == 1


def test_nuts_recovers_the_toy_posterior(tmp_path):
    from desilike_amd.samplers import NUTSSampler
    like = ToyGaussianLikelihood()
    sampler = NUTSSampler(like, chains=64, seed=4, step_size=0.05, adaptation={'niterations': 150}, save_fn=str(tmp_path / 'nuts_*.npy'))
    assert not sampler.device_resident
    chains = sampler.run(check_every=200, max_iterations=400, check={'max_eigen_gr': 0.05, 'stable_over': 1})
    assert len(chains) == 64 and chains[0]['a'].shape[0] in (200, 400)
    x = np.column_stack([np.concatenate([chain[name][50:] for chain in chains]) for name in ['a', 'b']])
    assert np.allclose(x.mean(axis=0), like.mean, atol=0.03)
    assert np.allclose(x.std(axis=0), np.diag(like.cov)**0.5, rtol=0.07)
    assert np.allclose(np.corrcoef(x.T)[0, 1], like.cov[0, 1] / np.sqrt(like.cov[0, 0] * like.cov[1, 1]), atol=0.07)
    assert 0.6 < sampler.acceptance_rate.mean() < 1. and sampler.divergences.sum() == 0
    assert np.allclose(np.diag(sampler.hyp['inverse_mass_matrix']), np.diag(like.cov), rtol=0.6)
    assert (tmp_path / 'nuts_63.npy').exists()


def test_nuts_samples_a_standard_normal():
    from scipy import stats
    from desilike_amd.nuts import _HostNUTS, run_batch
    f = lambda q: (-0.5 * q[:, 0] ** 2, -q)
    engine = _HostNUTS(f, 32, 1, seed=9)
    engine.set_mass(np.ones(1), 0.9)
    engine.set_state(np.random.RandomState(1).standard_normal((32, 1)))
    coords = run_batch(engine, 400)[0][:, 50::5, 0].ravel()
    assert stats.kstest(coords, 'norm').pvalue > 1e-3


# ---- host build of the device arithmetic ------------------------------------------------------------------------------------------------------------------------
def _emulation():
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, 'libdl_emulate_nuts.so')
    src = os.path.join(HERE, 'csrc', 'emulate_nuts.cpp')
    deps = [src] + [os.path.join(HERE, '..', 'desilike_amd', 'csrc', name) for name in ['dl_nuts.h', 'dl_philox.h']]
    if not os.path.isfile(so) or any(os.path.getmtime(dep) > os.path.getmtime(so) for dep in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', so, src])
    lib = ctypes.CDLL(so)
    lib.emu_nuts_kernel.argtypes = [ctypes.c_void_p] * 13 + [ctypes.c_int32] * 7 + [ctypes.c_double] * 3 + [ctypes.c_uint64, ctypes.c_int32]
    return lib


def _emu_engine_class():
    from desilike_amd.nuts import _HostNUTS

    class EmuNUTS(object):
        """The device's record (csrc/dl_nuts.h: 15 + 2 D vector fields, 13 double and 5 int fields per chain) on host arrays, stepped by dl_nuts.h compiled for
        the host; the interface of _HostNUTS."""
        NV, ND, NI = 15, 13, 5

        def __init__(self, f, C, P, D=10, seed=0, threshold=1000.):
            self.lib, self.f, self.C, self.P, self.D, self.seed, self.threshold = _emulation(), f, C, P, D, seed, threshold
            self.vec = np.zeros((self.NV + 2 * D, C, P)); self.dsc = np.zeros((self.ND, C)); self.isc = np.zeros((self.NI, C), dtype='i4')
            self.iter = np.zeros(C, dtype='i8'); self.ids = np.arange(C, dtype='i4')
            self.lp, self.g = np.zeros(C), np.zeros((C, P))
            self.adapt, self.target, self.steps = 0, 0.8, 0

        def set_mass(self, minv, step):
            self.minv = np.ascontiguousarray(minv, dtype='f8')
            self.dense = int(self.minv.ndim == 2)
            self.lmass = np.ascontiguousarray(np.linalg.cholesky(np.linalg.inv(self.minv)) if self.dense else np.zeros((self.P, self.P)))
            self.dsc[8] = self.dsc[10] = np.log(step)

        def set_state(self, coords):
            lp, g = self.f(coords)
            self.vec[6], self.vec[10], self.vec[7], self.dsc[0] = coords, coords, g, lp
            self.isc[4] = 0

        def buffers(self, quota):
            return (np.zeros((self.C, quota, self.P)), np.zeros((self.C, quota)), np.zeros((self.C, quota, 5)), np.zeros(self.C, dtype='i4'))

        def _kernel(self, buffers, quota, thin_by, mode):
            ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
            rc = self.lib.emu_nuts_kernel(ptr(self.vec), ptr(self.dsc), ptr(self.isc), ptr(self.iter), ptr(self.ids), ptr(self.minv), ptr(self.lmass), ptr(self.lp), ptr(self.g),
                                          *[ptr(b) for b in buffers], self.C, self.P, self.D, self.dense, quota, thin_by, self.adapt, self.threshold, 0., self.target,
                                          self.seed, mode)
            assert rc == 0

        def run(self, nsteps, quota, buffers, thin_by=1):
            self._kernel(buffers, quota, thin_by, 0)
            for _ in range(nsteps):
                lp, g = self.f(self.vec[10].copy())
                self.lp[...], self.g[...] = lp, g
                self._kernel(buffers, quota, thin_by, 1)
            self.steps += nsteps

        def counts(self, buffers):
            return buffers[3]

        def records(self, buffers):
            return buffers[:3]

    return EmuNUTS, _HostNUTS


def _toy_gradient():
    like = ToyGaussianLikelihood()

    def f(q):
        x = q - like.mean
        lp = -0.5 * np.einsum('ij,jk,ik->i', x, like.precision, x) - 0.5 * (q[:, 1] / 10.) ** 2
        g = -x @ like.precision
        g[:, 1] -= q[:, 1] / 100.
        return lp, g
    return like, f


@pytest.mark.parametrize('dense', [False, True])
def test_host_build_of_the_device_step_equals_the_numpy_driver(dense):
    from desilike_amd.nuts import run_batch
    EmuNUTS, HostNUTS = _emu_engine_class()
    like, f = _toy_gradient()
    minv = like.cov if dense else np.diag(like.cov).copy()
    start = like.mean + 0.1 * np.random.RandomState(2).standard_normal((16, 2))
    emu, host = EmuNUTS(f, 16, 2, seed=77), HostNUTS(f, 16, 2, seed=77)
    for engine in (emu, host):
        engine.set_mass(minv, 0.45)
        engine.set_state(start)
    ce, le, ie = run_batch(emu, 200, chunk=50)
    ch, lh, ih = run_batch(host, 200, chunk=50)
    assert np.array_equal(ie[..., :3], ih[..., :3])
    assert np.max(np.abs(ce - ch)) <= 1e-12 and np.allclose(le, lh, rtol=0, atol=1e-11)
    assert ie[..., 0].max() >= 2 and emu.steps == host.steps


# ---- counters, ranks, resume --------------------------------------------------------------------------------------------------------------------------------------
def test_chunking_does_not_change_the_chains():
    from desilike_amd.nuts import _HostNUTS, run_batch
    like, f = _toy_gradient()
    start = like.mean + 0.1 * np.random.RandomState(3).standard_normal((16, 2))
    out = []
    for chunk in (37, 5000):
        engine = _HostNUTS(f, 16, 2, seed=5)
        engine.set_mass(np.diag(like.cov).copy(), 0.4)
        engine.set_state(start)
        out.append(run_batch(engine, 200, chunk=chunk))
    for a, b in zip(*out): assert np.array_equal(a, b)


def _worker(rank, world, port, results):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from desilike_amd.samplers import NUTSSampler
    from desilike_amd.parallel import WalkerSharding
    sampler = NUTSSampler(ToyGaussianLikelihood(), chains=6, seed=4, step_size=0.1, adaptation={'niterations': 60}, sharding=WalkerSharding(min_shard_rows=0))
    assert sampler.chain_world == world
    chains = sampler.run(check_every=80, max_iterations=160)
    results[rank] = (np.array([chain['a'] for chain in chains]), sampler.step_size, np.asarray(sampler.inverse_mass_matrix).copy())
    dist.destroy_process_group()


def test_nuts_chains_over_two_ranks():
    """Chains distributed over a gloo group of two equal the one-process run bit for bit (the draws are keyed by chain id, the warm-up pools every chain)."""
    import torch.multiprocessing as mp
    from desilike_amd.samplers import NUTSSampler
    manager = mp.Manager()
    results = manager.dict()
    port = 41500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, results), nprocs=2, join=True)
    single = NUTSSampler(ToyGaussianLikelihood(), chains=6, seed=4, step_size=0.1, adaptation={'niterations': 60})
    chains = single.run(check_every=80, max_iterations=160)
    a = np.array([chain['a'] for chain in chains])
    for r in (0, 1):
        assert results[r][0].shape == (6, 160) and np.array_equal(results[r][0], a)
        assert results[r][1] == single.step_size and np.array_equal(results[r][2], single.inverse_mass_matrix)


def test_save_and_resume_continue_the_same_chains(tmp_path):
    from desilike_amd.samplers import NUTSSampler
    like = ToyGaussianLikelihood()
    a = NUTSSampler(like, chains=4, seed=6, step_size=0.1, adaptation={'niterations': 40}, save_fn=str(tmp_path / 'c_*.npy'))
    a.run(check_every=50, max_iterations=50)
    b = NUTSSampler(ToyGaussianLikelihood(), chains=[str(tmp_path / 'c_{:d}.npy'.format(i)) for i in range(4)])
    assert b.counter_seed == a.counter_seed and b.step_size == a.step_size and np.array_equal(b._state[2], a._state[2])
    a.save_fn = None
    ca, cb = a.run(check_every=30, max_iterations=30), b.run(check_every=30, max_iterations=30)
    for x, y in zip(ca, cb):
        assert x['a'].shape == (80,) and y['a'].shape == (30,)
        assert np.array_equal(x['a'][50:], y['a']) and np.array_equal(x['logposterior'][50:], y['logposterior'])


def test_arguments():
    from desilike_amd.samplers import NUTSSampler
    like = ToyGaussianLikelihood()
    with pytest.raises(ValueError): NUTSSampler(like, step_size=0.)
    with pytest.raises(ValueError): NUTSSampler(like, step_size=-1.)
    with pytest.raises(ValueError): NUTSSampler(like, max_num_doublings=0)
    with pytest.raises(NotImplementedError, match='integrator'): NUTSSampler(like, integrator='mclachlan')
    with pytest.raises(ValueError): NUTSSampler(like, gradient='jax')
