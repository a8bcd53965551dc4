"""Microcanonical Langevin sampler (desilike_amd/mclmc.py; the reference wraps blackjax.mclmc, samplers/mclmc.py) on the CPU: the momentum update against the
differential equation it solves, the order and reversibility of the integrators, the host build of the device arithmetic (csrc/dl_mclmc.h via
tests/csrc/emulate_mclmc.cpp, also under the sanitizers) against the NumPy statement, what it samples, the rule at a bound of the support, the warm-up, counters,
ranks and resume."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from emulation import SANITIZE_FLAGS
from test_samplers import ToyGaussianLikelihood

HERE = os.path.dirname(os.path.abspath(__file__))
INTEGRATORS = ['isokinetic_leapfrog', 'isokinetic_mclachlan']
_libs = {}


# ---- host build of the device arithmetic ------------------------------------------------------------------------------------------------------------------------
def _emulation():
    """tests/csrc/emulate_mclmc.cpp for the host; with DL_EMULATION_SANITIZE set (a child interpreter started with libasan preloaded: test_host_build_under_the_sanitizers)
    the AddressSanitizer + UndefinedBehaviorSanitizer build."""
    sanitize = bool(os.environ.get('DL_EMULATION_SANITIZE', ''))
    if sanitize in _libs: return _libs[sanitize]
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, 'libdl_emulate_mclmc{}.so'.format('_san' if sanitize else ''))
    src = os.path.join(HERE, 'csrc', 'emulate_mclmc.cpp')
    deps = [src] + [os.path.join(HERE, '..', 'desilike_amd', 'csrc', name) for name in ['dl_mclmc.h', 'dl_nuts.h', 'dl_philox.h']]
    if not os.path.isfile(so) or any(os.path.getmtime(dep) > os.path.getmtime(so) for dep in deps):
        subprocess.check_call(['g++', '-O1' if sanitize else '-O2', '-std=c++17', '-fPIC', '-shared'] + (SANITIZE_FLAGS if sanitize else []) + ['-o', so, src])
    lib = ctypes.CDLL(so)
    lib.emu_mclmc_bstep.argtypes = [ctypes.c_int32] + [ctypes.c_void_p] * 3 + [ctypes.c_double, ctypes.c_void_p]
    lib.emu_mclmc_kernel.argtypes = [ctypes.c_void_p] * 13 + [ctypes.c_int32] * 8 + [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32]
    lib.emu_mclmc_initial_momentum.argtypes = [ctypes.c_int32, ctypes.c_longlong, ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p]
    _libs[sanitize] = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class EmuMCLMC(object):
    """The device's record (csrc/dl_mclmc.h: 7 vector fields, 7 double and 2 int fields per chain) on host arrays, stepped by dl_mclmc.h compiled for the host; the
    interface of _HostMCLMC."""
    NV, ND, NI = 7, 7, 2

    def __init__(self, f, C, P, integrator='isokinetic_mclachlan', seed=0):
        self.lib, self.f, self.C, self.P, self.seed = _emulation(), f, C, P, seed
        self.integrator = INTEGRATORS.index(integrator)
        self.nstage = self.integrator + 1
        self.vec = np.zeros((self.NV, C, P)); self.dsc = np.zeros((self.ND, C)); self.isc = np.zeros((self.NI, C), dtype='i4')
        self.iter = np.zeros(C, dtype='i8'); self.ids = np.arange(C, dtype='i4')
        self.lp, self.g = np.zeros(C), np.zeros((C, P))
        self.hyper = np.array([1., 0., 5e-4, 1.5, 149. / 151.])
        self.adapt, self.moments, self.steps = 0, 0, 0

    def set_preconditioner(self, factor):
        self.fac = np.ascontiguousarray(np.tril(factor) if np.ndim(factor) == 2 else factor, dtype='f8')
        self.dense = int(self.fac.ndim == 2)
        self.fact = np.ascontiguousarray(self.fac.T if self.dense else np.zeros((self.P, self.P)))

    def set_hyper(self, step_size, L):
        self.dsc[1], self.hyper[0] = step_size, L

    def set_state(self, coords, momenta=None, counters=None):
        if counters is not None: self.iter[:] = counters
        if momenta is None:
            momenta = np.zeros((self.C, self.P))
            for c in range(self.C):
                assert self.lib.emu_mclmc_initial_momentum(self.P, int(self.iter[c]), int(self.ids[c]), self.seed, _ptr(momenta[c])) == 0
        lp, g = self.f(np.asarray(coords, dtype='f8'))
        self.vec[0], self.vec[4], self.vec[1], self.vec[2], self.dsc[0] = coords, coords, g, momenta, lp
        self.isc[...] = 0

    def get_state(self):
        return self.vec[0].copy(), self.vec[2].copy(), self.dsc[0].copy(), self.iter.copy(), self.dsc[1].copy()

    def set_adaptation(self, step_size_on, moments_on=False, desired_energy_var=5e-4, trust_in_estimate=1.5, num_effective_samples=150.):
        if step_size_on:
            self.hyper[2:] = desired_energy_var, trust_in_estimate, (num_effective_samples - 1.) / (num_effective_samples + 1.)
            self.dsc[3] = self.dsc[4] = 0.; self.dsc[2] = np.inf
        if moments_on:
            self.vec[5:7] = 0.; self.dsc[6] = 0.
        self.adapt, self.moments = int(bool(step_size_on)), int(bool(moments_on))

    def get_moments(self):
        return self.dsc[6].copy(), self.vec[5].copy(), self.vec[6].copy()

    def buffers(self, quota):
        return (np.zeros((self.C, quota, self.P)), np.zeros((self.C, quota)), np.zeros((self.C, quota, 3)), np.zeros(self.C, dtype='i4'))

    def _kernel(self, buffers, quota, thin_by, stage, open_next):
        rc = self.lib.emu_mclmc_kernel(_ptr(self.vec), _ptr(self.dsc), _ptr(self.isc), _ptr(self.iter), _ptr(self.ids), _ptr(self.fac), _ptr(self.fact), _ptr(self.lp), _ptr(self.g),
                                       *[_ptr(b) for b in buffers], self.C, self.P, self.dense, quota, thin_by, self.integrator, self.adapt, self.moments, _ptr(self.hyper),
                                       self.seed, stage, int(open_next))
        assert rc == 0

    def run(self, nsteps, quota, buffers, thin_by=1):
        if not nsteps: return
        self._kernel(buffers, quota, thin_by, -1, 0)
        for s in range(nsteps):
            for stage in range(self.nstage):
                lp, g = self.f(self.vec[4].copy())
                self.lp[...], self.g[...] = lp, g
                self._kernel(buffers, quota, thin_by, stage, s + 1 < nsteps)
        self.steps += nsteps

    def counts(self, buffers):
        return buffers[3]

    def records(self, buffers):
        return buffers[:3]


def _gaussian(mean, cov, box=None):
    """f(q [C, P]) -> (log-density, gradient) of N(mean, cov), -inf outside ``box`` = (lower, upper)."""
    prec = np.linalg.inv(cov)

    def f(q):
        x = q - mean
        lp, g = -0.5 * np.einsum('ij,jk,ik->i', x, prec, x), -x @ prec
        if box is not None:
            with np.errstate(invalid='ignore'):
                lp = np.where(np.all((q >= box[0]) & (q <= box[1]), axis=1), lp, -np.inf)
        return lp, g
    return f


def _host(f, C, P, fac, eps, L, start, integrator='isokinetic_mclachlan', seed=0, cls=None):
    from desilike_amd.mclmc import _HostMCLMC
    engine = (cls or _HostMCLMC)(f, C, P, integrator=integrator, seed=seed)
    engine.set_preconditioner(fac)
    engine.set_hyper(eps, L)
    engine.set_state(start)
    return engine


# ---- the momentum update ----------------------------------------------------------------------------------------------------------------------------------------
def _rk4_flow(u, g, d, nsub):
    """du/dt = (1 - u u^T) g / (d - 1) over unit time (g the gradient of the log-density: -grad S)."""
    rhs = lambda v: (g - v * (v @ g)) / (d - 1)
    h = 1. / nsub
    for _ in range(nsub):
        k1 = rhs(u); k2 = rhs(u + 0.5 * h * k1); k3 = rhs(u + 0.5 * h * k2); k4 = rhs(u + h * k3)
        u = u + (h / 6.) * (k1 + 2. * k2 + 2. * k3 + k4)
    return u


@pytest.mark.parametrize('d', [2, 5])
def test_b_step_is_the_exact_flow(d):
    """B(eps) against an RK4 integration of du/dt = -(1 - u u^T) grad S / (d - 1) (eps = 1, |g| = delta (d - 1)): 1e-10 on u with substeps whose halving moves the
    solution by less than 1e-11; |u| = 1 to 1e-15; dK against (d - 1) log(cosh delta + (e.u) sinh delta) in extended precision.  The flow contracts towards e, so the
    integration errors of large delta are damped.  Bound on dK: the inputs e.u and delta carry a few double roundings (relative 8 eps each: d (e.u) dK/d(e.u) and
    delta dK/d(delta) are at most (d - 1) delta and (d - 1) max(delta, 1)), the extended-precision reference log(1 + ...) an absolute 4 eps_long."""
    lib = _emulation()
    rng = np.random.RandomState(10 + d)
    eps_d, eps_l = np.finfo('f8').eps, np.finfo(np.longdouble).eps
    for delta, nsub in [(1e-8, 8), (1., 2000), (50., 40000)]:
        u0 = rng.standard_normal(d); u0 /= np.sqrt(u0 @ u0)
        g = rng.standard_normal(d); g *= delta * (d - 1) / np.sqrt(g @ g)
        u, dk = u0.copy(), np.zeros(1)
        assert lib.emu_mclmc_bstep(d, _ptr(u), _ptr(g), _ptr(np.ones(d)), 1., _ptr(dk)) == 0
        fine, coarse = _rk4_flow(u0, g, d, nsub), _rk4_flow(u0, g, d, nsub // 2)
        assert np.max(np.abs(fine - coarse)) < 1e-11
        assert np.max(np.abs(u - fine)) < 1e-10, (delta, u, fine)
        assert abs(np.sqrt(u @ u) - 1.) <= 1e-15
        gl, ul, dl = g.astype(np.longdouble), u0.astype(np.longdouble), np.longdouble(delta)
        eu = (gl @ ul) / np.sqrt(gl @ gl)
        dl = np.sqrt(gl @ gl) / (d - 1)
        if delta <= 1.: ref = (d - 1) * np.log(np.cosh(dl) + eu * np.sinh(dl))
        else: ref = (d - 1) * (dl + np.log(0.5 * (1. + eu) + 0.5 * (1. - eu) * np.exp(-2. * dl)))      # (the same quantity, cosh and sinh divided by exp(delta))
        assert abs(dk[0] - float(ref)) <= (d - 1) * (16. * eps_d * max(delta, 1.) * min(delta, 1.) + 4. * eps_l) + eps_d * abs(float(ref)), (delta, dk[0], float(ref))
    # |g| = 0: the identity
    u = u0.copy()
    assert lib.emu_mclmc_bstep(d, _ptr(u), _ptr(np.zeros(d)), _ptr(np.ones(d)), 1., _ptr(dk)) == 0
    assert np.array_equal(u, u0) and dk[0] == 0.


# ---- the integrators --------------------------------------------------------------------------------------------------------------------------------------------
COV3 = np.array([[1., 0.6, 0.3], [0.6, 1.5, -0.4], [0.3, -0.4, 0.8]])


def _energy_error(integrator, eps, time=6., C=8):
    from desilike_amd.mclmc import run_batch
    start = np.random.RandomState(5).multivariate_normal(np.zeros(3), COV3, size=C)
    engine = _host(_gaussian(np.zeros(3), COV3), C, 3, np.ones(3), eps, np.inf, start, integrator=integrator, seed=3)
    info = run_batch(engine, int(round(time / eps)), chunk=1000)[2]
    assert not info[..., 1].any()
    return np.max(np.abs(np.cumsum(info[..., 0], axis=1)))


def test_order_of_the_integrators():
    """Second order: halving eps divides max |sum dE| over a fixed integration time by 4.  Measured here (3-dimensional correlated Gaussian, 8 chains, time 6, L = inf):
    eps 0.05 -> 0.025: leapfrog 2.236e-3 -> 5.580e-4, ratio 4.007; mclachlan 1.530e-4 -> 3.805e-5, ratio 4.022."""
    errors = {}
    for integrator in INTEGRATORS:
        coarse, fine = _energy_error(integrator, 0.05), _energy_error(integrator, 0.025)
        print(integrator, coarse, fine, coarse / fine)
        assert 3.5 <= coarse / fine <= 4.5, (integrator, coarse, fine)
        errors[integrator] = coarse
    assert errors['isokinetic_mclachlan'] < errors['isokinetic_leapfrog']


@pytest.mark.parametrize('integrator', INTEGRATORS)
def test_time_reversal(integrator):
    from desilike_amd.mclmc import run_batch
    start = np.random.RandomState(6).multivariate_normal(np.zeros(3), COV3, size=8)
    fac = np.linalg.cholesky(COV3)
    engine = _host(_gaussian(np.zeros(3), COV3), 8, 3, fac, 0.1, np.inf, start, integrator=integrator, seed=4)
    u0 = engine.get_state()[1]
    run_batch(engine, 50)
    x, u, _, counters, _ = engine.get_state()
    assert np.max(np.abs(x - start)) > 0.5
    engine.set_state(x, momenta=-u, counters=counters)
    run_batch(engine, 50)
    x, u = engine.get_state()[:2]
    assert np.max(np.abs(x - start)) <= 1e-11 and np.max(np.abs(u + u0)) <= 1e-11


# ---- host build against the NumPy statement -----------------------------------------------------------------------------------------------------------------------
def _share(host, emu):
    """The state of the NumPy statement copied into the host build's record."""
    for field, name in enumerate(['x', 'g', 'u', 'u0', 'xn', 'sx', 'sxx']): emu.vec[field] = host.v[name]
    for field, name in enumerate(['lp', 'eps', 'epsmax', 'ca', 'cb', 'dk', 'sw']): emu.dsc[field] = host.d[name]
    emu.iter[:] = host.iter


@pytest.mark.parametrize('integrator', INTEGRATORS)
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('P', [2, 3, 64])
def test_host_build_of_the_device_stage_equals_the_numpy_statement(P, dense, integrator):
    """16 chains, 200 steps, the controller and the moments on for the first 80; a box on the first two components so that steps are undone.

    Same arithmetic in the same order, but libm and NumPy differ in the last bit of exp / log / sin / cos, from the first step on (measured: dE of step 0 differs by
    1.4e-17).  Carried freely over 200 steps the difference grows to 1e-14 .. 1e-13 on the positions, and an element that passes near zero then misses a relative
    1e-12; so, beside a free run of 200 steps (identical flags and counters; values to 1e-9, the carried last bits), the two are compared STEP BY STEP FROM A SHARED
    STATE: positions, log-posteriors, step sizes in use and adapted to rtol 1e-12 element by element (measured at most 7.6e-13, 1.3e-15, 0, 7.1e-13).  Two quantities
    cannot be held to 1e-12 of THEMSELVES by any arithmetic that has a last-bit difference in it, and are held to 1e-12 of what they are made of: a component of the
    unit momentum, relative to the vector's norm 1 (a component can be arbitrarily close to 0; measured 6e-12 of itself); dE = sum dK - (lp' - lp), a difference of
    terms up to 1e4 times larger than itself, relative to |lp'| + |lp| + |dE| (measured up to 7e-8 of itself where dE is about 1e-7)."""
    from desilike_amd.mclmc import run_batch
    rng = np.random.RandomState(P)
    B = rng.standard_normal((P, P)) / np.sqrt(P)
    cov = B @ B.T + np.eye(P)
    box = (np.array([-1.2, -1.5] + [-np.inf] * (P - 2)), np.array([1.5, 1.2] + [np.inf] * (P - 2)))
    f = _gaussian(np.zeros(P), cov, box=box)
    fac = np.linalg.cholesky(cov) if dense else np.sqrt(np.diag(cov))
    start = rng.uniform(-1., 1., size=(16, P))
    control = dict(desired_energy_var=1e-3, trust_in_estimate=1.5, num_effective_samples=50)
    # free run
    out = []
    for cls in (EmuMCLMC, None):
        engine = _host(f, 16, P, fac, 0.4, 1.5, start, integrator=integrator, seed=77, cls=cls)
        engine.set_adaptation(True, True, **control)
        first = run_batch(engine, 80, chunk=33)
        moments = engine.get_moments()
        engine.set_adaptation(False, False)
        second = run_batch(engine, 60, thin_by=2, chunk=50)
        out.append([np.concatenate([a, b], axis=1) for a, b in zip(first, second)] + list(engine.get_state()) + list(moments) + [engine.steps])
    ie, ih = out[0][2], out[1][2]
    assert np.array_equal(ie[..., 1], ih[..., 1]) and 0 < ie[..., 1].sum() < ie[..., 1].size / 2
    assert out[0][-1] == out[1][-1] == 200 and np.array_equal(out[0][6], np.full(16, 200)) and np.array_equal(out[1][6], np.full(16, 200))
    for a, b in zip(out[0][:-1], out[1][:-1]): assert np.allclose(a, b, rtol=1e-9, atol=1e-9)
    assert ie[:, :80, 2].std() > 0. and np.all(ie[:, 80:, 2] == ie[:, 80:81, 2])
    # step by step from a shared state
    emu = _host(f, 16, P, fac, 0.4, 1.5, start, integrator=integrator, seed=77, cls=EmuMCLMC)
    host = _host(f, 16, P, fac, 0.4, 1.5, start, integrator=integrator, seed=77)
    close = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=0.)
    nflag = 0
    for step in range(200):
        if step in (0, 80):
            for engine in (emu, host): engine.set_adaptation(step == 0, step == 0, **control)
        _share(host, emu)
        lp0 = host.d['lp'].copy()
        (ce, le, ie), (ch, lh, ih) = run_batch(emu, 1), run_batch(host, 1)
        assert np.array_equal(ie[..., 1], ih[..., 1])
        nflag += int(ih[..., 1].sum())
        assert close(ce, ch) and close(le, lh) and np.array_equal(ie[..., 2], ih[..., 2])
        assert np.all(np.abs(ie[:, 0, 0] - ih[:, 0, 0]) <= 1e-12 * (np.abs(lh[:, 0]) + np.abs(lp0) + np.abs(ih[:, 0, 0])))
        (xe, ue, lpe, ite, epse), (xh, uh, lph, ith, epsh) = emu.get_state(), host.get_state()
        assert close(xe, xh) and close(lpe, lph) and close(epse, epsh) and np.array_equal(ite, ith)
        assert np.max(np.abs(ue - uh)) <= 1e-12
        for a, b in zip(emu.get_moments(), host.get_moments()): assert close(a, b)
    assert nflag > 0


def _sanitized_run():
    from desilike_amd.mclmc import run_batch
    P = 5
    f = _gaussian(np.zeros(P), np.eye(P), box=(np.full(P, -1.5), np.full(P, 1.5)))
    start = np.random.RandomState(1).uniform(-1., 1., size=(5, P))
    for dense in (False, True):
        for integrator in INTEGRATORS:
            engine = _host(f, 5, P, np.eye(P) if dense else np.ones(P), 0.5, 2., start, integrator=integrator, seed=2, cls=EmuMCLMC)
            engine.set_adaptation(True, True)
            info = run_batch(engine, 40, thin_by=2, chunk=7)[2]
            assert info[..., 1].sum() > 0


def test_host_build_under_the_sanitizers():
    """csrc/dl_mclmc.h compiled with AddressSanitizer + UndefinedBehaviorSanitizer (tests/emulation.py SANITIZE_FLAGS), driven through the tests of this file in a child
    interpreter with libasan preloaded; any report fails the test."""
    import sys
    libasan = subprocess.check_output(['g++', '-print-file-name=libasan.so']).decode().strip()
    assert os.path.isabs(libasan) and os.path.isfile(libasan), 'libasan not found'
    code = ('import sys; sys.path.insert(0, {here!r}); sys.path.insert(0, {root!r})\n'
            'import test_mclmc as t\n'
            'for d in (2, 5): t.test_b_step_is_the_exact_flow(d)\n'
            't._sanitized_run()\n'
            't.test_host_build_of_the_device_stage_equals_the_numpy_statement(3, True, "isokinetic_mclachlan")\n'
            'print("sanitized emulation ok")\n').format(here=HERE, root=os.path.dirname(HERE))
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1', DL_EMULATION_SANITIZE='1')
    out = subprocess.run([sys.executable, '-c', code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = out.stderr.decode()
    assert out.returncode == 0 and 'sanitized emulation ok' in out.stdout.decode(), err[-3000:]
    assert 'AddressSanitizer' not in err and 'runtime error' not in err, err[-3000:]


# ---- what it samples --------------------------------------------------------------------------------------------------------------------------------------------
def _check_moments(coords, mean, var, nsigma=5.):
    """Means and variances of coords [C, n, P] within ``nsigma`` standard errors, the errors from the chains' own integrated autocorrelation times."""
    from desilike_amd.diagnostics import integrated_autocorrelation_time
    C, n, P = coords.shape
    flat = coords.reshape(-1, P)
    m, v = flat.mean(axis=0), flat.var(axis=0)
    se_mean = np.sqrt(v * integrated_autocorrelation_time(coords) / (C * n))
    squares = (coords - m)**2
    se_var = np.sqrt(squares.reshape(-1, P).var(axis=0) * integrated_autocorrelation_time(squares) / (C * n))
    print('mean', (m - mean) / se_mean, 'var', (v - var) / se_var if var is not None else None)
    assert np.all(np.abs(m - mean) < nsigma * se_mean), (m, mean, se_mean)
    if var is not None: assert np.all(np.abs(v - var) < nsigma * se_var), (v, var, se_var)


@pytest.mark.parametrize('integrator', INTEGRATORS)
def test_mclmc_samples_a_standard_normal(integrator):
    from desilike_amd.mclmc import run_batch
    start = np.random.RandomState(7).standard_normal((32, 4))
    engine = _host(_gaussian(np.zeros(4), np.eye(4)), 32, 4, np.ones(4), 0.4, 2., start, integrator=integrator, seed=8)
    coords = run_batch(engine, 1200, chunk=400)[0][:, 200:]
    _check_moments(coords, np.zeros(4), np.ones(4))


def test_mclmc_samples_a_correlated_gaussian_with_the_dense_preconditioner():
    from desilike_amd.mclmc import run_batch
    cov = np.array([[1., 0.9], [0.9, 1.]])
    start = np.random.RandomState(8).multivariate_normal(np.zeros(2), cov, size=32)
    engine = _host(_gaussian(np.zeros(2), cov), 32, 2, np.linalg.cholesky(cov), 0.3, 1.5, start, seed=9)
    coords = run_batch(engine, 1200, chunk=400)[0][:, 200:]
    _check_moments(coords, np.zeros(2), np.ones(2))
    rho = np.corrcoef(coords.reshape(-1, 2).T)[0, 1]
    assert abs(rho - 0.9) < 0.02


@pytest.mark.parametrize('integrator', INTEGRATORS)
def test_bounded_support(integrator):
    """Uniform on [0, 1]^2 times a Gaussian wider than the box: steps that leave it are undone, so no recorded point lies outside; the marginal means are right."""
    from desilike_amd.mclmc import run_batch
    f = _gaussian(np.full(2, 0.5), 4. * np.eye(2), box=(np.zeros(2), np.ones(2)))
    start = np.random.RandomState(9).uniform(0.05, 0.95, size=(32, 2))
    engine = _host(f, 32, 2, np.ones(2), 0.15, 0.6, start, integrator=integrator, seed=10)
    coords, logp, info = run_batch(engine, 1200, chunk=400)
    assert np.all((coords >= 0.) & (coords <= 1.)) and np.all(np.isfinite(logp))
    assert info[..., 1].sum() > 0 and np.all(info[..., 0][info[..., 1] == 1] == 0.)
    _check_moments(coords[:, 200:], np.full(2, 0.5), None)


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------------------------------
class AnisotropicLikelihood(ToyGaussianLikelihood):
    """Scales 1 : 100."""

    def __init__(self):
        super(AnisotropicLikelihood, self).__init__()
        self.mean, self.cov = np.array([0.5, -0.3]), np.diag([0.01**2, 1.])
        self.precision = np.linalg.inv(self.cov)


def test_warmup():
    """Diagonal preconditioning on scales 1 : 100 (the prior of b, N(0, 10), narrows its scale by 0.5 %): the recovered ratio within 20 %; E[dE^2] / d of a run after the
    warm-up within a factor 3 of desired_energy_var.  Measured here: ratio 99.8 (0.2 % off, bound 20 %), energy variance 0.62 x desired (a factor 1.6, bound 3)."""
    from desilike_amd.samplers import MCLMCSampler
    sampler = MCLMCSampler(AnisotropicLikelihood(), chains=16, seed=12, adaptation={'niterations': 1000})
    sampler.run(check_every=300, max_iterations=300)
    sigma = sampler.hyp['sqrt_diag_cov'] * sampler.scale
    ratio = sigma[1] / sigma[0]
    realised = np.mean(sampler.energy_change**2) / 2. / 5e-4
    print('ratio', ratio, 'energy variance / desired', realised, sampler.hyp)
    assert abs(ratio / 100. - 1.) < 0.2
    assert 1. / 3. < realised < 3.
    assert sampler.hyp['L'] > 0. and sampler.hyp['step_size'] > 0.


def test_mclmc_recovers_the_toy_posterior(tmp_path):
    from desilike_amd.samplers import MCLMCSampler
    like = ToyGaussianLikelihood()
    sampler = MCLMCSampler(like, chains=32, seed=4, adaptation={'niterations': 400, 'dense_preconditioning': True}, save_fn=str(tmp_path / 'mclmc_*.npy'))
    assert not sampler.device_resident
    chains = sampler.run(check_every=400, max_iterations=800, check={'max_eigen_gr': 0.05, 'stable_over': 1})
    x = np.column_stack([np.concatenate([chain[name][50:] for chain in chains]) for name in ['a', 'b']])
    assert np.allclose(x.mean(axis=0), like.mean, atol=0.03)
    assert np.allclose(x.std(axis=0), np.diag(like.cov)**0.5, rtol=0.07)
    assert sampler.hyp['factor'].shape == (2, 2) and (tmp_path / 'mclmc_31.npy').exists()


def test_chunking_does_not_change_the_chains():
    from desilike_amd.mclmc import run_batch
    f = _gaussian(np.zeros(3), COV3, box=(np.full(3, -2.), np.full(3, 2.)))
    start = np.random.RandomState(3).uniform(-1., 1., size=(16, 3))
    out = []
    for chunk in (7, 5000):
        engine = _host(f, 16, 3, np.ones(3), 0.5, 2., start, seed=5)
        engine.set_adaptation(True, True)
        out.append(run_batch(engine, 100, thin_by=2, chunk=chunk) + tuple(engine.get_state()) + tuple(engine.get_moments()))
    for a, b in zip(*out): assert np.array_equal(a, b)
    assert out[0][2][..., 1].sum() > 0


def _worker(rank, world, port, results):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from desilike_amd.samplers import MCLMCSampler
    from desilike_amd.parallel import WalkerSharding
    sampler = MCLMCSampler(ToyGaussianLikelihood(), chains=6, seed=4, adaptation={'niterations': 200}, sharding=WalkerSharding(min_shard_rows=0))
    assert sampler.chain_world == world
    chains = sampler.run(check_every=80, max_iterations=160)
    results[rank] = (np.array([chain['a'] for chain in chains]), sampler.hyp)
    dist.destroy_process_group()


def test_mclmc_chains_over_two_ranks():
    """Chains distributed over a gloo group of two equal the one-process run bit for bit (the draws are keyed by chain id, the warm-up pools every chain)."""
    import torch.multiprocessing as mp
    from desilike_amd.samplers import MCLMCSampler
    manager = mp.Manager()
    results = manager.dict()
    port = 43500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, results), nprocs=2, join=True)
    single = MCLMCSampler(ToyGaussianLikelihood(), chains=6, seed=4, adaptation={'niterations': 200})
    chains = single.run(check_every=80, max_iterations=160)
    a = np.array([chain['a'] for chain in chains])
    for r in (0, 1):
        assert results[r][0].shape == (6, 160) and np.array_equal(results[r][0], a)
        assert results[r][1]['step_size'] == single.hyp['step_size'] and results[r][1]['L'] == single.hyp['L']
        assert np.array_equal(results[r][1]['sqrt_diag_cov'], single.hyp['sqrt_diag_cov'])


def test_save_and_resume_continue_the_same_chains(tmp_path):
    from desilike_amd.samplers import MCLMCSampler
    like = ToyGaussianLikelihood()
    a = MCLMCSampler(like, chains=4, seed=6, integrator='isokinetic_leapfrog', adaptation={'niterations': 200}, save_fn=str(tmp_path / 'c_*.npy'))
    a.run(check_every=50, max_iterations=50)
    b = MCLMCSampler(ToyGaussianLikelihood(), chains=[str(tmp_path / 'c_{:d}.npy'.format(i)) for i in range(4)])
    assert b.counter_seed == a.counter_seed and b.step_size == a.step_size and b.L == a.L and np.array_equal(b._state[2], a._state[2])
    assert b.mclmc_integrator == 'isokinetic_leapfrog' and np.array_equal(b._momenta, a._momenta) and np.array_equal(b.preconditioner, a.preconditioner)
    a.save_fn = None
    ca, cb = a.run(check_every=30, max_iterations=30), b.run(check_every=30, max_iterations=30)
    for x, y in zip(ca, cb):
        assert x['a'].shape == (80,) and y['a'].shape == (30,)
        assert np.array_equal(x['a'][50:], y['a']) and np.array_equal(x['logposterior'][50:], y['logposterior'])


def test_arguments():
    from desilike_amd.samplers import MCLMCSampler
    from desilike_amd.mclmc import _HostMCLMC
    like = ToyGaussianLikelihood()
    with pytest.raises(ValueError): MCLMCSampler(like, step_size=0.)
    with pytest.raises(ValueError): MCLMCSampler(like, L=-1.)
    with pytest.raises(ValueError, match='integrator'): MCLMCSampler(like, integrator='velocity_verlet')
    with pytest.raises(ValueError): MCLMCSampler(like, gradient='jax')
    with pytest.raises(ValueError): MCLMCSampler(like, chains=0)
    one = ToyGaussianLikelihood()
    one.varied_params = type(one.varied_params)([one.varied_params['a']])
    with pytest.raises(ValueError, match='d - 1 = 0'): MCLMCSampler(one)
    f = _gaussian(np.zeros(1), np.eye(1))
    with pytest.raises(ValueError, match='d - 1 = 0'): _HostMCLMC(f, 4, 1)
    with pytest.raises(ValueError, match='integrator'): _HostMCLMC(f, 4, 2, integrator='yoshida')
    engine = _HostMCLMC(_gaussian(np.zeros(2), np.eye(2)), 2, 2)
    with pytest.raises(ValueError, match='unit'): engine.set_state(np.zeros((2, 2)), momenta=np.ones((2, 2)))
    with pytest.raises(ValueError, match='finite'): engine.set_state(np.full((2, 2), np.nan))
    # without adaptation: L and step_size as given, identity preconditioner in the proposal-scaled coordinates
    sampler = MCLMCSampler(like, chains=4, seed=1, adaptation=False, L=0.7, step_size=0.2)
    sampler.run(check_every=10, max_iterations=10)
    assert sampler.hyp['L'] == 0.7 and sampler.hyp['step_size'] == 0.2 and np.array_equal(sampler.hyp['sqrt_diag_cov'], np.ones(2))
    with pytest.raises(AttributeError): sampler.mean_tree_depth
    assert np.all(sampler.acceptance_rate <= 1.)
