"""Oracle of the posterior draws of analytically solved parameters (tests/test_sample_solved.py, tests/test_gpu_sample_solved.py): a NumPy restatement of the
reference's ``Chain.sample_solved`` (desilike/samples/chain.py:229-263) with its ``_get_solved_covariance`` (46-76), the Python mirror of the draw addressing of
csrc/dl_sample_solved.h, and the CPU build of the device's lane function (tests/csrc/emulate_sample_solved.cpp).  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

from desilike_amd.samplers import CounterRNG

HERE = os.path.dirname(os.path.abspath(__file__))
SOLVED_STREAM = 80
EPS = np.finfo('f8').eps


def gauss(seed, index, draw, ns):
    """Standard Gaussians ``[len(index), len(draw), ns]``: Philox4x32-10 keyed by ``seed``, counter (index lo, index hi, draw, 80 | pair << 8), Box-Muller pair
    ``pair`` -> components 2 pair, 2 pair + 1."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    index, draw = np.asarray(index, dtype=np.uint64)[:, None], np.asarray(draw, dtype=np.uint32)[None, :]
    shape = (index.shape[0], draw.shape[1])
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32), shape + (2,))
    z = np.empty(shape + (ns + (ns & 1),), dtype='f8')
    for pair in range((ns + 1) // 2):
        counter = np.empty(shape + (4,), dtype=np.uint32)
        counter[..., 0], counter[..., 1] = (index & np.uint64(0xFFFFFFFF)).astype(np.uint32), (index >> np.uint64(32)).astype(np.uint32)
        counter[..., 2], counter[..., 3] = draw, SOLVED_STREAM | (pair << 8)
        z[..., 2 * pair], z[..., 2 * pair + 1] = CounterRNG.box_muller(CounterRNG.philox4x32(counter, key))
    return z[..., :ns]


def solved_covariance(hessian_l, prec):
    """chain.py:46-63: Hessian of loglikelihood + logprior w.r.t. the solved parameters, covariance = symmetrised inverse of minus it."""
    hessian = np.asarray(hessian_l, dtype='f8') - np.diag(prec)
    covariance = np.linalg.inv(-hessian)
    return (np.swapaxes(covariance, -1, -2) + covariance) / 2., hessian


def sample_solved(xhat, hessian_l, prec, is_marg, z):
    """One point: ``xhat [ns]``, likelihood Hessian ``hessian_l [ns, ns]``, prior precisions ``prec [ns]``, ``is_marg [ns]``, standard Gaussians ``z [size, ns]`` ->
    (x [size, ns], dloglike [size], dlogprior [size]).

    chain.py:241-262 line by line, but for the square root of the covariance: the reference multiplies its noise by the lower Cholesky factor of the covariance,
    the device by C^-T with C C^T = -hessian (the factor it has anyway).  Both roots R satisfy R R^T = covariance; the values are those of the device's root so
    that the same ``z`` gives comparable numbers."""
    xhat, prec, z = np.asarray(xhat, dtype='f8'), np.asarray(prec, dtype='f8'), np.atleast_2d(np.asarray(z, dtype='f8'))
    covariance, hessian = solved_covariance(hessian_l, prec)
    np.linalg.cholesky(covariance)                                       # (chain.py:242: raises unless the covariance is positive definite)
    root = np.linalg.inv(np.linalg.cholesky(-hessian)).T                 # C^-T
    assert np.allclose(root.dot(root.T), covariance, rtol=1e-8, atol=1e-12 * np.abs(covariance).max())
    values = z.dot(root.T)                                               # chain.py:248: sum_j L[i, j] noise[j]
    x = xhat + values                                                    # 250
    dlogs = []
    for hess in [np.asarray(hessian_l, dtype='f8'), -np.diag(prec)]:     # 252-256: loglikelihood, logprior
        dlogs.append(0.5 * np.einsum('di,ij,dj->d', values, hess, values))
    marg = np.flatnonzero(is_marg)
    if marg.size:                                                        # 257-261
        dlogs[0] = dlogs[0] + 0.5 * np.linalg.slogdet(-hessian[np.ix_(marg, marg)])[1]
    return x, dlogs[0], dlogs[1]


def draw_bound(hessian_l, prec):
    """(C, bound): NumPy's Cholesky factor of A = -hessian_l + diag(prec) and the bound 100 cond(A) eps on every component of |C^T (x - xhat) - z|."""
    A = -np.asarray(hessian_l, dtype='f8') + np.diag(prec)
    return np.linalg.cholesky(A), 100. * np.linalg.cond(A) * EPS


# ---- CPU build of the lane function ---------------------------------------------------------------------------------------------------------
SANITIZE_FLAGS = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g']
_emu = None


def _build(target, flags):
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, target)
    src = os.path.join(HERE, 'csrc', 'emulate_sample_solved.cpp')
    deps = [src] + [os.path.join(HERE, '..', 'desilike_amd', 'csrc', header) for header in ['dl_sample_solved.h', 'dl_philox.h', 'dl_fullshape.h']]
    if not os.path.isfile(out) or any(os.path.getmtime(dep) > os.path.getmtime(out) for dep in deps):
        subprocess.check_call(['g++', '-std=c++17'] + flags + ['-o', out, src])
    return out


def load_emulation():
    """The shared object (no sanitizer), loaded by ctypes."""
    global _emu
    if _emu is None:
        lib = ctypes.CDLL(_build('libdl_emulate_sample_solved.so', ['-O2', '-fPIC', '-shared']))
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        lib.ss_sample_solved.argtypes = [ctypes.c_int32, dp, dp, dp, ip, dp, dp, ip, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, dp, dp, dp, ip]
        lib.ss_sample_solved.restype = ctypes.c_int
        _emu = lib
    return _emu


def build_standalone():
    """The same source as a program of its own under the address / undefined-behaviour sanitizers (host code only; nothing of it is loaded into python)."""
    return _build('emulate_sample_solved_asan', ['-O1', '-DSS_STANDALONE'] + SANITIZE_FLAGS)


def emulate(hessian_l, xhat, prec, is_marg, loglike, logprior, status, index0, size, seed):
    """The lane function on the CPU: ``hessian_l [B, ns, ns]``, ``xhat [B, ns]``, ... -> (x [B, size, ns], loglike [B, size], logprior [B, size], status [B])."""
    lib = load_emulation()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    hessian_l, xhat = np.ascontiguousarray(hessian_l, dtype='f8'), np.ascontiguousarray(xhat, dtype='f8')
    B, ns = xhat.shape
    prec, is_marg = np.ascontiguousarray(prec, dtype='f8'), np.ascontiguousarray(is_marg, dtype='i4')
    loglike, logprior = np.ascontiguousarray(np.broadcast_to(loglike, B), dtype='f8'), np.ascontiguousarray(np.broadcast_to(logprior, B), dtype='f8')
    status = np.ascontiguousarray(np.broadcast_to(status, B), dtype='i4')
    x, ll, lp, st = np.empty((B, size, ns)), np.empty((B, size)), np.empty((B, size)), np.empty(B, dtype='i4')
    rc = lib.ss_sample_solved(ns, hessian_l.ctypes.data_as(dp), xhat.ctypes.data_as(dp), prec.ctypes.data_as(dp), is_marg.ctypes.data_as(ip), loglike.ctypes.data_as(dp),
                              logprior.ctypes.data_as(dp), status.ctypes.data_as(ip), B, int(index0), int(size), int(seed) & 0xFFFFFFFFFFFFFFFF, x.ctypes.data_as(dp),
                              ll.ctypes.data_as(dp), lp.ctypes.data_as(dp), st.ctypes.data_as(ip))
    assert rc == 0
    return x, ll, lp, st


def random_case(rng, B, ns, pattern, gaussian):
    """Inputs of the host tests: H_L = -T T^T with T [ns, ns + 4] standard normal (well conditioned by construction), ``pattern`` 'marg' | 'mixed' | 'best',
    ``gaussian``: every other parameter has a Gaussian prior, else all flat."""
    T = rng.standard_normal((B, ns, ns + 4))
    hessian_l = -np.einsum('bik,bjk->bij', T, T)
    xhat = rng.standard_normal((B, ns))
    is_marg = {'marg': np.ones(ns, dtype='i4'), 'best': np.zeros(ns, dtype='i4'), 'mixed': (np.arange(ns) % 2 == 0).astype('i4')}[pattern]
    prec = np.where(np.arange(ns) % 2 == 1, 0.5 + np.arange(ns), 0.) if gaussian else np.zeros(ns)
    if gaussian and ns == 1: prec = np.array([0.7])
    return hessian_l, xhat, prec, is_marg
