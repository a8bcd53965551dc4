"""Shared pieces of the BAO phase-shift tests (tests/test_bao_phaseshift.py, tests/test_gpu_bao_phaseshift.py): fixtures of tests/golden/make_phaseshift_fixture.py, the same
pipelines from the mirror classes, and the CPU emulation of the new device phases (tests/csrc/emulate_phaseshift.cpp).  Test infrastructure only."""
import ctypes
import os
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ['pk', 'xi', 'models', 'clip']
_cache = {}


def load_fixture(name):
    """(archive, {dl_config key: array}) of ``boundary_phaseshift_<name>.npz``, read once."""
    if name not in _cache:
        g = np.load(os.path.join(HERE, 'golden', 'boundary_phaseshift_{}.npz'.format(name)))
        g = {key: g[key] for key in g.files}
        _cache[name] = (g, {key[4:]: value for key, value in g.items() if key.startswith('cfg/')})
    return _cache[name]


def covariance(n, scale, seed=4):
    """The covariance of the generator (tests/golden/make_phaseshift_fixture.py::covariance)."""
    rng = np.random.RandomState(seed)
    A = rng.standard_normal((n, n)) * scale
    return A.dot(A.T) + (10. * scale)**2 * np.eye(n)


def make_likelihood(name, **template_options):
    """The pipeline of fixture 'pk', 'xi' or 'clip' from the mirror classes; the data vector is the fixture's."""
    from desilike_amd.theories.galaxy_clustering import (BAOPhaseShiftPowerSpectrumTemplate, DampedBAOWigglesTracerPowerSpectrumMultipoles,
                                                         DampedBAOWigglesTracerCorrelationFunctionMultipoles)
    from desilike_amd.observables.galaxy_clustering import TracerCorrelationFunctionMultipolesObservable, TracerPowerSpectrumMultipolesObservable
    from desilike_amd.likelihoods import ObservablesGaussianLikelihood
    g, cfg = load_fixture(name)
    options = dict(z=0.5, fiducial='synthetic')
    if name == 'clip': options.update(apmode='qiso', klim_wiggles=(2e-4, 1.01))
    options.update(template_options)
    template = BAOPhaseShiftPowerSpectrumTemplate(**options)
    if name == 'xi':
        theory = DampedBAOWigglesTracerCorrelationFunctionMultipoles(template=template, mode='reciso')
        obs = TracerCorrelationFunctionMultipolesObservable(data=cfg['obs0.flatdata'], s=np.linspace(22.5, 167.5, 30), ells=(0, 2), theory=theory)
        cov = covariance(60, 3e-4)
    else:
        theory = DampedBAOWigglesTracerPowerSpectrumMultipoles(template=template)
        obs = TracerPowerSpectrumMultipolesObservable(data=cfg['obs0.flatdata'], kedges=np.linspace(0.02, 0.3, 57), ells=(0, 2), wmatrix={'resolution': 3}, theory=theory)
        cov = covariance(112, 30.)
    for pname in ['sigmapar', 'sigmaper']:
        theory.init.params[pname].update(fixed=False, ref=dict(dist='norm', loc=8., scale=0.5))
    return g, ObservablesGaussianLikelihood(observables=[obs], covariance=cov)


# ---- CPU emulation of the device phases -------------------------------------------------------------------------------------------------------
SANITIZE_FLAGS = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g']
_emu = None


def _build(target, flags):
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, target)
    src = os.path.join(HERE, 'csrc', 'emulate_phaseshift.cpp')
    deps = [src] + [os.path.join(HERE, '..', 'desilike_amd', 'csrc', header) for header in ['dl_fullshape.h', 'dl_host.hpp', 'dl_tns.h']]
    if not os.path.isfile(out) or any(os.path.getmtime(dep) > os.path.getmtime(out) for dep in deps):
        subprocess.check_call(['g++', '-std=c++17'] + flags + ['-o', out, src])
    return out


def load_emulation():
    """The shared object (no sanitizer), loaded by ctypes."""
    global _emu
    if _emu is None:
        lib = ctypes.CDLL(_build('libdl_emulate_phaseshift.so', ['-O2', '-fPIC', '-shared']))
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        lib.ps_config_new.restype = ctypes.c_void_p
        lib.ps_config_free.argtypes = [ctypes.c_void_p]
        lib.ps_config_set_f64.argtypes = [ctypes.c_void_p, ctypes.c_char_p, dp, ctypes.c_int64]
        lib.ps_config_set_i32.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ip, ctypes.c_int64]
        lib.ps_last_error.restype = ctypes.c_char_p
        lib.ps_n_in.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.ps_eval_theory.argtypes = [ctypes.c_void_p, dp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, dp]
        _emu = lib
    return _emu


def build_standalone():
    """The same source as a program of its own under the address / undefined-behaviour sanitizers (host code only; nothing of it is loaded into python)."""
    return _build('emulate_phaseshift_asan', ['-O1', '-DPS_STANDALONE'] + SANITIZE_FLAGS)


def _typed(cfg):
    for key, value in cfg.items():
        value = np.asarray(value)
        yield key, np.ascontiguousarray(value.ravel(), dtype='i4' if value.dtype.kind in 'iub' else 'f8')


def emulate_wiggle_power(cfg, theta, nthr):
    """Wiggle multipoles of every observable, concatenated [B, sum n_in], by the emulated phases with ``nthr`` threads per point."""
    lib = load_emulation()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    handle = lib.ps_config_new()
    try:
        for key, array in _typed(cfg):
            (lib.ps_config_set_i32 if array.dtype.kind == 'i' else lib.ps_config_set_f64)(handle, key.encode(), array.ctypes.data_as(ip if array.dtype.kind == 'i' else dp), array.size)
        theta = np.ascontiguousarray(theta, dtype='f8')
        out = []
        for iobs in range(int(cfg['n_obs'][0])):
            power = np.zeros((len(theta), lib.ps_n_in(handle, iobs)), dtype='f8')
            rc = lib.ps_eval_theory(handle, theta.ctypes.data_as(dp), len(theta), iobs, nthr, power.ctypes.data_as(dp))
            if rc: raise RuntimeError(lib.ps_last_error().decode())
            out.append(power)
    finally:
        lib.ps_config_free(handle)
    return np.hstack(out)


def write_flat_spec(fn, cfg, theta):
    """The flat file the stand-alone program reads (tests/csrc/emulate_phaseshift.cpp::main)."""
    theta = np.ascontiguousarray(theta, dtype='f8')
    with open(fn, 'wb') as file:
        for key, array in _typed(cfg):
            name = key.encode()
            file.write(struct.pack('<ii', 1 if array.dtype.kind == 'i' else 0, len(name)) + name + struct.pack('<q', array.size) + array.tobytes())
        file.write(struct.pack('<i', 2) + struct.pack('<qq', *theta.shape) + theta.tobytes())
