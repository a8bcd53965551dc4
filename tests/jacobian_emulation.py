"""Build + ctypes-load the CPU emulation of the Jacobian workgroup (tests/csrc/emulate_jac.cpp: the phase functions of desilike_amd/csrc/dl_fullshape_jac.h): test
infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

from emulation import HERE, SANITIZE_FLAGS

_jac = None


def build_jacobian_emulation(sanitize=False):
    """Compile tests/csrc/emulate_jac.cpp (it includes emulate.cpp); ``sanitize``: the AddressSanitizer + UndefinedBehaviorSanitizer build, to be loaded in a process
    started with libasan preloaded (tests/test_jacobian.py::test_jacobian_under_sanitizers)."""
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, 'libdl_emulate_jac_asan.so' if sanitize else 'libdl_emulate_jac.so')
    src = os.path.join(HERE, 'csrc', 'emulate_jac.cpp')
    deps = [src, os.path.join(HERE, 'csrc', 'emulate.cpp')] + [os.path.join(HERE, '..', 'desilike_amd', 'csrc', name)
                                                              for name in ['dl_fullshape.h', 'dl_fullshape_grad.h', 'dl_fullshape_jac.h', 'dl_host.hpp', 'dl_tns.h']]
    if not os.path.isfile(so) or any(os.path.getmtime(dep) > os.path.getmtime(so) for dep in deps):
        subprocess.check_call(['g++', '-O1' if sanitize else '-O2', '-std=c++17', '-fPIC', '-shared'] + (SANITIZE_FLAGS if sanitize else []) + ['-o', so, src])
    return so


def load_jacobian_emulation():
    global _jac
    if _jac is None:
        lib = ctypes.CDLL(build_jacobian_emulation(sanitize=os.environ.get('DL_EMULATION_SANITIZE', '0') == '1'))
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        lib.emu_config_new.restype = ctypes.c_void_p
        lib.emu_config_free.argtypes = [ctypes.c_void_p]
        lib.emu_config_set_f64.argtypes = [ctypes.c_void_p, ctypes.c_char_p, dp, ctypes.c_int64]
        lib.emu_config_set_i32.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ip, ctypes.c_int64]
        lib.emu_last_error.restype = ctypes.c_char_p
        lib.emu_jac_ncols.restype = ctypes.c_int64
        lib.emu_jac_ncols.argtypes = [ctypes.c_void_p]
        lib.emu_eval_jac.argtypes = [ctypes.c_void_p, dp, ctypes.c_int64, ctypes.c_int64, dp]
        lib.emu_eval_grad_given_y.argtypes = [ctypes.c_void_p, dp, ctypes.c_int64, dp, dp]
        _jac = lib
    return _jac


class JacobianEmulation(object):
    """``spec``: the nested likelihood spec (``golden_utils.spec_from_golden``)."""

    def __init__(self, spec):
        from desilike_amd._lib import fill_config
        self.lib = load_jacobian_emulation()
        self.cfg = self.lib.emu_config_new()
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        fill_config(spec, lambda key, a: self.lib.emu_config_set_f64(self.cfg, key.encode(), a.ctypes.data_as(dp), a.size),
                    lambda key, a: self.lib.emu_config_set_i32(self.cfg, key.encode(), a.ctypes.data_as(ip), a.size))
        self.n_cols = int(self.lib.emu_jac_ncols(self.cfg))
        if self.n_cols < 0: raise RuntimeError(self.lib.emu_last_error().decode())

    def eval_jac(self, theta, k_pad=None):
        """d(theory vector) / d theta ``[B, P, k_pad]`` (``k_pad`` >= the number of columns; the buffer starts as NaN: every column must be written); None if the
        configuration is outside the scope."""
        theta = np.ascontiguousarray(theta, dtype='f8')
        k_pad = self.n_cols if k_pad is None else int(k_pad)
        jac = np.full(theta.shape + (k_pad,), np.nan)
        dp = ctypes.POINTER(ctypes.c_double)
        rc = self.lib.emu_eval_jac(self.cfg, theta.ctypes.data_as(dp), len(theta), k_pad, jac.ctypes.data_as(dp))
        if rc == 2: return None
        if rc: raise RuntimeError(self.lib.emu_last_error().decode())
        return jac

    def eval_grad_given_y(self, theta, Y):
        """The gradient phase's contraction of the same derivatives with ``Y [B, n_cols]``, chained to the theta columns: ``[B, P]``."""
        theta, Y = np.ascontiguousarray(theta, dtype='f8'), np.ascontiguousarray(Y, dtype='f8')
        assert Y.shape == (len(theta), self.n_cols)
        grad = np.empty(theta.shape)
        dp = ctypes.POINTER(ctypes.c_double)
        rc = self.lib.emu_eval_grad_given_y(self.cfg, theta.ctypes.data_as(dp), len(theta), Y.ctypes.data_as(dp), grad.ctypes.data_as(dp))
        if rc == 2: return None
        if rc: raise RuntimeError(self.lib.emu_last_error().decode())
        return grad

    def __del__(self):
        self.lib.emu_config_free(self.cfg)
