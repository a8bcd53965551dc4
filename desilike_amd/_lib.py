"""ctypes binding of the C ABI declared in ``include/desilike_amd.h`` (thin: plain pointers and sizes).

The shared library holds the hand-written HIP kernels for gfx950.  There is NO CPU fallback:
if the library is missing, or no GPU is visible, evaluation raises.
"""
import ctypes
import os

import numpy as np

_LIB_PATH = os.environ.get('DL_LIB_PATH') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib', 'libdesilike_amd.so')   # DL_LIB_PATH: another build of the same library (A/B runs of a kernel change on one box)
_lib = None

_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_int32_p = ctypes.POINTER(ctypes.c_int32)

# every symbol include/desilike_amd.h declares: (restype, argtypes)
SYMBOLS = {
    'dl_config_new': (ctypes.c_void_p, []),
    'dl_config_set_f64': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, _c_double_p, ctypes.c_int64]),
    'dl_config_set_i32': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, _c_int32_p, ctypes.c_int64]),
    'dl_config_free': (None, [ctypes.c_void_p]),
    'dl_options_refresh': (None, []),
    'dl_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p]),
    'dl_destroy': (None, [ctypes.c_void_p]),
    'dl_last_error': (ctypes.c_char_p, [ctypes.c_void_p]),
    'dl_info': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p]),
    'dl_eval_batch': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_eval_batch_derived': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_sample_solved': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p]),
    'dl_eval_logposterior': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_eval_logposterior_grad': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_eval_fisher': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_data_set': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int32]),
    'dl_data_set_solved': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int32]),
    'dl_eval_solved_data': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_sample_solved_data': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_eval_logposterior_data': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_eval_fisher_data': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_eval_fisher_analytic': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_eval_fisher_analytic_data': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_eval_logposterior_grad_data': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_eval_theory': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_eval_batch_host': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64, _c_double_p, _c_double_p, _c_double_p, _c_int32_p, _c_double_p]),
    'dl_eval_tns_tables': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_eval_theory_host': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, _c_double_p]),
    'dl_eval_logposterior_host': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int64, _c_double_p, _c_int32_p]),
    'dl_profile_enable': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'dl_profile_read': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int32]),
    'dl_fftlog_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _c_double_p, _c_double_p, _c_double_p]),
    'dl_fftlog_apply': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_fftlog_destroy': (None, [ctypes.c_void_p]),
    'dl_comm_unique_id': (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p]),
    'dl_comm_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p]),
    'dl_comm_destroy': (None, [ctypes.c_void_p]),
    'dl_comm_info': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p]),
    'dl_comm_allgather_f64': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    'dl_comm_broadcast_f64': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    'dl_ensemble_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_uint64, ctypes.c_double, ctypes.c_void_p]),
    'dl_ensemble_destroy': (None, [ctypes.c_void_p]),
    'dl_ensemble_set_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.c_void_p]),
    'dl_ensemble_run': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_ensemble_get_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    'dl_ensemble_set_counter': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    'dl_ensemble_info': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p]),
    'dl_ensemble_data_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int32, _c_int32_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32, ctypes.c_double, ctypes.c_double]),
    'dl_ensemble_data_destroy': (None, [ctypes.c_void_p]),
    'dl_ensemble_data_set_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.c_void_p]),
    'dl_ensemble_data_run': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_ensemble_data_get_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    'dl_ensemble_data_set_counter': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    'dl_ensemble_data_info': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p]),
    'dl_mh_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                    ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_double, ctypes.c_uint64, ctypes.c_double, ctypes.c_int64]),
    'dl_mh_destroy': (None, [ctypes.c_void_p]),
    'dl_mh_set_covariance': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_void_p]),
    'dl_mh_set_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.c_void_p]),
    'dl_mh_run': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_mh_run_host': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p]),
    'dl_mh_get_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p]),
    'dl_mh_info': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p]),
    'dl_nuts_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_double,
                                      ctypes.c_uint64, ctypes.c_double, ctypes.c_int32, _c_double_p, _c_double_p]),
    'dl_nuts_destroy': (None, [ctypes.c_void_p]),
    'dl_nuts_set_mass': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p]),
    'dl_nuts_set_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    'dl_nuts_get_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int64), _c_double_p, ctypes.c_void_p]),
    'dl_nuts_set_adaptation': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]),
    'dl_nuts_run': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_nuts_info': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p]),
    'dl_mclmc_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_uint64,
                                       ctypes.c_double, ctypes.c_int32, _c_double_p, _c_double_p]),
    'dl_mclmc_destroy': (None, [ctypes.c_void_p]),
    'dl_mclmc_set_preconditioner': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_int32, ctypes.c_void_p]),
    'dl_mclmc_set_hyper': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]),
    'dl_mclmc_set_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    'dl_mclmc_get_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int64), _c_double_p, ctypes.c_void_p]),
    'dl_mclmc_set_adaptation': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]),
    'dl_mclmc_get_moments': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, _c_double_p, ctypes.c_void_p]),
    'dl_mclmc_run': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_mclmc_info': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p]),
    'dl_smc_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_uint64, ctypes.c_double,
                                     _c_double_p]),
    'dl_smc_destroy': (None, [ctypes.c_void_p]),
    'dl_smc_set_hyper': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]),
    'dl_smc_set_particles': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_void_p]),
    'dl_smc_set_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int64), _c_double_p, _c_double_p,
                                        ctypes.c_void_p]),
    'dl_smc_get_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int64), _c_double_p, _c_double_p,
                                        ctypes.c_void_p]),
    'dl_smc_get_decisions': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.c_void_p]),
    'dl_smc_run': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_smc_info': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p]),
    'dl_nested_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_uint64, ctypes.c_double,
                                        _c_double_p]),
    'dl_nested_destroy': (None, [ctypes.c_void_p]),
    'dl_nested_set_hyper': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]),
    'dl_nested_set_live': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_void_p]),
    'dl_nested_set_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int64), _c_double_p,
                                           ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p]),
    'dl_nested_get_state': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int64), _c_double_p,
                                           ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p]),
    'dl_nested_get_decisions': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _c_double_p, _c_double_p, ctypes.c_void_p]),
    'dl_nested_run': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_nested_info': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p]),
    'dl_mlp_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int32, _c_int32_p, ctypes.c_int32, _c_double_p]),
    'dl_mlp_destroy': (None, [ctypes.c_void_p]),
    'dl_mlp_info': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p]),
    'dl_mlp_train': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                    ctypes.c_double, _c_double_p, ctypes.c_void_p]),
    'dl_mlp_loss_and_grad': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _c_double_p, _c_double_p, ctypes.c_void_p]),
    'dl_mlp_forward': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_mlp_get_weights': (ctypes.c_int, [ctypes.c_void_p, _c_double_p, ctypes.c_void_p]),
    'dl_cov_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int32, ctypes.c_int32, _c_int32_p, _c_int32_p, _c_int32_p, _c_double_p, ctypes.c_int64, _c_int32_p,
                                     _c_double_p, ctypes.c_int64, _c_int32_p, _c_double_p, ctypes.c_int32, _c_double_p, ctypes.c_int64, _c_int32_p]),
    'dl_cov_apply': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    'dl_cov_destroy': (None, [ctypes.c_void_p]),
}


class LibraryError(RuntimeError):
    """Raised when the HIP library is missing or a C-ABI call fails."""


def lib_path():
    return _LIB_PATH


def load():
    """Load ``libdesilike_amd.so`` (built by ``__graft_entry__.build()`` / ``make -C desilike_amd/csrc``)."""
    global _lib
    if _lib is None:
        if not os.path.isfile(_LIB_PATH):
            raise LibraryError('HIP library {} not found: build it with `python -c "import __graft_entry__ as g; g.build()"`; there is no CPU fallback'.format(_LIB_PATH))
        # kernel arguments in device memory (latency-bound launches wait for them first; the runtime's default on ROCm 7, stated for older defaults; no effect once
        # HIP is initialised)
        os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
        try:
            # PyTorch-ROCm wheels bundle their own libamdhip64: load it FIRST so that this library binds to the same HIP runtime
            # (two HIP runtimes in one process do not see each other's devices: "No HIP GPUs are available")
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(_LIB_PATH)
        for name, (restype, argtypes) in SYMBOLS.items():
            func = getattr(lib, name)
            func.restype, func.argtypes = restype, argtypes
        _lib = lib
    return _lib


def refresh_options():
    """Re-read the library's diagnostic switches (environment variables ``DL_*``, include/desilike_amd.h) -- they are read once per process; the tests flip them in place."""
    load().dl_options_refresh()


def rccl_library_path():
    """RCCL to bind (``dl_comm_*`` load it with dlopen): ``DL_RCCL_PATH`` if set, else the copy PyTorch-ROCm bundles (the one already mapped into this process when
    torch is imported: one RCCL and one HIP runtime per process), else ``None`` (the library's own search: already-loaded copy, default path, /opt/rocm/lib)."""
    path = os.environ.get('DL_RCCL_PATH', None)
    if path:
        return path
    try:
        import torch
        path = os.path.join(os.path.dirname(os.path.abspath(torch.__file__)), 'lib', 'librccl.so')
        if os.path.isfile(path): return path
    except ImportError:
        pass
    return None


def _f64_ptr(array):
    return None if array is None else array.ctypes.data_as(_c_double_p)


def _i32_ptr(array):
    return None if array is None else array.ctypes.data_as(_c_int32_p)


_POINTERS = {'f8': _c_double_p, 'i8': ctypes.POINTER(ctypes.c_int64), 'i4': _c_int32_p}


def _ptr(array):
    """Pointer of the array's own type (float64 / int64 / int32; ``None`` stays ``None``): a state array travels with the dtype its table gives it."""
    return None if array is None else array.ctypes.data_as(_POINTERS[array.dtype.str[1:]])


def _seed(seed):
    return ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)


def _seeds(seeds):
    """64-bit keys as a contiguous uint64 array (through Python integers: NumPy makes float64 of a list that mixes keys below and above 2^63)."""
    return np.ascontiguousarray([int(seed) & 0xFFFFFFFFFFFFFFFF for seed in np.ravel(np.asarray(seeds, dtype=object))], dtype=np.uint64)


def _refuse_expand(ctx, does='sampler moves'):
    """The device-resident samplers work in the columns of the device context, which do not hold the parameters derived by an expression."""
    if ctx.expand is not None:
        raise NotImplementedError('the device-resident {} in the columns of the device context: parameters derived by an expression need the host-driven sampler'.format(does))


def _ids(ids, n, unit):
    """``<unit>_ids`` (default 0 .. n - 1) as contiguous int32 [n]."""
    ids = np.ascontiguousarray(np.arange(n) if ids is None else ids, dtype='i4')
    if len(ids) != n: raise ValueError('{0}_ids must have one entry per {0}'.format(unit))
    return ids


def _fd_table(table, n_params):
    """Steps or prior bounds [P, 2] of the central differences (``None``: the library's default)."""
    return None if table is None else np.ascontiguousarray(table, dtype='f8').reshape(n_params, 2)


def _state_in(values, table):
    """The arrays of a ``set_state`` in the dtypes and shapes of the owner's state ``table`` [(dtype, shape), ...]."""
    return [np.ascontiguousarray(value, dtype=dtype).reshape(shape) for value, (dtype, shape) in zip(values, table)]


def _state_out(table):
    return [np.empty(shape, dtype=dtype) for dtype, shape in table]


def _record_buffers(device, table):
    """One tensor on ``cuda:device`` per (dtype, shape, fill) of ``table``; fill ``None``: not initialised."""
    import torch
    device, dtypes = torch.device('cuda', device), {'f8': torch.float64, 'i8': torch.int64, 'i4': torch.int32}
    return tuple(torch.empty(shape, dtype=dtypes[dtype], device=device) if fill is None else torch.full(shape, fill, dtype=dtypes[dtype], device=device)
                 for dtype, shape, fill in table)


class _Handle(object):
    """Owner of one C handle of the family ``<_prefix>_*`` (include/desilike_amd.h): made by ``<_prefix>_create``, destroyed once by ``<_prefix>_destroy``.  ``device``
    (set by the subclass) is the GPU whose current stream is the default of every call."""
    _prefix = None

    def _create(self, *args):
        """``<_prefix>_create(&handle, *args)``; until it has succeeded there is no ``_handle``, and :meth:`close` / ``__del__`` of a half-built owner do nothing."""
        self._lib = load()
        handle = ctypes.c_void_p()
        if getattr(self._lib, self._prefix + '_create')(ctypes.byref(handle), *args) != 0:
            raise LibraryError(self._lib.dl_last_error(None).decode())
        self._handle = handle

    def _check(self, rc):
        if rc != 0:
            raise LibraryError(self._lib.dl_last_error(None).decode())

    def _stream(self, stream):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(torch.device('cuda', self.device)).cuda_stream if stream is None else stream)

    def info(self, key):
        """``<_prefix>_info`` (the families that export it)."""
        return int(getattr(self._lib, self._prefix + '_info')(self._handle, key.encode()))

    def close(self):
        if getattr(self, '_handle', None):
            getattr(self._lib, self._prefix + '_destroy')(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fill_config(spec, set_f64, set_i32):
    """Flatten a likelihood ``spec`` (nested dict, see ``desilike_amd.compile``) into config keys (include/desilike_amd.h).

    ``set_f64(key, float64 array)`` and ``set_i32(key, int32 array)`` receive contiguous 1-D arrays.
    """
    def put(key, value):
        value = np.asarray(value)
        if value.dtype.kind in 'iub':
            set_i32(key, np.ascontiguousarray(value.ravel(), dtype=np.int32))
        else:
            set_f64(key, np.ascontiguousarray(value.ravel(), dtype=np.float64))

    for key, value in spec.items():
        if key.startswith('_'):    # host-side entries (Context reads '_expand')
            continue
        if key == 'observables':
            for iobs, obs in enumerate(value):
                for okey, ovalue in obs.items():
                    if okey == 'inputs':
                        for name, (col, const) in ovalue.items():
                            if name in ('ct', 'sn', 'pass', 'x', 'vp', 'ml', 'band'):
                                put('obs{:d}.in.{}'.format(iobs, name), np.array([[c, v] for c, v in zip(np.ravel(col), np.ravel(const))], dtype='f8'))
                            else:
                                put('obs{:d}.in.{}'.format(iobs, name), np.array([col, const], dtype='f8'))
                    elif okey.startswith('emu') and isinstance(ovalue, dict):
                        for name, array in ovalue.items():
                            put('obs{:d}.{}.{}'.format(iobs, okey, name), array)
                    elif okey == 'marg':
                        for name, index in ovalue.items():
                            put('obs{:d}.marg.{}'.format(iobs, name), np.asarray(index, dtype='i4'))
                    elif ovalue is not None:
                        put('obs{:d}.{}'.format(iobs, okey), ovalue)
            put('n_obs', np.array([len(value)], dtype='i4'))
        elif key == 'marg':
            for name, array in value.items():
                put('marg.{}'.format(name), array)
        elif value is not None:
            put(key, value)


def check_data_batch(flatdata, n_data):
    """``flatdata`` as a contiguous float64 array ``[M, n_data]``; raises :class:`ValueError` for another shape, more than 65536 vectors or a NaN / infinite entry."""
    flatdata = np.asarray(flatdata, dtype='f8')
    if flatdata.ndim == 1 and flatdata.size == n_data: flatdata = flatdata[None, :]
    if flatdata.ndim != 2 or flatdata.shape[1] != n_data:
        raise ValueError('a data batch must have shape (M, {:d}), found {}'.format(n_data, flatdata.shape))
    if flatdata.shape[0] > 65536:
        raise ValueError('a data batch holds at most 65536 data vectors, found {:d}'.format(flatdata.shape[0]))
    bad = np.flatnonzero(~np.isfinite(flatdata).all(axis=1))
    if bad.size:
        raise ValueError('data vector {:d} of the batch has a NaN or infinite entry'.format(bad[0]))
    return np.ascontiguousarray(flatdata)


class Context(_Handle):
    """Owner of one ``dl_ctx`` (device constants + workspaces) on one GPU."""
    _prefix = 'dl'

    def __init__(self, spec, device=0):
        lib = load()
        cfg = lib.dl_config_new()
        keep = []

        def set_f64(key, array):
            keep.append(array)
            if lib.dl_config_set_f64(cfg, key.encode(), _f64_ptr(array), array.size): raise LibraryError(lib.dl_last_error(None).decode())

        def set_i32(key, array):
            keep.append(array)
            if lib.dl_config_set_i32(cfg, key.encode(), _i32_ptr(array), array.size): raise LibraryError(lib.dl_last_error(None).decode())

        try:
            fill_config(spec, set_f64, set_i32)
            self._create(int(device), cfg)
        finally:
            lib.dl_config_free(cfg)
        self.device = int(device)
        self.n_params, self.n_data, self.n_obs, self.n_solved = (self.info(name) for name in ['n_params', 'n_data', 'n_obs', 'n_solved'])
        # parameters derived from others by an expression (parameter.py:758-807) are extra theta columns of the device context, computed here from the caller's
        # columns: ``expand(theta [B, n_params]) -> [B, n_device_params]`` (numpy array or torch tensor, whatever it is given), set by the likelihood
        self.emulated = any('emu0' in obs for obs in spec.get('observables', []))   # an emulated theory (dl_emu_jac.h is its analytic Jacobian)
        self.n_device_params, self.expand = self.n_params, None
        if spec.get('_expand', None) is not None:
            self.set_expand(*spec['_expand'])

    def set_expand(self, expand, n_params):
        """Callers pass ``theta [B, n_params]``; the device context receives ``expand(theta) [B, n_device_params]``."""
        self.expand, self.n_params = expand, int(n_params)

    def _host_theta(self, theta):
        theta = np.ascontiguousarray(np.atleast_2d(theta), dtype='f8')
        if theta.shape[1] != self.n_params:
            raise ValueError('theta must have shape (B, {:d}), found {}'.format(self.n_params, theta.shape))
        if self.expand is not None:
            theta = np.ascontiguousarray(self.expand(theta), dtype='f8')
            assert theta.shape[1] == self.n_device_params
        return theta

    def _device_theta(self, theta, stream):
        import torch
        assert theta.is_contiguous() and theta.dtype == torch.float64 and theta.shape[1] == self.n_params
        if self.expand is not None:
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=theta.device)):   # the extra columns are computed on the stream the evaluation runs on
                theta = self.expand(theta).contiguous()
            assert theta.shape[1] == self.n_device_params
            self._expanded = theta    # alive until the next call on this context (calls on one context are serialised: include/desilike_amd.h)
        return theta

    def _check(self, rc):      # (a context keeps its own last message)
        if rc != 0:
            raise LibraryError(self._lib.dl_last_error(self._handle).decode())

    # ---- host-pointer entry points (numpy in / numpy out) ----
    def eval_batch_host(self, theta, return_flattheory=False, return_solved=False):
        """numpy in / numpy out: (loglike, logprior, status[, flattheory][, solved])."""
        theta = self._host_theta(theta)
        B = theta.shape[0]
        loglike, logprior, status = np.empty(B, dtype='f8'), np.empty(B, dtype='f8'), np.empty(B, dtype='i4')
        flat = np.empty((B, self.n_data), dtype='f8') if return_flattheory else None
        solved = np.empty((B, self.n_solved), dtype='f8') if return_solved else None
        self._check(self._lib.dl_eval_batch_host(self._handle, _f64_ptr(theta), B, _f64_ptr(loglike), _f64_ptr(logprior), _f64_ptr(flat), _i32_ptr(status),
                                                 _f64_ptr(solved) if self.n_solved else None))
        toret = (loglike, logprior, status)
        if return_flattheory: toret += (flat,)
        if return_solved: toret += (solved,)
        return toret

    def eval_logposterior_host(self, theta):
        """numpy in / numpy out: (logposterior [B], status [B]) with the samplers' -inf conventions applied on the device (samplers/base.py:144-200)."""
        theta = self._host_theta(theta)
        B = theta.shape[0]
        logposterior, status = np.empty(B, dtype='f8'), np.empty(B, dtype='i4')
        self._check(self._lib.dl_eval_logposterior_host(self._handle, _f64_ptr(theta), B, _f64_ptr(logposterior), _i32_ptr(status)))
        return logposterior, status

    def eval_batch_derived_host(self, theta):
        """numpy in / numpy out: (loglike, logprior, status, solved [B, n_solved], hessian [B, n_solved, n_solved]); stages through device tensors."""
        import torch
        theta = np.ascontiguousarray(np.atleast_2d(theta), dtype='f8')    # (columns of derived-by-expression parameters are added by eval_batch_derived)
        B, ns = theta.shape[0], self.n_solved
        device = torch.device('cuda', self.device)
        th = torch.as_tensor(theta, dtype=torch.float64, device=device).contiguous()
        loglike, logprior = torch.empty(B, dtype=torch.float64, device=device), torch.empty(B, dtype=torch.float64, device=device)
        status = torch.empty(B, dtype=torch.int32, device=device)
        solved, hessian = torch.empty((B, ns), dtype=torch.float64, device=device), torch.empty((B, ns, ns), dtype=torch.float64, device=device)
        if B:
            self.eval_batch_derived(th, loglike=loglike, logprior=logprior, status=status, solved=solved, hessian=hessian,
                                    stream=torch.cuda.current_stream(device).cuda_stream)
            torch.cuda.synchronize(device)
        return tuple(t.cpu().numpy() for t in (loglike, logprior, status, solved, hessian))

    def eval_theory_host(self, theta, iobs=0, return_tables=False):
        theta = self._host_theta(theta)
        B = theta.shape[0]
        n_ell, n_kin = self.info('n_ell_obs{:d}'.format(iobs)), self.info('n_kin_obs{:d}'.format(iobs))
        power = np.empty((B, n_ell, n_kin), dtype='f8')
        tables = np.empty((B, 3, n_ell, n_kin), dtype='f8') if return_tables else None
        self._check(self._lib.dl_eval_theory_host(self._handle, _f64_ptr(theta), B, int(iobs), _f64_ptr(power), _f64_ptr(tables)))
        return (power, tables) if return_tables else power

    # ---- device-pointer entry points (torch tensors as the array container) ----
    def eval_batch(self, theta, loglike=None, logprior=None, flattheory=None, status=None, solved=None, stream=None):
        """All arguments are CUDA(ROCm) torch tensors on this context's device; asynchronous on ``stream``."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(theta.device).cuda_stream
        B = theta.shape[0]
        theta = self._device_theta(theta, stream)

        def ptr(tensor, dtype, shape):
            if tensor is None: return None
            assert tensor.is_contiguous() and tensor.dtype == dtype and tuple(tensor.shape) == shape, (tensor.shape, shape)
            return ctypes.c_void_p(tensor.data_ptr())

        self._check(self._lib.dl_eval_batch(self._handle, ctypes.c_void_p(theta.data_ptr()), B, ptr(loglike, torch.float64, (B,)), ptr(logprior, torch.float64, (B,)),
                                            ptr(flattheory, torch.float64, (B, self.n_data)), ptr(status, torch.int32, (B,)),
                                            ptr(solved, torch.float64, (B, self.n_solved)), ctypes.c_void_p(stream)))

    def eval_batch_derived(self, theta, loglike=None, logprior=None, status=None, solved=None, hessian=None, stream=None):
        """``eval_batch`` plus ``hessian [B, n_solved, n_solved]``: likelihood Hessian w.r.t. the analytically solved parameters (torch tensors, asynchronous)."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(theta.device).cuda_stream
        B = theta.shape[0]
        theta = self._device_theta(theta, stream)

        def ptr(tensor, dtype, shape):
            if tensor is None: return None
            assert tensor.is_contiguous() and tensor.dtype == dtype and tuple(tensor.shape) == shape, (tensor.shape, shape)
            return ctypes.c_void_p(tensor.data_ptr())

        self._check(self._lib.dl_eval_batch_derived(self._handle, ctypes.c_void_p(theta.data_ptr()), B, ptr(loglike, torch.float64, (B,)), ptr(logprior, torch.float64, (B,)),
                                                    ptr(status, torch.int32, (B,)), ptr(solved, torch.float64, (B, self.n_solved)),
                                                    ptr(hessian, torch.float64, (B, self.n_solved, self.n_solved)), ctypes.c_void_p(stream)))

    def sample_solved(self, theta, index0=0, size=1, seed=42, stream=None):
        """Posterior draws of the analytically solved parameters at the points ``theta [B, n_params]`` (``dl_sample_solved``; samples/chain.py:229-263):
        ``(solved [B, size, n_solved], loglike [B, size], logprior [B, size], status [B])`` -- the draws and the log-likelihood / log-prior corrected so that their sum
        is the un-marginalised log-posterior at (theta, draw); NaN where ``status`` is not 0.  ``index0``: global index of the first point in its chain (a draw is a
        pure function of (seed, index0 + row, draw, component)).  ``theta``: a device tensor (device tensors are returned, asynchronous on ``stream``) or an array
        (arrays are returned).  Raises ``ValueError`` when the context has no analytically solved parameter, or for ``size < 1``."""
        import torch
        size, index0, seed = int(size), int(index0), int(seed) & 0xFFFFFFFFFFFFFFFF
        if size < 1:
            raise ValueError('sample_solved: size must be at least 1, found {:d}'.format(size))
        if index0 < 0:
            raise ValueError('sample_solved: index0 must not be negative')
        if self.n_solved == 0:
            raise ValueError('sample_solved: the context has no analytically solved parameter')
        host = not torch.is_tensor(theta)
        device = torch.device('cuda', self.device)
        if host:
            theta = torch.as_tensor(np.ascontiguousarray(np.atleast_2d(theta), dtype='f8'), device=device)
        if stream is None:
            stream = torch.cuda.current_stream(device).cuda_stream
        B, ns = theta.shape[0], self.n_solved
        theta = self._device_theta(theta, stream)
        solved = torch.empty((B, size, ns), dtype=torch.float64, device=device)
        loglike, logprior = torch.empty((B, size), dtype=torch.float64, device=device), torch.empty((B, size), dtype=torch.float64, device=device)
        status = torch.empty(B, dtype=torch.int32, device=device)
        if B:
            rc = self._lib.dl_sample_solved(self._handle, ctypes.c_void_p(theta.data_ptr()), B, index0, size, seed, ctypes.c_void_p(solved.data_ptr()),
                                            ctypes.c_void_p(loglike.data_ptr()), ctypes.c_void_p(logprior.data_ptr()), ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(stream))
            if rc == 2:
                raise ValueError('sample_solved: the context has no analytically solved parameter')
            self._check(rc)
        if host:
            torch.cuda.synchronize(device)
            return tuple(t.cpu().numpy() for t in (solved, loglike, logprior, status))
        return solved, loglike, logprior, status

    def eval_logposterior(self, theta, logposterior, status=None, stream=None):
        """``logposterior[B]`` = loglikelihood + logprior, -inf where the sampler would reject the point (samplers/base.py:185-191); torch tensors, asynchronous."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(theta.device).cuda_stream
        B = theta.shape[0]
        theta = self._device_theta(theta, stream)
        assert logposterior.is_contiguous() and logposterior.dtype == torch.float64 and tuple(logposterior.shape) == (B,)
        assert status is None or (status.is_contiguous() and status.dtype == torch.int32 and tuple(status.shape) == (B,))
        self._check(self._lib.dl_eval_logposterior(self._handle, ctypes.c_void_p(theta.data_ptr()), B, ctypes.c_void_p(logposterior.data_ptr()),
                                                   None if status is None else ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(stream)))

    def eval_theory(self, theta, power, iobs=0, tables=None, stream=None):
        """Theory multipoles of observable ``iobs`` into the device tensor ``power [B, n_ell, n_kin]`` (``dl_eval_theory``; torch tensors, asynchronous)."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(theta.device).cuda_stream
        B = theta.shape[0]
        n_ell, n_kin = self.info('n_ell_obs{:d}'.format(iobs)), self.info('n_kin_obs{:d}'.format(iobs))
        theta = self._device_theta(theta, stream)
        assert power.is_contiguous() and power.dtype == torch.float64 and tuple(power.shape) == (B, n_ell, n_kin)
        assert tables is None or (tables.is_contiguous() and tables.dtype == torch.float64 and tuple(tables.shape) == (B, 3, n_ell, n_kin))
        self._check(self._lib.dl_eval_theory(self._handle, ctypes.c_void_p(theta.data_ptr()), B, int(iobs), ctypes.c_void_p(power.data_ptr()),
                                             None if tables is None else ctypes.c_void_p(tables.data_ptr()), ctypes.c_void_p(stream)))
        return power

    def eval_tns_tables(self, theta, n_k11, iobs=0, stream=None):
        """The 29 one-loop tables ``[B, 29, n_k11]`` of a TNS observable before AP / damping / projection (``dl_eval_tns_tables``); ``theta``: array or device tensor."""
        import torch
        if not torch.is_tensor(theta):
            theta = torch.as_tensor(np.ascontiguousarray(theta, dtype='f8'), device='cuda:{:d}'.format(self.device))
        if stream is None:
            stream = torch.cuda.current_stream(theta.device).cuda_stream
        B = theta.shape[0]
        theta = self._device_theta(theta, stream)
        tables = torch.empty((B, 29, int(n_k11)), dtype=torch.float64, device=theta.device)
        self._check(self._lib.dl_eval_tns_tables(self._handle, ctypes.c_void_p(theta.data_ptr()), B, int(iobs), ctypes.c_void_p(tables.data_ptr()), ctypes.c_void_p(stream)))
        return tables

    def eval_logposterior_grad(self, theta, logposterior=None, grad=None, status=None, stream=None):
        """Log-posterior ``[B]`` and its analytic gradient ``[B, P]`` (``dl_eval_logposterior_grad``; float64 device tensors, allocated if ``None``; asynchronous).
        Returns ``(logposterior, grad)``, or ``None`` when the context is outside the analytic gradient's scope (the caller differentiates numerically)."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(theta.device).cuda_stream
        if self.expand is not None:
            return None      # parameters derived by an expression: chain rule through the expression is not implemented
        B = theta.shape[0]
        assert theta.is_contiguous() and theta.dtype == torch.float64 and theta.shape[1] == self.n_params
        if logposterior is None: logposterior = torch.empty(B, dtype=torch.float64, device=theta.device)
        if grad is None: grad = torch.empty((B, self.n_params), dtype=torch.float64, device=theta.device)
        rc = self._lib.dl_eval_logposterior_grad(self._handle, ctypes.c_void_p(theta.data_ptr()), B, ctypes.c_void_p(logposterior.data_ptr()), ctypes.c_void_p(grad.data_ptr()),
                                                 None if status is None else ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(stream))
        if rc == 2: return None
        self._check(rc)
        return logposterior, grad

    def eval_fisher(self, centers, steps, hessian=None, gradient=None, offset=None, stream=None):
        """Fisher algebra on the device (``dl_eval_fisher``): ``centers [B, P]``, ``steps [B, P, 2]`` (lower, upper) -> ``hessian [B, P, P]``, ``gradient [B, P]``,
        ``offset [B]`` (float64 device tensors, allocated if ``None``); asynchronous on ``stream``."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(centers.device).cuda_stream
        B, P = centers.shape
        if self.expand is not None:
            raise NotImplementedError('Fisher algebra with parameters derived by an expression: differentiate w.r.t. the device columns and apply the chain rule on the host')
        assert P == self.n_params and centers.is_contiguous() and centers.dtype == torch.float64
        assert steps.is_contiguous() and steps.dtype == torch.float64 and tuple(steps.shape) == (B, P, 2)
        if hessian is None: hessian = torch.empty((B, P, P), dtype=torch.float64, device=centers.device)
        if gradient is None: gradient = torch.empty((B, P), dtype=torch.float64, device=centers.device)
        if offset is None: offset = torch.empty(B, dtype=torch.float64, device=centers.device)
        for tensor, shape in [(hessian, (B, P, P)), (gradient, (B, P)), (offset, (B,))]:
            assert tensor.is_contiguous() and tensor.dtype == torch.float64 and tuple(tensor.shape) == shape
        self._check(self._lib.dl_eval_fisher(self._handle, ctypes.c_void_p(centers.data_ptr()), ctypes.c_void_p(steps.data_ptr()), B, ctypes.c_void_p(hessian.data_ptr()),
                                             ctypes.c_void_p(gradient.data_ptr()), ctypes.c_void_p(offset.data_ptr()), ctypes.c_void_p(stream)))
        return hessian, gradient, offset

    # ---- data batch (dl_data_set; csrc/dl_data_batch.h): many data vectors against one context ----
    def set_data_batch(self, flatdata, solved=False):
        """Give the context ``flatdata [M, n_data]`` (host array, rows in the order of the context's own data vector) as its data batch (``dl_data_set``); ``None`` or
        an empty array frees it.  Shape and finiteness are checked here, before any device call.  ``solved=True``: ``dl_data_set_solved``, which contexts with
        analytically solved parameters accept too -- their data-batch calls solve these parameters per point and per data vector (csrc/dl_data_batch_marg.h)."""
        if flatdata is None: flatdata = np.empty((0, self.n_data), dtype='f8')
        flatdata = check_data_batch(flatdata, self.n_data)
        setter = self._lib.dl_data_set_solved if solved else self._lib.dl_data_set
        self._check(setter(self._handle, _f64_ptr(flatdata), flatdata.shape[0]))
        return flatdata.shape[0]

    @property
    def n_data_batch(self):
        return self.info('n_data_batch')

    def eval_logposterior_data(self, theta, index=None, out=None, status=None, stream=None):
        """Log-posteriors against the data batch (``dl_eval_logposterior_data``): ``theta [B, P]`` float64 device tensor; ``index`` ``None`` -> ``out [B, M]`` (every
        point against every data vector), else an int32 device tensor ``[B]`` -> ``out [B]`` (point b against data vector ``index[b]``).  Asynchronous."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(theta.device).cuda_stream
        B = theta.shape[0]
        theta = self._device_theta(theta, stream)
        shape = (B, self.n_data_batch) if index is None else (B,)
        if index is not None: assert index.is_contiguous() and index.dtype == torch.int32 and tuple(index.shape) == (B,)
        if out is None: out = torch.empty(shape, dtype=torch.float64, device=theta.device)
        assert out.is_contiguous() and out.dtype == torch.float64 and tuple(out.shape) == shape
        assert status is None or (status.is_contiguous() and status.dtype == torch.int32 and tuple(status.shape) == (B,))
        self._check(self._lib.dl_eval_logposterior_data(self._handle, ctypes.c_void_p(theta.data_ptr()), B, None if index is None else ctypes.c_void_p(index.data_ptr()),
                                                        ctypes.c_void_p(out.data_ptr()), None if status is None else ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(stream)))
        return out

    def eval_logposterior_data_host(self, theta, index=None):
        """numpy in / numpy out: (logposterior [B, M] or [B], status [B]); stages through device tensors."""
        import torch
        theta = np.ascontiguousarray(np.atleast_2d(theta), dtype='f8')
        device = torch.device('cuda', self.device)
        th = torch.as_tensor(theta, dtype=torch.float64, device=device).contiguous()
        if index is not None:
            index = np.ascontiguousarray(index, dtype='i4')
            if index.shape != (theta.shape[0],): raise ValueError('index must have shape ({:d},), found {}'.format(theta.shape[0], index.shape))
            index = torch.as_tensor(index, device=device)
        status = torch.zeros(theta.shape[0], dtype=torch.int32, device=device)
        out = self.eval_logposterior_data(th, index=index, status=status)
        torch.cuda.synchronize(device)
        return out.cpu().numpy(), status.cpu().numpy()

    def eval_solved_data(self, theta, index, out=None, status=None, solved=None, stream=None):
        """The paired call of :meth:`eval_logposterior_data` on a context with solved parameters, plus their values (``dl_eval_solved_data``): ``theta [B, P]`` float64
        device tensor, ``index [B]`` int32 device tensor -> ``(out [B], solved [B, n_solved])``, point b given data vector ``index[b]``.  Asynchronous."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(theta.device).cuda_stream
        B = theta.shape[0]
        theta = self._device_theta(theta, stream)
        assert index.is_contiguous() and index.dtype == torch.int32 and tuple(index.shape) == (B,)
        if out is None: out = torch.empty((B,), dtype=torch.float64, device=theta.device)
        if solved is None: solved = torch.empty((B, self.n_solved), dtype=torch.float64, device=theta.device)
        assert out.is_contiguous() and out.dtype == torch.float64 and tuple(out.shape) == (B,)
        assert solved.is_contiguous() and solved.dtype == torch.float64 and tuple(solved.shape) == (B, self.n_solved)
        assert status is None or (status.is_contiguous() and status.dtype == torch.int32 and tuple(status.shape) == (B,))
        self._check(self._lib.dl_eval_solved_data(self._handle, ctypes.c_void_p(theta.data_ptr()), B, ctypes.c_void_p(index.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                                  None if status is None else ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(solved.data_ptr()), ctypes.c_void_p(stream)))
        return out, solved

    def eval_solved_data_host(self, theta, index):
        """numpy in / numpy out: (logposterior [B], status [B], solved [B, n_solved]); stages through device tensors."""
        import torch
        theta = np.ascontiguousarray(np.atleast_2d(theta), dtype='f8')
        index = np.ascontiguousarray(index, dtype='i4')
        if index.shape != (theta.shape[0],): raise ValueError('index must have shape ({:d},), found {}'.format(theta.shape[0], index.shape))
        device = torch.device('cuda', self.device)
        th = torch.as_tensor(theta, dtype=torch.float64, device=device).contiguous()
        status = torch.zeros(theta.shape[0], dtype=torch.int32, device=device)
        out, solved = self.eval_solved_data(th, torch.as_tensor(index, device=device), status=status)
        torch.cuda.synchronize(device)
        return out.cpu().numpy(), status.cpu().numpy(), solved.cpu().numpy()

    def sample_solved_data(self, theta, index, index0=0, size=1, seed=42, stream=None):
        """:meth:`sample_solved` against the data batch (``dl_sample_solved_data``): posterior draws of the analytically solved parameters of point b of
        ``theta [B, n_params]`` given data vector ``index[b]`` (``index [B]`` int32) -> ``(solved [B, size, n_solved], loglike [B, size], logprior [B, size],
        status [B])``; loglike + logprior is the un-marginalised log-posterior at (theta, draw) against that data vector; NaN where ``status`` is not 0.  A draw is a
        pure function of (seed, index0 + row, draw, component): not of ``index``.  ``theta`` and ``index``: device tensors (device tensors are returned, asynchronous
        on ``stream``) or arrays (arrays are returned).  ``ValueError``, before any device call: ``size < 1``, ``index0 < 0``, no analytically solved parameter,
        ``index`` not B 32-bit integers."""
        import torch
        size, index0, seed = int(size), int(index0), int(seed) & 0xFFFFFFFFFFFFFFFF
        if size < 1:
            raise ValueError('sample_solved_data: size must be at least 1, found {:d}'.format(size))
        if index0 < 0:
            raise ValueError('sample_solved_data: index0 must not be negative')
        if self.n_solved == 0:
            raise ValueError('sample_solved_data: the context has no analytically solved parameter')
        host = not torch.is_tensor(theta)
        if host:
            theta = np.ascontiguousarray(np.atleast_2d(theta), dtype='f8')
        B, ns = theta.shape[0], self.n_solved
        if torch.is_tensor(index):
            index_ok = index.dtype == torch.int32 and tuple(index.shape) == (B,) and index.is_contiguous()
        else:
            index = np.asarray(index)
            index_ok = index.dtype == np.int32 and index.shape == (B,)
        if not index_ok:
            raise ValueError('sample_solved_data: index must be {:d} contiguous 32-bit integers, found shape {} and type {}'.format(B, tuple(index.shape), index.dtype))
        device = torch.device('cuda', self.device)
        if host:
            theta = torch.as_tensor(theta, device=device)
        if not torch.is_tensor(index):
            index = torch.as_tensor(np.ascontiguousarray(index), device=device)
        if stream is None:
            stream = torch.cuda.current_stream(device).cuda_stream
        theta = self._device_theta(theta, stream)
        solved = torch.empty((B, size, ns), dtype=torch.float64, device=device)
        loglike, logprior = torch.empty((B, size), dtype=torch.float64, device=device), torch.empty((B, size), dtype=torch.float64, device=device)
        status = torch.empty(B, dtype=torch.int32, device=device)
        if B:
            self._check(self._lib.dl_sample_solved_data(self._handle, ctypes.c_void_p(theta.data_ptr()), B, ctypes.c_void_p(index.data_ptr()), index0, size, seed,
                                                        ctypes.c_void_p(solved.data_ptr()), ctypes.c_void_p(loglike.data_ptr()), ctypes.c_void_p(logprior.data_ptr()),
                                                        ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(stream)))
        if host:
            torch.cuda.synchronize(device)
            return tuple(t.cpu().numpy() for t in (solved, loglike, logprior, status))
        return solved, loglike, logprior, status

    def eval_fisher_data(self, centers, steps, index, hessian=None, gradient=None, offset=None, stream=None):
        """:meth:`eval_fisher` with the residual of centre b taken against data vector ``index[b]`` of the data batch (``dl_eval_fisher_data``; ``index`` int32 device
        tensor ``[B]``)."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(centers.device).cuda_stream
        B, P = centers.shape
        if self.expand is not None:
            raise NotImplementedError('Fisher algebra with parameters derived by an expression: differentiate w.r.t. the device columns and apply the chain rule on the host')
        assert P == self.n_params and centers.is_contiguous() and centers.dtype == torch.float64
        assert steps.is_contiguous() and steps.dtype == torch.float64 and tuple(steps.shape) == (B, P, 2)
        assert index.is_contiguous() and index.dtype == torch.int32 and tuple(index.shape) == (B,)
        if hessian is None: hessian = torch.empty((B, P, P), dtype=torch.float64, device=centers.device)
        if gradient is None: gradient = torch.empty((B, P), dtype=torch.float64, device=centers.device)
        if offset is None: offset = torch.empty(B, dtype=torch.float64, device=centers.device)
        for tensor, shape in [(hessian, (B, P, P)), (gradient, (B, P)), (offset, (B,))]:
            assert tensor.is_contiguous() and tensor.dtype == torch.float64 and tuple(tensor.shape) == shape
        self._check(self._lib.dl_eval_fisher_data(self._handle, ctypes.c_void_p(centers.data_ptr()), ctypes.c_void_p(steps.data_ptr()), B, ctypes.c_void_p(index.data_ptr()),
                                                  ctypes.c_void_p(hessian.data_ptr()), ctypes.c_void_p(gradient.data_ptr()), ctypes.c_void_p(offset.data_ptr()), ctypes.c_void_p(stream)))
        return hessian, gradient, offset

    def eval_fisher_analytic(self, centers, hessian=None, gradient=None, offset=None, stream=None):
        """The Fisher algebra from exact derivative rows (``dl_eval_fisher_analytic``; csrc/dl_fullshape_jac.h for Kaiser theories, csrc/dl_emu_jac.h for one
        velocileptors observable on an MLP- or Taylor-emulated PT node with every solved parameter varied): ``centers [B, P]`` -> ``(hessian [B, P, P],
        gradient [B, P], offset [B])`` (float64 device tensors, allocated if ``None``; ``False``: that output is not wanted -- a NULL pointer -- and comes back as
        ``None``); asynchronous on ``stream``.  Returns ``None`` when the context is outside the Jacobian kernels' scope (the caller uses :meth:`eval_fisher`)."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(centers.device).cuda_stream
        B, P = centers.shape
        if self.expand is not None:
            raise NotImplementedError('Fisher algebra with parameters derived by an expression: differentiate w.r.t. the device columns and apply the chain rule on the host')
        assert P == self.n_params and centers.is_contiguous() and centers.dtype == torch.float64
        outputs = []
        for tensor, shape in [(hessian, (B, P, P)), (gradient, (B, P)), (offset, (B,))]:
            if tensor is None: tensor = torch.empty(shape, dtype=torch.float64, device=centers.device)
            if tensor is False: tensor = None
            else: assert tensor.is_contiguous() and tensor.dtype == torch.float64 and tuple(tensor.shape) == shape
            outputs.append(tensor)
        rc = self._lib.dl_eval_fisher_analytic(self._handle, ctypes.c_void_p(centers.data_ptr()), B, *[None if tensor is None else ctypes.c_void_p(tensor.data_ptr()) for tensor in outputs],
                                               ctypes.c_void_p(stream))
        if rc == 2: return None
        self._check(rc)
        return tuple(outputs)

    def eval_fisher_analytic_data(self, centers, index, hessian=None, gradient=None, offset=None, stream=None):
        """:meth:`eval_fisher_analytic` with the residual of centre b taken against data vector ``index[b]`` of the data batch (``dl_eval_fisher_analytic_data``;
        ``index`` int32 device tensor ``[B]``): exact derivative rows, one theory row per centre; the Hessian does not depend on ``index``.  Returns ``None`` outside
        the scope of :meth:`eval_fisher_analytic` (the caller uses :meth:`eval_fisher_data`)."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(centers.device).cuda_stream
        B, P = centers.shape
        if self.expand is not None:
            raise NotImplementedError('Fisher algebra with parameters derived by an expression: differentiate w.r.t. the device columns and apply the chain rule on the host')
        assert P == self.n_params and centers.is_contiguous() and centers.dtype == torch.float64
        assert index.is_contiguous() and index.dtype == torch.int32 and tuple(index.shape) == (B,)
        outputs = []
        for tensor, shape in [(hessian, (B, P, P)), (gradient, (B, P)), (offset, (B,))]:
            if tensor is None: tensor = torch.empty(shape, dtype=torch.float64, device=centers.device)
            if tensor is False: tensor = None
            else: assert tensor.is_contiguous() and tensor.dtype == torch.float64 and tuple(tensor.shape) == shape
            outputs.append(tensor)
        rc = self._lib.dl_eval_fisher_analytic_data(self._handle, ctypes.c_void_p(centers.data_ptr()), B, ctypes.c_void_p(index.data_ptr()),
                                                    *[None if tensor is None else ctypes.c_void_p(tensor.data_ptr()) for tensor in outputs], ctypes.c_void_p(stream))
        if rc == 2: return None
        self._check(rc)
        return tuple(outputs)

    def eval_logposterior_grad_data(self, theta, index, logposterior=None, grad=None, status=None, stream=None):
        """:meth:`eval_logposterior_grad` of point b given data vector ``index[b]`` of the data batch (``dl_eval_logposterior_grad_data``; ``index`` int32 device
        tensor ``[B]``).  Returns ``(logposterior [B], grad [B, P])``, or ``None`` outside the scope (the Kaiser branch of :meth:`eval_logposterior_grad`: the caller
        differentiates :meth:`eval_logposterior_data` numerically)."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(theta.device).cuda_stream
        if self.expand is not None:
            return None      # parameters derived by an expression: chain rule through the expression is not implemented
        B = theta.shape[0]
        assert theta.is_contiguous() and theta.dtype == torch.float64 and theta.shape[1] == self.n_params
        assert index.is_contiguous() and index.dtype == torch.int32 and tuple(index.shape) == (B,)
        if logposterior is None: logposterior = torch.empty(B, dtype=torch.float64, device=theta.device)
        if grad is None: grad = torch.empty((B, self.n_params), dtype=torch.float64, device=theta.device)
        assert status is None or (status.is_contiguous() and status.dtype == torch.int32 and tuple(status.shape) == (B,))
        rc = self._lib.dl_eval_logposterior_grad_data(self._handle, ctypes.c_void_p(theta.data_ptr()), B, ctypes.c_void_p(index.data_ptr()),
                                                      ctypes.c_void_p(logposterior.data_ptr()), ctypes.c_void_p(grad.data_ptr()),
                                                      None if status is None else ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(stream))
        if rc == 2: return None
        self._check(rc)
        return logposterior, grad

    def profile_enable(self, every=1, only=None):
        """Attach HIP events to the kernels' dispatch packets on one ``eval_batch`` call out of ``every`` (0 / False: off); ``only``: 'theory' /
        'window_gemm' / 'finalize' -- a single kernel per sampled call (short runs: every kernel launched with events costs the step ~3 us)."""
        flags = 0
        if only is not None and every:
            flags = (1 << 16) | (['theory', 'window_gemm', 'finalize'].index(only) << 17)
        self._check(self._lib.dl_profile_enable(self._handle, int(every) | flags))

    def profile_read(self):
        ms = np.zeros(9, dtype='f8')
        self._check(self._lib.dl_profile_read(self._handle, _f64_ptr(ms), 9))
        return dict(theory=ms[0], window_gemm=ms[1], finalize=ms[2], total=ms[3], event_overhead=ms[4], samples=int(ms[5]),
                    samples_per_kernel=dict(theory=int(ms[6]), window_gemm=int(ms[7]), finalize=int(ms[8])))


class FFTLogPlan(_Handle):
    """Owner of one ``dl_fftlog`` plan (include/desilike_amd.h): batched FFTLog Hankel transform of ``fun [B, n_ell, n]`` on one GPU."""
    _prefix = 'dl_fftlog'

    def __init__(self, n, npad, pre, u, post, device=0):
        pre = np.ascontiguousarray(pre, dtype='f8')
        u = np.ascontiguousarray(u, dtype='f8')          # [n_ell, npad // 2 + 1, 2]
        post = np.ascontiguousarray(post, dtype='f8')    # [n_ell, n]
        self.n, self.npad, self.n_ell, self.device = int(n), int(npad), int(post.shape[0]), int(device)
        if pre.shape != (self.n,) or u.shape != (self.n_ell, self.npad // 2 + 1, 2) or post.shape != (self.n_ell, self.n):
            raise ValueError('inconsistent FFTLog plan arrays: pre {}, u {}, post {}'.format(pre.shape, u.shape, post.shape))
        self._create(self.device, self.n, self.npad, self.n_ell, _f64_ptr(pre), _f64_ptr(u), _f64_ptr(post))

    def apply(self, fun, out=None, stream=None):
        """``fun``: contiguous float64 CUDA(ROCm) tensor [B, n_ell, n] on this plan's device; returns ``out`` (allocated if None); asynchronous on ``stream``."""
        import torch
        assert fun.is_cuda and fun.is_contiguous() and fun.dtype == torch.float64 and tuple(fun.shape[1:]) == (self.n_ell, self.n), fun.shape
        if out is None: out = torch.empty_like(fun)
        assert out.is_contiguous() and out.dtype == torch.float64 and out.shape == fun.shape and out.device == fun.device
        if stream is None: stream = torch.cuda.current_stream(fun.device).cuda_stream
        self._check(self._lib.dl_fftlog_apply(self._handle, ctypes.c_void_p(fun.data_ptr()), fun.shape[0], ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream)))
        return out


class DeviceEnsemble(_Handle):
    """Owner of one ``dl_ensemble`` (include/desilike_amd.h): affine-invariant ensemble sampler resident on the GPU of ``ctx``; ``group``: an
    :class:`desilike_amd.parallel.RcclGroup` to shard every half-step's proposals over the ranks (or ``None``)."""
    _prefix = 'dl_ensemble'

    def __init__(self, ctx, nwalkers, a=2., seed=0, offset=0., group=None):
        _refuse_expand(ctx, 'ensemble proposes')
        self._create(ctx._handle, int(nwalkers), float(a), _seed(seed), float(offset), getattr(group, 'handle', None))
        self._ctx, self._group = ctx, group   # (the context and the group must outlive the ensemble)
        self.nwalkers, self.n_params, self.device = int(nwalkers), ctx.n_params, ctx.device

    def set_state(self, coords, logposterior=None, stream=None):
        coords = np.ascontiguousarray(coords, dtype='f8')
        if coords.shape != (self.nwalkers, self.n_params):
            raise ValueError('coords must have shape ({:d}, {:d}), found {}'.format(self.nwalkers, self.n_params, coords.shape))
        if logposterior is not None:
            logposterior = np.ascontiguousarray(logposterior, dtype='f8')
            if logposterior.shape != (self.nwalkers,): raise ValueError('logposterior must have shape ({:d},)'.format(self.nwalkers))
        self._check(self._lib.dl_ensemble_set_state(self._handle, _f64_ptr(coords), _f64_ptr(logposterior), self._stream(stream)))

    def set_counter(self, iteration, naccepted=None, stream=None):
        """Resume: iteration counter of the counter-based generator (and accepted counts per walker)."""
        if naccepted is not None:
            naccepted = np.ascontiguousarray(naccepted, dtype='i8')
            if naccepted.shape != (self.nwalkers,): raise ValueError('naccepted must have shape ({:d},)'.format(self.nwalkers))
        self._check(self._lib.dl_ensemble_set_counter(self._handle, int(iteration), _ptr(naccepted), self._stream(stream)))

    def run(self, niterations, thin_by=1, chain=None, chain_logp=None, stream=None):
        """Enqueue ``niterations`` ensemble updates (asynchronous); ``chain [niterations // thin_by, nwalkers, P]`` / ``chain_logp [niterations // thin_by, nwalkers]``:
        float64 device tensors receiving the ensemble after every ``thin_by``-th update (optional)."""
        import torch
        nrec = int(niterations) // int(thin_by)

        def ptr(tensor, shape):
            if tensor is None: return None
            assert tensor.is_cuda and tensor.is_contiguous() and tensor.dtype == torch.float64 and tuple(tensor.shape) == shape, (tensor.shape, shape)
            return ctypes.c_void_p(tensor.data_ptr())

        self._check(self._lib.dl_ensemble_run(self._handle, int(niterations), int(thin_by), ptr(chain, (nrec, self.nwalkers, self.n_params)),
                                              ptr(chain_logp, (nrec, self.nwalkers)), self._stream(stream)))

    def get_state(self, stream=None):
        """(coords [nwalkers, P], logposterior [nwalkers], naccepted [nwalkers]) as numpy arrays; synchronises the stream."""
        coords, logp = np.empty((self.nwalkers, self.n_params), dtype='f8'), np.empty(self.nwalkers, dtype='f8')
        nacc = np.empty(self.nwalkers, dtype='i8')
        self._check(self._lib.dl_ensemble_get_state(self._handle, _f64_ptr(coords), _f64_ptr(logp), _ptr(nacc), self._stream(stream)))
        return coords, logp, nacc


class DeviceEnsembleData(_Handle):
    """Owner of one ``dl_ensemble_data`` (include/desilike_amd.h): ``len(data_index)`` ensembles of ``nwalkers`` walkers resident on the GPU of ``ctx``, ensemble e sampling
    the posterior given data vector ``data_index[e]`` of the context's data batch with the draws of key ``seeds[e]``, all advancing in lockstep.  The arrays of
    :class:`DeviceEnsemble` with a leading ensemble axis."""
    _prefix = 'dl_ensemble_data'

    def __init__(self, ctx, data_index, seeds, nwalkers, a=2., offset=0.):
        _refuse_expand(ctx, 'ensembles propose')
        data_index = np.ascontiguousarray(data_index, dtype='i4').ravel()
        seeds = _seeds(seeds)
        if seeds.shape != data_index.shape: raise ValueError('provide one seed per ensemble')
        self._create(ctx._handle, int(data_index.size), _i32_ptr(data_index), seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), int(nwalkers), float(a), float(offset))
        self._ctx = ctx   # (the context must outlive the ensembles)
        self.n_ensembles, self.nwalkers, self.n_params, self.device = int(data_index.size), int(nwalkers), ctx.n_params, ctx.device
        self.data_index, self.seeds = data_index, seeds

    def set_state(self, coords, logposterior=None, stream=None):
        shape = (self.n_ensembles, self.nwalkers, self.n_params)
        coords = np.ascontiguousarray(coords, dtype='f8')
        if coords.shape != shape: raise ValueError('coords must have shape {}, found {}'.format(shape, coords.shape))
        if logposterior is not None:
            logposterior = np.ascontiguousarray(logposterior, dtype='f8')
            if logposterior.shape != shape[:2]: raise ValueError('logposterior must have shape {}'.format(shape[:2]))
        self._check(self._lib.dl_ensemble_data_set_state(self._handle, _f64_ptr(coords), _f64_ptr(logposterior), self._stream(stream)))

    def set_counter(self, iteration, naccepted=None, stream=None):
        """Resume: the shared iteration counter of the counter-based generators (and accepted counts per ensemble and walker)."""
        if naccepted is not None:
            naccepted = np.ascontiguousarray(naccepted, dtype='i8')
            if naccepted.shape != (self.n_ensembles, self.nwalkers): raise ValueError('naccepted must have shape {}'.format((self.n_ensembles, self.nwalkers)))
        self._check(self._lib.dl_ensemble_data_set_counter(self._handle, int(iteration), _ptr(naccepted), self._stream(stream)))

    def run(self, niterations, thin_by=1, chain=None, chain_logp=None, stream=None):
        """Enqueue ``niterations`` updates of every ensemble (asynchronous); ``chain [niterations // thin_by, E, nwalkers, P]`` / ``chain_logp [niterations // thin_by, E,
        nwalkers]``: float64 device tensors receiving the ensembles after every ``thin_by``-th update (optional)."""
        import torch
        nrec = int(niterations) // int(thin_by)

        def ptr(tensor, shape):
            if tensor is None: return None
            assert tensor.is_cuda and tensor.is_contiguous() and tensor.dtype == torch.float64 and tuple(tensor.shape) == shape, (tensor.shape, shape)
            return ctypes.c_void_p(tensor.data_ptr())

        self._check(self._lib.dl_ensemble_data_run(self._handle, int(niterations), int(thin_by), ptr(chain, (nrec, self.n_ensembles, self.nwalkers, self.n_params)),
                                                   ptr(chain_logp, (nrec, self.n_ensembles, self.nwalkers)), self._stream(stream)))

    def get_state(self, stream=None):
        """(coords [E, nwalkers, P], logposterior [E, nwalkers], naccepted [E, nwalkers]) as numpy arrays; synchronises the stream."""
        shape = (self.n_ensembles, self.nwalkers, self.n_params)
        coords, logp, nacc = np.empty(shape, dtype='f8'), np.empty(shape[:2], dtype='f8'), np.empty(shape[:2], dtype='i8')
        self._check(self._lib.dl_ensemble_data_get_state(self._handle, _f64_ptr(coords), _f64_ptr(logp), _ptr(nacc), self._stream(stream)))
        return coords, logp, nacc


class CovariancePlan(_Handle):
    """Owner of one ``dl_cov`` plan (include/desilike_amd.h): Gaussian covariance of multipole observables from theory spectra resident on the GPU.  ``arrays``: dict with the
    plan's host arrays (built by ``desilike_amd.observables.galaxy_clustering.covariance``)."""
    _prefix = 'dl_cov'

    def __init__(self, n, n_ell, n_k, ell0, shotnoise, cell_i, cell_d, pt_i, pt_d, gtab, sym, device=0):
        n_ell, n_k, ell0 = (np.ascontiguousarray(a, dtype=np.int32) for a in (n_ell, n_k, ell0))
        shotnoise = np.ascontiguousarray(shotnoise, dtype='f8')
        cell_i, pt_i, sym = (np.ascontiguousarray(a, dtype=np.int32) for a in (np.reshape(cell_i, (-1, 8)), np.reshape(pt_i, (-1, 2)), np.reshape(sym, (-1, 2))))
        cell_d, pt_d, gtab = (np.ascontiguousarray(a, dtype='f8') for a in (np.reshape(cell_d, (-1, 4)), np.reshape(pt_d, (-1, 6)), np.reshape(gtab, (-1, 5, 5))))
        self._create(int(device), int(n), len(n_ell), _i32_ptr(n_ell), _i32_ptr(n_k), _i32_ptr(ell0), _f64_ptr(shotnoise), len(cell_i), _i32_ptr(cell_i), _f64_ptr(cell_d), len(pt_i),
                     _i32_ptr(pt_i), _f64_ptr(pt_d), len(gtab), _f64_ptr(gtab), len(sym), _i32_ptr(sym))
        self.device, self.n, self.shapes = int(device), int(n), [(int(a), int(b)) for a, b in zip(n_ell, n_k)]

    def apply(self, powers, out=None, stream=None):
        """``powers``: one float64 device tensor ``[B, n_ell, n_k]`` per theory; returns the covariance matrices ``[B, n, n]`` (device tensor; asynchronous)."""
        import torch
        B = powers[0].shape[0]
        for power, shape in zip(powers, self.shapes):
            assert power.is_cuda and power.is_contiguous() and power.dtype == torch.float64 and tuple(power.shape) == (B,) + shape, (power.shape, shape)
        if out is None: out = torch.empty((B, self.n, self.n), dtype=torch.float64, device=powers[0].device)
        assert out.is_contiguous() and out.dtype == torch.float64 and tuple(out.shape) == (B, self.n, self.n)
        if stream is None: stream = torch.cuda.current_stream(powers[0].device).cuda_stream
        ptrs = (ctypes.c_void_p * len(powers))(*[power.data_ptr() for power in powers])
        self._check(self._lib.dl_cov_apply(self._handle, ptrs, B, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream)))
        return out


class MLPTrainer(_Handle):
    """Owner of one ``dl_mlp`` (include/desilike_amd.h): fp64 Adam training of a dense network on one GPU.  ``layers``: list of (kernel [n_in, n_out], bias [n_out])
    initial values; ``activation``: 'silu' / 'relu' / 'tanh'."""
    _prefix = 'dl_mlp'

    def __init__(self, layers, activation='silu', device=0):
        self.shapes = [(np.shape(kernel), np.shape(bias)) for kernel, bias in layers]
        widths = np.array([self.shapes[0][0][0]] + [shape[0][1] for shape in self.shapes], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.concatenate([np.ravel(kernel), np.ravel(bias)]) for kernel, bias in layers]), dtype='f8')
        self._create(int(device), len(layers), _i32_ptr(widths), {'silu': 0, 'relu': 1, 'tanh': 2}[activation], _f64_ptr(flat))
        self.device, self.n_weights = int(device), self.info('n_weights')

    def train(self, x, y, batch, nsteps, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, return_loss=True, stream=None):
        """``nsteps`` Adam steps on consecutive chunks of ``batch`` rows of the device tensors ``x [S, n_in]``, ``y [S, n_out]``; returns the batch losses [nsteps]."""
        import torch
        assert x.is_cuda and y.is_cuda and x.is_contiguous() and y.is_contiguous() and x.dtype == y.dtype == torch.float64 and x.shape[0] == y.shape[0]
        loss = np.empty(int(nsteps), dtype='f8') if return_loss else None
        self._check(self._lib.dl_mlp_train(self._handle, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), x.shape[0], int(batch), int(nsteps), float(lr), float(beta1),
                                           float(beta2), float(eps), _f64_ptr(loss), self._stream(stream)))
        return loss

    def loss_and_grad(self, x, y, stream=None):
        loss, grad = np.empty(1, dtype='f8'), np.empty(self.n_weights, dtype='f8')
        self._check(self._lib.dl_mlp_loss_and_grad(self._handle, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), x.shape[0], _f64_ptr(loss), _f64_ptr(grad), self._stream(stream)))
        return float(loss[0]), grad

    def forward(self, x, stream=None):
        import torch
        out = torch.empty((x.shape[0], self.info('n_out')), dtype=torch.float64, device=x.device)
        self._check(self._lib.dl_mlp_forward(self._handle, ctypes.c_void_p(x.data_ptr()), x.shape[0], ctypes.c_void_p(out.data_ptr()), self._stream(stream)))
        return out

    def layers(self, stream=None):
        """Current parameters as a list of (kernel [n_in, n_out], bias [n_out])."""
        flat = np.empty(self.n_weights, dtype='f8')
        self._check(self._lib.dl_mlp_get_weights(self._handle, _f64_ptr(flat), self._stream(stream)))
        out, off = [], 0
        for kshape, bshape in self.shapes:
            nk, nb = int(np.prod(kshape)), int(np.prod(bshape))
            out.append((flat[off:off + nk].reshape(kshape).copy(), flat[off + nk:off + nk + nb].copy()))
            off += nk + nb
        return out


class DeviceMH(_Handle):
    """Owner of one ``dl_mh`` (include/desilike_amd.h): ``nchains`` blocked Metropolis-Hastings chains x ``vectorize`` speculative proposals per try, resident on the
    GPU of ``ctx``.  ``order``: sorted (block) position -> column of the context; ``blocks`` / ``oversample``: block sizes (slowest first) and oversampling factors."""

    _prefix = 'dl_mh'

    def __init__(self, ctx, nchains, vectorize=1, blocks=None, oversample=None, order=None, chain_ids=None, proposal_scale=2.4, seed=0, offset=0., max_tries=1000):
        _refuse_expand(ctx, 'sampler proposes')
        P = ctx.n_params
        blocks = np.ascontiguousarray([P] if blocks is None else blocks, dtype='i4')
        oversample = np.ascontiguousarray(np.ones(len(blocks)) if oversample is None else oversample, dtype='i4')
        order = np.ascontiguousarray(np.arange(P) if order is None else order, dtype='i4')
        chain_ids = np.ascontiguousarray(np.arange(nchains) if chain_ids is None else chain_ids, dtype='i4')
        if len(oversample) != len(blocks) or len(order) != P or len(chain_ids) != nchains:
            raise ValueError('blocks / oversample / order / chain_ids have inconsistent sizes')
        self._create(ctx._handle, int(nchains), int(vectorize), _ptr(chain_ids), _ptr(order), _ptr(blocks), _ptr(oversample), len(blocks), float(proposal_scale), _seed(seed),
                     float(offset), int(max_tries))
        self._ctx = ctx     # (the context must outlive the sampler)
        self.nchains, self.vectorize, self.n_params, self.device = int(nchains), int(vectorize), P, ctx.device

    def set_covariance(self, cholesky, stream=None):
        """Lower-triangular Cholesky factor [P, P] of the proposal covariance, parameters in sorted (block) order."""
        cholesky = np.ascontiguousarray(cholesky, dtype='f8')
        if cholesky.shape != (self.n_params,) * 2: raise ValueError('cholesky must have shape ({0:d}, {0:d})'.format(self.n_params))
        self._check(self._lib.dl_mh_set_covariance(self._handle, _f64_ptr(cholesky), self._stream(stream)))

    def set_state(self, coords, logposterior=None, weight=None, naccepted=None, tries=0, stream=None):
        coords = np.ascontiguousarray(coords, dtype='f8')
        if coords.shape != (self.nchains, self.n_params):
            raise ValueError('coords must have shape ({:d}, {:d}), found {}'.format(self.nchains, self.n_params, coords.shape))

        def vector(values, dtype):
            if values is None: return None
            values = np.ascontiguousarray(values, dtype=dtype)
            if values.shape != (self.nchains,): raise ValueError('expected one value per chain')
            return values

        logposterior, weight, naccepted = vector(logposterior, 'f8'), vector(weight, 'i8'), vector(naccepted, 'i8')
        self._check(self._lib.dl_mh_set_state(self._handle, _f64_ptr(coords), _f64_ptr(logposterior), _ptr(weight), _ptr(naccepted), int(tries), self._stream(stream)))

    def run(self, ntries, thin_by=1, stream=None):
        """Enqueue ``ntries`` tries of every chain (asynchronous); returns the device tensors (coords [nchains, ntries, P], logposterior [nchains, ntries],
        weight [nchains, ntries], count [nchains]) that hold the ``count`` states recorded by this call once the stream has run."""
        ntries = int(ntries)
        C, n, P = self.nchains, max(ntries, 1), self.n_params
        coords, logp, weight, count = _record_buffers(self.device, [('f8', (C, n, P), None), ('f8', (C, n), None), ('i8', (C, n), None), ('i4', (C,), 0)])
        self._check(self._lib.dl_mh_run(self._handle, ntries, int(thin_by), ctypes.c_void_p(coords.data_ptr()), ctypes.c_void_p(logp.data_ptr()), ctypes.c_void_p(weight.data_ptr()),
                                        ctypes.c_void_p(count.data_ptr()), self._stream(stream)))
        return coords, logp, weight, count

    def get_state(self, stream=None):
        """(coords [nchains, P], logposterior, weight, naccepted, consecutive failed tries) as numpy arrays; synchronises the stream."""
        coords, logp = np.empty((self.nchains, self.n_params), dtype='f8'), np.empty(self.nchains, dtype='f8')
        weight, nacc, fails = np.empty(self.nchains, dtype='i8'), np.empty(self.nchains, dtype='i8'), np.empty(self.nchains, dtype='i4')
        self._check(self._lib.dl_mh_get_state(self._handle, _f64_ptr(coords), _f64_ptr(logp), _ptr(weight), _ptr(nacc), _ptr(fails), self._stream(stream)))
        return coords, logp, weight, nacc, fails


class DeviceNUTS(_Handle):
    """Owner of one ``dl_nuts`` (include/desilike_amd.h): ``nchains`` No-U-Turn chains resident on the GPU of ``ctx``, advanced one leapfrog step per call of the
    gradient.  ``gradient``: 'auto', 'analytic' or 'finite'; ``fd_delta`` / ``fd_limits`` [P, 2]: steps and prior bounds of the central differences."""
    _prefix = 'dl_nuts'
    MODES = {'auto': 0, 'analytic': 1, 'finite': 2}

    def __init__(self, ctx, nchains, chain_ids=None, max_num_doublings=10, divergence_threshold=1000., seed=0, offset=0., gradient='auto', fd_delta=None, fd_limits=None):
        _refuse_expand(ctx)
        P = ctx.n_params
        self._create(ctx._handle, int(nchains), _ptr(_ids(chain_ids, nchains, 'chain')), int(max_num_doublings), float(divergence_threshold), _seed(seed), float(offset),
                     self.MODES[gradient], _ptr(_fd_table(fd_delta, P)), _ptr(_fd_table(fd_limits, P)))
        self._ctx = ctx     # (the context must outlive the sampler)
        self.nchains, self.n_params, self.device = int(nchains), P, ctx.device

    def set_mass(self, inverse_mass, step_size, stream=None):
        """Inverse mass matrix: its diagonal [P] or the matrix [P, P]; the step size of every chain."""
        minv = np.ascontiguousarray(inverse_mass, dtype='f8')
        if minv.shape not in [(self.n_params,), (self.n_params,) * 2]: raise ValueError('inverse_mass must have shape ({0:d},) or ({0:d}, {0:d})'.format(self.n_params))
        self._check(self._lib.dl_nuts_set_mass(self._handle, _f64_ptr(minv), int(minv.ndim == 2), float(step_size), self._stream(stream)))

    def set_state(self, coords, logposterior=None, iterations=None, stream=None):
        coords = np.ascontiguousarray(coords, dtype='f8')
        if coords.shape != (self.nchains, self.n_params):
            raise ValueError('coords must have shape ({:d}, {:d}), found {}'.format(self.nchains, self.n_params, coords.shape))
        logposterior = None if logposterior is None else np.ascontiguousarray(logposterior, dtype='f8').reshape(self.nchains)
        iterations = None if iterations is None else np.ascontiguousarray(iterations, dtype='i8').reshape(self.nchains)
        self._check(self._lib.dl_nuts_set_state(self._handle, _f64_ptr(coords), _f64_ptr(logposterior), _ptr(iterations), self._stream(stream)))

    def get_state(self, stream=None):
        """(points [nchains, P], log-posteriors, iteration counters, log step sizes) as numpy arrays; synchronises."""
        coords, logp, logeps = np.empty((self.nchains, self.n_params)), np.empty(self.nchains), np.empty(self.nchains)
        iterations = np.empty(self.nchains, dtype='i8')
        self._check(self._lib.dl_nuts_get_state(self._handle, _f64_ptr(coords), _f64_ptr(logp), _ptr(iterations), _f64_ptr(logeps), self._stream(stream)))
        return coords, logp, iterations, logeps

    def set_adaptation(self, enabled, target_acceptance=0.8, initial_step_size=1., stream=None):
        self._check(self._lib.dl_nuts_set_adaptation(self._handle, int(bool(enabled)), float(target_acceptance), float(np.log(initial_step_size)), self._stream(stream)))

    def buffers(self, quota):
        """Record buffers of one batch: coords [nchains, quota, P], logposterior [nchains, quota], info [nchains, quota, 5], count [nchains] (zeroed)."""
        C, P = self.nchains, self.n_params
        return _record_buffers(self.device, [('f8', (C, quota, P), None), ('f8', (C, quota), None), ('f8', (C, quota, 5), None), ('i4', (C,), 0)])

    def run(self, nsteps, quota, buffers, thin_by=1, stream=None):
        """Enqueue ``nsteps`` leapfrog steps of every chain into the record ``buffers`` of a batch of ``quota`` records per chain (asynchronous)."""
        coords, logp, info, count = buffers
        self._check(self._lib.dl_nuts_run(self._handle, int(nsteps), int(quota), int(thin_by), ctypes.c_void_p(coords.data_ptr()), ctypes.c_void_p(logp.data_ptr()),
                                          ctypes.c_void_p(info.data_ptr()), ctypes.c_void_p(count.data_ptr()), self._stream(stream)))


class DeviceMCLMC(_Handle):
    """Owner of one ``dl_mclmc`` (include/desilike_amd.h): ``nchains`` microcanonical Langevin chains resident on the GPU of ``ctx``, one (isokinetic_leapfrog) or two
    (isokinetic_mclachlan) gradient batches per step.  ``gradient``, ``fd_delta``, ``fd_limits`` as :class:`DeviceNUTS`."""
    _prefix = 'dl_mclmc'
    MODES = DeviceNUTS.MODES
    INTEGRATORS = {'isokinetic_leapfrog': 0, 'isokinetic_mclachlan': 1}

    def __init__(self, ctx, nchains, chain_ids=None, integrator='isokinetic_mclachlan', seed=0, offset=0., gradient='auto', fd_delta=None, fd_limits=None):
        _refuse_expand(ctx)
        if isinstance(integrator, str):
            if integrator not in self.INTEGRATORS: raise ValueError('integrator must be one of {}, found {!r}'.format(sorted(self.INTEGRATORS), integrator))
            integrator = self.INTEGRATORS[integrator]
        P = ctx.n_params
        self._create(ctx._handle, int(nchains), _ptr(_ids(chain_ids, nchains, 'chain')), int(integrator), _seed(seed), float(offset), self.MODES[gradient],
                     _ptr(_fd_table(fd_delta, P)), _ptr(_fd_table(fd_limits, P)))
        self._ctx = ctx     # (the context must outlive the sampler)
        self.nchains, self.n_params, self.device = int(nchains), P, ctx.device

    def set_preconditioner(self, factor, stream=None):
        """A of x = x^ + A z: its diagonal [P] or a lower triangular factor [P, P]."""
        factor = np.ascontiguousarray(factor, dtype='f8')
        if factor.shape not in [(self.n_params,), (self.n_params,) * 2]: raise ValueError('factor must have shape ({0:d},) or ({0:d}, {0:d})'.format(self.n_params))
        self._check(self._lib.dl_mclmc_set_preconditioner(self._handle, _f64_ptr(factor), int(factor.ndim == 2), self._stream(stream)))

    def set_hyper(self, step_size, L, stream=None):
        self._check(self._lib.dl_mclmc_set_hyper(self._handle, float(step_size), float(L), self._stream(stream)))

    def set_state(self, coords, momenta=None, logposterior=None, counters=None, stream=None):
        coords = np.ascontiguousarray(coords, dtype='f8')
        if coords.shape != (self.nchains, self.n_params):
            raise ValueError('coords must have shape ({:d}, {:d}), found {}'.format(self.nchains, self.n_params, coords.shape))
        momenta = None if momenta is None else np.ascontiguousarray(momenta, dtype='f8').reshape(self.nchains, self.n_params)
        logposterior = None if logposterior is None else np.ascontiguousarray(logposterior, dtype='f8').reshape(self.nchains)
        counters = None if counters is None else np.ascontiguousarray(counters, dtype='i8').reshape(self.nchains)
        self._check(self._lib.dl_mclmc_set_state(self._handle, _f64_ptr(coords), _f64_ptr(momenta), _f64_ptr(logposterior), _ptr(counters), self._stream(stream)))

    def get_state(self, stream=None):
        """(points [nchains, P], momenta [nchains, P], log-posteriors, step counters, step sizes) as numpy arrays; synchronises."""
        coords, momenta = np.empty((self.nchains, self.n_params)), np.empty((self.nchains, self.n_params))
        logp, eps, counters = np.empty(self.nchains), np.empty(self.nchains), np.empty(self.nchains, dtype='i8')
        self._check(self._lib.dl_mclmc_get_state(self._handle, _f64_ptr(coords), _f64_ptr(momenta), _f64_ptr(logp), _ptr(counters), _f64_ptr(eps), self._stream(stream)))
        return coords, momenta, logp, counters, eps

    def set_adaptation(self, step_size_on, moments_on=False, desired_energy_var=5e-4, trust_in_estimate=1.5, num_effective_samples=150., stream=None):
        self._check(self._lib.dl_mclmc_set_adaptation(self._handle, int(bool(step_size_on)), int(bool(moments_on)), float(desired_energy_var), float(trust_in_estimate),
                                                      float(num_effective_samples), self._stream(stream)))

    def get_moments(self, stream=None):
        """Per chain (sum w [nchains], sum w x [nchains, P], sum w x^2 [nchains, P]); synchronises."""
        sw, sx, sxx = np.empty(self.nchains), np.empty((self.nchains, self.n_params)), np.empty((self.nchains, self.n_params))
        self._check(self._lib.dl_mclmc_get_moments(self._handle, _f64_ptr(sw), _f64_ptr(sx), _f64_ptr(sxx), self._stream(stream)))
        return sw, sx, sxx

    def buffers(self, quota):
        """Record buffers of one batch: coords [nchains, quota, P], logposterior [nchains, quota], info [nchains, quota, 3], count [nchains] (zeroed)."""
        C, P = self.nchains, self.n_params
        return _record_buffers(self.device, [('f8', (C, quota, P), None), ('f8', (C, quota), None), ('f8', (C, quota, 3), None), ('i4', (C,), 0)])

    def run(self, nsteps, quota, buffers, thin_by=1, stream=None):
        """Enqueue ``nsteps`` integrator steps of every chain into the record ``buffers`` of a batch of ``quota`` records per chain (asynchronous)."""
        coords, logp, info, count = buffers
        self._check(self._lib.dl_mclmc_run(self._handle, int(nsteps), int(quota), int(thin_by), ctypes.c_void_p(coords.data_ptr()), ctypes.c_void_p(logp.data_ptr()),
                                           ctypes.c_void_p(info.data_ptr()), ctypes.c_void_p(count.data_ptr()), self._stream(stream)))


class DeviceSMC(_Handle):
    """Owner of one ``dl_smc`` (include/desilike_amd.h): ``nsystems`` independent systems of ``nparticles`` particles of tempered sequential Monte Carlo resident on the
    GPU of ``ctx``; ``widths`` [P]: the width or scale of every parameter's prior."""
    _prefix = 'dl_smc'

    def __init__(self, ctx, nsystems, nparticles, widths, system_ids=None, seed=0, offset=0.):
        _refuse_expand(ctx)
        P = ctx.n_params
        self._create(ctx._handle, int(nsystems), int(nparticles), _ptr(_ids(system_ids, nsystems, 'system')), _seed(seed), float(offset),
                     _ptr(np.ascontiguousarray(widths, dtype='f8').reshape(P)))
        self._ctx = ctx     # (the context must outlive the sampler)
        self.nsystems, self.nparticles, self.n_params, self.device, self.n_steps = int(nsystems), int(nparticles), P, ctx.device, 0

    def set_hyper(self, ess_fraction, n_steps, target_acceptance, scale=1., stream=None):
        self._check(self._lib.dl_smc_set_hyper(self._handle, float(ess_fraction), int(n_steps), float(target_acceptance), float(scale), self._stream(stream)))
        self.n_steps = int(n_steps)

    def set_particles(self, coords, stream=None):
        coords = np.ascontiguousarray(coords, dtype='f8')
        if coords.shape != (self.nsystems, self.nparticles, self.n_params):
            raise ValueError('coords must have shape ({:d}, {:d}, {:d}), found {}'.format(self.nsystems, self.nparticles, self.n_params, coords.shape))
        self._check(self._lib.dl_smc_set_particles(self._handle, _f64_ptr(coords), self._stream(stream)))

    def _state_table(self):
        """(dtype, shape) of every array of the state, in the order of ``dl_smc_set_state`` / ``dl_smc_get_state``."""
        K, N, P = self.nsystems, self.nparticles, self.n_params
        return [('f8', (K, N, P)), ('f8', (K, N)), ('f8', (K, N)), ('f8', (K,)), ('f8', (K,)), ('i8', (K,)), ('f8', (K,)), ('f8', (K, P, P))]

    def set_state(self, coords, loglike, logprior, beta, logz, counters, scale, factor, stream=None):
        """What :meth:`get_state` returns."""
        arrays = _state_in([coords, loglike, logprior, beta, logz, counters, scale, factor], self._state_table())
        self._check(self._lib.dl_smc_set_state(self._handle, *[_ptr(a) for a in arrays], self._stream(stream)))

    def get_state(self, stream=None):
        """(coords [K, N, P], loglike [K, N], logprior [K, N], beta, logz (without the offset), counters, scale [K], factor [K, P, P]) as numpy arrays; synchronises."""
        arrays = _state_out(self._state_table())
        self._check(self._lib.dl_smc_get_state(self._handle, *[_ptr(a) for a in arrays], self._stream(stream)))
        return tuple(arrays)

    def get_decisions(self, stream=None):
        """Of the last iteration: (ancestors [K, N], accept flags [K, n_steps, N], mean [K, P], covariance [K, P, P] lower triangle); synchronises."""
        K, N, P = self.nsystems, self.nparticles, self.n_params
        anc, flags, mean, cov = np.empty((K, N), dtype='i4'), np.empty((K, self.n_steps, N), dtype='u1'), np.empty((K, P)), np.empty((K, P, P))
        self._check(self._lib.dl_smc_get_decisions(self._handle, anc.ctypes.data_as(ctypes.c_void_p), flags.ctypes.data_as(ctypes.c_void_p), _f64_ptr(mean), _f64_ptr(cov),
                                                   self._stream(stream)))
        return anc, flags.astype(bool), mean, np.tril(cov)

    def buffers(self, quota):
        """Record buffers of one batch: history [K, quota, 5], coords [K, quota, N, P], logposterior [K, quota, N], count [K, 2] (zeroed)."""
        K, N, P = self.nsystems, self.nparticles, self.n_params
        return _record_buffers(self.device, [('f8', (K, quota, 5), 0), ('f8', (K, quota, N, P), None), ('f8', (K, quota, N), None), ('i4', (K, 2), 0)])

    def run(self, niterations, quota, buffers, stream=None):
        """Enqueue ``niterations`` iterations of every system into the record ``buffers`` of a batch of ``quota`` records per system (asynchronous)."""
        history, coords, logp, count = buffers
        self._check(self._lib.dl_smc_run(self._handle, int(niterations), int(quota), ctypes.c_void_p(history.data_ptr()), ctypes.c_void_p(coords.data_ptr()),
                                         ctypes.c_void_p(logp.data_ptr()), ctypes.c_void_p(count.data_ptr()), self._stream(stream)))


class DeviceNested(_Handle):
    """Owner of one ``dl_nested`` (include/desilike_amd.h): ``nruns`` independent nested-sampling runs of ``nlive`` live points resident on the GPU of ``ctx``;
    ``widths`` [P]: the width or scale of every parameter's prior."""
    _prefix = 'dl_nested'

    def __init__(self, ctx, nruns, nlive, widths, run_ids=None, seed=0, offset=0.):
        _refuse_expand(ctx)
        P = ctx.n_params
        self._create(ctx._handle, int(nruns), int(nlive), _ptr(_ids(run_ids, nruns, 'run')), _seed(seed), float(offset), _ptr(np.ascontiguousarray(widths, dtype='f8').reshape(P)))
        self._ctx = ctx     # (the context must outlive the sampler)
        self.nruns, self.nlive, self.n_params, self.device, self.n_steps, self.ndelete = int(nruns), int(nlive), P, ctx.device, 0, 0

    def set_hyper(self, ndelete, n_steps, target_acceptance, dlogz, scale=1., stream=None):
        self._check(self._lib.dl_nested_set_hyper(self._handle, int(ndelete), int(n_steps), float(target_acceptance), float(dlogz), float(scale), self._stream(stream)))
        self.ndelete, self.n_steps = int(ndelete), int(n_steps)

    def set_live(self, coords, stream=None):
        coords = np.ascontiguousarray(coords, dtype='f8')
        if coords.shape != (self.nruns, self.nlive, self.n_params):
            raise ValueError('coords must have shape ({:d}, {:d}, {:d}), found {}'.format(self.nruns, self.nlive, self.n_params, coords.shape))
        self._check(self._lib.dl_nested_set_live(self._handle, _f64_ptr(coords), self._stream(stream)))

    def _state_table(self):
        """(dtype, shape) of every array of the state, in the order of ``dl_nested_set_state`` / ``dl_nested_get_state``."""
        K, N, P = self.nruns, self.nlive, self.n_params
        return [('f8', (K, N, P)), ('f8', (K, N)), ('f8', (K, N)), ('f8', (K,)), ('f8', (K,)), ('i8', (K,)), ('f8', (K,)), ('i4', (K,))]

    def set_state(self, coords, loglike, logprior, logx, logz, counters, scale, modes, stream=None):
        """What :meth:`get_state` returns."""
        arrays = _state_in([coords, loglike, logprior, logx, logz, counters, scale, modes], self._state_table())
        self._check(self._lib.dl_nested_set_state(self._handle, *[_ptr(a) for a in arrays], self._stream(stream)))

    def get_state(self, stream=None):
        """(coords [K, N, P], loglike [K, N], logprior [K, N], logx, logz (without the offset), counters, scale, modes [K]) as numpy arrays; synchronises."""
        arrays = _state_out(self._state_table())
        self._check(self._lib.dl_nested_get_state(self._handle, *[_ptr(a) for a in arrays], self._stream(stream)))
        return tuple(arrays)

    def get_decisions(self, stream=None):
        """Of the last iteration: (ranks [K, N], seeds [K, M], accept flags [K, n_steps, M], mean [K, P], covariance [K, P, P] lower triangle); synchronises."""
        K, N, P, M = self.nruns, self.nlive, self.n_params, self.ndelete
        ranks, seeds, flags = np.empty((K, N), dtype='i4'), np.empty((K, M), dtype='i4'), np.empty((K, self.n_steps, M), dtype='u1')
        mean, cov = np.empty((K, P)), np.empty((K, P, P))
        self._check(self._lib.dl_nested_get_decisions(self._handle, ranks.ctypes.data_as(ctypes.c_void_p), seeds.ctypes.data_as(ctypes.c_void_p), flags.ctypes.data_as(ctypes.c_void_p),
                                                      _f64_ptr(mean), _f64_ptr(cov), self._stream(stream)))
        return ranks, seeds, flags.astype(bool), mean, np.tril(cov)

    def buffers(self, quota):
        """Record buffers of one batch: history [K, quota, 6], dead coords [K, quota, M, P], dead loglike, logprior, logweight [K, quota, M], count [K] (zeroed), modes [K]."""
        K, M, P = self.nruns, self.ndelete, self.n_params
        return _record_buffers(self.device, [('f8', (K, quota, 6), 0), ('f8', (K, quota, M, P), None)] + [('f8', (K, quota, M), None)] * 3 + [('i4', (K,), 0), ('i4', (K,), 1)])

    def run(self, niterations, quota, buffers, stream=None):
        """Enqueue ``niterations`` iterations of every run into the record ``buffers`` of a batch of ``quota`` records per run (asynchronous)."""
        self._check(self._lib.dl_nested_run(self._handle, int(niterations), int(quota), *[ctypes.c_void_p(b.data_ptr()) for b in buffers], self._stream(stream)))
