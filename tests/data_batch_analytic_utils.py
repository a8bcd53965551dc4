"""Shared by tests/test_data_batch_analytic.py and tests/test_gpu_data_batch_analytic.py: the build of the stand-alone CPU program of the residual row of a
(point, data vector) pair (tests/csrc/emulate_data_resid.cpp).  Test infrastructure only."""
import os
import subprocess

from data_batch_utils import HERE, SANITIZE_FLAGS


def build_program(sanitize=False):
    """tests/csrc/emulate_data_resid.cpp as a program of its own (host code only; nothing of it is loaded into python); ``sanitize``: under ASan + UBSan."""
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, 'emulate_data_resid_asan' if sanitize else 'emulate_data_resid')
    src = os.path.join(HERE, 'csrc', 'emulate_data_resid.cpp')
    deps = [src] + [os.path.join(HERE, '..', 'desilike_amd', 'csrc', header) for header in ['dl_data_batch.h', 'dl_fullshape.h']]
    if not os.path.isfile(out) or any(os.path.getmtime(dep) > os.path.getmtime(out) for dep in deps):
        subprocess.check_call(['g++', '-std=c++17'] + (['-O1'] + SANITIZE_FLAGS if sanitize else ['-O2']) + ['-o', out, src])
    return out
