"""Shared by tests/test_data_batch_marg.py (CPU) and tests/test_gpu_data_batch_marg.py (GPU): the build of the stand-alone CPU program of the per-pair arithmetic
(tests/csrc/emulate_data_batch_marg.cpp), the mocks of the cases of tests/marg_counts_cases.py and their extended-precision references.  Test infrastructure only."""
import functools
import os
import subprocess

import numpy as np

import marg_reference as mr
import marg_counts_cases as mc
from data_batch_utils import SANITIZE_FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
MMAX = 65
MOCK_SEED = 123

# the cases of the GPU test, with the numbers of data vectors they run
RESIDUAL_CASES = [(57, n_s) for n_s in (1, 4, 5, 8, 9, 13, 16)] + [(20, 3), (120, 12), (360, 8), (512, 16)]
GRAM_CASES = [('mlp', 'physical', 5), ('mlp', 'standard', 7), ('taylor', 'physical', 3)]
# the cases of the CPU program
PROGRAM_CASES = [(57, 5), (57, 16), (20, 3), (120, 12), (512, 16), ('mlp', 'physical', 5)]


def case_id(key):
    return 'n{:d}-ns{:d}'.format(*key) if len(key) == 2 else '{}-{}-ns{:d}'.format(*key)


def get_case(key):
    return mc.get_case(*key) if len(key) == 2 else mc.get_gram_case(*key)


def data_sizes(key):
    """Numbers of data vectors M of the GPU test for this case."""
    if len(key) == 3: return [1, 3, 33]
    return [3] if key[0] >= 360 else [1, 33, 65]


def reference_mocks(M):
    """Data vectors compared with the extended-precision reference in a batch of M."""
    return sorted({0, M // 2, M - 1})


def build_program(sanitize=False):
    """tests/csrc/emulate_data_batch_marg.cpp as a program of its own (host code only; nothing of it is loaded into python); ``sanitize``: under ASan + UBSan."""
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, 'emulate_data_batch_marg_asan' if sanitize else 'emulate_data_batch_marg')
    src = os.path.join(HERE, 'csrc', 'emulate_data_batch_marg.cpp')
    deps = [src] + [os.path.join(HERE, '..', 'desilike_amd', 'csrc', header) for header in ['dl_data_batch_marg.h', 'dl_data_batch.h', 'dl_fullshape.h']]
    if not os.path.isfile(out) or any(os.path.getmtime(dep) > os.path.getmtime(out) for dep in deps):
        subprocess.check_call(['g++', '-std=c++17'] + (['-O1'] + SANITIZE_FLAGS if sanitize else ['-O2']) + ['-o', out, src])
    return out


@functools.lru_cache(maxsize=None)
def mocks(key):
    """[MMAX, n]: ``case.flatdata + RandomState(123).multivariate_normal(0, case.covariance, size=MMAX)``, the recipe of the cases' own data, drawn ONCE: a batch of M
    data vectors is the first M rows (a draw of another size consumes the same deviates row after row but may round their product with the factor differently)."""
    case = get_case(key)
    out = case.flatdata + np.random.RandomState(MOCK_SEED).multivariate_normal(np.zeros(case.n), case.covariance, size=MMAX)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _precision_ints(key):
    return mr.exact_ints(get_case(key).precision)


@functools.lru_cache(maxsize=None)
def gram(key, row, m):
    """Exact Gram matrix of row ``row`` of the case against data vector m: delta_m = case.delta[row] + case.flatdata - mock_m."""
    case = get_case(key)
    return mr.marg_gram(case.delta[row] + case.flatdata - mocks(key)[m], case.T[row], _precision_ints(key))


def reference(key, row, m, mask):
    case = get_case(key)
    return mr.marg_from_gram(gram(key, row, m), case.x0, case.prior_loc, case.prior_scale, mask)


def gpu_patterns(n_s):
    """'.marg' masks of the GPU test: all, none, the seeded half of ``mask_patterns`` (duplicates at small n_s dropped there)."""
    return [(name, mask) for name, mask in mc.mask_patterns(n_s, seed=n_s) if name in ('all', 'none', 'half')]


def program_input(key, M):
    """The float64 file of the CPU program for the '.marg' mask filled in by the caller: whitened with the Cholesky factor of the precision, y = L^T (theory - own data + own data)
    of the size of a whitened theory vector and bias_m = -L^T mock_m its near opposite, as on the device."""
    case = get_case(key)
    L = np.linalg.cholesky(case.precision if np.ndim(case.precision) == 2 else np.diag(case.precision))
    prec = np.where(np.isinf(case.prior_scale), 0., 1. / case.prior_scale**2)
    bias = -mocks(key)[:M].dot(L)
    rows = [np.vstack([(case.delta[i] + case.flatdata).dot(L)[None, :], np.atleast_2d(case.T[i]).dot(L)]) for i in range(mc.NROWS)]
    return case, prec, bias, rows


def run_program(program, key, M, mask, path):
    case, prec, bias, rows = program_input(key, M)
    parts = [np.array([case.n, case.n_s, M, mc.NROWS], dtype='f8'), prec, case.x0, case.prior_loc, np.asarray(mask, dtype='f8'), bias.ravel()] + [r.ravel() for r in rows]
    np.concatenate([np.ravel(np.asarray(part, dtype='f8')) for part in parts]).tofile(path)
    out = subprocess.run([program, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    table = np.array([[float(v) for v in line.split()] for line in out.stdout.strip().splitlines()])
    assert table.shape == (mc.NROWS * M, 5 + case.n_s), table.shape
    return table.reshape(mc.NROWS, M, -1)
