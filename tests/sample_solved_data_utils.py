"""Shared by tests/test_sample_solved_data.py (CPU) and tests/test_gpu_sample_solved_data.py (GPU): the build of the stand-alone CPU program of the per-pair draw of
dl_sample_solved_data (tests/csrc/emulate_sample_solved_data.cpp) and its runner on the cases of tests/marg_counts_cases.py with the data vectors of
tests/data_batch_marg_utils.py.  Test infrastructure only."""
import os
import subprocess

import numpy as np

import marg_counts_cases as mc
import data_batch_marg_utils as dbm
from data_batch_utils import SANITIZE_FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))


def build_program(sanitize=False):
    """tests/csrc/emulate_sample_solved_data.cpp as a program of its own (host code only; nothing of it is loaded into python); ``sanitize``: under ASan + UBSan."""
    build = os.path.join(HERE, 'csrc', '_build')
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, 'emulate_sample_solved_data_asan' if sanitize else 'emulate_sample_solved_data')
    src = os.path.join(HERE, 'csrc', 'emulate_sample_solved_data.cpp')
    headers = ['dl_sample_solved_data.h', 'dl_sample_solved.h', 'dl_philox.h', 'dl_data_batch_marg.h', 'dl_data_batch.h', 'dl_fullshape.h']
    deps = [src] + [os.path.join(HERE, '..', 'desilike_amd', 'csrc', header) for header in headers]
    if not os.path.isfile(out) or any(os.path.getmtime(dep) > os.path.getmtime(out) for dep in deps):
        subprocess.check_call(['g++', '-std=c++17'] + (['-O1'] + SANITIZE_FLAGS if sanitize else ['-O2']) + ['-o', out, src])
    return out


def run_program(program, key, M, mask, path, size=1, index0=0, seed=42, prec=None, m_range=None, lp=0., rows=None):
    """The program on case ``key`` against the first M data vectors of ``dbm.mocks(key)``.  ``prec``: prior precisions in the place of the case's own; ``m_range``:
    (m_lo, m_hi), the data indices every row is taken against (default: (0, M)); ``rows``: the rows of the case to run (default: all NROWS).
    Returns (pairs, draws): ``pairs [n_rows, n_m]`` dicts(status, ll, lps, hld, xhat [n_s], H [n_s, n_s]); ``draws`` dict(loglike [n_rows, n_m, size],
    logprior [n_rows, n_m, size], x [n_rows, n_m, size, n_s])."""
    case, case_prec, bias, case_rows = dbm.program_input(key, M)
    if prec is None: prec = case_prec
    if rows is None: rows = range(mc.NROWS)
    rows = [case_rows[i] for i in rows]
    m_lo, m_hi = (0, M) if m_range is None else m_range
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    head = np.array([case.n, case.n_s, M, len(rows), size, index0, seed & 0xFFFFFFFF, seed >> 32, m_lo, m_hi, lp], dtype='f8')
    parts = [head, prec, case.x0, case.prior_loc, np.asarray(mask, dtype='f8'), bias.ravel()] + [r.ravel() for r in rows]
    np.concatenate([np.ravel(np.asarray(part, dtype='f8')) for part in parts]).tofile(path)
    out = subprocess.run([program, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    assert 'Sanitizer' not in out.stderr and 'runtime error' not in out.stderr, out.stderr[-2000:]
    ns, nm = case.n_s, m_hi - m_lo
    pairs = [[None] * nm for _ in rows]
    draws = dict(loglike=np.empty((len(rows), nm, size)), logprior=np.empty((len(rows), nm, size)), x=np.empty((len(rows), nm, size, ns)))
    nlines = 0
    for line in out.stdout.splitlines():
        words = line.split()
        values = [float(v) for v in words[1:]]
        i, m = int(values[0]), int(values[1]) - m_lo
        if words[0] == 'P':
            assert len(values) == 6 + ns + ns * ns
            pairs[i][m] = dict(status=int(values[2]), ll=values[3], lps=values[4], hld=values[5], xhat=np.array(values[6:6 + ns]), H=np.array(values[6 + ns:]).reshape(ns, ns))
        else:
            d = int(values[2])
            draws['loglike'][i, m, d], draws['logprior'][i, m, d], draws['x'][i, m, d] = values[3], values[4], values[5:]
        nlines += 1
    assert nlines == len(rows) * nm * (1 + size), nlines
    return pairs, draws
