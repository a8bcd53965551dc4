"""CPU: the exact derivatives against a data batch (``dl_eval_fisher_analytic_data``, ``dl_eval_logposterior_grad_data``) -- the residual row of a (point, data vector)
pair as csrc/dl_data_batch.h states it, run by its stand-alone program (tests/csrc/emulate_data_resid.cpp) in a plain build and under the address / undefined-behaviour
sanitizers, and the Python-side checks that raise before any device call.  The device side: tests/test_gpu_data_batch_analytic.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import data_batch_utils as dbu
from data_batch_analytic_utils import build_program as build_resid_program


@pytest.mark.parametrize('sanitize', [False, True])
def test_residual_row_program(sanitize):
    """(n, slabs) in {1, 7, 8, 9, 120, 513} x {1, 2, 3, 9}: the live entries are the d_j of dl_db_step bit for bit, the tail [n, N_pad) is zero, a checked index of -1
    gives NaN and reads no table entry (the table is a heap block of exactly M N_pad doubles: the sanitizer build would report an overrun), and the kernel's
    distribution over threads gives the bits of the row function."""
    program = build_resid_program(sanitize=sanitize)
    result = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert result.returncode == 0, (result.stdout[-2000:], result.stderr[-2000:])
    assert 'Sanitizer' not in result.stderr and 'runtime error' not in result.stderr, result.stderr[-2000:]
    assert 'bit for bit' in result.stdout
    rows = {(int(m.group(1)), int(m.group(2))): (int(m.group(3)), m.group(4)) for m in
            re.finditer(r'n = +(\d+) +N_pad = +\d+ +slabs = (\d+) +entries off: (\d+) +thread distribution (same bits|DIFFERS)', result.stdout)}
    assert set(rows) == {(n, slabs) for n in [1, 7, 8, 9, 120, 513] for slabs in [1, 2, 3, 9]}
    for key, (off, same) in rows.items():
        assert off == 0 and same == 'same bits', (key, off, same)


def test_entries_declared_and_null_context():
    """The header declares the two entry points, the library exports them, a null context is an error and not a crash."""
    from desilike_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(dbu.HERE, '..', 'include', 'desilike_amd.h')).read()
    for name in ['dl_eval_fisher_analytic_data', 'dl_eval_logposterior_grad_data']:
        assert name in _lib.SYMBOLS and re.search(r'\b{}\('.format(name), header)
    assert lib.dl_eval_fisher_analytic_data(None, None, 1, None, None, None, None, None) == 1
    assert lib.dl_eval_logposterior_grad_data(None, None, 1, None, None, None, None, None) == 1
    assert b'null context' in lib.dl_last_error(None)


class _NoDevice(object):
    """Stands where a context would: any use of it is a device call."""

    def __getattr__(self, name):
        raise AssertionError('device call before the argument checks: {}'.format(name))


def _stub_batch(like, M=3, solve='constant'):
    from desilike_amd.likelihoods.base import DataBatch
    batch = DataBatch.__new__(DataBatch)
    batch.likelihood, batch.solve, batch.offset, batch.shift = like, solve, 0., 0.
    batch.flatdata = np.tile(like.flatdata, (M, 1))
    batch.context = _NoDevice()
    return batch


def test_logposterior_grad_argument_checks_raise_before_any_device_call():
    from bench_configs import make_cfg2
    g, like = make_cfg2()
    like.initialize()
    P = len(like.varied_params)
    values = np.tile([param.value for param in like.varied_params], (4, 1))
    batch = _stub_batch(like)
    index = np.arange(4) % 3
    with pytest.raises(ValueError, match='method'):
        batch.logposterior_grad(values, index, method='exact')
    for method in ['auto', 'analytic', 'finite']:
        with pytest.raises(ValueError, match='None'):
            batch.logposterior_grad(values, None, method=method)
        for bad in [index[:3], index.astype('f8'), np.full(4, 3), np.full(4, -1), index[None, :]]:
            with pytest.raises(ValueError, match='index'):
                batch.logposterior_grad(values, bad, method=method)
        with pytest.raises(ValueError, match='values'):
            batch.logposterior_grad(values[:, :P - 1], index, method=method)
        # solved parameters per point and per data vector: refused whatever the other arguments
        with pytest.raises(NotImplementedError, match="solve='point'"):
            _stub_batch(like, solve='point').logposterior_grad(values, index, method=method)
    assert not like._contexts      # nothing was compiled


def test_fisher_evaluate_data_index_checks_raise_before_any_device_call():
    from desilike_amd.fisher import Fisher
    from bench_configs import make_cfg2
    g, like = make_cfg2()
    like.initialize()
    centers = np.tile([param.value for param in like.varied_params], (4, 1))
    for method in ['analytic', 'finite', 'auto']:
        fisher = Fisher(like, method=method)
        with pytest.raises(ValueError, match='set_data_batch'):
            fisher.evaluate(centers, data_index=np.zeros(4, dtype='i4'))
        fisher._data_ctx = _NoDevice()
        for bad in [np.zeros(3, dtype='i4'), np.zeros(4), np.zeros((1, 4), dtype='i4')]:
            with pytest.raises(ValueError, match='integers'):
                fisher.evaluate(centers, data_index=bad)
        fisher._data_ctx = None
    assert not like._contexts
