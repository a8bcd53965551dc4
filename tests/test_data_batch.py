"""CPU: the data batch (csrc/dl_data_batch.h) -- the per-pair reduction the kernels share, run by its stand-alone program (tests/csrc/emulate_data_batch.cpp) in a plain
build and under the address / undefined-behaviour sanitizers, and the Python-side checks that raise before any device call.  The device side: tests/test_gpu_data_batch.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import data_batch_utils as dbu


@pytest.mark.parametrize('sanitize', [False, True])
def test_reduction_program(sanitize):
    """dl_db_pair_chi2 against a long-double sum for n in {1, 63, 64, 65, 120, 257} (and two sizes beyond one staged chunk of the paired kernel), the slab sum for
    1 .. 19 slabs, and the cross / paired kernels' orders replayed on the CPU: the same bits.  The bounds are derived in the program's header."""
    program = dbu.build_program(sanitize=sanitize)
    result = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert result.returncode == 0, (result.stdout[-2000:], result.stderr[-2000:])
    assert 'Sanitizer' not in result.stderr and 'runtime error' not in result.stderr, result.stderr[-2000:]
    assert 'kernel orders give the same bits' in result.stdout
    rows = {int(m.group(1)): (float(m.group(2)), float(m.group(3)), m.group(4)) for m in
            re.finditer(r'n = +(\d+) .* error = (\S+) +bound = (\S+) +cross / paired orders (same bits|DIFFER)', result.stdout)}
    assert set(rows) >= {1, 63, 64, 65, 120, 257}
    for n, (error, bound, same) in rows.items():
        assert error <= bound and same == 'same bits', (n, error, bound, same)
        assert bound <= ((n + 7) // 8 + 8) * 2.**-52 * 2. * n      # (the residuals of the program are below sqrt(2) in size: chi2 <= 2 n; the bound is the documented one)


def test_entries_declared_and_null_context():
    """The header declares the three entry points, the library exports them, a null context is an error and not a crash."""
    from desilike_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(dbu.HERE, '..', 'include', 'desilike_amd.h')).read()
    for name in ['dl_data_set', 'dl_eval_logposterior_data', 'dl_eval_fisher_data']:
        assert name in _lib.SYMBOLS and re.search(r'\b{}\('.format(name), header)
    assert lib.dl_data_set(None, None, 0) == 1
    assert lib.dl_eval_logposterior_data(None, None, 1, None, None, None, None) == 1
    assert lib.dl_eval_fisher_data(None, None, None, 1, None, None, None, None, None) == 1
    assert 'n_data_batch' in header


def test_shape_and_finiteness_checks_raise_before_any_device_call():
    """``likelihood.data_batch`` / ``Fisher.set_data_batch`` / ``maximize_batch`` with a wrong shape, too many vectors or a NaN: ValueError, raised on a machine without a
    GPU as well -- no context has been created by then (creating one here is a LibraryError: no CPU fallback)."""
    import warnings
    from desilike_amd._lib import check_data_batch
    from desilike_amd.fisher import Fisher
    from desilike_amd.profilers import GaussNewtonProfiler
    from bench_configs import make_cfg2
    g, like = make_cfg2()
    like.initialize()
    n = like.flatdata.size
    good = np.tile(like.flatdata, (3, 1))
    assert check_data_batch(good, n).shape == (3, n) and check_data_batch(like.flatdata, n).shape == (1, n)
    nan, inf = good.copy(), good.copy()
    nan[1, 7], inf[2, 0] = np.nan, -np.inf
    bad = [good[:, :-1], good[None, ...], np.zeros((0, n + 1)), nan, inf, [good, good], 'data']
    for data in bad:
        with pytest.raises(ValueError):
            like.data_batch(data)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            with pytest.raises(ValueError):
                Fisher(like).set_data_batch(data)
            with pytest.raises(ValueError):
                GaussNewtonProfiler(like, seed=1).maximize_batch(data, start=np.zeros((1, len(like.varied_params))))
    with pytest.raises(ValueError, match='65536'):
        check_data_batch(np.zeros((65537, 2)), 2)
    with pytest.raises(ValueError, match='data vector 1 '):
        check_data_batch(nan, n)
    assert not like._contexts      # nothing was compiled


def test_list_of_observables_flattens_in_flatdata_order():
    """``data`` given observable by observable, in the order the constructor takes the observables: vector m of the batch is the concatenation of vector m of every
    observable -- the order of ``flatdata``."""
    from desilike_amd.likelihoods.base import flatten_data_batch
    from bench_configs import make_cfg5
    g, like = make_cfg5()
    like.initialize()
    fused = getattr(like, '_fused', like)
    sizes = [obs.wmatrix.size for obs in fused.observables]
    assert len(sizes) == 2 and sum(sizes) == like.flatdata.size
    rng = np.random.RandomState(0)
    M = 4
    blocks = [rng.standard_normal((M, size)) for size in sizes]
    flat = flatten_data_batch(blocks, sizes)
    assert flat.shape == (M, sum(sizes))
    for m in range(M):
        assert np.array_equal(flat[m], np.concatenate([block[m] for block in blocks]))
    assert np.array_equal(flatten_data_batch([block.tolist() for block in blocks], sizes), flat)      # plain lists
    assert np.array_equal(flatten_data_batch(flat, sizes), flat)                                      # the array form
    # the likelihood's own data, observable by observable, is its flatdata
    own = flatten_data_batch([obs.flatdata for obs in fused.observables], sizes)
    assert own.shape == (1, sum(sizes)) and np.array_equal(own[0], like.flatdata)
    for data in [blocks[::-1] if sizes[0] != sizes[1] else [blocks[0]], [blocks[0], blocks[1][:2]], [blocks[0]]]:
        with pytest.raises(ValueError):
            flatten_data_batch(data, sizes)
    # one observable: [array (M, n)] is the per-observable form, an (M, n) array or M rows the array form
    assert np.array_equal(flatten_data_batch([blocks[0]], sizes[:1]), blocks[0]) and np.array_equal(flatten_data_batch(list(blocks[0]), sizes[:1]), blocks[0])
