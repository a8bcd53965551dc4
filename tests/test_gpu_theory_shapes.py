"""GPU (-m gpu): the TNS, BAO and PNG kernels (csrc/dl_tns.hip, csrc/dl_kernels.hip::dl_bao_kernel / dl_png_kernel) at the shapes of tests/theory_shapes_cases.py -- table
wavenumbers that do not fill a workgroup's waves, template knots that need padding (and fewer pairs than the loop kernel's floor), 2 to 48 projection cosines, n_kin on
both sides of the BAO kernel's workgroup sizes, batches with a remainder at every number of points per assembly workgroup -- against the NumPy oracle at 1e-10 (pinned on
the reference at the reference's shapes by tests/test_theory_shapes_cases.py), the same rows whatever batch they sit in, and NaN rows in a ragged tile."""
import numpy as np
import pytest

import theory_shapes_cases as tsc

pytestmark = pytest.mark.gpu
TOL = 1e-10


class State(object):
    """A case, its context, the batch of its size and the oracle on the compared rows: built once per module."""

    def __init__(self, name):
        self.name = name
        self.like, self.info = tsc.build(name)
        self.ctx = self.like._get_context()
        self.size = tsc.batch_size(name)
        self.theta = tsc.sample(self.like, self.size, seed=300 + tsc.names().index(name))
        self.rows = tsc.spread_rows(self.size)
        self._ref = self._out = None

    @property
    def ref(self):
        if self._ref is None: self._ref = tsc.oracle_rows(self.like, self.info, self.theta[self.rows])
        return self._ref

    @property
    def out(self):
        if self._out is None: self._out = self.ctx.eval_batch_host(self.theta, return_flattheory=True)
        return self._out


@pytest.fixture(scope='module')
def states():
    cache = {}

    def get(name):
        if name not in cache: cache[name] = State(name)
        return cache[name]

    yield get
    for state in cache.values(): state.ctx.close()


def relative(got, ref):
    return np.abs(got - ref) / np.maximum(1., np.abs(ref))


def of_largest(got, ref):
    """Largest error of every row of ``got`` in units of the row's largest reference magnitude."""
    got, ref = got.reshape(len(got), -1), ref.reshape(len(ref), -1)
    return np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)


@pytest.mark.parametrize('name', tsc.names())
def test_case_against_the_oracle(states, name):
    s = states(name)
    loglike, logprior, status, flat = s.out
    assert (status == 0).all(), (s.info, np.flatnonzero(status != 0)[:10], status[status != 0][:10])
    ref_ll, ref_flat, ref_tables = s.ref
    err_ll, err_flat = relative(loglike[s.rows], ref_ll), of_largest(flat[s.rows], ref_flat)
    print('{}: (n_kin, n11, knots, cosines) = {}, B = {:d}: log-likelihood {:.1e}, theory vector {:.1e} of its largest entry'.format(name, s.info['shape'], s.size, err_ll.max(), err_flat.max()))
    assert (err_ll <= TOL).all(), (s.info, s.rows, err_ll)
    assert (err_flat <= TOL).all(), (s.info, s.rows, err_flat)
    assert np.allclose(logprior, tsc.oracle_logprior(s.like, s.theta), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize('name', tsc.names())
def test_multipoles_and_tables_against_the_oracle(states, name):
    """``eval_theory_host`` (the multipoles in front of the window) on three of the compared rows, and for the one-loop theory ``eval_tns_tables``: each of the 29 tables to
    1e-10 of its largest entry, the bound of tests/test_gpu_tns.py."""
    s = states(name)
    three = s.rows[[0, len(s.rows) // 2, -1]] if len(s.rows) >= 3 else s.rows
    theta = s.theta[three]
    ref = tsc.oracle_power(s.like, s.info, theta)
    err = of_largest(s.ctx.eval_theory_host(theta, iobs=0), ref)
    worst = 0.
    if s.info['family'] == 'tns':
        n11 = s.info['shape'][1]
        ref_tables = s.ref[2][[list(s.rows).index(row) for row in three]]
        tables = s.ctx.eval_tns_tables(theta, n11).cpu().numpy()
        assert tables.shape == ref_tables.shape == (len(three), 29, n11)
        for i in range(len(three)):
            for r in range(29):
                scale = np.abs(ref_tables[i, r]).max()
                worst = max(worst, np.abs(tables[i, r] - ref_tables[i, r]).max() / scale)
                assert np.abs(tables[i, r] - ref_tables[i, r]).max() <= TOL * scale, (s.info, i, r, np.abs(tables[i, r] - ref_tables[i, r]).max() / scale)
    print('{}: multipoles {:.1e} of their largest entry{}'.format(name, err.max(), ', one-loop tables {:.1e}'.format(worst) if worst else ''))
    assert (err <= TOL).all(), (s.info, err)


def padded_size(name):
    if tsc.CASES[name]['family'] == 'bao': return 4100      # across both thresholds of the BAO kernel's workgroup size
    if name == 'tns_7_11_61_4': return 8193                 # a second pass of the one-loop kernels, with one point in it
    return 2100


@pytest.mark.parametrize('name', tsc.names())
def test_same_rows_in_a_padded_batch(states, name):
    """The compared rows twice in a larger batch -- in its first tile and spread to its very end, the last three at the end: bit-equal between their two places, and equal to
    the first batch to 1e-12 (the bound of tests/test_gpu_tns.py::test_large_batch_properties: other kernel variants add in another order, nothing else)."""
    s = states(name)
    size = padded_size(name)
    assert size > s.size
    theta = np.repeat(s.theta[:1], size, axis=0)
    first = np.arange(len(s.rows))
    second = tsc.spread_rows(size, count=len(s.rows))
    theta[first], theta[second] = s.theta[s.rows], s.theta[s.rows]
    loglike, logprior, status, flat = s.ctx.eval_batch_host(theta, return_flattheory=True)
    assert (status == 0).all()
    assert np.array_equal(loglike[first], loglike[second]) and np.array_equal(flat[first], flat[second]), (s.info, np.flatnonzero(loglike[first] != loglike[second]))
    filler = np.setdiff1d(np.arange(size), np.concatenate([first, second]))
    assert (loglike[filler] == loglike[filler[0]]).all() and (flat[filler] == flat[filler[0]]).all()
    err_ll, err_flat = relative(loglike[first], s.out[0][s.rows]), of_largest(flat[first], s.out[3][s.rows])
    print('{}: batch {:d} against batch {:d}: log-likelihood {:.1e}, theory vector {:.1e}'.format(name, size, s.size, err_ll.max(), err_flat.max()))
    assert (err_ll <= 1e-12).all() and (err_flat <= 1e-12).all(), (s.info, err_ll, err_flat)


@pytest.mark.parametrize('name', ['bao_258', 'bao_ps_258'])
def test_bao_batch_thresholds(states, name):
    """The same 64 rows inside batches of 2047, 2048, 4095 and 4096 points (256, 128 and 64 threads per point for the 258 wavenumbers): equal to 1e-12, and every eighth
    against the oracle."""
    s = states(name)
    rows = tsc.sample(s.like, 64, seed=77)
    ref = tsc.oracle_rows(s.like, s.info, rows[::8])
    results = {}
    for size in (2047, 2048, 4095, 4096):
        theta = np.repeat(rows[:1], size, axis=0)
        place = np.concatenate([np.arange(0, 32), np.arange(size - 32, size)])
        theta[place] = rows
        loglike, logprior, status, flat = s.ctx.eval_batch_host(theta, return_flattheory=True)
        assert (status == 0).all()
        results[size] = (loglike[place], flat[place])
        assert (relative(loglike[place][::8], ref[0]) <= TOL).all() and (of_largest(flat[place][::8], ref[1]) <= TOL).all(), (size, relative(loglike[place][::8], ref[0]))
    for size in (2048, 4095, 4096):
        err_ll, err_flat = relative(results[size][0], results[2047][0]), of_largest(results[size][1], results[2047][1])
        print('{}: batch {:d} against 2047: log-likelihood {:.1e}, theory vector {:.1e}'.format(name, size, err_ll.max(), err_flat.max()))
        assert (err_ll <= 1e-12).all() and (err_flat <= 1e-12).all(), (size, err_ll.max(), err_flat.max())


@pytest.mark.parametrize('name', ['tns_9_14_14_16', 'bao_64', 'png_26_48_130'])
def test_nan_row_in_the_ragged_tile(states, name):
    """273 points: the last tile of 32 holds 17.  A NaN parameter in row 270 gives that row status 3 and leaves every other row as it was, bit for bit."""
    s = states(name)
    assert s.size == 273
    theta = s.theta.copy()
    theta[270, 0] = np.nan
    loglike, logprior, status, flat = s.ctx.eval_batch_host(theta, return_flattheory=True)
    others = np.arange(s.size) != 270
    assert status[270] == 3 and (status[others] == 0).all()
    assert np.array_equal(loglike[others], s.out[0][others]) and np.array_equal(flat[others], s.out[3][others]) and np.array_equal(logprior[others], s.out[1][others])
