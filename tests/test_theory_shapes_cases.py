"""CPU: the cases of tests/theory_shapes_cases.py (shapes of the TNS, BAO and PNG kernels beyond the reference's defaults) -- that every case builds without the device
library, that the oracle driver ``oracle_rows`` reproduces the REFERENCE at the reference's own shapes (tests/golden/boundary_<name>.npz and its prior-box companion), that
the table of cases reaches the ragged branches it is there for, that every row the GPU test draws lies inside the priors with a finite oracle value (so the GPU test can
demand status 0 on all of them), and that the compared numbers notice a dropped ragged tail."""
import os
import subprocess
import sys

import numpy as np
import pytest

import priorbox_utils as pbu
import theory_shapes_cases as tsc

HERE = os.path.dirname(os.path.abspath(__file__))
_built = {}


def built(name):
    if name not in _built: _built[name] = tsc.build(name)
    return _built[name]


def gpu_theta(name):
    """The batch tests/test_gpu_theory_shapes.py evaluates for the case and the rows it compares."""
    like, info = built(name)
    size = tsc.batch_size(name)
    return tsc.sample(like, size, seed=300 + tsc.names().index(name)), tsc.spread_rows(size)


@pytest.mark.parametrize('name', tsc.names())
def test_case_builds_without_the_device_library(name):
    like, info = built(name)
    case = tsc.CASES[name]
    n_kin, n11, knots, nmu = info['shape']
    assert knots == case['knots'] and nmu == case['mu']
    assert n_kin == (300 if 's' in case else case['kedges'][2] * case['resolution'])
    if case['family'] == 'tns': assert n11 == int(1.6 * n_kin + 0.5)
    assert like.flatdata.size == info['n'] and np.isfinite(like.flatdata).all() and np.isfinite(like.precision).all()
    # chi2 per point of O(1) at the parameters the data were generated at
    theta0 = np.array([[param.value for param in like.varied_params]])
    loglike = tsc.oracle_rows(like, info, theta0)[0][0]
    assert 0.05 < -2. * loglike / info['n'] < 20., loglike


def test_no_case_opens_the_device_library():
    """A fresh interpreter builds every case and evaluates the oracle on one: the device library is still closed and torch was never imported."""
    code = ('import sys; sys.path.insert(0, {!r}); sys.path.insert(0, {!r})\n'
            'import theory_shapes_cases as tsc\n'
            'for name in tsc.names(): like, info = tsc.build(name)\n'
            'tsc.oracle_rows(like, info, tsc.sample(like, 2, 0))\n'
            'lib = sys.modules.get("desilike_amd._lib")\n'
            'assert (lib is None or lib._lib is None) and "torch" not in sys.modules\n'
            'print("closed")\n').format(os.path.dirname(HERE), HERE)
    out = subprocess.run([sys.executable, '-W', 'ignore', '-c', code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0 and 'closed' in out.stdout.decode(), out.stderr.decode()[-1500:]


@pytest.mark.parametrize('name', [name for name in tsc.names() if 'pin' in tsc.CASES[name]])
def test_driver_reproduces_the_reference_at_its_own_shape(name):
    """``oracle_rows`` on the mirror of the reference's pipeline, with the fixture's data and precision, against the reference's own log-likelihoods (the rows of
    boundary_<pin>.npz) and theory vectors (the first rows of priorbox_<pin>.npz: centre and corners of the prior box) at 1e-10, relative above 1 (theory vectors: of the row's largest entry)."""
    pin = tsc.CASES[name]['pin']
    g, cfg = pbu.load_companion(pin)
    like, info = tsc.build(name, data=cfg['obs0.flatdata'], precision=cfg['precision'].reshape(cfg['obs0.flatdata'].size, -1))
    varied, rnames = like.varied_params.names(), [str(n) for n in g['names']]
    assert sorted(varied) == sorted(rnames)
    assert info['shape'][0] == len(cfg['obs0.kin']) and info['shape'][2] == len(cfg['obs0.k_t']) and info['shape'][3] == len(cfg['obs0.mu'])
    cols = [rnames.index(pname) for pname in varied]
    ok = np.isfinite(g['theta']).all(axis=1) & np.isfinite(g['loglikelihood'])
    loglike = tsc.oracle_rows(like, info, g['theta'][ok][:, cols])[0]
    ref = g['loglikelihood'][ok]
    assert ok.sum() >= 12 and (np.abs(loglike - ref) <= 1e-10 * np.maximum(1., np.abs(ref))).all(), (np.abs(loglike - ref) / np.maximum(1., np.abs(ref))).max()
    assert np.allclose(tsc.oracle_logprior(like, g['theta'][:, cols]), g['logprior'], rtol=1e-13, atol=1e-13)
    box = pbu.load_priorbox(pin)
    assert [str(n) for n in box['names']] == rnames
    rows = np.flatnonzero(~box['row_bad'])[:24]
    loglike, flat, _ = tsc.oracle_rows(like, info, box['theta'][rows][:, cols])
    ref, ref_flat = box['loglikelihood'][rows], box['flattheory'][rows]
    assert (np.abs(loglike - ref) <= 1e-10 * np.maximum(1., np.abs(ref))).all(), (np.abs(loglike - ref) / np.maximum(1., np.abs(ref))).max()
    scale = np.maximum(1., np.abs(ref_flat).max(axis=1))[:, None]      # (of the row's largest entry, as the GPU test compares theory vectors: entries that nearly cancel carry the rounding of the large ones)
    assert (np.abs(flat - ref_flat) <= 1e-10 * scale).all(), (np.abs(flat - ref_flat) / scale).max()


def test_cases_reach_the_ragged_branches():
    """Properties of ``CASES`` itself (the launchers' rules are not restated here)."""
    shapes = {name: built(name)[1]['shape'] for name in tsc.names()}
    tns = [shapes[name] for name in tsc.names('tns')]
    ragged = [n11 for _, n11, _, _ in tns if n11 % 8 != 0]
    assert len(ragged) >= 2 and any(n11 % 2 == 1 for n11 in ragged)
    assert {10, 11, 14, 35, 62} <= {n11 for _, n11, _, _ in tns}
    assert any(10 * knots < 128 for _, _, knots, _ in tns)
    assert sum(knots % 4 != 0 for _, _, knots, _ in tns) >= 2 and {12, 14, 37, 61, 130, 203} <= {knots for _, _, knots, _ in tns}
    assert {2, 3, 4, 5, 16} <= {nmu for _, _, _, nmu in tns}
    assert {(0,), (0, 2), (0, 2, 4)} <= {tuple(tsc.CASES[name]['ells']) for name in tsc.names('tns')}
    assert {'lorentzian', 'gaussian'} <= {tsc.CASES[name].get('options', {}).get('fog') for name in tsc.names('tns')}
    assert any('EFTLike' in tsc.CASES[name]['theory'] and tsc.batch_size(name) == 1537 for name in tsc.names('tns'))
    assert any('CorrelationFunction' in tsc.CASES[name]['theory'] and shapes[name][2] == 203 for name in tsc.names('tns'))
    assert any('kaiser' in tsc.CASES[name] for name in tsc.names('tns'))
    bao = [shapes[name][0] for name in tsc.names('bao')]
    assert min(bao) < 64 < max(bao) and 64 in bao and any(63 <= n < 64 for n in bao) and any(64 < n <= 65 for n in bao)
    assert any(n > 256 and n % 64 for n in bao) and any(n <= 256 for n in bao) and {9, 63, 64, 65, 192, 258} <= set(bao)
    assert {130, 257, 401} <= {shapes[name][2] for name in tsc.names('bao')} and {3, 7} <= {shapes[name][3] for name in tsc.names('bao')}
    assert {shapes[name][0] for name in tsc.names('bao') if tsc.CASES[name]['template'] == 'phaseshift'} == {9, 258}
    assert any('s' in tsc.CASES[name] and tsc.CASES[name]['s'][2] == 7 for name in tsc.names('bao'))
    assert {'Damped', 'Resummed', 'Flexible'} <= {tsc.CASES[name]['theory'][:-len('BAOWigglesTracerPowerSpectrumMultipoles')] for name in tsc.names('bao') if 's' not in tsc.CASES[name]}
    png = {shapes[name][0::2] + (shapes[name][3],) for name in tsc.names('png')}      # (n_kin, knots, cosines)
    assert {(7, 123, 5), (99, 301, 33), (26, 130, 48)} <= png and any(nmu == 48 for _, _, nmu in png)
    assert any('Velocity' in tsc.CASES[name]['theory'] for name in tsc.names('png'))
    # every batch size of the rotation is used, in every family that has enough cases
    assert set(tsc.BATCHES) <= {tsc.batch_size(name) for name in tsc.names('tns')} and set(tsc.BATCHES) <= {tsc.batch_size(name) for name in tsc.names('bao')}


def test_spread_rows_end_with_the_tail_of_the_batch():
    for size in tsc.BATCHES + [2, 3, 12, 13]:
        rows = tsc.spread_rows(size)
        assert len(rows) == min(12, size) == len(set(rows)) and rows.min() >= 0 and set(range(max(0, size - 3), size)) <= set(rows)


@pytest.mark.parametrize('name', tsc.names())
def test_every_row_of_the_gpu_batch_is_inside(name):
    """Finite oracle log-prior on EVERY row of the batch the GPU test evaluates, finite oracle log-likelihood on the rows it compares (and on the three NaN-test
    neighbours, which are among them)."""
    like, info = built(name)
    theta, rows = gpu_theta(name)
    assert np.isfinite(theta).all() and np.isfinite(tsc.oracle_logprior(like, theta)).all()
    loglike, flat, tables = tsc.oracle_rows(like, info, theta[rows])
    assert np.isfinite(loglike).all() and np.isfinite(flat).all() and (tables is None or np.isfinite(tables).all())


# one ragged case per family (two for the one-loop tables: n11 = 10 and the odd n11 = 11)
SENSITIVE = ['tns_6_10_12_3', 'tns_7_11_61_4', 'bao_9', 'bao_258', 'bao_ps_258', 'png_7_5_123', 'png_99_33_301']


@pytest.mark.parametrize('name', SENSITIVE)
def test_compared_numbers_notice_a_dropped_tail(name):
    """Without the last table wavenumber (TNS) or the last ``kin`` column (BAO, PNG) the oracle's log-likelihood moves by more than 1e-6 relative on every compared row, ten
    thousand times the bound of the GPU comparison: a kernel that drops or duplicates its ragged tail cannot pass."""
    like, info = built(name)
    theta, rows = gpu_theta(name)
    loglike, flat, _ = tsc.oracle_rows(like, info, theta[rows])
    dropped, dflat, _ = tsc.oracle_rows(like, info, theta[rows], drop_last=True)
    moved = np.abs(dropped - loglike) / np.maximum(1., np.abs(loglike))
    print('{}: log-likelihood moves by {:.1e} .. {:.1e} relative, theory vector by {:.1e} of its largest entry'.format(name, moved.min(), moved.max(), (np.abs(dflat - flat).max(axis=1) / np.abs(flat).max(axis=1)).min()))
    assert (moved > 1e-6).all(), moved
    assert (np.abs(dflat - flat).max(axis=1) > 1e-6 * np.abs(flat).max(axis=1)).all()
