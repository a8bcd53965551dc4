"""GPU (-m gpu): examples/fit_mocks.py runs; the best fits scatter around the truth as their errors say and each maximises the posterior of its own mock."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'examples'))


def test_fit_mocks():
    import fit_mocks
    out = fit_mocks.main(nmocks=6)
    truth = np.array([out['truth'][name] for name in out['names']])
    assert out['best'].shape == (6, len(truth)) and np.isfinite(out['best']).all()
    assert (np.abs(out['best'] - truth) <= 5. * out['error']).all(), np.abs((out['best'] - truth) / out['error']).max()      # (5 sigma: 30 draws)
    table = out['table']
    assert table.shape == (6, 6) and (np.diag(table)[None, :] >= table - 1e-6).all()
