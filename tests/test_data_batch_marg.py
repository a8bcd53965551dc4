"""CPU: the data batch of likelihoods with analytically solved parameters (csrc/dl_data_batch_marg.h; ``data_batch(data, solve='point')``).

1. The per-pair arithmetic the device compiles -- direct difference, dot products in their fixed order, the two substitutions, the assembly of the value -- built with g++
   as a program of its own (tests/csrc/emulate_data_batch_marg.cpp), plain and under ASan + UBSan, on inputs dumped from tests/marg_counts_cases.py, against the
   extended-precision reference tests/marg_reference.py with delta_m = case.delta[i] + case.flatdata - mock_m: log-likelihood and solved log-prior to 1e-11 max(1, |.|) (the
   project's bound for the float64 oracle), solved values to rtol 1e-8, atol 1e-10.  The program itself checks that the cross kernel's staged order and the padded size give the
   bits of the plain statement.
2. The INPUT CONDITIONS of tests/test_marg_reference.py for every (case, data vector) this file or tests/test_gpu_data_batch_marg.py compares with that reference:
   (a) chi2(x0) <= 1e4, (b) float64 oracle against the reference <= 1e-11 max(1, |.|) on every quantity and '.marg' pattern.
3. What the Python layer refuses before any device call."""
import numpy as np
import pytest

from oracle import np_oracle as orc
import marg_counts_cases as mc
import data_batch_marg_utils as dbm
from test_marg_reference import worst

M_PROGRAM = 3


@pytest.mark.parametrize('key', dbm.PROGRAM_CASES, ids=[dbm.case_id(key) for key in dbm.PROGRAM_CASES])
def test_program_vs_reference(key, tmp_path):
    case = dbm.get_case(key)
    programs = [dbm.build_program(), dbm.build_program(sanitize=True)]
    errs = np.zeros(3)
    for name, mask in mc.mask_patterns(case.n_s, seed=case.n_s):
        tables = [dbm.run_program(program, key, M_PROGRAM, mask, str(tmp_path / 'input.f64')) for program in programs]
        assert np.array_equal(tables[0][..., :3], tables[1][..., :3])
        # (-O2 and -O1 builds: the shared functions leave nothing to contraction, the host factorisation is plain C++ and may differ in the last bits)
        assert np.allclose(tables[0], tables[1], rtol=1e-13, atol=1e-13)
        for table in tables:
            for i in range(mc.NROWS):
                for m in range(M_PROGRAM):
                    ref = dbm.reference(key, i, m, mask)
                    row, mm, ok, ll, lps = table[i, m, :5]
                    assert (row, mm, ok) == (i, m, 1)
                    e = [abs(ll - ref['loglikelihood']) / max(1., abs(ref['loglikelihood'])), abs(lps - ref['logprior_solved']) / max(1., abs(ref['logprior_solved']))]
                    errs = np.maximum(errs, e + [(np.abs(table[i, m, 5:] - ref['x']) / (1e-10 + 1e-8 * np.abs(ref['x']))).max()])
                    assert e[0] <= 1e-11, (key, name, i, m, 'loglikelihood', ll, ref['loglikelihood'], e[0])
                    assert e[1] <= 1e-11, (key, name, i, m, 'logprior', lps, ref['logprior_solved'], e[1])
                    assert np.allclose(table[i, m, 5:], ref['x'], rtol=1e-8, atol=1e-10), (key, name, i, m, table[i, m, 5:], ref['x'])
    print('\n{}: program vs reference, M = {:d}: loglike {:.1e} logprior {:.1e} solved {:.3f} tol'.format(dbm.case_id(key), M_PROGRAM, *errs))


ALL_CASES = sorted(set(dbm.RESIDUAL_CASES + dbm.GRAM_CASES + dbm.PROGRAM_CASES), key=str)


@pytest.mark.parametrize('key', ALL_CASES, ids=[dbm.case_id(key) for key in ALL_CASES])
def test_input_conditions(key):
    case = dbm.get_case(key)
    compared = set()
    if key in dbm.PROGRAM_CASES: compared |= set(range(M_PROGRAM))
    if key in dbm.RESIDUAL_CASES + dbm.GRAM_CASES:
        for M in dbm.data_sizes(key): compared |= set(dbm.reference_mocks(M))
    chi2_max, err_max = 0., 0.
    for m in sorted(compared):
        delta_shift = case.flatdata - dbm.mocks(key)[m]
        for i in range(mc.NROWS):
            for name, mask in mc.mask_patterns(case.n_s, seed=case.n_s):
                ref = dbm.reference(key, i, m, mask)
                sol = orc.solve_marginalized(case.delta[i] + delta_shift, case.T[i], case.precision, case.x0, case.prior_loc, case.prior_scale, mask)
                chi2_max, err_max = max(chi2_max, ref['chi2_x0']), max(err_max, worst(sol, ref))
    print('\n{}: data vectors {}: (a) max chi2(x0) = {:.1f} <= 1e4, (b) float64 oracle vs reference {:.1e} <= 1e-11'.format(dbm.case_id(key), sorted(compared), chi2_max, err_max))
    assert chi2_max <= 1e4, (key, chi2_max)
    assert err_max <= 1e-11, (key, err_max)


def test_mocks_do_not_depend_on_their_number():
    """Row m of the seeded draw comes from the same normal deviates whatever the number of rows drawn; the product with the factor of the covariance may round differently
    with the size, so the tests take a batch of M data vectors as the first M rows of ONE draw of MMAX (bit-equal rows across M)."""
    case = dbm.get_case((20, 3))
    for M in (1, 3, 33):
        draw = case.flatdata + np.random.RandomState(dbm.MOCK_SEED).multivariate_normal(np.zeros(case.n), case.covariance, size=M)
        assert np.allclose(draw, dbm.mocks((20, 3))[:M], rtol=1e-12, atol=1e-9)


def test_python_checks_before_any_device_call(monkeypatch):
    """``solve`` values, ``DataBatch.solved`` on a 'constant' batch, shape and dtype of ``index``: ValueError without touching the library."""
    from desilike_amd.likelihoods.base import DataBatch, ObservablesGaussianLikelihood, SumLikelihood
    import desilike_amd._lib as _lib

    def no_device(*args, **kwargs):
        raise AssertionError('device call')

    monkeypatch.setattr(_lib, 'load', no_device)
    monkeypatch.setattr(_lib.Context, '__init__', no_device)
    like = mc.build(20, 3)[0]
    for bad in ('marg', 'Point', None, True):
        with pytest.raises(ValueError, match='solve must be'):
            like.data_batch(np.zeros((2, 20)), solve=bad)
        with pytest.raises(ValueError, match='solve must be'):
            SumLikelihood(likelihoods=[like]).data_batch(np.zeros((2, 20)), solve=bad)
    assert ObservablesGaussianLikelihood.data_batch.__defaults__ == ('constant',) and SumLikelihood.data_batch.__defaults__ == ('constant',)

    class Stub(object):
        def eval_solved_data_host(self, *args): raise AssertionError('device call')
        eval_logposterior_data_host = eval_solved_data_host

    batch = DataBatch.__new__(DataBatch)
    batch.likelihood, batch.flatdata, batch.offset, batch.context = like, np.zeros((4, 20)), 0., Stub()
    like.initialize()
    values = np.zeros((3, len(like.varied_params)))
    batch.solve = 'constant'
    with pytest.raises(ValueError, match="solve='point'"):
        batch.solved(values, np.zeros(3, dtype='i4'))
    batch.solve = 'point'
    for index in (None, np.zeros(2, dtype='i4'), np.zeros((3, 1), dtype='i4'), np.zeros(3), np.array([0, 1, 4]), np.array([-1, 0, 0])):
        with pytest.raises(ValueError, match='index must'):
            batch.solved(values, index)
        if index is not None:
            with pytest.raises(ValueError, match='index must'):
                batch.logposterior(values, index)
    with pytest.raises(ValueError, match='values must have shape'):
        batch.solved(np.zeros((3, len(like.varied_params) + 1)), np.zeros(3, dtype='i4'))
