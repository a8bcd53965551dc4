"""CPU: the cases of tests/cov_cases.py for the covariance plan -- that the plan ``CovariancePlanBuilder`` lists, replayed by tests/cov_plan_numpy.py with the arithmetic
of ``dl_cov_kernel`` / ``dl_cov_sym_kernel``, is the oracle's matrix; that the table reaches the branches it names; that the comparison notices a lost integration point
and a misplaced shot noise.  No device library.

Symmetrisation: the blocks of one observable with itself are symmetric before ``(C + C^T) / 2`` up to the order of a few products (the Legendre integrals of
(la, lb, l1, l2) and (la, lb, l2, l1) are the same number, the theories on both sides are the same), so that no input the oracle can express lets a skipped
symmetrisation move an element by more than rounding: measured here at most 2e-3 of the tolerance.  What a skipped symmetrisation breaks is the exact symmetry of the
result, which tests/test_gpu_cov_shapes.py asserts bit for bit; here: the replay without it is not bit-symmetric in the cases listed, with it always."""
import numpy as np
import pytest

import cov_cases as cc
import cov_plan_numpy as cpn

_plans = {}


def plan(name):
    if name not in _plans: _plans[name] = cc.plan_arguments(name)
    return _plans[name]


def replay(name, ipoint, **kwargs):
    arrays, n_ell, n_k, ell0, shotnoise = plan(name)
    return cpn.apply_plan(arrays, ell0, shotnoise, [power[ipoint] for power in cc.spectra(name)], **kwargs)


@pytest.mark.parametrize('name', cc.names())
def test_case_is_well_formed(name):
    case = cc.CASES[name]
    arrays, n_ell, n_k, ell0, shotnoise = plan(name)
    assert 1 <= len(case['observables']) <= 8 and arrays['n'] <= 60 and max(n_k) <= 40 and max(n_ell) <= cpn.MAX_ELLS and case['resolution'] in (1, 2, 5)
    for obs, power in zip(case['observables'], cc.spectra(name)):
        assert power.shape == (cc.B, len(obs['theory_ells']), len(obs['theory_k'])) and (power > 0.).all() and set(obs['ells']) <= set(obs['theory_ells'])
        assert len(obs['edges']) == len(obs['ells']) and all(e.ndim == 2 and e.shape[1] == 2 and (e[:, 0] < e[:, 1]).all() for e in obs['edges'])
        assert np.all(np.diff(obs['theory_k']) > 0.)
    # what dl_cov_create validates: indices in range, intervals below n_k - 1
    cell_i, pt_i = arrays['cell_i'], arrays['pt_i']
    assert (cell_i[:, :2] >= 0).all() and (cell_i[:, :2] < arrays['n']).all() and (cell_i[:, 6] + cell_i[:, 7] <= len(pt_i)).all() and (cell_i[:, 7] > 0).all()
    assert len(set(map(tuple, cell_i[:, :2]))) == len(cell_i)          # every element is written by one cell
    for cell in cell_i:
        q = slice(cell[6], cell[6] + cell[7])
        assert (pt_i[q, 0] >= 0).all() and (pt_i[q, 0] <= n_k[cell[2]] - 2).all() and (pt_i[q, 1] >= 0).all() and (pt_i[q, 1] <= n_k[cell[3]] - 2).all()
    ref = cc.reference(name)
    assert ref.shape == (cc.B, arrays['n'], arrays['n']) and np.isfinite(ref).all() and np.array_equal(ref, np.swapaxes(ref, 1, 2))
    assert not np.allclose(ref[0], ref[1], rtol=1e-3, atol=0.)          # the draws differ


@pytest.mark.parametrize('name', cc.names())
def test_plan_replay_vs_oracle(name):
    """Builder + replay = oracle at the project's tolerance for this kernel, with the absolute part per block (``cov_cases.tolerance``)."""
    ref = cc.reference(name)
    for ipoint in range(cc.B):
        got = replay(name, ipoint)
        tol = cc.tolerance(name, ref[ipoint])
        assert (tol <= cc.RTOL * np.abs(ref[ipoint]) + cc.ATOL * np.abs(ref[ipoint]).max()).all()          # never wider than the whole-matrix bound
        assert (np.abs(got - ref[ipoint]) <= tol).all(), (np.abs(got - ref[ipoint]) / tol).max()
        assert np.array_equal(got, got.T)
        # the oracle lies well inside the rounding bound of the replay (the GPU test holds the kernel to that bound against the replay)
        arrays, n_ell, n_k, ell0, shotnoise = plan(name)
        bound = cpn.rounding_bound(arrays, ell0, shotnoise, [power[ipoint] for power in cc.spectra(name)])
        assert (bound >= 0.).all() and ((bound > 0.) == (got != 0.)).all()


def test_table_reaches_its_branches():
    seen = set()
    n_cells = {}
    for name, case in cc.CASES.items():
        arrays, n_ell, n_k, ell0, shotnoise = plan(name)
        cell_i, cell_d, pt_i, pt_d = arrays['cell_i'], arrays['cell_d'], arrays['pt_i'], arrays['pt_d']
        observables = case['observables']
        kinds = [obs['kind'] for obs in observables]
        have = set()
        if -1 in ell0: have.add('ell0_none')
        if 5 in n_ell: have.add('n_ell_5')
        if len(observables) == 8: have.add('eight_observables')
        if len(cell_i) < 256: have.add('under_256_cells')
        if any(a == 'xi' and 'pk' in kinds[i + 1:] for i, a in enumerate(kinds)): have.add('xi_before_pk')
        if any(a == 'pk' and 'xi' in kinds[i + 1:] for i, a in enumerate(kinds)): have.add('pk_before_xi')
        xis = [obs for obs in observables if obs['kind'] == 'xi']
        if len(xis) >= 2 and not np.array_equal(xis[0]['theory_k'], xis[1]['theory_k']) and (pt_i[:, 0] != pt_i[:, 1]).any(): have.add('xi_xi_two_grids')
        if (cell_d[:, 3] != 0.).any() and ((cell_i[:, 5] != 0) & (cell_d[:, 3] == 0.)).any(): have.add('const')          # overlapping and non-overlapping s-bins
        if any(len(set(len(e) for e in obs['edges'])) > 1 and min(len(e) for e in obs['edges']) == 1 for obs in observables): have.add('one_bin')
        # clipping: a P observable whose bins reach below and above its theory's k range, and points of P-type cells at a = 0 in the first / a = h in the last interval
        pks = [(io, obs) for io, obs in enumerate(observables) if obs['kind'] == 'pk']
        outside = [io for io, obs in pks if min(e.min() for e in obs['edges']) < obs['theory_k'][0] and max(e.max() for e in obs['edges']) > obs['theory_k'][-1]]
        if outside:
            below = above = False
            for cell in cell_i[(cell_i[:, 5] == 0) & np.isin(cell_i[:, 2], outside)]:
                q = slice(cell[6], cell[6] + cell[7])
                below |= bool(((pt_i[q, 0] == 0) & (pt_d[q, 0] == 0.)).any())
                above |= bool(((pt_i[q, 0] == n_k[cell[2]] - 2) & (pt_d[q, 0] == pt_d[q, 1])).any())
            if below and above: have.add('clipping')
        # two P observables: empty, partial and full (one bin inside the other) intersections
        if len(pks) >= 2:
            kinds_of_overlap = set()
            for b1 in np.concatenate(pks[0][1]['edges']):
                for b2 in np.concatenate(pks[1][1]['edges']):
                    lo, hi = max(b1[0], b2[0]), min(b1[1], b2[1])
                    kinds_of_overlap.add('empty' if lo >= hi else 'inside' if (lo, hi) in ((b1[0], b1[1]), (b2[0], b2[1])) else 'partial')
            if kinds_of_overlap == {'empty', 'inside', 'partial'}: have.add('partial_intersections')
        assert set(case['reaches']) <= have, (name, set(case['reaches']) - have)
        seen |= set(case['reaches'])
        n_cells[name] = len(cell_i)
    assert seen == {'ell0_none', 'n_ell_5', 'eight_observables', 'under_256_cells', 'xi_before_pk', 'pk_before_xi', 'xi_xi_two_grids', 'const', 'one_bin', 'clipping',
                    'partial_intersections'}
    assert {case['resolution'] for case in cc.CASES.values()} == {1, 2, 5}
    assert any(n > 256 and n % 256 != 0 for n in n_cells.values()), n_cells          # more than one workgroup, the last one not full
    assert any((plan(name)[0]['cell_i'][:, 5] != 0).any() for name in cc.names())                                               # the zero-lag flag


@pytest.mark.parametrize('name', cc.names())
def test_comparison_notices_a_lost_integration_point(name):
    ref = cc.reference(name)[0]
    moved = np.abs(replay(name, 0, drop_last_point=True) - ref)
    assert (moved >= 1e3 * cc.tolerance(name, ref)).any()
    # and in every block that has cells, not just in the largest
    for rows in cc.block_slices(name):
        for cols in cc.block_slices(name):
            if np.abs(ref[rows, cols]).max() > 0.: assert (moved[rows, cols] >= 1e3 * cc.tolerance(name, ref)[rows, cols]).any(), (name, rows, cols)


@pytest.mark.parametrize('name', [name for name in cc.names() if 'ell0_none' in cc.CASES[name]['reaches']])
def test_comparison_notices_shot_noise_on_the_wrong_multipole(name):
    """``ell0`` ignored (the first multipole taken for the monopole): in the blocks of the theories without monopole the shot noise lands on the quadrupole."""
    ref = cc.reference(name)[0]
    arrays, n_ell, n_k, ell0, shotnoise = plan(name)
    moved = np.abs(replay(name, 0, ignore_ell0=True) - ref)
    tol = cc.tolerance(name, ref)
    blocks = cc.block_slices(name)
    for io, e in enumerate(ell0):
        if e == -1: assert (moved[blocks[io], blocks[io]] >= 1e3 * tol[blocks[io], blocks[io]]).any(), (name, io)
        elif e == 0: assert np.array_equal(replay(name, 0, ignore_ell0=True)[blocks[io], blocks[io]], replay(name, 0)[blocks[io], blocks[io]])


def test_symmetrisation_is_what_makes_the_result_exactly_symmetric():
    asymmetric = []
    for name in cc.names():
        ref = cc.reference(name)[0]
        raw = replay(name, 0, symmetrise=False)
        tol = cc.tolerance(name, ref)
        assert (np.abs(raw - ref) <= tol).all() and (np.abs(raw - raw.T) <= 1e-2 * tol).all()          # rounding only (see the module's docstring)
        if not np.array_equal(raw, raw.T): asymmetric.append(name)
        assert np.array_equal(replay(name, 0), replay(name, 0).T)
    assert len(asymmetric) >= 3, asymmetric
