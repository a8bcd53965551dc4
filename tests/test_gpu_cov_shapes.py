"""GPU (-m gpu): ``dl_cov_kernel`` / ``dl_cov_sym_kernel`` (csrc/dl_cov.hip, ``_lib.CovariancePlan``) on the plans of tests/cov_cases.py: theories without monopole,
five multipoles, partly overlapping bins of two P observables, xi before P and P before xi, two xi observables on different k grids, points outside a theory's k range,
eight observables, cell counts below and across a workgroup.  Against the oracle at the project's tolerance for this kernel (absolute part per block,
``cov_cases.tolerance``) and against the NumPy replay of the same plan (tests/cov_plan_numpy.py) at the rounding bound of ``cov_plan_numpy.rounding_bound``: a worst-case
count of roundings times 2^-53 times the absolute sum each element is made of -- the device contracts a * b + c into FMAs, the replay does not, nothing else differs.
On the CPU the replay itself sits on the oracle at <= 8e-5 of the tolerance (tests/test_cov_cases.py), so the bound against the replay is the sharper of the two.
Measured on an MI355X: <= 1.5e-4 of the tolerance against the oracle, <= 0.05 of the rounding bound against the replay, over the 7 cases x 3 draws."""
import numpy as np
import pytest

import cov_cases as cc
import cov_plan_numpy as cpn

pytestmark = pytest.mark.gpu


def make_plan(name):
    from desilike_amd._lib import CovariancePlan
    arrays, n_ell, n_k, ell0, shotnoise = cc.plan_arguments(name)
    plan = CovariancePlan(arrays['n'], n_ell, n_k, ell0, shotnoise, arrays['cell_i'], arrays['cell_d'], arrays['pt_i'], arrays['pt_d'], arrays['gtab'], arrays['sym'], device=0)
    return plan, (arrays, ell0, shotnoise)


def on_device(powers):
    import torch
    return [torch.as_tensor(np.ascontiguousarray(power), dtype=torch.float64, device='cuda:0').contiguous() for power in powers]


@pytest.mark.parametrize('name', cc.names())
def test_plan_on_the_device_vs_oracle_and_replay(name):
    import torch
    plan, (arrays, ell0, shotnoise) = make_plan(name)
    spectra = cc.spectra(name)
    powers = on_device(spectra)
    got = plan.apply(powers).cpu().numpy()
    ref = cc.reference(name)
    assert got.shape == ref.shape == (cc.B, arrays['n'], arrays['n'])
    tol = cc.tolerance(name, ref)
    print('vs oracle, of the tolerance', (np.abs(got - ref) / tol).max())
    assert (np.abs(got - ref) <= tol).all()
    assert np.allclose(got, ref, rtol=cc.RTOL, atol=cc.ATOL * np.abs(ref).max())          # (the whole-matrix form of the bound, implied)
    for ipoint in range(cc.B):
        point = [power[ipoint] for power in spectra]
        replay, bound = cpn.apply_plan(arrays, ell0, shotnoise, point), cpn.rounding_bound(arrays, ell0, shotnoise, point)
        with np.errstate(invalid='ignore', divide='ignore'):
            print('vs replay, of the rounding bound', np.nanmax(np.where(bound > 0., np.abs(got[ipoint] - replay) / bound, 0.)))
        assert (np.abs(got[ipoint] - replay) <= bound).all()          # (bound 0 where no cell writes: exactly 0 there)
    assert np.array_equal(got, np.swapaxes(got, 1, 2))                # symmetric, exactly
    # any position of a batch of 37, into a preallocated output, on a non-default stream
    index = np.arange(37) % cc.B
    big = on_device([power[index] for power in spectra])
    out = torch.full((37, arrays['n'], arrays['n']), float('nan'), dtype=torch.float64, device='cuda:0')
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    assert plan.apply(big, out=out, stream=side.cuda_stream) is out
    side.synchronize()
    batch = out.cpu().numpy()
    assert all(np.array_equal(batch[i], got[index[i]]) for i in range(37))
    # an empty batch
    empty = plan.apply([power[:0].contiguous() for power in powers])
    assert tuple(empty.shape) == (0, arrays['n'], arrays['n']) and empty.dtype == torch.float64
    plan.close()


def test_bad_plans_are_errors_of_create():
    """Arguments ``dl_cov_create`` must refuse on the host, before anything is uploaded or launched."""
    from desilike_amd._lib import CovariancePlan, LibraryError
    arrays, n_ell, n_k, ell0, shotnoise = cc.plan_arguments('two_pk')

    def create(n_ell=n_ell, n_k=n_k, ell0=ell0, shotnoise=shotnoise, **changed):
        a = dict(arrays, **changed)
        return CovariancePlan(a['n'], n_ell, n_k, ell0, shotnoise, a['cell_i'], a['cell_d'], a['pt_i'], a['pt_d'], a['gtab'], a['sym'], device=0)

    create().close()          # the unchanged plan is fine
    with pytest.raises(LibraryError, match='dl_cov_create: invalid argument'):          # 9 observables
        create(n_ell=[3] * 9, n_k=[25] * 9, ell0=[0] * 9, shotnoise=[1e3] * 9)
    for bad in (dict(n_ell=[6, 3]), dict(n_k=[25, 1])):
        with pytest.raises(LibraryError, match='dl_cov_create: a theory needs 1 to 5 multipoles and at least 2 wavenumbers'):
            create(**bad)
    last = len(arrays['cell_i']) - 1
    for column, value in [(0, arrays['n']), (1, -1), (2, 2), (3, -1), (4, len(arrays['gtab'])), (7, len(arrays['pt_i']) + 1)]:
        cell_i = arrays['cell_i'].copy()
        cell_i[last, column] = value
        with pytest.raises(LibraryError, match='dl_cov_create: cell {:d} out of range'.format(last)):
            create(cell_i=cell_i)
    cell = arrays['cell_i'][last]
    for column, value in [(0, n_k[cell[2]] - 1), (1, n_k[cell[3]] - 1), (0, -1)]:
        pt_i = arrays['pt_i'].copy()
        pt_i[cell[6], column] = value
        with pytest.raises(LibraryError, match='dl_cov_create: interpolation interval out of range in cell'):
            create(pt_i=pt_i)
    sym = arrays['sym'].copy()
    sym[0, 1] = arrays['n']
    with pytest.raises(LibraryError, match='dl_cov_create: symmetrisation pair out of range'):
        create(sym=sym)
