"""GPU (-m gpu): the two kernels of csrc/dl_fftlog.hip over the cases of tests/fftlog_cases.py -- the generic kernel at every FFT length it accepts (L = 3 .. 12: every
fused-stage schedule, the raised LDS limit of npad = 8192), without padding, with odd, unequal and wide padding and 1 to 5 multipoles; the persistent kernel of the
reference's grid with more transforms than resident workgroups (the loop, the prefetch of the next row, the state carried from one transform to the next, the multipole
tables re-pointed between iterations, the ragged end); non-finite rows next to finite ones; the same rows in batches of different sizes.
Reference: the batched NumPy restatement, which tests/test_fftlog_cases.py pins bit for bit on oracle/np_fftlog.py and to 1e-14 on an O(N^2) long-double DFT.
Tolerance: 1e-13 of the transform's largest |xi s^{3/2}|, the tolerance of tests/test_gpu_fftlog.py (float64 FFTs of at most 8192 points: measured 2e-16 .. 6e-16)."""
import numpy as np
import pytest

import fftlog_cases as fc

pytestmark = pytest.mark.gpu
TOL = 1e-13
GRID = np.logspace(-4., 3., 2048)           # the reference's grid: npad = 4096, the persistent kernel


def device_ptc(name, lowring=True):
    from desilike_amd.fftlog import PowerToCorrelation
    case = fc.CASES[name]
    return PowerToCorrelation(fc.grid(case['n']), ell=case['ells'], lowring=lowring, minfolds=case['minfolds'], device=0)


def run(dev, fun):
    """``fun [B, n_ell, n]`` (host) through the device plan -> host array: one launch."""
    import torch
    out = dev.apply_device(torch.as_tensor(np.ascontiguousarray(fun), dtype=torch.float64, device='cuda:0'))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(a, b):
    """Equal as bit patterns (NaN payloads and signed zeros included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view('u8'), b.view('u8'))


# ---- (a), (b): the generic kernel over the table

@pytest.mark.parametrize('name', fc.names())
def test_generic_kernel_case(name):
    case = fc.CASES[name]
    assert (case['n'], case['npad']) != (2048, 4096)
    fun = fc.case_input(name, B=3)
    dev = device_ptc(name)
    try:
        s, xi = dev(fun)
        sr, ref = fc.restate(dev, fun)
        assert xi.shape == fun.shape and np.array_equal(s, sr) and np.array_equal(s, fc.host(name)(fun[0])[0])
        err = fc.row_errors(s, xi, ref)
        print('{}: npad = {:d}, pad = {:d}, ells = {}: {:.1e} of the row maximum'.format(name, dev.npad, dev.pad, case['ells'], err.max()))
        assert (err <= TOL).all(), (name, err)
        assert same_bits(dev(fun)[1], xi)
    finally:
        dev.close()


def test_generic_kernel_without_low_ringing():
    name = 'L8_n129_f2'
    fun = fc.case_input(name, B=3)
    dev = device_ptc(name, lowring=False)
    try:
        s, xi = dev(fun)
        sr, ref = fc.restate(dev, fun)
        assert np.array_equal(s, sr) and not np.array_equal(s, fc.restate(fc.host(name), fun)[0])        # (another output grid than with the low-ringing offset)
        err = fc.row_errors(s, xi, ref)
        print('{} (lowring = False): {:.1e} of the row maximum'.format(name, err.max()))
        assert (err <= TOL).all(), err
    finally:
        dev.close()


@pytest.mark.parametrize('name', [name for name in fc.names() if 'lds_attr' in fc.CASES[name]['edges']])
def test_largest_plan_is_created_and_runs(name):
    """npad = 8192 asks for more dynamic LDS than a kernel gets by default: the plan either works -- creation, launch and a sane result, here on a batch of several workgroups
    per multipole -- or is refused AT CREATION with a message that names npad; a launch that fails later, or a plan that quietly computes nothing, is a bug."""
    from desilike_amd._lib import LibraryError
    dev = device_ptc(name)
    assert fc.lds_bytes(dev.npad) == 69648
    try:
        dev._get_plan()
    except LibraryError as exc:
        assert '8192' in str(exc) and 'npad' in str(exc), str(exc)
        pytest.fail('the device refuses the plan of npad = 8192: {}'.format(exc))
    try:
        fun = fc.random_input(dev.k, (7, len(dev.ells)), seed=12)
        s, ref = fc.restate(dev, fun)
        err = fc.row_errors(s, run(dev, fun), ref)
        assert (err <= TOL).all(), err
    finally:
        dev.close()


# ---- (c): the persistent kernel beyond one residency

def resident():
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return n_cu, 4 * n_cu


def persistent_batches():
    """(ells, B) with B n_ell just above the number R of resident workgroups for 1, 2 and a number of multipoles that does not divide R, and one between 2 R and 3 R."""
    n_cu, R = resident()
    odd = (0, 2, 4) if R % 3 else (0, 2, 4, 6, 8)
    assert R % len(odd) != 0
    batches = [((0,), R + 4), ((0, 2), R // 2 + 4), (odd, R // len(odd) + 4), (odd, (2 * R + R // 3) // len(odd) + 1)]
    for ells, B in batches[:3]: assert R < B * len(ells) <= R + 4 * len(ells)
    total = batches[3][1] * len(odd)
    assert 2 * R < total < 3 * R and total % R != 0
    return batches


def carried(total, n_ell, R):
    """(source, destination) transforms: sources in the first pass of the persistent loop (id < R), destinations in the second and (if the batch reaches it) third pass with
    the same multipole and, where there is room, in another workgroup than the source."""
    pairs = []
    for lo in (R, 2 * R):
        cursor = lo
        for src in [R - 1, 0, R // 2 + 1, 1, R // 3, 2, R - 2]:
            dst = cursor
            while dst < total and ((dst - src) % n_ell != 0 or dst % R == src): dst += 1      # (the launch has R workgroups: transform id runs in workgroup id % R)
            if dst >= total: break
            pairs.append((src, dst))
            cursor = dst + 1
    return pairs


@pytest.mark.parametrize('ibatch', range(4))
def test_persistent_kernel_beyond_one_residency(ibatch):
    from desilike_amd.fftlog import PowerToCorrelation
    n_cu, R = resident()
    ells, B = persistent_batches()[ibatch]
    n_ell, n = len(ells), GRID.size
    total = B * n_ell
    flat = fc.random_input(GRID, (total,), seed=40 + ibatch)                   # distinct rows
    pairs = carried(total, n_ell, R)
    assert len(pairs) >= 3 and all(src < R <= dst < total and (dst - src) % n_ell == 0 for src, dst in pairs)
    assert ibatch < 3 or any(dst >= 2 * R for _, dst in pairs)
    for src, dst in pairs: flat[dst] = flat[src]
    fun = flat.reshape(B, n_ell, n)
    dev = PowerToCorrelation(GRID, ell=ells, device=0)
    try:
        assert (dev.npad, dev.k.size) == (4096, 2048)
        xi = run(dev, fun)
        s, ref = fc.restate(dev, fun)
        err = fc.row_errors(s, xi, ref)
        print('persistent kernel: {:d} CUs, R = {:d}, ells = {}, B = {:d}, total = {:d} ({:d} full passes + {:d}): {:.1e} of the row maximum'.format(n_cu, R, ells, B, total, total // R, total % R, err.max()))
        assert (err <= TOL).all(), (np.argwhere(err > TOL)[:10], err.max())
        out = xi.reshape(total, n)
        for src, dst in pairs:
            assert same_bits(out[dst], out[src]), (src, dst)
            # ... and the bits of the same row in a batch of its own: one transform per workgroup, nothing carried
            alone = np.zeros((1, n_ell, n))
            alone[0, src % n_ell] = flat[src]
            assert same_bits(run(dev, alone)[0, src % n_ell], out[src]), src
        assert same_bits(run(dev, fun), xi)
    finally:
        dev.close()


# ---- (d): isolation

def check_isolation(dev, fun, ids):
    """Transforms ``ids`` = (NaN row, +inf row, zero row) of the flattened batch: every other transform keeps its bits."""
    B, n_ell, n = fun.shape
    clean = run(dev, fun).reshape(B * n_ell, n)
    assert np.isfinite(clean).all()
    dirty = fun.copy().reshape(B * n_ell, n)
    inan, iinf, izero = ids
    dirty[inan], dirty[iinf], dirty[izero] = np.nan, np.inf, 0.
    out = run(dev, dirty.reshape(fun.shape)).reshape(B * n_ell, n)
    others = np.setdiff1d(np.arange(B * n_ell), ids)
    assert same_bits(out[others], clean[others]), np.flatnonzero((out[others] != clean[others]).any(axis=1))[:10]
    assert not np.isfinite(out[inan]).any() and not np.isfinite(out[iinf]).any()
    assert (out[izero] == 0.).all()


def test_isolation_persistent_kernel():
    from desilike_amd.fftlog import PowerToCorrelation
    n_cu, R = resident()
    ells, B = persistent_batches()[2]
    total = B * len(ells)
    ids = (1, 4, min(7, total - R - 1))
    assert len(set(ids)) == 3 and all(0 <= i < R and i + R < total for i in ids)          # each has a successor in its workgroup
    dev = PowerToCorrelation(GRID, ell=ells, device=0)
    try:
        check_isolation(dev, fc.random_input(GRID, (B, len(ells)), seed=50), ids)
    finally:
        dev.close()


def test_isolation_generic_kernel():
    name = 'L8_n129_f2'
    dev = device_ptc(name)
    try:
        check_isolation(dev, fc.case_input(name, B=5), (1, 4, 7))
    finally:
        dev.close()


# ---- (e): batch-size independence of the generic kernel

def test_generic_kernel_whatever_the_batch():
    name = 'L10_n1000_f2'
    dev = device_ptc(name)
    n_ell = len(dev.ells)
    try:
        fun = fc.random_input(dev.k, (257, n_ell), seed=60)
        X, Y = fun[200].copy(), fun[17].copy()
        fun[0], fun[100], fun[256], fun[1] = X, X, X, Y
        one, two, many = run(dev, X[None]), run(dev, np.array([Y, X])), run(dev, fun)
        s, ref = fc.restate(dev, fun)
        assert (fc.row_errors(s, many, ref) <= TOL).all()
        for got in (two[1], many[0], many[100], many[200], many[256]): assert same_bits(got, one[0])
        for got in (many[1], many[17]): assert same_bits(got, two[0])
    finally:
        dev.close()
