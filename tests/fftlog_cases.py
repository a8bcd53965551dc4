"""TEST INFRASTRUCTURE, no GPU: the cases of the FFTLog sweep (tests/test_fftlog_cases.py on the CPU, tests/test_gpu_fftlog_shapes.py on the device) and their references.

``CASES``: named ``(n, minfolds, ells)`` -- every FFT length the generic kernel of csrc/dl_fftlog.hip accepts (L = log2(npad / 2) = 3 .. 12: every fused-stage schedule
``Slast = (L & 3) ? (L & 3) : 4``, the 69.6 KB LDS request of npad = 8192), the padding geometries (none, none on one side, odd, unequal left and right, 4 and 8 folds)
and 1, 2, 3 and 5 multipoles.  Every case states the edges it is there for (``edges``); tests/test_fftlog_cases.py holds it to them.

``restate``: the arithmetic of ``oracle/np_fftlog.py::PowerToCorrelation.__call__`` on ``[..., n_ell, n]`` at once (numpy.fft along the last axis, the grid constants of the
object), so that the thousands of rows of the persistent-kernel tests cost milliseconds.

``longdouble_reference``: the plain statement of the operation -- zero-pad, O(N^2) DFT with the cosines and sines of 2 pi (j m mod N) / N, times the Hermitian extension
of u, inverse DFT, reverse, un-pad, scale -- in ``numpy.longdouble``.  It shares nothing with an FFT.  It uses the float64 grid constants of the object (k^{3/2}, u, prefactor,
s^{-3/2}) promoted to long double: the operation under test is defined on those constants."""
from collections import OrderedDict

import numpy as np

from oracle.np_fftlog import PowerToCorrelation as HostPowerToCorrelation

THREADS = 128            # csrc/dl_fftlog.hip: DL_FF_THREADS
ELL_SETS = [(0,), (2,), (0, 2), (0, 2, 4), (0, 2, 4, 6, 8)]

# edge -> condition on (n, minfolds, npad, pad, L)
EDGES = OrderedDict([
    ('full', lambda n, f, npad, pad, L: n == npad),                                   # no padding at all: the reversed read touches both ends of the sequence
    ('pad0', lambda n, f, npad, pad, L: pad == 0),
    ('even_pad', lambda n, f, npad, pad, L: pad > 0 and pad % 2 == 0 and (npad - n) % 2 == 0),
    ('odd_pad', lambda n, f, npad, pad, L: pad % 2 == 1),                             # a complex LDS element holds one padding zero and one sample
    ('unequal', lambda n, f, npad, pad, L: (npad - n) % 2 == 1),                      # one more zero on the right than on the left
    ('wide_pad', lambda n, f, npad, pad, L: 2 * pad >= 3 * n),                        # beyond minfolds = 2, where pad < 3 n / 2
    ('folds4', lambda n, f, npad, pad, L: f == 4),
    ('folds8', lambda n, f, npad, pad, L: f == 8),
    ('all4', lambda n, f, npad, pad, L: L % 4 == 0),                                  # every pass fuses four stages; the inverse opens with one at hl = 1
    ('generic4096', lambda n, f, npad, pad, L: npad == 4096 and n != 2048),           # L = 11 on the generic kernel
    ('lds_attr', lambda n, f, npad, pad, L: lds_bytes(npad) > 48 * 1024),             # dl_fftlog_create raises the kernel's dynamic LDS limit
    ('short_row', lambda n, f, npad, pad, L: n < THREADS),                            # fewer samples than threads
])


def lds_bytes(npad):
    """Dynamic LDS of the generic kernel: N2 complex numbers, one slot of padding every 16."""
    N2 = npad // 2
    return (N2 + (N2 >> 4) + 1) * 16


_TABLE = [
    # L, npad, n, minfolds, edges
    (3, 16, 8, 2, ('even_pad', 'short_row')),
    (3, 16, 16, 1, ('full', 'pad0')),
    (3, 16, 9, 1, ('unequal', 'odd_pad')),
    (4, 32, 16, 2, ('all4', 'even_pad')),
    (4, 32, 11, 2, ('all4', 'unequal')),
    (4, 32, 10, 2, ('all4', 'odd_pad')),               # odd, equal pads
    (5, 64, 20, 2, ('even_pad',)),
    (5, 64, 33, 1, ('unequal', 'odd_pad')),
    (6, 128, 128, 1, ('full', 'pad0')),
    (7, 256, 100, 2, ('even_pad', 'short_row')),
    (7, 256, 255, 1, ('pad0', 'unequal')),             # no zero on the left, one on the right
    (8, 512, 256, 2, ('all4', 'even_pad')),
    (8, 512, 129, 2, ('all4', 'unequal', 'odd_pad')),
    (9, 1024, 100, 8, ('folds8', 'wide_pad')),
    (10, 2048, 1000, 2, ('even_pad',)),
    (10, 2048, 2048, 1, ('full', 'pad0')),
    (11, 4096, 1500, 2, ('generic4096', 'even_pad')),
    (11, 4096, 2047, 2, ('generic4096', 'unequal')),   # the neighbour of the specialised shape
    (11, 4096, 4096, 1, ('generic4096', 'full', 'pad0')),
    (12, 8192, 4096, 2, ('all4', 'lds_attr', 'even_pad')),
    (12, 8192, 3001, 2, ('all4', 'lds_attr', 'unequal', 'odd_pad')),
    (12, 8192, 2048, 4, ('all4', 'lds_attr', 'folds4', 'wide_pad')),
    (12, 8192, 8192, 1, ('all4', 'lds_attr', 'full', 'pad0')),
]

CASES = OrderedDict()
for _i, (_L, _npad, _n, _f, _edges) in enumerate(_TABLE):
    CASES['L{:d}_n{:d}_f{:d}'.format(_L, _n, _f)] = dict(L=_L, npad=_npad, n=_n, minfolds=_f, ells=ELL_SETS[_i % len(ELL_SETS)], edges=_edges)


def names(max_npad=None):
    return [name for name, case in CASES.items() if max_npad is None or case['npad'] <= max_npad]


def grid(n):
    return np.logspace(-4., 3., n)


def geometry(name):
    """(n, minfolds, npad, pad, L) of the case as ``PowerToCorrelation`` lays it out (NOT read from the table: the table's L and npad are claims the CPU test checks)."""
    case = CASES[name]
    n, f = case['n'], case['minfolds']
    npad = int(2**np.ceil(np.log2(f * n)))
    return n, f, npad, (npad - n) // 2, int(np.log2(npad // 2))


def host(name, lowring=True):
    case = CASES[name]
    return HostPowerToCorrelation(grid(case['n']), ell=case['ells'], lowring=lowring, minfolds=case['minfolds'])


def random_input(k, shape, seed):
    """The input family of tests/test_gpu_fftlog.py::test_device_fftlog_vs_host_restatement: ``shape + (len(k),)`` seeded normal deviates under a smooth envelope."""
    rng = np.random.RandomState(seed)
    return rng.standard_normal(tuple(shape) + (k.size,)) * ((k / 0.1)**-1.2 * np.exp(-(np.log(k / 0.05) / 3.)**2))


def case_input(name, B=3):
    case = CASES[name]
    return random_input(grid(case['n']), (B, len(case['ells'])), seed=1000 + names().index(name))


def scaled(s, xi):
    return xi * s**1.5


def row_errors(s, got, ref):
    """Largest error of every transform in units of the transform's largest |xi s^{3/2}| (the measure of tests/test_gpu_fftlog.py)."""
    a, r = scaled(s, got), scaled(s, ref)
    return np.abs(a - r).max(axis=-1) / np.abs(r).max(axis=-1)


def restate(ptc, fun, chunk=512):
    """``oracle/np_fftlog.py::PowerToCorrelation.__call__`` on ``fun [..., n_ell, n]`` at once -> ``(s [n_ell, n], xi [..., n_ell, n])``; ``ptc``: any ``PowerToCorrelation``
    (host or device flavour: only its grid constants are used)."""
    fun = np.asarray(fun, dtype='f8')
    n, n_ell, npad, pad = ptc.k.size, len(ptc.ells), ptc.npad, ptc.pad
    assert fun.shape[-2:] == (n_ell, n), fun.shape
    sl = slice(pad, pad + n)
    u = np.array(ptc.u)                                         # [n_ell, npad / 2 + 1]
    s = np.array([s[sl] for s in ptc.s])
    spow = np.array([s[sl]**(-1.5) for s in ptc.s])
    pre = ptc.k**1.5
    flat = fun.reshape((-1, n_ell, n))
    xi = np.empty_like(flat)
    for start in range(0, len(flat), chunk):                   # (bounds the padded copies of a large batch)
        part = flat[start:start + chunk]
        a = np.zeros(part.shape[:-1] + (npad,), dtype='f8')
        a[..., sl] = part * pre
        A = np.fft.irfft(np.fft.rfft(a, axis=-1) * u, npad, axis=-1)[..., ::-1]
        for ill in range(n_ell): xi[start:start + chunk, ill] = ptc.prefactor[ill] * A[:, ill, sl] * spow[ill]
    return s, xi.reshape(fun.shape)


def longdouble_reference(ptc, fun, chunk=128):
    """The transform by its definition, in long double: ``fun [..., n_ell, n]`` -> ``xi [..., n_ell, n]`` (numpy.longdouble)."""
    ld = np.longdouble
    n, n_ell, N, pad = ptc.k.size, len(ptc.ells), ptc.npad, ptc.pad
    fun = np.asarray(fun, dtype='f8')
    assert fun.shape[-2:] == (n_ell, n), fun.shape
    flat = fun.reshape((-1, n_ell, n))
    a = np.zeros((len(flat), n_ell, N), dtype=ld)
    a[..., pad:pad + n] = flat.astype(ld) * (ptc.k**1.5).astype(ld)
    pi = ld(4.) * np.arctan(ld(1.))
    angle = ld(2.) * pi * np.arange(N).astype(ld) / ld(N)
    ctab, stab = np.cos(angle), np.sin(angle)
    index = np.arange(N, dtype='i8')
    # Hermitian extension of u: U[m] = u[m] (m <= N / 2), U[N - m] = conj(u[m]); u[0] and u[N / 2] are real (irfft ignores the imaginary parts of both bins)
    ur, ui = np.empty((n_ell, N), dtype=ld), np.empty((n_ell, N), dtype=ld)
    for ill, u in enumerate(ptc.u):
        assert u.shape == (N // 2 + 1,) and u.imag[0] == 0. and u.imag[-1] == 0.
        ur[ill, :N // 2 + 1], ui[ill, :N // 2 + 1] = u.real, u.imag
        ur[ill, N // 2 + 1:], ui[ill, N // 2 + 1:] = u.real[1:N // 2][::-1], -u.imag[1:N // 2][::-1]
    # forward: X[m] = sum_j a[j] exp(-2 pi i j m / N), the DFT matrix in chunks of rows m
    xr, xim = np.empty(a.shape, dtype=ld), np.empty(a.shape, dtype=ld)
    for start in range(0, N, chunk):
        jm = (index[start:start + chunk, None] * index[None, :]) % N             # [m, j]
        xr[..., start:start + chunk] = a @ ctab[jm].T
        xim[..., start:start + chunk] = -(a @ stab[jm].T)
    yr, yi = xr * ur - xim * ui, xr * ui + xim * ur
    # inverse: a'[j] = 1 / N sum_m Re(Y[m] exp(+2 pi i j m / N)) (Y is Hermitian: the imaginary part of the sum vanishes)
    back = np.empty(a.shape, dtype=ld)
    for start in range(0, N, chunk):
        jm = (index[start:start + chunk, None] * index[None, :]) % N             # [j, m]
        back[..., start:start + chunk] = (yr @ ctab[jm].T - yi @ stab[jm].T) / ld(N)
    A = back[..., ::-1][..., pad:pad + n]
    xi = np.empty(flat.shape, dtype=ld)
    for ill in range(n_ell):
        xi[:, ill] = ld(ptc.prefactor[ill]) * A[:, ill] * (ptc.s[ill][pad:pad + n]**(-1.5)).astype(ld)
    return xi.reshape(fun.shape)
