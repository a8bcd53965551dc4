"""CPU: the cases and references of tests/fftlog_cases.py (the FFTLog sweep that tests/test_gpu_fftlog_shapes.py runs on the device) -- that every case sits on the edges it
is named for and the table as a whole covers every FFT length, pass schedule and padding geometry of csrc/dl_fftlog.hip; that the batched NumPy restatement the device
is compared with IS ``oracle/np_fftlog.py`` (bit for bit) and equals the O(N^2) long-double statement of the transform to 1e-14 of the row's largest |xi s^{3/2}|, an order
of magnitude inside the device tolerance of 1e-13; and that the compared numbers move by far more than that tolerance under the mistakes the sweep is there to catch."""
import numpy as np
import pytest

import fftlog_cases as fc


def test_every_case_sits_on_its_edges():
    for name in fc.names():
        case = fc.CASES[name]
        n, f, npad, pad, L = fc.geometry(name)
        ptc = fc.host(name)
        assert (ptc.k.size, ptc.npad, ptc.pad) == (n, npad, pad), name
        assert (npad, L) == (case['npad'], case['L']) and 2 << L == npad and 1 <= n <= npad, name
        assert case['edges'] and set(case['edges']) <= set(fc.EDGES), name
        for edge in case['edges']: assert fc.EDGES[edge](n, f, npad, pad, L), (name, edge)
        assert (n, npad) != (2048, 4096), name             # that shape runs the specialised kernel: it is not a case of the generic one
        assert case['ells'] in fc.ELL_SETS


def test_table_covers_lengths_schedules_and_paddings():
    geo = {name: fc.geometry(name) for name in fc.names()}
    required = {(8, 2), (16, 1), (9, 1), (16, 2), (11, 2), (20, 2), (33, 1), (128, 1), (100, 2), (255, 1), (256, 2), (129, 2), (100, 8), (1000, 2), (2048, 1),
                (1500, 2), (2047, 2), (4096, 1), (4096, 2), (3001, 2), (2048, 4), (8192, 1)}
    assert required <= {(n, f) for n, f, _, _, _ in geo.values()}
    assert {L for _, _, _, _, L in geo.values()} == set(range(3, 13))
    assert {L % 4 for _, _, _, _, L in geo.values()} == {0, 1, 2, 3}
    assert {4, 8, 12} <= {L for _, _, _, _, L in geo.values() if L % 4 == 0}
    assert any(pad == 0 and n == npad for n, _, npad, pad, _ in geo.values()) and any(pad == 0 and n < npad for n, _, npad, pad, _ in geo.values())
    assert any(pad % 2 == 1 for _, _, _, pad, _ in geo.values())
    assert sum((npad - n) % 2 == 1 for n, _, npad, _, _ in geo.values()) >= 5
    assert any(pad % 2 == 1 and (npad - n) % 2 == 0 for n, _, npad, pad, _ in geo.values())
    assert {f for _, f, _, _, _ in geo.values()} == {1, 2, 4, 8}
    assert {len(fc.CASES[name]['ells']) for name in fc.names()} == {1, 2, 3, 5}
    # every edge has a case, and so has every edge the persistent kernel does not have at every FFT length it could matter
    assert {edge for name in fc.names() for edge in fc.CASES[name]['edges']} == set(fc.EDGES)
    at = lambda edge: {fc.CASES[name]['L'] for name in fc.names() if edge in fc.CASES[name]['edges']}
    assert at('all4') == {4, 8, 12} and at('lds_attr') == {12} and at('generic4096') == {11}
    assert {3, 6, 10, 11, 12} <= at('full') and {3, 5, 8, 12} <= at('odd_pad') and {3, 4, 5, 7, 8, 11, 12} <= at('unequal')
    # the multipole table selection (blockIdx % n_ell) is exercised with more than one multipole at L % 4 == 0 and at the LDS branch
    assert any(len(fc.CASES[name]['ells']) > 1 for name in fc.names() if 'all4' in fc.CASES[name]['edges'])
    assert any(len(fc.CASES[name]['ells']) > 1 for name in fc.names() if 'lds_attr' in fc.CASES[name]['edges'])
    # the LDS request of the largest plan (csrc/dl_fftlog.hip: N2 + N2 / 16 + 1 complex numbers)
    assert fc.lds_bytes(8192) == 69648 and fc.lds_bytes(4096) <= 48 * 1024


@pytest.mark.parametrize('name', fc.names())
def test_restatement_is_the_oracle_bit_for_bit(name):
    ptc, fun = fc.host(name), fc.case_input(name)
    s, xi = fc.restate(ptc, fun)
    assert xi.shape == fun.shape and np.isfinite(xi).all() and (np.abs(xi).max(axis=-1) > 0.).all()
    for b in range(len(fun)):
        sh, xh = ptc(fun[b])
        assert np.array_equal(s, sh) and np.array_equal(xi[b], xh), (name, b)
    # ... whatever the batch around a row (the FFT of a batch works on several rows at once), and through the chunks of a large batch
    big = np.concatenate([fun[::-1], fun, fun[1:2]] * 3)
    _, xb = fc.restate(ptc, big, chunk=4)
    assert np.array_equal(xb, np.concatenate([xi[::-1], xi, xi[1:2]] * 3))


def test_restatement_without_low_ringing_is_the_oracle():
    name = 'L8_n129_f2'
    ptc, fun = fc.host(name, lowring=False), fc.case_input(name)
    assert all(offset == 0. for offset in ptc.offsets) and not np.array_equal(ptc.s, fc.host(name).s)
    s, xi = fc.restate(ptc, fun)
    for b in range(len(fun)):
        sh, xh = ptc(fun[b])
        assert np.array_equal(s, sh) and np.array_equal(xi[b], xh)


_worst = {}


@pytest.mark.parametrize('name', fc.names(max_npad=1024))
def test_restatement_against_long_double(name):
    """numpy.fft against the O(N^2) long-double DFT: 1e-14 of the row's largest |xi s^{3/2}| (measured: at most 3.1e-16 for ell = 0 .. 8 up to npad = 8192, which takes minutes
    and is therefore not a case here)."""
    ptc, fun = fc.host(name), fc.case_input(name)
    s, xi = fc.restate(ptc, fun)
    ref = fc.longdouble_reference(ptc, fun)
    assert ref.dtype == np.longdouble and ref.shape == xi.shape
    err = fc.row_errors(s.astype(np.longdouble), xi.astype(np.longdouble), ref)
    _worst[name] = float(err.max())
    print('{}: npad = {:d}, ells = {}: restatement vs long double {:.1e} of the row maximum (largest so far {:.1e})'.format(name, ptc.npad, fc.CASES[name]['ells'], _worst[name], max(_worst.values())))
    assert (err <= 1e-14).all(), (name, err)


def test_long_double_reference_on_closed_forms():
    """The long-double reference on inputs whose transform is known without any DFT: u = 1 turns the operation into reverse-in-place, so the reference must return
    prefactor * s^{-3/2} * (fun k^{3/2}) with sample i taken from padded position npad - 1 - pad - i."""
    name = 'L5_n33_f1'
    ptc, fun = fc.host(name), fc.case_input(name, B=2)
    n, npad, pad = ptc.k.size, ptc.npad, ptc.pad
    ptc.u = [np.ones_like(u) for u in ptc.u]
    ref = fc.longdouble_reference(ptc, fun)
    ld = np.longdouble
    padded = np.zeros(fun.shape[:-1] + (npad,), dtype=ld)
    padded[..., pad:pad + n] = fun.astype(ld) * (ptc.k**1.5).astype(ld)
    expected = np.array([ld(ptc.prefactor[ill]) * padded[:, ill, ::-1][:, pad:pad + n] * (ptc.s[ill][pad:pad + n]**(-1.5)).astype(ld) for ill in range(len(ptc.ells))]).transpose(1, 0, 2)
    assert np.abs(ref - expected).max() <= 1e-17 * np.abs(expected).max() * npad
    assert (npad - n) % 2 == 1 and np.abs(expected[..., 0]).max() == 0.      # unequal pads: the first output comes from the longer right-hand padding


@pytest.mark.parametrize('name', ['L3_n9_f1', 'L4_n10_f2', 'L7_n255_f1', 'L8_n129_f2', 'L9_n100_f8', 'L5_n20_f2'])
def test_compared_numbers_notice_a_wrong_pad_or_multipole(name):
    """One sample of left padding more or less (the mistake unequal or odd pads invite), or the coefficients of the neighbouring multipole (a wrong ``id % n_ell``), move every
    row by more than 1e-4 of its maximum: a billion times the device tolerance."""
    ptc, fun = fc.host(name), fc.case_input(name)
    s, xi = fc.restate(ptc, fun)
    moved = []
    for shift in (-1, 1):
        if not 0 <= ptc.pad + shift <= ptc.npad - ptc.k.size: continue
        other = fc.host(name)
        other.pad += shift
        moved.append(fc.row_errors(s, fc.restate(other, fun)[1], xi).min())
    assert moved
    if len(ptc.ells) > 1:
        other = fc.host(name)
        other.u = other.u[1:] + other.u[:1]
        moved.append(fc.row_errors(s, fc.restate(other, fun)[1], xi).min())
    print('{}: a wrong pad or multipole moves every row by at least {:.1e} of its maximum'.format(name, min(moved)))
    assert min(moved) > 1e-4, moved
