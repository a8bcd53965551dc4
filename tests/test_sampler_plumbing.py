"""What the samplers share on the Python side: the owner of a C handle (``_lib._Handle``), the pointer helper, the file names of the chains and the ``chains``
argument (``samplers._chain_file_names``, ``samplers._parse_chains``).  No GPU, no library: the handle base runs against a stub that records its calls."""
import ctypes
import gc

import numpy as np
import pytest

from desilike_amd import _lib
from desilike_amd.samplers import _chain_file_names, _parse_chains


class StubLibrary(object):
    """Stands for the loaded library: ``dl_stub_create`` / ``dl_stub_destroy`` / ``dl_stub_info`` / ``dl_last_error``, every call recorded."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def dl_stub_create(self, handle, *args):
        self.calls.append(('create',) + args)
        if self.rc == 0: handle._obj.value = 0x1234      # (handle: the byref of the owner's c_void_p)
        return self.rc

    def dl_stub_destroy(self, handle):
        self.calls.append(('destroy', handle.value))

    def dl_stub_info(self, handle, key):
        self.calls.append(('info', key))
        return 7

    def dl_last_error(self, handle):
        self.calls.append(('last_error', handle))
        return b'the stub refuses'


class Owner(_lib._Handle):
    _prefix = 'dl_stub'

    def __init__(self, size, fail_early=False):
        if fail_early: raise ValueError('before the handle')
        self._create(int(size))


@pytest.fixture
def stub(monkeypatch):
    library = StubLibrary()
    monkeypatch.setattr(_lib, 'load', lambda: library)
    return library


def test_handle_create_and_info(stub):
    owner = Owner(3)
    assert stub.calls == [('create', 3)] and owner._handle.value == 0x1234
    assert owner.info('n') == 7 and stub.calls[-1] == ('info', b'n')


def test_handle_create_failure_raises_the_library_message(stub):
    stub.rc = 1
    with pytest.raises(_lib.LibraryError, match='the stub refuses'):
        Owner(3)
    assert ('last_error', None) in stub.calls and not any(call[0] == 'destroy' for call in stub.calls)


def test_handle_close_twice_destroys_once(stub):
    owner = Owner(3)
    owner.close()
    owner.close()
    assert [call for call in stub.calls if call[0] == 'destroy'] == [('destroy', 0x1234)]
    assert owner._handle is None
    del owner
    gc.collect()
    assert sum(call[0] == 'destroy' for call in stub.calls) == 1


def test_handle_collected_destroys(stub):
    Owner(3)
    gc.collect()
    assert stub.calls[-1] == ('destroy', 0x1234)


def test_handle_del_of_a_half_built_owner_is_silent(stub, recwarn, capsys):
    for kwargs in (dict(fail_early=True), dict()):
        stub.rc = 1      # (the second owner fails in create: it has a library but no handle)
        with pytest.raises((ValueError, _lib.LibraryError)):
            Owner(3, **kwargs)
    half = Owner.__new__(Owner)      # nothing of the constructor has run
    half.close()
    half.__del__()
    del half
    gc.collect()
    assert not any(call[0] == 'destroy' for call in stub.calls)
    assert capsys.readouterr().err == '' and not len(recwarn)     # (an exception in __del__ would be printed as "Exception ignored in ...")


def test_handle_check(stub):
    owner = Owner(3)
    owner._check(0)
    with pytest.raises(_lib.LibraryError, match='the stub refuses'):
        owner._check(1)


def test_every_owner_derives_from_the_handle():
    owners = [_lib.Context, _lib.FFTLogPlan, _lib.DeviceEnsemble, _lib.CovariancePlan, _lib.MLPTrainer, _lib.DeviceMH, _lib.DeviceNUTS, _lib.DeviceMCLMC, _lib.DeviceSMC,
              _lib.DeviceNested]
    for owner in owners:
        assert issubclass(owner, _lib._Handle)
        assert owner._prefix + '_create' in _lib.SYMBOLS and owner._prefix + '_destroy' in _lib.SYMBOLS
        assert 'close' not in vars(owner) and '__del__' not in vars(owner)


def test_pointer_by_dtype():
    for dtype, ctype in [('f8', ctypes.c_double), ('i8', ctypes.c_int64), ('i4', ctypes.c_int32)]:
        array = np.arange(3, dtype=dtype)
        pointer = _lib._ptr(array)
        assert isinstance(pointer, ctypes.POINTER(ctype))
        assert [pointer[i] for i in range(3)] == [0, 1, 2]
    assert _lib._ptr(None) is None


def test_ids():
    ids = _lib._ids(None, 3, 'chain')
    assert ids.dtype == np.int32 and ids.flags['C_CONTIGUOUS'] and ids.tolist() == [0, 1, 2]
    assert _lib._ids([4, 2], 2, 'run').tolist() == [4, 2]
    with pytest.raises(ValueError, match='system_ids must have one entry per system'):
        _lib._ids([1, 2, 3], 2, 'system')


def test_chain_file_names():
    assert _chain_file_names('chain_*.npy', 3) == ['chain_0.npy', 'chain_1.npy', 'chain_2.npy']
    assert _chain_file_names(('a.npy', 'b.npy'), 2, distinct=True) == ['a.npy', 'b.npy']
    assert _chain_file_names('one.npy', 1, distinct=True) == ['one.npy']
    with pytest.raises(ValueError, match='^provide one file name per chain$'):
        _chain_file_names(['a.npy'], 2)
    with pytest.raises(ValueError, match=r'^provide one file name per chain \(or a template with \*\)$'):
        _chain_file_names(['a.npy'], 2, distinct=True)
    with pytest.raises(ValueError, match=r'^provide one file name per chain \(or a template with \*\)$'):
        _chain_file_names(['a.npy', 'a.npy'], 2, distinct=True)
    with pytest.raises(ValueError, match=r'^provide one file name per chain \(or a template with \*\)$'):
        _chain_file_names('same.npy', 2, distinct=True)      # (no * in the template: both chains would share the file)
    assert _chain_file_names('same.npy', 2) == ['same.npy', 'same.npy']     # (save(fn) has never asked for distinct names)


def test_parse_chains():
    class WithArrays(object):
        arrays = {}

    assert _parse_chains(4) == (4, None)
    assert _parse_chains(np.int64(2)) == (2, None)
    assert _parse_chains('chain.npy') == (1, ['chain.npy'])
    source = {'a': np.zeros(3)}
    nchains, resume = _parse_chains(source)
    assert nchains == 1 and resume[0] is source
    source = WithArrays()
    nchains, resume = _parse_chains(source)
    assert nchains == 1 and resume[0] is source
    assert _parse_chains(['a.npy', 'b.npy']) == (2, ['a.npy', 'b.npy'])
    for chains in (0, []):
        with pytest.raises(ValueError, match='chains must be >= 1'):
            _parse_chains(chains)
