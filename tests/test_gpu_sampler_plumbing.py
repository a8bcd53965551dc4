"""GPU: the life of the six owners that are bound to a device context (``_lib._Handle``: DeviceEnsemble, DeviceMH, DeviceNUTS, DeviceMCLMC, DeviceSMC, DeviceNested), each
at its smallest legal size on the two-parameter Kaiser likelihood of the sampler tests: create, one ``info`` read, ``close()`` twice, collection.  No sampler kernel runs."""
import gc

import numpy as np
import pytest

from test_gpu_smc import _like

pytestmark = pytest.mark.gpu


class _NoLibrary(object):
    """In the place of an owner's library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError('a closed owner called {}'.format(name))


def test_owners_create_info_close_twice_collect():
    from desilike_amd import _lib
    like = _like('two')
    ctx, offset = like._get_posterior_context()
    assert ctx.n_params == 2
    widths = np.array([param.prior.limits[1] - param.prior.limits[0] if param.prior.dist == 'uniform' else param.prior.std() for param in like.varied_params], dtype='f8')
    makers = [lambda: _lib.DeviceEnsemble(ctx, 8, seed=1, offset=offset), lambda: _lib.DeviceMH(ctx, 2, seed=1, offset=offset), lambda: _lib.DeviceNUTS(ctx, 2, seed=1, offset=offset),
              lambda: _lib.DeviceMCLMC(ctx, 2, seed=1, offset=offset), lambda: _lib.DeviceSMC(ctx, 1, 64, widths, seed=1, offset=offset),
              lambda: _lib.DeviceNested(ctx, 1, 64, widths, seed=1, offset=offset)]
    for make in makers:
        owner = make()
        assert isinstance(owner, _lib._Handle) and owner._handle
        assert owner.info('n_params') == 2
        owner.close()
        assert owner._handle is None
        owner._lib = _NoLibrary()
        owner.close()              # the second call does not reach the library
        del owner
        gc.collect()
    for make in makers:            # collected without close(): __del__ destroys
        make()
    gc.collect()
    assert ctx.info('n_params') == 2      # the context outlives its owners
