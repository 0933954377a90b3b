"""The batched spectral-norm entry points' C ABI without a GPU: the workspace query and every bad-argument return code, which are
decided before anything is launched."""
import ctypes
import os

import pytest
import torch

from tartangan_amd import backend

TG_EINVAL, TG_EUNSUPPORTED, TG_EWORKSPACE = -1, -2, -3
NEW = ('tg_sn_batch_workspace', 'tg_sn_batch_fwd', 'tg_sn_batch_bwd')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(backend.LIBRARY):
        pytest.fail(f'{backend.LIBRARY} is missing: build it first (python __graft_entry__.py build)')
    handle = ctypes.CDLL(backend.LIBRARY)
    protos = backend.parse_header()
    for name in NEW:
        ret, params = protos[name]
        fn = getattr(handle, name)
        fn.restype = backend._CTYPES[ret]
        fn.argtypes = [backend._CTYPES[t] for t, _ in params]
    return handle


def table(*rows):
    return torch.tensor(rows, dtype=torch.int64)


P = 256                           # never dereferenced: every call below is refused before a launch
PP = ctypes.c_void_p(P)
GOOD = [P, P, P, P, P, P, 70, 333]


def test_the_new_entry_points_are_declared_and_exported(lib):
    protos = backend.parse_header()
    assert all(n in protos and hasattr(lib, n) for n in NEW)
    lib.tg_version.restype = ctypes.c_int
    assert lib.tg_version() >= 107


def test_workspace_query(lib):
    one, two = table(GOOD), table(GOOD, [P, P, P, P, 0, 0, 1, 1])
    n1, n2 = lib.tg_sn_batch_workspace(one.data_ptr(), 1), lib.tg_sn_batch_workspace(two.data_ptr(), 2)
    # per layer: the W^T u partials of every 64-row slab, the scratch u', one <g, w> partial per 2048 elements
    assert n1 >= 4 * (2 * 333 + 70 + 12) and n1 % 4 == 0
    assert n2 > n1
    assert lib.tg_sn_batch_workspace(None, 1) == 0 and lib.tg_sn_batch_workspace(one.data_ptr(), 0) == 0
    assert lib.tg_sn_batch_workspace(table([P, P, P, P, P, P, 0, 4]).data_ptr(), 1) == 0


def bad_tables():
    for f in range(4):                                    # a null address among w_orig, u, v, w_sn
        row = list(GOOD)
        row[f] = 0
        yield row
    yield [P, P, P + 2, P, P, P, 70, 333]                 # an address that is no multiple of 4
    yield [P, P, P, P, P, P, 0, 333]
    yield [P, P, P, P, P, P, 70, -1]


def test_bad_arguments_return_codes(lib):
    good = table(GOOD)
    need = lib.tg_sn_batch_workspace(good.data_ptr(), 1)
    fwd = lambda items, n, sigma, ws, nbytes: lib.tg_sn_batch_fwd(items, n, sigma, ws, nbytes, 1, 1e-12, None)
    bwd = lambda items, n, sigma, ws, nbytes: lib.tg_sn_batch_bwd(items, n, sigma, ws, nbytes, 1, None)
    for call in (fwd, bwd):
        assert call(good.data_ptr(), 0, PP, PP, need) == TG_EINVAL
        assert call(good.data_ptr(), -3, PP, PP, need) == TG_EINVAL
        assert call(None, 1, PP, PP, need) == TG_EINVAL
        assert call(good.data_ptr(), 1, None, PP, need) == TG_EINVAL
        assert call(good.data_ptr(), 1, PP, None, need) == TG_EINVAL
        assert call(good.data_ptr(), 1, PP, PP, need - 4) == TG_EWORKSPACE
        assert call(good.data_ptr(), 1, PP, PP, 0) == TG_EWORKSPACE
        for row in bad_tables():
            t = table(GOOD, row)                          # the second of two layers is the bad one: nothing of the first is launched
            assert call(t.data_ptr(), 2, PP, PP, 1 << 30) == TG_EINVAL, row
        big = table([P, P, P, P, P, P, 1 << 16, 1 << 15])
        assert call(big.data_ptr(), 1, PP, PP, 1 << 40) == TG_EUNSUPPORTED
    # the gradient fields: optional for the forward (it would pass the checks and launch, so only the backward is asked here)
    nograd = table([P, P, P, P, 0, P, 70, 333])
    assert bwd(nograd.data_ptr(), 1, PP, PP, need) == TG_EINVAL
    nograd = table([P, P, P, P, P, 0, 70, 333])
    assert bwd(nograd.data_ptr(), 1, PP, PP, need) == TG_EINVAL
