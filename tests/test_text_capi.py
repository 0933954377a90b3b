"""The text kernels' C ABI without a GPU: the host queries (tg_conv1d_supported, the workspace sizes) and the bad-argument return
codes of every new entry point, which are decided before anything is launched."""
import ctypes
import os

import pytest

from tartangan_amd import backend

TG_EINVAL, TG_EUNSUPPORTED, TG_EWORKSPACE = -1, -2, -3
NEW = ('tg_conv1d_supported', 'tg_conv1d_fwd', 'tg_conv1d_dgrad', 'tg_conv1d_wgrad_workspace', 'tg_conv1d_wgrad', 'tg_up2x1d', 'tg_pool2_1d',
       'tg_skipgram_workspace', 'tg_skipgram_step', 'tg_embed_gather_t', 'tg_embed_lookup')


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


def test_the_new_entry_points_are_declared_and_exported(lib):
    protos = backend.parse_header()
    assert all(n in protos and hasattr(lib, n) for n in NEW)
    lib.tg_version.restype = ctypes.c_int
    assert lib.tg_version() >= 105


def test_conv1d_host_queries(lib):
    for ks in (1, 3):
        assert lib.tg_conv1d_supported(128, 64, 64, 64, ks) == 1 and lib.tg_conv1d_supported(1, 1, 1, 1, ks) == 1
    for bad in ((128, 64, 64, 64, 5), (128, 64, 64, 64, 2), (0, 64, 64, 64, 3), (128, 0, 64, 64, 3), (128, 64, -1, 64, 3), (128, 64, 64, 0, 3),
                (1 << 20, 8, 8, 1 << 11, 3),          # B * L = 2^31 columns
                (1, 1 << 20, 8, 1 << 11, 3)):         # one sample of x holds 2^31 elements
        assert lib.tg_conv1d_supported(*bad) == 0 and lib.tg_conv1d_wgrad_workspace(*bad) == 0, bad
    for B, Cin, Cout, L, ks in ((3, 5, 7, 1, 3), (128, 64, 128, 64, 3), (7, 128, 128, 4, 1)):
        n = lib.tg_conv1d_wgrad_workspace(B, Cin, Cout, L, ks)
        assert n >= 4 * Cout * (Cin * ks + 1) and n % (4 * Cout * (Cin * ks + 1)) == 0        # whole partial blocks, bias column included


def test_skipgram_host_queries(lib):
    assert lib.tg_skipgram_workspace(128, 6, 64) == 4 * (128 + 2 * 128 * 6 + 2 * 128 * 64)
    assert lib.tg_skipgram_workspace(128, 6, 1025) == 0 and lib.tg_skipgram_workspace(1 << 15, 2, 8) == 0
    assert lib.tg_skipgram_workspace(0, 6, 64) == 0


P = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before a launch


def test_bad_arguments_return_codes(lib):
    assert lib.tg_conv1d_fwd(None, P, None, None, P, 2, 3, 4, 5, 3, None) == TG_EINVAL
    assert lib.tg_conv1d_fwd(P, P, None, None, None, 2, 3, 4, 5, 3, None) == TG_EINVAL
    assert lib.tg_conv1d_fwd(P, P, None, None, P, 0, 3, 4, 5, 3, None) == TG_EINVAL
    assert lib.tg_conv1d_fwd(P, P, None, None, P, 2, 3, 4, 5, 5, None) == TG_EUNSUPPORTED
    assert lib.tg_conv1d_dgrad(P, None, P, 2, 3, 4, 5, 3, None) == TG_EINVAL
    assert lib.tg_conv1d_dgrad(P, P, P, 2, 3, 4, 5, 7, None) == TG_EUNSUPPORTED
    assert lib.tg_conv1d_wgrad(P, P, None, None, P, 1 << 20, 2, 3, 4, 5, 3, 0, None) == TG_EINVAL
    assert lib.tg_conv1d_wgrad(P, P, P, None, P, 1 << 20, 2, 3, 4, 5, 4, 0, None) == TG_EUNSUPPORTED
    need = lib.tg_conv1d_wgrad_workspace(2, 3, 4, 5, 3)
    assert lib.tg_conv1d_wgrad(P, P, P, P, P, need - 1, 2, 3, 4, 5, 3, 0, None) == TG_EWORKSPACE
    assert lib.tg_up2x1d(None, P, 1.0, 2, 3, None) == TG_EINVAL and lib.tg_up2x1d(P, P, 1.0, 2, 0, None) == TG_EINVAL
    assert lib.tg_pool2_1d(P, None, None, 2, 3, None) == TG_EINVAL and lib.tg_pool2_1d(P, None, P, -1, 3, None) == TG_EINVAL
    need = lib.tg_skipgram_workspace(4, 6, 8)
    assert lib.tg_skipgram_step(None, P, P, P, P, 0.1, -1, P, P, need, 4, 6, 8, 23, None) == TG_EINVAL
    assert lib.tg_skipgram_step(P, P, P, P, P, 0.1, -1, P, P, need, 4, 6, 8, 23, None) == TG_EINVAL            # one table given twice
    Q = ctypes.c_void_p(512)
    assert lib.tg_skipgram_step(P, Q, P, P, P, 0.1, -1, P, P, need, 4, 6, 8, 0, None) == TG_EINVAL
    assert lib.tg_skipgram_step(P, Q, P, P, P, 0.1, -1, P, P, need, 4, 6, 1025, 23, None) == TG_EUNSUPPORTED
    assert lib.tg_skipgram_step(P, Q, P, P, P, 0.1, -1, P, P, need - 4, 4, 6, 8, 23, None) == TG_EWORKSPACE
    assert lib.tg_embed_gather_t(P, None, P, 2, 3, 4, 5, None) == TG_EINVAL and lib.tg_embed_gather_t(P, P, P, 2, 3, 4, 0, None) == TG_EINVAL
    assert lib.tg_embed_lookup(P, P, None, 2, 3, 4, 5, None) == TG_EINVAL and lib.tg_embed_lookup(P, P, P, 2, 3, 4, 1, None) == TG_EINVAL
    assert lib.tg_embed_lookup(P, P, P, 2, 3, 1025, 5, None) == TG_EUNSUPPORTED
