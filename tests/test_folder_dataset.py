"""The folder dataset without a GPU: Pillow's taps restated on the host, the resampler's arithmetic (over the emulator), the folder
walk, the cache, and the new entry point's return codes on the compiled library."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dataset_cases as DC
from tartangan_amd import backend
from tartangan_amd import image_folder_dataset as IF
from tartangan_amd.image_bytes_dataset import ImageBytesDataset

TG_EINVAL, TG_EUNSUPPORTED = -1, -2


@pytest.fixture(autouse=True)
def emulated():
    prev = backend._set_backend_for_testing(DC.DatasetEmulator())
    yield
    backend._set_backend_for_testing(prev)


# ------------------------------------------------------------------------------------------------ coefficients + arithmetic
def test_coefficients_have_pillows_layout():
    k, b = IF.pil_resample_coefficients(53, 16)
    scale = 53 / 16
    assert k.dtype == np.int32 and b.dtype == np.int32
    assert k.shape == (16, int(np.ceil(3 * scale)) * 2 + 1) and b.shape == (16, 2)
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= 53).all() and (b[:, 1] <= k.shape[1]).all()
    for o in range(16):                                   # normalised rows: the taps sum to 2^22 up to their own rounding
        assert abs(int(k[o, :b[o, 1]].sum()) - (1 << 22)) <= b[o, 1] and not k[o, b[o, 1]:].any()
    assert IF.pil_resample_coefficients(53, 16)[0] is k   # cached per (in, out)
    up_k, up_b = IF.pil_resample_coefficients(9, 16)      # up-scaling: support 3, seven taps
    assert up_k.shape == (16, 7)
    # worst-case accumulator: 255 * (sum of the positive taps) + 2^21 stays below 2^31 for every size the tests use
    for n_in, n_out in ((53, 16), (9, 16), (1, 4), (1000, 16), (4000, 64)):
        kk = IF.pil_resample_coefficients(n_in, n_out)[0].astype(np.int64)
        assert 255 * int(np.where(kk > 0, kk, 0).sum(axis=1).max()) + (1 << 21) < (1 << 31)


@pytest.mark.parametrize('kind', ('noise', 'binary'))
@pytest.mark.parametrize('shape', DC.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_coefficients_and_emulator_equal_pillow_exactly(shape, kind):
    H, W, C, S = shape
    img = DC.image(H, W, C, kind)
    want = DC.pil(img, S)
    if (H, W) == (S, S):
        with pytest.raises(backend.KernelError):          # no pass at all: the host copies
            DC.DatasetEmulator().resample_u8(*DC.resample_args(img[None], S))
    else:
        args = DC.resample_args(np.stack([img, img[::-1].copy()]), S)
        DC.DatasetEmulator().resample_u8(*args)
        assert np.array_equal(args[1][0].numpy(), want)
        assert np.array_equal(args[1][1].numpy(), DC.pil(img[::-1].copy(), S))
    got = IF.device_resize([img], S, device='cpu')
    assert got.dtype == torch.uint8 and np.array_equal(got[0].numpy(), want)


def test_sliver_takes_the_host_path_and_equals_pillow():
    H, W, C, S = DC.SLIVER
    img = DC.image(H, W, C)
    assert IF._on_host((H, W, C), S) and not IF._on_host((W, H, C), S) and not IF._on_host((H, 10, C), S)

    class NoKernel(DC.DatasetEmulator):
        def resample_u8(self, *a):
            raise AssertionError('a sliver went to the kernel')
    backend._set_backend_for_testing(NoKernel())
    want = DC.pil(img, S)
    assert np.array_equal(IF.device_resize([img], S, device='cpu')[0].numpy(), want)
    # and the quirk is real: horizontal-first does not give Pillow's bytes here
    args = DC.resample_args(img[None], S)
    DC.DatasetEmulator().resample_u8(*args)
    assert not np.array_equal(args[1][0].numpy(), want)


def test_device_resize_groups_shapes_and_keeps_order():
    shapes = [(20, 24), (16, 16), (20, 24), (31, 17), (20, 24), (20, 24), (16, 16), (40, 16)]
    imgs = [DC.image(h, w, 3, seed=i) for i, (h, w) in enumerate(shapes)]
    calls = []

    class Counting(DC.DatasetEmulator):
        def resample_u8(self, src, dst, tmp, kx, bx, ky, by, N, H, W, *rest):
            calls.append((N, H, W, tmp is not None))
            return super().resample_u8(src, dst, tmp, kx, bx, ky, by, N, H, W, *rest)
    backend._set_backend_for_testing(Counting())
    got = IF.device_resize(imgs, 16, device='cpu')
    assert sorted(calls) == [(1, 31, 17, True), (1, 40, 16, False), (4, 20, 24, True)]            # one launch per shape, none for 16 x 16
    for i, img in enumerate(imgs):
        assert np.array_equal(got[i].numpy(), DC.pil(img, 16)), i
    with pytest.raises(ValueError):
        IF.device_resize([], 16, device='cpu')
    with pytest.raises(ValueError):
        IF.device_resize([imgs[0], DC.image(8, 8, 1)], 16, device='cpu')


# -------------------------------------------------------------------------------------------------------------- the folder
@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    return DC.write_folder(tmp_path_factory.mktemp('folder'), n=12, extras=True)


def test_folder_order_count_archive_and_batches(folder, capsys):
    with open(os.path.join(folder, 'broken.png'), 'wb') as f:
        f.write(b'not a png at all')
    try:
        ds = IF.ImageFolderDataset(folder, 16, device='cpu')
    finally:
        os.remove(os.path.join(folder, 'broken.png'))
    out = capsys.readouterr().out
    assert 'Skipping' in out and 'broken.png' in out                      # an unreadable file is reported and skipped
    files = DC.reference_file_list(folder)
    assert ds.image_filenames == files and len(ds) == 12                  # .txt and .PNG are not taken, the grayscale file is
    assert not any(f.endswith(('notes.txt', 'SHOUT.PNG')) for f in files) and any('deeper' in f for f in files)
    assert ds.images.shape == (12, 16, 16, 3) and ds.images.dtype == torch.uint8 and ds.image_size == 16
    assert np.array_equal(ds.images.numpy(), DC.pil_archive(files, 16))
    u8 = ds.images[[3, 0, 7]].permute(0, 3, 1, 2).float()
    assert torch.equal(ds.batch([3, 0, 7]), ((u8 / 255) - .5) / .5)
    # no crop offsets are drawn: an epoch consumes the generator exactly like a DataLoader over fixed-size items
    torch.manual_seed(3)
    batches = list(ds.loader(4))
    after = torch.rand(1)
    torch.manual_seed(3)
    torch.empty((), dtype=torch.int64).random_()
    order = torch.randperm(12, generator=torch.Generator().manual_seed(int(torch.empty((), dtype=torch.int64).random_().item())))
    assert torch.equal(torch.rand(1), after) and len(batches) == 3
    assert torch.equal(batches[1], ds.batch(order[4:8]))
    halves = [torch.cat([b for b in IF.ImageFolderDataset.loader(ds, 2, rank=r, world=2)]) for r in (0, 1)]       # sharding, inherited
    assert halves[0].shape == (6, 3, 16, 16)


def test_cache_round_trip_and_loads_as_image_bytes(folder, tmp_path):
    ds = IF.ImageFolderDataset(folder, 16, device='cpu')
    path = str(tmp_path / 'cache' / 'abc_16.pkl')
    ds.save_cache(path)
    assert os.path.exists(path)                                           # under exactly the name asked for
    with np.load(path) as z:
        assert sorted(z.files) == ['filenames', 'images'] and [str(s) for s in z['filenames']] == ds.image_filenames

    class NoKernel(DC.DatasetEmulator):
        def resample_u8(self, *a):
            raise AssertionError('the cache was not used')
    backend._set_backend_for_testing(NoKernel())
    again = IF.ImageFolderDataset(folder, 16, device='cpu', cache_path=path)
    assert torch.equal(again.images, ds.images) and again.image_filenames == ds.image_filenames
    plain = ImageBytesDataset.from_path(path, crop_size=16, device='cpu')
    assert torch.equal(plain.images, ds.images) and torch.equal(plain.batch([1, 2]), ds.batch([1, 2]))
    backend._set_backend_for_testing(DC.DatasetEmulator())
    other = IF.ImageFolderDataset(folder, 8, device='cpu', cache_path=path)      # a cache for another size is not taken
    assert other.images.shape == (12, 8, 8, 3)
    assert IF.ImageFolderDataset(folder, 16, device='cpu', cache_path=str(tmp_path / 'missing.pkl')).images.shape == (12, 16, 16, 3)


def test_an_empty_folder_is_an_error(tmp_path):
    (tmp_path / 'notes.txt').write_text('nothing here')
    with pytest.raises(ValueError, match='no readable image'):
        IF.ImageFolderDataset(str(tmp_path), 16, device='cpu')


# -------------------------------------------------------------------------------------------------- the compiled entry point
@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(backend.LIBRARY):
        pytest.fail(f'{backend.LIBRARY} is missing: build it first (python __graft_entry__.py build)')
    handle = ctypes.CDLL(backend.LIBRARY)
    ret, params = backend.parse_header()['tg_resample_u8']
    handle.tg_resample_u8.restype = backend._CTYPES[ret]
    handle.tg_resample_u8.argtypes = [backend._CTYPES[t] for t, _ in params]
    return handle


P = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before the bounds are fetched or a kernel launched


def test_return_codes_of_the_new_entry_point(lib):
    lib.tg_version.restype = ctypes.c_int
    assert lib.tg_version() >= 110
    call = lib.tg_resample_u8
    ok = dict(src=P, dst=P, tmp=P, kx=P, bx=P, ky=P, by=P, N=2, H=9, W=11, C=3, OH=16, OW=16, ksx=7, ksy=7)

    def rc(**change):
        a = dict(ok, **change)
        return call(*[a[k] for k in ok], None)
    assert rc(src=None) == TG_EINVAL and rc(dst=None) == TG_EINVAL
    for dim in ('N', 'H', 'W', 'OH', 'OW'):
        assert rc(**{dim: 0}) == TG_EINVAL and rc(**{dim: -3}) == TG_EINVAL
    assert rc(C=2) == TG_EUNSUPPORTED and rc(C=4) == TG_EUNSUPPORTED and rc(C=0) == TG_EUNSUPPORTED
    assert rc(kx=None, ky=None, H=16, W=16) == TG_EINVAL                   # both passes missing: the host copies
    assert rc(tmp=None) == TG_EINVAL                                       # both passes need the intermediate
    assert rc(bx=None) == TG_EINVAL and rc(by=None) == TG_EINVAL
    assert rc(ksx=0) == TG_EINVAL and rc(ksy=0) == TG_EINVAL
    assert rc(kx=None, bx=None) == TG_EINVAL                               # no horizontal pass but W != OW
    assert rc(ky=None, by=None) == TG_EINVAL                               # no vertical pass but H != OH
