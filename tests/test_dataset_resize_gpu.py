"""tg_resample_u8 (csrc/dataset.hip) on the GPU, every call behind guard bands (guarded.run_both: the outputs and the intermediate
handed over filled), aligned and one element off, the smallest case with each pointer shifted alone, against the integer emulator
at tolerance 0 -- and against ``PIL.Image.resize(..., LANCZOS)`` itself for equality.

(This file sorts in front of test_guard_bands_gpu.py on purpose: that file's completeness test wants every entry point with a
pointer parameter to have gone through the guarded harness earlier in the same process.)"""
import numpy as np
import pytest
import torch

import dataset_cases as DC
from guarded import run_both
from tartangan_amd import backend

pytestmark = pytest.mark.gpu
EMU = DC.DatasetEmulator()
OUTS, SCRATCH = [1], [2]
RESIZED = [s for s in DC.SHAPES if (s[0], s[1]) != (s[3], s[3])]
SMALLEST = (1, 1, 3, 4)


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(None)
    yield backend.get()
    backend._set_backend_for_testing(prev)


def _run(K, args, placement, **kw):
    scratch = SCRATCH if args[2] is not None else []
    return run_both(K, 'resample_u8', args, OUTS, tol=0.0, scratch=scratch, placement=placement, emulator=EMU, **kw)


@pytest.mark.parametrize('kind', ('noise', 'binary'))
@pytest.mark.parametrize('shape', RESIZED, ids=lambda s: 'x'.join(map(str, s)))
def test_resample_equals_the_emulator_and_pillow(K, shape, kind):
    H, W, C, S = shape
    imgs = np.stack([DC.image(H, W, C, kind), DC.image(H, W, C, kind, seed=1), DC.image(H, W, C, kind, seed=2)])
    args = DC.resample_args(imgs, S)
    placements = ['aligned', 'shifted']
    if shape == SMALLEST:
        placements += [i for i, a in enumerate(args) if torch.is_tensor(a)]          # each pointer shifted alone
        assert placements[2:] == [0, 1, 2, 3, 4, 5, 6]
    for pl in placements:
        dev = _run(K, args, pl)
        got = dev[1].cpu().numpy()
        for n in range(3):
            assert np.array_equal(got[n], DC.pil(imgs[n], S)), (pl, n)


@pytest.mark.parametrize('shape', DC.PATH_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_resample_paths(K, shape):
    N, H, W, C, OH, OW = shape
    g = torch.Generator().manual_seed(H + W)
    imgs = torch.randint(0, 256, (N, H, W, C), generator=g, dtype=torch.uint8).numpy()
    _run(K, DC.resample_args(imgs, (OH, OW)), ['aligned', 'shifted'])


def test_one_pass_needs_no_intermediate(K):
    img = DC.image(33, 16, 3)[None]
    args = DC.resample_args(img, 16)
    assert args[2] is None and args[3] is None and args[5] is not None
    dev = _run(K, args, ['aligned', 'shifted'])
    assert np.array_equal(dev[1].cpu().numpy()[0], DC.pil(img[0], 16))


def test_documented_rejections_write_nothing(K):
    img = DC.image(9, 11, 3)[None]
    ok = DC.resample_args(img, 16)

    def rejected(**change):
        names = ('src', 'dst', 'tmp', 'kx', 'bx', 'ky', 'by', 'N', 'H', 'W', 'C', 'OH', 'OW', 'ksx', 'ksy')
        a = dict(zip(names, ok), **change)
        args = [a[n] for n in names]
        run_both(K, 'resample_u8', args, OUTS, tol=0.0, scratch=SCRATCH if args[2] is not None else [], placement=['aligned', 'shifted'],
                 expect='rejected', emulator=EMU)
        with pytest.raises(backend.KernelError):             # the emulator documents the same refusals
            EMU.resample_u8(*[t.clone() if torch.is_tensor(t) else t for t in args])

    def bounds(which, row, first=None, count=None):
        b = ok[which].clone()
        if first is not None:
            b[row, 0] = first
        if count is not None:
            b[row, 1] = count
        return b
    rejected(bx=bounds(4, 3, count=ok[13] + 1))              # count > ks
    rejected(by=bounds(6, 15, count=ok[14] + 1))
    rejected(bx=bounds(4, 15, first=9))                      # first + count past the input
    rejected(by=bounds(6, 0, first=-1))
    rejected(bx=bounds(4, 0, count=-2))
    rejected(tmp=None)                                       # both passes need the intermediate
    rejected(kx=None, bx=None)                               # no horizontal pass although W != OW
    rejected(ky=None, by=None)
    rejected(kx=None, bx=None, ky=None, by=None, tmp=None, H=16, W=16)          # nothing to do: the host copies
    rejected(bx=None)
    rejected(N=0)
    rejected(OW=0)
    rejected(C=2)
    rejected(ksx=0)


def test_device_resize_and_folder_archive_equal_pillow(K, tmp_path):
    from tartangan_amd import image_folder_dataset as IF
    shapes = [(20, 24), (16, 16), (20, 24), (31, 17), (1000, 3), (20, 24), (40, 16)]
    imgs = [DC.image(h, w, 3, seed=i) for i, (h, w) in enumerate(shapes)]
    got = IF.device_resize(imgs, 16).cpu().numpy()
    for i, img in enumerate(imgs):
        assert np.array_equal(got[i], DC.pil(img, 16)), i
    folder = DC.write_folder(tmp_path / 'data', n=12, extras=True)
    ds = IF.ImageFolderDataset(folder, 16)
    assert ds.images.is_cuda and np.array_equal(ds.images.cpu().numpy(), DC.pil_archive(DC.reference_file_list(folder), 16))
    u8 = ds.images[[5, 2]].cpu().permute(0, 3, 1, 2).float()          # (on the CPU: ATen's GPU division by a scalar multiplies by 1/255)
    assert torch.equal(ds.batch([5, 2]).cpu(), ((u8 / 255) - .5) / .5)
