"""Helpers of the folder-dataset and epoch-loop tests (not collected).

* ``DatasetEmulator``: ``tests/emulator.Emulator`` plus ``tg_resample_u8`` in integer torch from the header's formula: the taps as a
  dense (out, in) int64 matrix, the sum exact in int64 and then wrapped to 32 bits, an arithmetic shift, the clip.
* ``SHAPES``: the resize cases (H, W, C, S) of the issue; ``image`` / ``pil`` their inputs and Pillow's answer.
* ``write_folder``: a PNG folder with mixed sizes, a grayscale file, a nested directory, a ``.txt`` and an upper-case ``.PNG``.
"""
import os

import numpy as np
import torch

from emulator import Emulator

# H, W, C, S: both ways down, both ways up, down / up, one pass (W == S), one pass (H == S), copy, tiny, one pixel, one channel
SHAPES = ((37, 53, 3, 16), (9, 11, 3, 16), (64, 17, 3, 16), (17, 64, 3, 16), (33, 16, 3, 16), (16, 33, 3, 16), (16, 16, 3, 16), (5, 7, 3, 4), (1, 1, 3, 4),
          (37, 53, 1, 16))
SLIVER = (1000, 3, 3, 16)             # H > 100 W and the height shrinks: Pillow runs the vertical pass first


def _kernel_error(code):
    from tartangan_amd import backend
    return backend.KernelError(f'tg_resample_u8 failed with code {code}')


def _dense(k, bounds, n_in, ks):
    """(out, ks) taps + (out, 2) bounds -> (out, in) int64 matrix."""
    n_out = bounds.shape[0]
    dense = torch.zeros(n_out, n_in, dtype=torch.int64)
    k = k.view(n_out, ks).to(torch.int64)
    tap = torch.arange(ks)[None, :]
    used = tap < bounds[:, 1:2]
    rows = torch.arange(n_out)[:, None].expand(n_out, ks)
    dense[rows[used], (bounds[:, 0:1] + tap)[used]] = k[used]
    return dense


def _finish(acc):
    acc = acc + (1 << 21)
    acc = ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)          # what 32-bit wrap-around leaves, read as int32
    return (acc >> 22).clamp_(0, 255).to(torch.uint8)


class DatasetEmulator(Emulator):
    def resample_u8(self, src, dst, tmp, kx, bx, ky, by, N, H, W, C, OH, OW, ksx, ksy):
        if src is None or dst is None or min(N, H, W, OH, OW) < 1:
            raise _kernel_error(-1)
        if C not in (1, 3):
            raise _kernel_error(-2)
        if (kx is None and ky is None) or (kx is not None and tmp is None and ky is not None):
            raise _kernel_error(-1)
        for k, b, ks, n_in, n_out in ((kx, bx, ksx, W, OW), (ky, by, ksy, H, OH)):
            if k is None:
                if n_in != n_out:
                    raise _kernel_error(-1)
                continue
            b = None if b is None else b.view(n_out, 2)
            if b is None or ks < 1 or bool(((b[:, 0] < 0) | (b[:, 1] < 0) | (b[:, 1] > ks) | (b[:, 0] + b[:, 1] > n_in)).any()):
                raise _kernel_error(-1)
        x = src.view(N, H, W, C).to(torch.int64)
        if kx is not None:
            x = _finish(torch.einsum('ow,nhwc->nhoc', _dense(kx, bx.view(OW, 2), W, ksx), x))
            if ky is not None:
                tmp.view(N, H, OW, C).copy_(x)
            x = x.to(torch.int64)
        if ky is not None:
            x = _finish(torch.einsum('oh,nhwc->nowc', _dense(ky, by.view(OH, 2), H, ksy), x))
        dst.view(N, OH, OW, C).copy_(x)
        return 0


def image(H, W, C, kind='noise', seed=0):
    """(H, W, C) uint8: uniform noise, or only 0 and 255 (the largest swings the negative lobes can see)."""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + C + seed)
    x = torch.randint(0, 256, (H, W, C), generator=g, dtype=torch.uint8)
    if kind == 'binary':
        x = (x > 127).to(torch.uint8) * 255
    return x.numpy()


def pil(img, size):
    """``Image.resize((size, size), Image.LANCZOS)`` of an (H, W, C) array, C = 1 as mode 'L'."""
    from PIL import Image
    C = img.shape[2]
    p = Image.fromarray(img[:, :, 0] if C == 1 else img)
    return np.asarray(p.resize((size, size), Image.LANCZOS)).reshape(size, size, C)


def resample_args(imgs, size):
    """The argument list of ``resample_u8`` for a (N, H, W, C) uint8 array and a target ``size`` (S, or (OH, OW)), CPU tensors
    (tmp is given whenever both passes run)."""
    from tartangan_amd.image_folder_dataset import pil_resample_coefficients
    N, H, W, C = imgs.shape
    OH, OW = (size, size) if isinstance(size, int) else size
    t = lambda a: torch.from_numpy(np.array(a))
    kx, bx = (t(a) for a in pil_resample_coefficients(W, OW)) if W != OW else (None, None)
    ky, by = (t(a) for a in pil_resample_coefficients(H, OH)) if H != OH else (None, None)
    tmp = torch.zeros(N, H, OW, C, dtype=torch.uint8) if kx is not None and ky is not None else None
    return [torch.from_numpy(imgs.copy()), torch.zeros(N, OH, OW, C, dtype=torch.uint8), tmp, kx, bx, ky, by, N, H, W, C, OH, OW,
            kx.shape[1] if kx is not None else 0, ky.shape[1] if ky is not None else 0]


# (N, H, W, C, OH, OW): where the kernels take another path than at the sizes above
PATH_SHAPES = (
    (2, 5, 700, 3, 5, 150),         # horizontal alone: three column tiles, the last one 22 wide; 10 rows in groups of 4
    (1, 3, 6000, 3, 3, 70),         # a tile's span is 18 KB: two rows staged per workgroup instead of four
    (1, 3, 12000, 3, 3, 70),        # 36 KB: one row per workgroup
    (1, 300000, 2, 1, 300000, 3),   # more row groups than a grid dimension holds: the workgroups loop
    (66000, 2, 4, 1, 3, 4),         # vertical alone, more images than a grid dimension holds
    (1, 2, 4, 1, 70000, 4),         # ... and more output rows
    (1, 9, 400, 3, 16, 400),        # vertical alone, 1200-byte rows: dword path, two workgroups along the row, the second partial
    (2, 9, 11, 3, 16, 5),           # 15-byte rows: never dword-aligned
)


# ------------------------------------------------------------------------------------------------------------------ folders
FOLDER_SIZES = ((16, 16), (20, 24), (16, 16), (31, 17), (16, 16), (20, 24), (8, 8), (40, 40))      # (H, W), cycled


def write_folder(root, n=24, extras=True, seed=0):
    """``n`` RGB PNGs at mixed sizes under ``root`` (every third one in a nested directory); with ``extras`` one of them is a
    grayscale file, and a ``notes.txt`` and an upper-case ``SHOUT.PNG`` (which the reference's case-sensitive match skips) are
    added -> root."""
    from PIL import Image
    root = str(root)
    os.makedirs(os.path.join(root, 'nested', 'deeper'), exist_ok=True)
    for i in range(n):
        H, W = FOLDER_SIZES[i % len(FOLDER_SIZES)]
        where = os.path.join(root, 'nested', 'deeper') if i % 3 == 2 else os.path.join(root, 'nested') if i % 3 == 1 else root
        arr = image(H, W, 3, seed=seed + i)
        im = Image.fromarray(arr[:, :, 0]) if (extras and i == 4) else Image.fromarray(arr)
        im.save(os.path.join(where, f'img_{i:03d}.png'), format='png')
    if extras:
        with open(os.path.join(root, 'notes.txt'), 'w') as f:
            f.write('not an image\n')
        Image.fromarray(image(16, 16, 3, seed=99)).save(os.path.join(root, 'SHOUT.PNG'), format='png')
    return root


def reference_file_list(root):
    """reference image_folder_dataset.py:40-49 restated: os.walk order, the extension looked up in torchvision's tuple as is."""
    exts = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')
    files = []
    for path, _, names in os.walk(root):
        files += [os.path.join(path, n) for n in names if os.path.splitext(n)[1] in exts]
    return files


def pil_archive(files, size):
    """Per file what the reference's transform makes of it before ToTensor: convert('RGB'), resize((size, size), LANCZOS)."""
    from PIL import Image
    out = []
    for f in files:
        with open(f, 'rb') as fh:
            out.append(np.asarray(Image.open(fh).convert('RGB').resize((size, size), Image.LANCZOS)))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------------------- the epoch loop
def loop_emulator():
    """One stand-in backend for every trainer's ``main()``: the family emulators joined (each adds its own entry points)."""
    from info_cases import InfoEmulator
    from scene_cases import SceneEmulator
    from shared_iqn_cases import SharedIQNEmulator
    from text_cases import TextEmulator

    class LoopEmulator(DatasetEmulator, InfoEmulator, SceneEmulator, SharedIQNEmulator, TextEmulator):
        pass
    return LoopEmulator()


class Spy:
    """A component that records every event as (name, steps[, epoch], {log key: length}) and may interrupt at one batch end."""

    def __init__(self, interrupt_at=None):
        self.events, self.interrupt_at = [], interrupt_at

    def _record(self, name, *args):
        *head, logs = args
        self.events.append((name, *head, {k: len(v) for k, v in logs.items() if k in ('g_loss', 'd_loss', 'gp')}))

    def on_train_begin(self, steps, logs): self._record('train_begin', steps, logs)
    def on_train_end(self, steps, logs): self._record('train_end', steps, logs)
    def on_batch_begin(self, steps, logs): self._record('batch_begin', steps, logs)
    def on_epoch_begin(self, steps, epoch, logs): self._record('epoch_begin', steps, epoch, logs)
    def on_epoch_end(self, steps, epoch, logs): self._record('epoch_end', steps, epoch, logs)

    def on_batch_end(self, steps, logs):
        self._record('batch_end', steps, logs)
        if steps == self.interrupt_at:
            raise KeyboardInterrupt


def expected_events(per_epoch, epochs, first_step=0, first_epoch=1, keys=('g_loss', 'd_loss', 'gp')):
    """The reference's loop (trainer.py:87-115) written out as the events a component sees; the log lengths count from this run's
    start (``logs`` is made anew by every ``train()``)."""
    lens = lambda n: {k: n for k in keys} if n else {}
    ev, s = [('train_begin', first_step, {})], first_step
    for e in range(first_epoch, first_epoch + epochs):
        ev.append(('epoch_begin', s, e, lens(s - first_step)))
        for _ in range(per_epoch):
            ev.append(('batch_begin', s, lens(s - first_step)))
            ev.append(('batch_end', s, lens(s - first_step + 1)))
            s += 1
        ev.append(('epoch_end', s, e, lens(s - first_step)))
    ev.append(('train_end', s, lens(s - first_step)))
    return ev


def loop_argv(folder, out, run_id, *extra, epochs=2, cuda=False):
    return [str(folder), '--config', '16', '--batch-size', '8', '--epochs', str(epochs), '--output', str(out), '--run-id', run_id,
            '--quiet-logs', *([] if cuda else ['--no-cuda']), *extra]


def hand_driven(cls, argv, epochs, seed):
    """The loop by hand from ``seed``: models, the folder dataset, the stock sampler and checkpoint components' hooks around a
    plain ``for batch in loader: train_batch(batch)`` -> the list of ``train_batch`` results."""
    import argparse
    from tartangan_amd.image_folder_dataset import ImageFolderDataset
    from tartangan_amd.trainers.components import ImageSamplerComponent, ModelCheckpointComponent
    from tartangan_amd.trainers.utils import set_device_from_args
    p = argparse.ArgumentParser()
    cls.add_args_to_parser(p)
    cls.add_loop_args_to_parser(p)
    ModelCheckpointComponent.add_args_to_parser(p)
    args = p.parse_args(argv)
    set_device_from_args(args)
    torch.manual_seed(seed)
    np.random.seed(seed)
    tr = cls(args)
    comps = [ImageSamplerComponent(args), ModelCheckpointComponent(args)]
    tr.attach(*comps)
    tr.build_models()
    ds = ImageFolderDataset(args.data_path, tr.g.max_size, device=args.device)
    logs, results = {}, []
    for c in comps:
        c.on_train_begin(0, logs)
    for _ in range(epochs):
        for batch in ds.loader(args.batch_size):
            step = tr.steps
            results.append(tr.train_batch(batch))
            tr.steps = step                      # (train_batch counts its own calls; components see the loop's count)
            for c in comps:
                c.on_batch_end(step, logs)
            tr.steps = step + 1
    return results
