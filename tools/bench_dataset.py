"""Time the building of a folder dataset: Pillow on the host against upload + tg_resample_u8 on the GPU, and the whole first epoch's
data path with the decode named separately.

    python tools/bench_dataset.py [--iters 20] [--warmup 3] [--files 256] [--out profiles/dataset_build]

Per case (256 x 256 -> 64, 1024 x 1024 -> 128, 1500 wide x 1000 high -> 128; RGB noise, a batch of same-shaped images), per image:

  pil      ``Image.resize((S, S), LANCZOS)`` on the host, one image at a time (one thread), a host clock
  upload   pageable host array -> the device staging buffer, as ``device_resize`` does it, a host clock around copy + synchronise
  h, v     the horizontal and the vertical pass, each as its own ``tg_resample_u8`` call (W -> S at height H; H -> S at width S),
           a host clock around call + synchronise: the call fetches and checks its bounds first, so this is the time of the call,
           not of the kernel alone
  both     one call with both passes

and for each pass the bytes it has to move (source read once + result written once) over its time, against the 8 TB/s HBM peak --
a whole-call rate, named as such.  The first image's result is compared with Pillow's for equality.

The folder: ``--files`` PNGs of 256 x 256 noise written to a temporary directory; decode alone (``Image.open(f).convert('RGB')``),
decode + Pillow resize (the reference's host path up to ToTensor) and ``ImageFolderDataset`` (decode + upload + device resize), each
as images per second of wall time.  Noise compresses badly, so the decode here is on the expensive side for its size.
No GPU, no measurement: the tool fails without one."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]

HBM_PEAK = 8.0e12
CASES = (('256x256->64', 256, 256, 64, 128), ('1024x1024->128', 1024, 1024, 128, 16), ('1500x1000->128', 1000, 1500, 128, 16))      # name, H, W, S, images


def host_ms(fn, sync=True):
    t = time.perf_counter()
    fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def median_of(fn, iters, warmup, sync=True):
    for _ in range(warmup):
        host_ms(fn, sync)
    t = [host_ms(fn, sync) for _ in range(iters)]
    return dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))


def bench_case(name, H, W, S, n, iters, warmup):
    from PIL import Image
    from tartangan_amd import backend
    from tartangan_amd.image_folder_dataset import pil_resample_coefficients
    K = backend.get()
    rng = np.random.default_rng(H + W)
    imgs = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    pils = [Image.fromarray(im) for im in imgs]
    want = np.asarray(pils[0].resize((S, S), Image.LANCZOS))
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()       # noqa: E731
    kx, bx = map(dev, pil_resample_coefficients(W, S))
    ky, by = map(dev, pil_resample_coefficients(H, S))
    ksx, ksy = kx.shape[1], ky.shape[1]
    src = torch.empty(n, H, W, 3, dtype=torch.uint8, device='cuda')
    tmp = torch.empty(n, H, S, 3, dtype=torch.uint8, device='cuda')
    dst = torch.empty(n, S, S, 3, dtype=torch.uint8, device='cuda')
    host = torch.from_numpy(imgs)
    row = dict(case=name, images=n, H=H, W=W, S=S, iters=iters)
    row['pil'] = median_of(lambda: [p.resize((S, S), Image.LANCZOS) for p in pils], max(3, iters // 4), 1, sync=False)
    row['upload'] = median_of(lambda: src.copy_(host), iters, warmup)
    row['h'] = median_of(lambda: K.resample_u8(src, tmp, None, kx, bx, None, None, n, H, W, 3, H, S, ksx, 0), iters, warmup)
    row['v'] = median_of(lambda: K.resample_u8(tmp, dst, None, None, None, ky, by, n, H, S, 3, S, S, 0, ksy), iters, warmup)
    row['both'] = median_of(lambda: K.resample_u8(src, dst, tmp, kx, bx, ky, by, n, H, W, 3, S, S, ksx, ksy), iters, warmup)
    row['equals_pil'] = bool(np.array_equal(dst[0].cpu().numpy(), want))
    row['bytes'] = dict(h=n * H * (W + S) * 3, v=n * (H + S) * S * 3)
    for p in ('h', 'v'):
        rate = row['bytes'][p] / (row[p]['median_ms'] * 1e-3)
        row[p].update(bytes_per_s=rate, share_of_hbm_peak=rate / HBM_PEAK)
    per = lambda k: row[k]['median_ms'] / n       # noqa: E731
    lines = [f'{name}: {n} images per batch, per image: pil {per("pil"):.4f} ms | upload {per("upload"):.4f} ms, h {per("h"):.4f} ms, '
             f'v {per("v"):.4f} ms, both passes in one call {per("both"):.4f} ms | equals PIL: {row["equals_pil"]}',
             f'    whole-call rate: h {row["h"]["bytes_per_s"] / 1e9:.1f} GB/s ({100 * row["h"]["share_of_hbm_peak"]:.2f} % of the 8 TB/s peak), '
             f'v {row["v"]["bytes_per_s"] / 1e9:.1f} GB/s ({100 * row["v"]["share_of_hbm_peak"]:.2f} %); '
             f'pil / (upload + both) = {per("pil") / (per("upload") + per("both")):.1f}']
    return row, lines


def bench_folder(files, repeats):
    from PIL import Image
    from tartangan_amd.image_folder_dataset import ImageFolderDataset, list_image_files
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as root:
        for i in range(files):
            Image.fromarray(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)).save(os.path.join(root, f'{i:05d}.png'))
        names = list_image_files(root)

        def decode():
            out = []
            for f in names:
                with open(f, 'rb') as fh:
                    out.append(np.asarray(Image.open(fh).convert('RGB')))
            return out

        def host_path():
            for f in names:
                with open(f, 'rb') as fh:
                    Image.open(fh).convert('RGB').resize((64, 64), Image.LANCZOS)

        row = dict(files=files, size='256x256->64')
        row['decode'] = median_of(decode, repeats, 1, sync=False)
        row['decode_and_pil_resize'] = median_of(host_path, repeats, 1, sync=False)
        row['image_folder_dataset'] = median_of(lambda: ImageFolderDataset(root, 64), repeats, 1)
    rate = lambda k: files / (row[k]['median_ms'] * 1e-3)       # noqa: E731
    lines = [f'folder of {files} PNGs (256 x 256 noise) -> 64: decode alone {rate("decode"):.0f} img/s; decode + PIL resize (host path) '
             f'{rate("decode_and_pil_resize"):.0f} img/s; ImageFolderDataset (decode + upload + device resize) {rate("image_folder_dataset"):.0f} img/s']
    return row, lines


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--files', type=int, default=256)
    p.add_argument('--out', default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), 'bench_dataset needs the GPU (no CPU timing)'
    torch.set_num_threads(1)
    rows, lines = [], []
    for case in CASES:
        row, text = bench_case(*case, args.iters, args.warmup)
        rows.append(row)
        lines += text
    folder, text = bench_folder(args.files, max(3, args.iters // 4))
    lines += text
    print('\n'.join(lines))
    if args.out:
        with open(args.out + '.json', 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'cases': rows, 'folder': folder}, f, indent=1)
        with open(args.out + '.txt', 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
