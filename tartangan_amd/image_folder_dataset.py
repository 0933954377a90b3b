"""A folder of image files as a device-resident training archive (reference image_folder_dataset.py:10-49 with the transform the
trainer puts on it, ``Resize((S, S), LANCZOS) -> ToTensor -> Normalize(.5, .5)``, trainers/trainer.py:55-66).

The reference resizes one image at a time through PIL on the host and keeps the resulting float tensors in a dict.  Here the files
are decoded on the host (unavoidable), same-shaped images are uploaded together and resized on the device by ``tg_resample_u8``
into the uint8 (N, S, S, 3) archive an ``ImageBytesDataset`` trains from; ``tg_image_bytes_batch`` then does ToTensor + Normalize
per batch.  Pillow's 8-bit resampler is integer arithmetic on fixed-point taps (Resample.c), so the archive is bit-identical to
``Image.resize((S, S), Image.LANCZOS)`` per file: ``pil_resample_coefficients`` restates Pillow's tap computation in float64.
"""
import functools
import math
import os

import numpy as np
import torch

from . import backend as _be
from .image_bytes_dataset import ImageBytesDataset

# torchvision.datasets.folder.IMG_EXTENSIONS; matched case-sensitively, as the reference does (image_folder_dataset.py:43-45)
IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')
PRECISION_BITS = 32 - 8 - 2
ROW_SPAN_LIMIT = 64 * 1024 - 8        # bytes of one image row the horizontal pass can stage (tg_resample_u8: TG_EUNSUPPORTED above)
CHUNK_BYTES = 64 << 20                # source bytes uploaded and resized per launch


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_FILTERS = {'lanczos': (_lanczos, 3.0)}


@functools.lru_cache(maxsize=None)
def pil_resample_coefficients(in_size, out_size, filter='lanczos'):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` -> (k int32 (out, ks), bounds int32 (out, 2) = (first, count)).
    float64 throughout, through Python's ``math``; the weights of a row are summed in order and divided by the sum."""
    fn, filter_support = _FILTERS[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = filter_support * fs
    ks = int(math.ceil(support)) * 2 + 1
    k = np.zeros((out_size, ks), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        total = 0.0
        for v in w:
            total += v
        for x, v in enumerate(w):
            if total != 0.0:
                v = v / total
            k[xx, x] = int((-0.5 if v < 0 else 0.5) + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    k.setflags(write=False)
    bounds.setflags(write=False)
    return k, bounds


def _on_host(shape, size):
    """Does PIL resize this shape on the host?  Pillow runs the VERTICAL pass first when H > 100 W and the height shrinks (the
    intermediate is clipped to uint8 either way, so the order shows in the bytes); the kernel is horizontal-first only.  A row
    wider than the horizontal pass can stage goes the same way."""
    H, W, C = shape
    return (H > 100 * W and size < H) or W * C > ROW_SPAN_LIMIT or C not in (1, 3)


def pil_resize(image, size):
    from PIL import Image
    image = np.ascontiguousarray(image)
    pil = Image.fromarray(image[:, :, 0] if image.shape[2] == 1 else image)
    out = np.asarray(pil.resize((size, size), Image.LANCZOS))
    return out.reshape(size, size, image.shape[2])


class _Buffers:
    """One staging buffer and one intermediate for a whole ``device_resize``; they only ever grow."""

    def __init__(self, device):
        self.device = device
        self.staging = self.tmp = None
        self._coef = {}

    def take(self, name, nbytes):
        buf = getattr(self, name)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            setattr(self, name, buf)
        return buf[:nbytes]

    def coefficients(self, in_size, out_size):
        key = (in_size, out_size)
        if key not in self._coef:
            k, b = pil_resample_coefficients(in_size, out_size)
            self._coef[key] = (torch.from_numpy(k.copy()).to(self.device), torch.from_numpy(b.copy()).to(self.device), k.shape[1])
        return self._coef[key]


def device_resize(images_u8, size, device='cuda'):
    """images_u8: a sequence of (H, W, C) uint8 arrays with one C -> the (N, size, size, C) uint8 archive on ``device``, every image
    what ``Image.resize((size, size), Image.LANCZOS)`` gives.  Same-shaped images share launches (``CHUNK_BYTES`` of source at a
    time); a run of consecutive images is written straight into its slice of the archive.  Images that already have the size are
    copied; slivers (see ``_on_host``) are resized by PIL on the host."""
    n = len(images_u8)
    if n == 0:
        raise ValueError('no images to resize')
    C = images_u8[0].shape[2]
    if any(im.ndim != 3 or im.shape[2] != C or im.dtype != np.uint8 for im in images_u8):
        raise ValueError('images must be uint8 (H, W, C) arrays with the same number of channels')
    out = torch.empty(n, size, size, C, dtype=torch.uint8, device=device)
    groups = {}
    for i, im in enumerate(images_u8):
        groups.setdefault(im.shape, []).append(i)
    bufs = _Buffers(device)
    K = _be.get()
    for (H, W, _), members in groups.items():
        per_image = H * W * C
        host = (H, W) == (size, size) or _on_host((H, W, C), size)
        step = max(1, CHUNK_BYTES // per_image)
        for at in range(0, len(members), step):
            idx = members[at:at + step]
            m = len(idx)
            if host:
                block = np.stack([images_u8[i] if (H, W) == (size, size) else pil_resize(images_u8[i], size) for i in idx])
                result = torch.from_numpy(np.ascontiguousarray(block)).to(device)
            else:
                src = bufs.take('staging', m * per_image).view(m, H, W, C)
                src.copy_(torch.from_numpy(np.stack([images_u8[i] for i in idx])))
                consecutive = idx[-1] - idx[0] + 1 == m
                result = out[idx[0]:idx[0] + m] if consecutive else torch.empty(m, size, size, C, dtype=torch.uint8, device=device)
                kx, bx, ksx = bufs.coefficients(W, size) if W != size else (None, None, 0)
                ky, by, ksy = bufs.coefficients(H, size) if H != size else (None, None, 0)
                tmp = bufs.take('tmp', m * H * size * C) if (kx is not None and ky is not None) else None
                K.resample_u8(src, result, tmp, kx, bx, ky, by, m, H, W, C, size, size, ksx, ksy)
                if consecutive:
                    continue
            out[torch.as_tensor(idx, device=device)] = result
    return out


def list_image_files(root, extensions=IMG_EXTENSIONS):
    """``os.walk`` order, per directory the files whose extension is in ``extensions`` exactly (image_folder_dataset.py:40-49)."""
    found = []
    for path, _, files in os.walk(root):
        found.extend(os.path.join(path, name) for name in files if os.path.splitext(name)[1] in extensions)
    return found


class ImageFolderDataset(ImageBytesDataset):
    """Just batches of some images from a folder: every file squashed to ``size`` x ``size`` RGB.  The stored size is the crop
    size, so no crop offsets are drawn -- the folder path of the reference has no RandomCrop.  ``batch()``, ``loader()`` and
    sharding by rank are ``ImageBytesDataset``'s."""

    def __init__(self, root, size, device='cuda', cache_path=None):
        self.root = os.path.expanduser(root)
        self.size = size
        self.device = device
        self.crop_size = size
        self.image_filenames = list_image_files(self.root)
        if not (cache_path and self.load_cache(cache_path)):
            self._build()

    def _build(self):
        from PIL import Image
        decoded, kept = [], []
        for filename in self.image_filenames:
            try:
                with open(filename, 'rb') as f:                      # torchvision's pil_loader
                    decoded.append(np.asarray(Image.open(f).convert('RGB')))
                kept.append(filename)
            except Exception as e:                                   # an unreadable file is reported and skipped
                print(f'Skipping {filename}: {e}')
        if not decoded:
            raise ValueError(f'no readable image files under {self.root}')
        self.image_filenames = kept
        self.images = device_resize(decoded, self.size, self.device)

    def save_cache(self, filename):
        """``np.savez_compressed(images=, filenames=)`` under exactly this name: also a valid ``ImageBytesDataset.from_path``."""
        if os.path.dirname(filename):
            os.makedirs(os.path.dirname(filename), exist_ok=True)
        with open(filename, 'wb') as f:
            np.savez_compressed(f, images=self.images.cpu().numpy(), filenames=np.array(self.image_filenames))

    def load_cache(self, filename):
        """Adopt a cache written by ``save_cache`` for the same files at the same size -> whether it was taken."""
        if not os.path.exists(filename):
            return False
        with np.load(filename) as z:
            images, names = z['images'], [str(s) for s in z['filenames']]
        if images.shape[1:3] != (self.size, self.size) or len(names) != len(images) or not set(names) <= set(self.image_filenames):
            print(f'Ignoring dataset cache {filename}: it does not describe {self.root} at size {self.size}')
            return False
        self.image_filenames = names
        self.images = torch.from_numpy(images).to(self.device)
        return True
