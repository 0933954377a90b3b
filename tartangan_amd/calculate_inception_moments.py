"""Data-set moments for FID: the ``mu`` / ``sigma`` file that ``--inception-moments`` and ``prepare_inception_metrics`` read.

Every batch of a data set goes through the Inception network; the pooled 2048-feature rows are collected on the device, and
their mean and covariance come from numpy (``np.mean(pool, 0)``, ``np.cov(pool, rowvar=False)``).  The Inception score of the
data itself is printed on the way, from the same forward passes.

    python -m tartangan_amd.calculate_inception_moments images.npz moments.npz --batch-size 32 \\
        --inception-weights inception_v3_google.pth

``source`` is an ``ImageBytesDataset`` archive.  A batch reaches the network the way the training-time metric sees real data:
pixel / 255, the VGG mean / std, and ``WrapInception``'s own normalisation and 299 x 299 resize on top -- here the first
normalisation is one ``tg_inception_preprocess`` launch on the [-1, 1] batch the data set produces."""
import argparse
import sys

import numpy as np
import torch

from . import inception_utils
from .image_bytes_dataset import ImageBytesDataset


class _Progress:
    """'<n> batches, <m> images' every ``every`` batches, on one line (carriage return) or one line each."""

    def __init__(self, every, newlines, quiet):
        self.every, self.end, self.quiet = max(int(every), 1), '\n' if newlines else '\r', quiet
        self.batches = self.images = 0

    def step(self, n_images):
        self.batches += 1
        self.images += n_images
        if not self.quiet and self.batches % self.every == 0:
            print(f'[moments] {self.batches} batches, {self.images} images', end=self.end, flush=True)

    def close(self):
        if not self.quiet:
            print(f'[moments] {self.batches} batches, {self.images} images: done')


def pooled_activations(loader, net, progress=None):
    """-> (pool (N, D), class probabilities (N, classes)) of every batch of ``loader``, device tensors."""
    rows, probs = [], []
    with torch.no_grad():
        for batch in loader:
            if not rows:
                net = net.to(batch.device)
            pool, logits = net(batch)
            rows.append(pool)
            probs.append(inception_utils._softmax_rows(logits))
            if progress is not None:
                progress.step(batch.shape[0])
    if not rows:
        raise ValueError('calculate_inception_moments: the loader is empty')
    return torch.cat(rows, 0), torch.cat(probs, 0)


def calculate_inception_moments(loader, use_newlines=False, log_iters=10, quiet_logs=False, net=None, weights=None):
    """``loader``: an iterable of normalised (B, 3, H, W) device batches.  Returns ``(mu, sigma)`` as numpy arrays and prints
    the data set's Inception score (ten splits, so at least ten images).  ``net``: a ``WrapInception`` or a bare network for
    it; ``weights``: a state-dict path for the native network (see ``inception_utils.load_inception_net``)."""
    if not isinstance(net, inception_utils.WrapInception):
        net = inception_utils.load_inception_net(net=net, weights=weights)
    progress = _Progress(log_iters, use_newlines, quiet_logs)
    pool, probs = pooled_activations(loader, net, progress)
    progress.close()
    score, spread = inception_utils.calculate_inception_score(probs)
    print(f'[moments] Inception score of the data: {score:.5f} +/- {spread:.5f} ({pool.shape[0]} images)')
    features = pool.cpu().numpy()
    return np.mean(features, axis=0), np.cov(features, rowvar=False)


def normalised_batches(dataset, batch_size):
    """One shuffled epoch of full batches of ``dataset``, each after pixel / 255 and the VGG mean / std."""
    for batch in dataset.loader(batch_size, shuffle=True, drop_last=True):
        yield inception_utils.inception_preprocess(batch, None, 1)


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tartangan_amd.calculate_inception_moments', description=__doc__.split('\n')[0])
    p.add_argument('source', help='image archive: .npz with an `images` array (N, H, W, 3) uint8, or a bare .npy')
    p.add_argument('destination', help='.npz to write, with arrays `mu` (D,) and `sigma` (D, D)')
    p.add_argument('--batch-size', type=int, default=32, help='images per forward pass; a trailing partial batch is left out')
    p.add_argument('--inception-weights', default=None, metavar='PATH',
                   help='torchvision-format Inception-v3 state dict; default: the TG_INCEPTION_WEIGHTS environment variable')
    p.add_argument('--log-iters', type=int, default=10, help='report progress every this many batches')
    p.add_argument('--quiet-logs', action='store_true', help='no progress reports')
    p.add_argument('--log-newlines', action='store_true', help='one progress report per line (for log files)')
    p.add_argument('--device', default='cuda', help='where the archive and the network live')
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    dataset = ImageBytesDataset.from_path(args.source, device=args.device)
    print(f'[moments] {len(dataset)} images from {args.source}, batches of {args.batch_size} on {args.device}')
    mu, sigma = calculate_inception_moments(normalised_batches(dataset, args.batch_size), use_newlines=args.log_newlines,
                                            log_iters=args.log_iters, quiet_logs=args.quiet_logs, weights=args.inception_weights)
    np.savez(args.destination, mu=mu, sigma=sigma)
    print(f'[moments] wrote mu {mu.shape} and sigma {sigma.shape} to {args.destination}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
