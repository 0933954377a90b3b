"""Find a generator code for a given image (reference explore/find_image.py).

The reference runs up to 100 000 optimiser steps through a frozen generator at batch 2; around the generator each step is a dozen
tiny ATen ops and three separate read-backs.  Here a step of ``--optimizer adam`` / ``sgd`` is

  1. the stochastic clip of z (``tg_latent_step``, clip only) with that step's noise,
  2. the generator forward (eval mode, parameters frozen),
  3. ``tg_recon_loss``: normalisation, summed loss and image gradient in one pass,
  4. the backward to z inside ``input_grads_only()`` -- no weight gradient is launched,
  5. ``tg_latent_step``: reported loss, L2 term, the optimiser update and min / mean / max of z, one launch, four floats,

and ``enable_graphs()`` replays 1.-5. from one HIP graph.  What a seeded run draws on the host is the reference's: the latents,
then one ``randn(z.shape)`` per step from the CPU default generator whether or not anything clips -- drawn ``noise_chunk`` steps
ahead and uploaded together, so that a replayed step draws nothing.  ``--optimizer lbfgs`` runs ``torch.optim.LBFGS`` over an eager
closure on the same loss kernel.  ``--vgg`` is refused: the VGG-16 weights cannot be had offline.

Two flags are new: ``--save-every N`` and ``--log-every N`` (default 1, the reference's behaviour) skip the per-step PNG and the
per-step read-back of the four floats.
"""
import sys

import torch

from .. import backend as _be
from .. import functional as TF
from .base import GOutputApp, set_device_from_args

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def load_target(path, size):
    """``Resize(size, LANCZOS)`` of the smaller edge, ``RandomCrop((size, size))``, ``ToTensor``, ``Normalize`` through Pillow
    -> (3, size, size) on the CPU.  The crop draws its two offsets with ``torch.randint`` unless the image already fits exactly."""
    from PIL import Image
    import numpy as np
    img = Image.open(path).convert('RGB')
    w, h = img.size
    if min(w, h) != size:
        ow, oh = (size, int(size * h / w)) if w <= h else (int(size * w / h), size)
        img = img.resize((ow, oh), Image.LANCZOS)
        w, h = img.size
    if (w, h) != (size, size):
        top = int(torch.randint(0, h - size + 1, size=(1,)))
        left = int(torch.randint(0, w - size + 1, size=(1,)))
        img = img.crop((left, top, left + size, top + size))
    t = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255)
    return t.sub_(torch.tensor(MEAN).view(3, 1, 1)).div_(torch.tensor(STD).view(3, 1, 1))


class FindImage(GOutputApp):
    """Find a generator code for a given image."""
    app_name = 'Find image'
    noise_chunk = 64

    def __init__(self, args):
        super().__init__(args)
        self._graph_requested = False
        self._graph = None

    def enable_graphs(self):
        """Replay the fused step from one captured HIP graph.  If the capture is refused the run continues eagerly (stderr)."""
        if getattr(self.args, 'optimizer', 'adam') == 'lbfgs':
            raise ValueError('L-BFGS evaluates its closure a varying number of times per step: it does not replay from a graph')
        self._graph_requested = True

    # ------------------------------------------------------------------ hooks a caller (or a test) may override
    def log(self, i, loss, z_min, z_mean, z_max):
        if self._progress is not None:
            self._progress.set_postfix(loss=loss, z_min=z_min, z_mean=z_mean, z_max=z_max)

    def _steps(self):
        try:
            import tqdm
            self._progress = tqdm.tqdm(range(self.args.max_steps))
            return self._progress
        except ImportError:
            self._progress = None
            return range(self.args.max_steps)

    # ------------------------------------------------------------------ the run
    def run(self):
        args = self.args
        if args.vgg:
            raise NotImplementedError('--vgg is not supported: the pretrained VGG-16 weights cannot be downloaded here, and a '
                                      'backward pass through VGG is not implemented')
        if args.optimizer not in ('adam', 'sgd', 'lbfgs'):
            raise KeyError(args.optimizer)
        if args.loss not in TF.RECON_KINDS:
            raise KeyError(args.loss)
        if args.optimizer == 'lbfgs' and self._graph_requested:
            raise ValueError('L-BFGS does not replay from a graph')
        set_device_from_args(args)
        self.load_generator()
        self.g = self.g.eval()
        self.g.requires_grad_(False)
        self.make_output_dir()
        size = self.g.max_size
        target = load_target(args.target_image, size).to(args.device)
        self.target_imgs = target.repeat(args.num_samples, 1, 1, 1).contiguous()
        self.z = self.sample_z(args.num_samples).contiguous()
        self.z.requires_grad_(True)
        if args.optimizer == 'lbfgs':
            return self._run_lbfgs()
        return self._run_fused()

    def _refill(self, first, steps):
        """The clip noise of steps first .. first + steps - 1: one randn(z.shape) each, in order, one upload."""
        return torch.stack([torch.randn(self.z.shape) for _ in range(steps)]).to(self.args.device)

    def _fused_step(self):
        z, args = self.z, self.args
        TF.latent_step(z, None, None, None, None, self._noise, None, None, 'clip')
        imgs = self.g(z)
        if imgs.shape != self.target_imgs.shape:
            raise ValueError(f'the generator renders {tuple(imgs.shape)}, the target is {tuple(self.target_imgs.shape)}')
        imgs_c = imgs.detach().contiguous()
        dimgs = torch.empty_like(imgs_c)
        TF.recon_loss_into(imgs_c, self.target_imgs, dimgs, self._recon, TF.RECON_KINDS[args.loss])
        with TF.input_grads_only():
            gz, = torch.autograd.grad(imgs, z, dimgs)
        TF.latent_step(z, gz.contiguous(), self._m, self._v, self._step, None, self._stats, self._recon, args.optimizer,
                       lr=args.lr, l2=args.l2)
        return imgs_c

    def _capture(self):
        """Everything the captured step reads or keeps exists, initialised, before the capture starts: the state tensors below
        are built by the caller, and one dry forward / backward (its results dropped; an eval-mode generator changes nothing)
        makes the layers build whatever they cache lazily.  A capture that fails can therefore leave nothing half-made behind."""
        import gc
        z = self.z
        with TF.input_grads_only():
            dry = self.g(z)
            torch.autograd.grad(dry, z, torch.zeros_like(dry))
        del dry
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        was_enabled = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            with torch.cuda.graph(graph):
                self._static_imgs = self._fused_step()
        finally:
            if was_enabled:
                gc.enable()
        return graph

    def prepare_fused(self):
        """The step's device state (clip noise, loss, statistics, Adam moments and step counter), built and zeroed before any
        capture, then the capture if graphs were asked for.  Needs ``g``, ``z``, ``target_imgs`` and ``args``."""
        dev = self.args.device
        self._noise = torch.zeros_like(self.z, requires_grad=False)
        self._recon = torch.zeros(1, device=dev)
        self._stats = torch.zeros(4, device=dev)
        self._m, self._v = torch.zeros_like(self._noise), torch.zeros_like(self._noise)
        self._step = torch.zeros(1, dtype=torch.int64, device=dev)
        self._graph, self._chunk, self._chunk_first = None, None, 0
        if self._graph_requested:
            if dev != 'cuda':
                raise RuntimeError('HIP graphs need a ROCm device')
            try:
                self._graph = self._capture()
            except _be.KernelError:
                raise
            except RuntimeError as exc:
                print(f'find_image: HIP-graph capture failed ({exc!r}); continuing in eager mode', file=sys.stderr)
                self._graph = None

    def step(self, i):
        """Step ``i`` (in order from 0) -> the images it rendered.  Replayed, it costs one device-to-device copy of that step's
        noise and one graph launch; the host draws only when a chunk of noise runs out."""
        if self._chunk is None or i - self._chunk_first >= len(self._chunk):
            self._chunk_first = i
            self._chunk = self._refill(i, max(1, min(self.noise_chunk, self.args.max_steps - i)))
        self._noise.copy_(self._chunk[i - self._chunk_first])
        if self._graph is not None:
            self._graph.replay()
            return self._static_imgs
        return self._fused_step()

    def _run_fused(self):
        args = self.args
        self.prepare_fused()
        imgs = None
        for i in self._steps():
            imgs = self.step(i)
            if args.save_every and i % args.save_every == 0:
                self.save_image(imgs, f'{args.output_prefix}_{i}.png')
            if args.log_every and i % args.log_every == 0:
                self.log(i, *self._stats.tolist())
        self.imgs = imgs
        return self.z

    def _run_lbfgs(self):
        args, z = self.args, self.z
        optimizer = torch.optim.LBFGS([z], args.lr)
        kind = TF.RECON_KINDS[args.loss]

        for i in self._steps():
            def train_step():
                optimizer.zero_grad()
                imgs = self.g(z)
                loss = TF.recon_loss(imgs, self.target_imgs, kind)
                loss = loss + z.pow(2).mean() * args.l2          # L2 regularization of latent code
                loss.backward()
                if args.save_every and i % args.save_every == 0:
                    self.save_image(imgs, f'{args.output_prefix}_{i}.png')
                self.imgs = imgs.detach()
                return loss

            noise = torch.randn(z.shape).to(args.device)
            TF.latent_step(z, None, None, None, None, noise, None, None, 'clip')
            loss = optimizer.step(train_step)
            if args.log_every and i % args.log_every == 0:
                zd = z.detach()
                self.log(i, float(loss.detach()), float(zd.min()), float(zd.mean()), float(zd.max()))
        return self.z

    @classmethod
    def add_args_to_parser(cls, p):
        super().add_args_to_parser(p)
        p.add_argument('target_image', help='Path to image to be found in G')
        p.add_argument('--max-steps', default=100000, type=int)
        p.add_argument('--num-samples', default=2, type=int)
        p.add_argument('--lr', default=0.5, type=float)
        p.add_argument('--vgg', action='store_true')
        p.add_argument('--vgg-layers', default=(9, 16, 23), type=int, nargs='+')
        p.add_argument('--optimizer', default='adam')
        p.add_argument('--l2', default=0., type=float)
        p.add_argument('--loss', default='mse')
        p.add_argument('--save-every', default=1, type=int, help='Write the PNG of every Nth step (0: never)')
        p.add_argument('--log-every', default=1, type=int, help='Read the loss and z statistics back every Nth step (0: never)')


if __name__ == '__main__':
    FindImage.run_from_cli()
