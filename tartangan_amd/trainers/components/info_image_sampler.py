"""Code sweeps of the InfoGAN trainer (reference components/info_image_sampler.py:13-61).

At train begin, after the stock component's ``sample_z(32)``: one ``sample_z(1)`` is repeated into a (7, min(4, K) + 1, latent)
sweep whose column ``i`` runs continuous code ``C + i`` over ``linspace(-2, 2, 7)`` and whose last column runs the last latent;
with categorical codes two more latents are drawn (``sample_z(2)``) and each of the three is repeated ``C`` times with the
identity matrix in the categorical columns.  The draws come from the trainer, in this order, so a seeded run sees the reference's
values.  ``output_samples`` renders ``target_g`` on both sweeps (flattened to 2-d: the generator's kernels take (rows, latent))
and writes ``info_cat_<name>.png`` / ``info_cont_<name>.png`` with one sweep step per grid row.  Only rank 0 writes.
"""
import os

import torch

from .image_sampler import ImageSamplerComponent, image_grid_uint8


class InfoImageSamplerComponent(ImageSamplerComponent):
    num_points_per_dim = 7

    def on_train_begin(self, steps, logs):
        super().on_train_begin(steps, logs)
        cat = self.trainer.args.info_cat_dims
        self.num_cont_dims = min(4, self.trainer.args.info_cont_dims)
        base_z = self.trainer.sample_z(1)
        self.continuous_samples = base_z[None, ...].repeat(self.num_points_per_dim, self.num_cont_dims + 1, 1)
        pts = torch.linspace(-2, 2, self.num_points_per_dim, device=base_z.device)
        for i in range(self.num_cont_dims):
            self.continuous_samples[:, i, cat + i] = pts
        self.continuous_samples[:, -1, -1] = pts          # a latent no code controls, for comparison
        self.categorical_samples = None
        if cat:
            base_z = torch.cat([base_z, self.trainer.sample_z(2)], dim=0)
            self.categorical_samples = base_z[:, None, ...].repeat(1, cat, 1)
            self.categorical_samples[..., :cat] = torch.eye(cat, device=base_z.device)

    def render_sweeps(self):
        """-> [(name, images (rows * cols, C, S, S), cols)] for the sweeps there are."""
        out = []
        with torch.no_grad():
            for name, samples in (('cat', self.categorical_samples), ('cont', self.continuous_samples)):
                if samples is not None:
                    out.append((name, self.trainer.target_g(samples.reshape(-1, samples.shape[-1])), samples.shape[1]))
        return out

    def output_samples(self, filename, n=None):
        sweeps = self.render_sweeps()          # every rank renders (BatchNorm statistics stay in step); rank 0 writes
        dp = getattr(self.trainer, 'data_parallel', None)
        if dp is not None and dp.rank != 0:
            return
        from PIL import Image
        for name, imgs, nrow in sweeps:
            grid_filename = os.path.join(os.path.dirname(filename), f'info_{name}_{os.path.basename(filename)}')
            Image.fromarray(image_grid_uint8(imgs, nrow=nrow)).save(grid_filename, format='png')
