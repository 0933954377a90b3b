"""Render a circuit of images through latent space (reference explore/render_tour.py).

``num_points`` latents are drawn, each is joined to the next (the last to the first) by ``seg_frames`` slerp steps, the end point
left out; ONE generator call renders the whole path, in whatever mode the module was pickled in, and every frame becomes
``<output_prefix>_<i>.png``.  The interpolants are float32 (what the reference's pinned numpy 1.x produces, see
``image_sampler.sample_latent_grid``).
"""
import numpy as np
import torch

from ..trainers.components.image_sampler import slerp
from .base import GOutputApp, set_device_from_args


class RenderTour(GOutputApp):
    """Renders a circuit of images"""
    app_name = 'Render tour'

    def tour_path(self):
        points = self.sample_z(self.args.num_points).cpu().numpy()
        path = []
        for p_a, p_b in zip(points, np.concatenate([points[1:], points[0:1]], axis=0)):
            for i in np.linspace(0, 1, self.args.seg_frames + 1)[:-1]:      # trim the final 1.0 value from the space
                path.append(slerp(i, p_a, p_b))
        return torch.from_numpy(np.stack(path)).to(self.args.device, torch.float32)

    def run(self):
        set_device_from_args(self.args)
        self.load_generator()
        imgs = self.g(self.tour_path())
        self.make_output_dir()
        for i, img in enumerate(imgs):
            self.save_image(img, f'{self.args.output_prefix}_{i}.png')
        return imgs

    @classmethod
    def add_args_to_parser(cls, p):
        p.add_argument('checkpoint_root', help='Path to root of checkpoint files.')
        p.add_argument('output_prefix', help='Prefix for output files.')
        p.add_argument('--num-points', type=int, default=2, help='Number of points to visit')
        p.add_argument('--seg-frames', type=int, default=3, help='Number of points to visit')
        p.add_argument('--trunc-norm', type=float, default=None, help='Sample from truncated normal distribution')


if __name__ == '__main__':
    RenderTour.run_from_cli()
