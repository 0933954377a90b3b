"""Apps that load a generator checkpoint and render from it (reference utils/app.py, explore/base.py).

``GOutputApp`` keeps the reference's positional arguments, flags and defaults, its order of host draws (``torch.randn`` from the
CPU default generator, or ``scipy.stats.truncnorm.rvs`` from numpy's global generator under ``--trunc-norm``) and the pixel
arithmetic of ``torchvision.utils.save_image(..., normalize=True, range=(-1, 1))`` (through
``image_sampler.image_grid_uint8`` and Pillow: torchvision is not a dependency).  Checkpoints are whole pickled modules, as
``ModelCheckpointComponent`` writes them, read from local paths only.
"""
import argparse
import os

import torch

from ..trainers.components.image_sampler import image_grid_uint8


class App:
    app_name = 'base app'

    def __init__(self, args):
        self.args = args

    def run(self):
        pass

    @classmethod
    def run_from_cli(cls):
        cls.create_from_cli().run()

    @classmethod
    def create_from_cli(cls, argv=None):
        return cls(cls.parse_cli_args(argv))

    @classmethod
    def parse_cli_args(cls, argv=None):
        p = argparse.ArgumentParser(description=cls.app_name, fromfile_prefix_chars='@')
        cls.add_args_to_parser(p)
        return p.parse_args(argv)

    @classmethod
    def add_args_to_parser(cls, p):
        pass


def set_device_from_args(args):
    """trainers/utils.py:5-11 (an app without --no-cuda takes the device that is there)."""
    args.device = 'cuda' if torch.cuda.is_available() and not getattr(args, 'no_cuda', False) else 'cpu'


def _local_path(path):
    if '://' in str(path):
        raise ValueError(f'{path}: only local checkpoint and output paths are supported (no remote file systems)')
    return path


def check_image_generator(g):
    """The explore apps work with image generators: a module with ``config.latent_dims``, ``max_size`` and 3 output channels
    over 2-D layers.  Anything else (a discriminator, a text generator, a bare state_dict) is refused here, not deep in a kernel."""
    from ..models.layers import Conv1d
    cfg = getattr(g, 'config', None)
    ok = isinstance(g, torch.nn.Module) and cfg is not None and hasattr(cfg, 'latent_dims') and hasattr(g, 'max_size')
    if ok and (getattr(cfg, 'data_dims', 3) != 3 or any(isinstance(m, Conv1d) for m in g.modules())):
        ok = False
    if not ok:
        raise ValueError(f'the checkpoint holds a {type(g).__name__}, not an image generator (config.latent_dims, max_size, '
                         f'3 output channels); text-generator checkpoints are not supported')
    return g


class GOutputApp(App):
    def sample_z(self, n):
        latent_dims = self.g.config.latent_dims
        if self.args.trunc_norm is not None:
            from scipy.stats import truncnorm
            z = truncnorm.rvs(-self.args.trunc_norm, self.args.trunc_norm, size=n * latent_dims)
            return torch.from_numpy(z.reshape((n, latent_dims))).float().to(self.args.device)
        return torch.randn(n, latent_dims).to(self.args.device)

    def _load(self, default_name):
        root = _local_path(self.args.checkpoint_root)
        filename = root if os.path.isfile(root) else f'{root}/{default_name}'
        with open(filename, 'rb') as infile:
            return torch.load(infile, map_location=self.args.device, weights_only=False)

    def load_generator(self, target=True):
        self.g = check_image_generator(self._load('g_target.pt' if target else 'g.pt'))

    def load_disciminator(self):
        self.d = self._load('d.pt')

    def make_output_dir(self):
        dirname = os.path.dirname(_local_path(self.args.output_prefix))
        if dirname:
            os.makedirs(dirname, exist_ok=True)

    def save_image(self, img, filename, range=(-1, 1)):
        from PIL import Image
        img = img.detach()
        if img.dim() == 3:
            img = img[None]
        # (make_grid returns a single image as it is, without the 2-pixel frame)
        arr = image_grid_uint8(img, padding=2 if len(img) > 1 else 0, value_range=range)
        Image.fromarray(arr).save(_local_path(filename), format='png')

    @classmethod
    def add_args_to_parser(cls, p):
        super().add_args_to_parser(p)
        p.add_argument('checkpoint_root', help='Path to root of checkpoint files.')
        p.add_argument('output_prefix', help='Prefix for output files.')
        p.add_argument('--no-cuda', action='store_true')
        p.add_argument('--trunc-norm', type=float, default=None, help='Sample from truncated normal distribution')
