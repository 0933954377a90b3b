#!/usr/bin/env python3
"""Generate the explore apps' fixtures (tests/golden/explore_*.json) by running the REFERENCE implementation.

What is executed is the reference's own, unmodified ``tartangan.explore.find_image.FindImage.run``,
``render_tour.RenderTour.run`` and ``continuous_interp.ContinuousInterp.run`` on the CPU, over a checkpoint of the reference's own
``Generator`` at config ``16`` with ``oracle.procedural`` weights; the fixtures hold recorded numbers only.  ``make_golden``'s inert
third-party stand-ins are extended here, at run time, by what these apps call:

  * ``torchvision.utils.save_image`` records what it is handed (L2 and 8 probe pixels) instead of encoding a PNG;
  * ``tqdm.tqdm`` (as the find-image module sees it) records ``set_postfix``'s loss, z_min, z_mean, z_max -- and a copy of z, which
    it can reach because the app's ``sample_z`` is wrapped to remember the tensor it returned;
  * ``smart_open.open`` is ``open``; ``torchvision.transforms`` are the few Pillow-backed classes the app composes;
    ``torchvision.models.vgg16`` is an inert module (the fixtures run without ``--vgg``).

The target image is already 16 x 16: the resize is an identity and the crop draws nothing.

numpy: with numpy 2 the reference's slerp promotes its interpolants to float64 and hands the generator float64 latents, which a
float32 generator refuses; the numpy 1.x it was written for produced float32.  The checkpoint module pickled here is therefore a
wrapper (``Float32Input``) that casts its input to float32 and otherwise is the reference's Generator.

Every case also (a) runs the reference once more with the generator in float64 (``Float64Twin``: generator, normalisation and loss
in float64; z and its optimiser stay float32, as their draws do) and asserts the fp32 run is within ROOM of it, and (b) runs THIS
package's app over the CPU emulator (tests/explore_cases.ExploreEmulator) and asserts agreement to ROOM = 3e-5 (the tests assert
1e-4).  Adam's first step is lr * sign(g): a latent whose gradient is zero up to rounding is a knife edge.  If a seed fails,
change the seed, not the tolerance.  Seeds tried are listed at CASES.  One adam case asserts that its recorded steps contain a
stochastic clip.

Usage:  python tests/golden/make_explore_golden.py [case ...]
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

os.environ.setdefault('TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD', '1')       # the reference's torch.load predates weights_only

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (installs the stand-ins, puts the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import smart_open  # noqa: E402  (inert)
import torchvision.models  # noqa: E402  (inert)
import torchvision.transforms  # noqa: E402  (inert)
import torchvision.utils  # noqa: E402  (inert)

import explore_cases as EC  # noqa: E402
from oracle.procedural import procedural_state  # noqa: E402

ROOM = 3e-5
NP_SEED = 2468
TARGET_SEED = 77
CASES = {
    # name: (app, flags, weight seed, must contain a clip).  Weight seed 17 was the first tried for every case and held.
    'explore_find_adam_mse': ('find_image', ['--max-steps', '4'], 17, True),
    'explore_find_sgd_l1': ('find_image', ['--max-steps', '3', '--optimizer', 'sgd', '--loss', 'l1', '--l2', '0.1', '--lr', '0.01'], 17, False),
    'explore_find_adam_trunc': ('find_image', ['--max-steps', '3', '--trunc-norm', '1.5'], 17, False),
    'explore_tour': ('render_tour', ['--num-points', '3', '--seg-frames', '2'], 17, False),
    'explore_interp': ('continuous_interp', ['--output-size', '20', '--num-points', '6'], 17, False),
    'explore_interp_tile': ('continuous_interp', ['--output-size', '20', '--num-points', '6', '--tile'], 17, False),
}


# ----------------------------------------------------------------------------------------------------------- stand-ins
class Recorder:
    def __init__(self):
        self.images, self.steps, self.z = [], [], None

    def save_image(self, img, output_file, **kw):
        assert kw.get('normalize') is True and tuple(kw.get('range')) == (-1, 1) and kw.get('format') == 'png', kw
        self.images.append(EC.image_entry(img))

    def remember_z(self, sample_z):
        def wrapped(n):
            self.z = sample_z(n)
            return self.z
        return wrapped


RECORDER = Recorder()


class RecordingTqdm:
    def __init__(self, iterable):
        self.iterable = iterable

    def __iter__(self):
        return iter(self.iterable)

    def set_postfix(self, **kw):
        RECORDER.steps.append(dict(kw, z=[float(v) for v in RECORDER.z.detach().double().reshape(-1)]))


class _Compose:
    def __init__(self, fns):
        self.fns = fns

    def __call__(self, x):
        for fn in self.fns:
            x = fn(x)
        return x


class _Resize:
    def __init__(self, size, interpolation=None):
        self.size, self.interpolation = size, interpolation

    def __call__(self, img):
        w, h = img.size
        if min(w, h) == self.size:
            return img
        ow, oh = (self.size, int(self.size * h / w)) if w <= h else (int(self.size * w / h), self.size)
        return img.resize((ow, oh), self.interpolation)


class _RandomCrop:
    def __init__(self, size):
        self.size = size

    def __call__(self, img):
        w, h = img.size
        th, tw = self.size
        if (w, h) == (tw, th):
            return img
        i, j = int(torch.randint(0, h - th + 1, size=(1,))), int(torch.randint(0, w - tw + 1, size=(1,)))
        return img.crop((j, i, j + tw, i + th))


PIXEL_DTYPE = [torch.float32]          # float64 while the float64 twin runs


class _ToTensor:
    def __call__(self, img):
        return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).to(PIXEL_DTYPE[0]).div(255)


class _Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = torch.tensor(mean).view(-1, 1, 1), torch.tensor(std).view(-1, 1, 1)

    def __call__(self, t):
        return t.clone().sub_(self.mean.to(t.dtype)).div_(self.std.to(t.dtype))


class _InertVGG(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.features = torch.nn.Sequential()


def install_stand_ins():
    smart_open.open = open
    torchvision.utils.save_image = RECORDER.save_image
    T = torchvision.transforms
    T.Compose, T.Resize, T.RandomCrop, T.ToTensor, T.Normalize = _Compose, _Resize, _RandomCrop, _ToTensor, _Normalize
    torchvision.models.vgg16 = lambda **kw: _InertVGG()
    if not hasattr(Image, 'LANCZOS'):
        Image.LANCZOS = Image.Resampling.LANCZOS


install_stand_ins()

from tartangan.explore import continuous_interp as R_CI  # noqa: E402
from tartangan.explore import find_image as R_FI  # noqa: E402
from tartangan.explore import render_tour as R_RT  # noqa: E402

R_FI.tqdm = types.SimpleNamespace(tqdm=RecordingTqdm)
REFERENCE_APPS = {'find_image': R_FI.FindImage, 'render_tour': R_RT.RenderTour, 'continuous_interp': R_CI.ContinuousInterp}


class Float32Input(torch.nn.Module):
    """The reference's Generator behind a cast of its input to float32 (see the module docstring: numpy 2)."""
    dtype = torch.float32

    def __init__(self, g):
        super().__init__()
        self.g = g

    config = property(lambda self: self.g.config)
    max_size = property(lambda self: self.g.max_size)

    def forward(self, z):
        return self.g(z.to(self.dtype))


class Float64Twin(Float32Input):
    dtype = torch.float64


def reference_generator(weight_seed, twin=False):
    tr = MG.build_trainer('16', 'cnn', 2)
    g = tr.target_g
    g.load_state_dict(procedural_state(g.state_dict(), weight_seed))
    g.train()
    return Float64Twin(g.double()) if twin else Float32Input(g)


def my_apps():
    from tartangan_amd.explore.continuous_interp import ContinuousInterp
    from tartangan_amd.explore.find_image import FindImage
    from tartangan_amd.explore.render_tour import RenderTour
    return {'find_image': FindImage, 'render_tour': RenderTour, 'continuous_interp': ContinuousInterp}


# ----------------------------------------------------------------------------------------------------------- running
def argv_of(app, flags, root, tmp):
    argv = [root, os.path.join(tmp, 'out', 'frame')]
    if app == 'find_image':
        argv.append(os.path.join(tmp, 'target.png'))
    return argv + list(flags)


def run_reference(name, weight_seed, twin=False):
    """-> dict(steps, images, rng_after) of the reference's run()."""
    app, flags = CASES[name][:2]
    cls = REFERENCE_APPS[app]
    fx = dict(size=16, target_seed=TARGET_SEED)
    RECORDER.__init__()
    PIXEL_DTYPE[0] = torch.float64 if twin else torch.float32
    with tempfile.TemporaryDirectory() as tmp:
        torch.save(reference_generator(weight_seed, twin), os.path.join(tmp, 'g_target.pt'))
        EC.write_target(fx, os.path.join(tmp, 'target.png'))
        obj = cls(EC.app_args(cls, argv_of(app, flags, tmp, tmp)))
        obj.sample_z = RECORDER.remember_z(obj.sample_z)
        torch.manual_seed(MG.RNG_SEED)
        np.random.seed(NP_SEED)
        with contextlib.redirect_stdout(io.StringIO()):
            obj.run()
        assert not any(p.requires_grad for p in obj.g.parameters()) or app != 'find_image'
    return dict(steps=RECORDER.steps, images=RECORDER.images, rng_after=EC.rng_after())


def run_mine(name, fixture):
    """This package's app over the emulator -> the same record."""
    from tartangan_amd import backend
    app, flags = CASES[name][:2]
    cls = my_apps()[app]
    rec = dict(steps=[], images=[])

    class Recording(cls):
        def save_image(self, img, filename, range=(-1, 1)):
            rec['images'].append(EC.image_entry(img))

        def log(self, i, loss, z_min, z_mean, z_max):
            rec['steps'].append(dict(loss=loss, z_min=z_min, z_mean=z_mean, z_max=z_max,
                                     z=[float(v) for v in self.z.detach().double().reshape(-1)]))

    prev = backend._set_backend_for_testing(EC.ExploreEmulator())
    try:
        with tempfile.TemporaryDirectory() as tmp:
            EC.save_checkpoint(fixture, tmp)
            EC.write_target(fixture, os.path.join(tmp, 'target.png'))
            obj = Recording(EC.app_args(cls, argv_of(app, flags, tmp, tmp) + (['--no-cuda'] if app != 'render_tour' else [])))
            EC.seed_streams(fixture)
            with contextlib.redirect_stderr(io.StringIO()):
                obj.run()
        rec['rng_after'] = EC.rng_after()
    finally:
        backend._set_backend_for_testing(prev)
    return rec


def _dev(a, b, scale=None):
    return abs(a - b) / max(abs(b) if scale is None else scale, 1e-12)


def deviation(got, want):
    """Largest relative difference between two records: loss, z_min, z_max and image L2 relative to themselves, z and probe
    pixels relative to the largest of their vector -- and so is z_mean, a cancelling sum (measured against max|z|, not itself)."""
    worst = (0.0, 'nowhere')
    assert len(got['steps']) == len(want['steps']) and len(got['images']) == len(want['images'])
    for k, (g, w) in enumerate(zip(got['steps'], want['steps'])):
        for key in ('loss', 'z_min', 'z_max'):
            worst = max(worst, (_dev(g[key], w[key]), f'step {k} {key}'))
        zs = max(abs(v) for v in w['z'])
        worst = max(worst, (_dev(g['z_mean'], w['z_mean'], zs), f'step {k} z_mean'))
        worst = max(worst, (max(_dev(a, b, zs) for a, b in zip(g['z'], w['z'])), f'step {k} z'))
    for k, (g, w) in enumerate(zip(got['images'], want['images'])):
        worst = max(worst, (_dev(g['l2'], w['l2']), f'image {k} l2'))
        ps = max(abs(v) for v in w['probes'])
        worst = max(worst, (max(_dev(a, b, ps) for a, b in zip(g['probes'], w['probes'])), f'image {k} probes'))
    return worst


def run_case(name):
    app, flags, weight_seed, wants_clip = CASES[name]
    ref = run_reference(name, weight_seed)
    twin = run_reference(name, weight_seed, twin=True)
    assert twin['rng_after'] == ref['rng_after']
    d64, where64 = deviation(ref, twin)
    assert d64 <= ROOM, f'{name}: the reference in fp32 is {d64:.2e} off its float64 twin at {where64}; change the weight seed'
    fixture = dict(
        case=name, app=app, flags=flags, config='16', size=16, weight_seed=weight_seed, rng_seed=MG.RNG_SEED, np_seed=NP_SEED,
        target_seed=TARGET_SEED, g_training=True, torch_version=torch.__version__, numpy_version=np.__version__,
        source='reference tartangan v0.4.0 code under torch %s CPU fp32' % torch.__version__,
        steps=ref['steps'], images=ref['images'], rng_after=ref['rng_after'], parser=EC.parser_spec(REFERENCE_APPS[app]),
        float64_twin=dict(worst_relative_deviation=d64, where=where64),
    )
    if wants_clip:
        clipped = [k + 1 for k, s in enumerate(ref['steps'][:-1]) if any(abs(v) > 3 for v in s['z'])]
        assert clipped, f'{name}: no latent leaves [-3, 3] within the recorded steps; choose another seed or lr'
        fixture['clip_steps'] = clipped
    mine = run_mine(name, fixture)
    assert mine['rng_after'] == ref['rng_after'], (mine['rng_after'], ref['rng_after'])
    dev, where = deviation(mine, ref)
    fixture['emulated_engine'] = dict(worst_relative_deviation=dev, where=where, room=ROOM)
    assert dev <= ROOM, f'{name}: the emulated engine is {dev:.2e} off at {where}; change the weight seed'
    path = os.path.join(HERE, f'{name}.json')
    with open(path, 'w') as f:
        json.dump(fixture, f, indent=None, separators=(',', ':'))
    print(f'wrote {path} ({os.path.getsize(path) / 1024:.0f} KB; fp32 vs float64 twin {d64:.2e} at {where64}; '
          f'emulated engine off by {dev:.2e} at {where})')


def main():
    torch.set_num_threads(1)
    for n in sys.argv[1:] or list(CASES):
        run_case(n)


if __name__ == '__main__':
    main()
