#!/usr/bin/env python3
"""Generate the scene-trainer fixtures (tests/golden/scene_*.json) by running the REFERENCE implementation.

Like make_golden.py (whose inert third-party stand-ins, argument namespace and summaries it reuses): what is executed is the
reference's own, unmodified ``tartangan.trainers.scene.SceneTrainer`` -- ``build_models()`` and ``train_batch()`` -- with
``tartangan.models.pluggan.StructuredSceneGenerator``; the fixtures hold recorded numbers only.  The files are named
``scene_*`` so that ``conftest.golden_cases()`` (the cnn / iqn fixtures, ``c<size>...``) does not pick them up.

Bilinear sampling has a kink at integer texel coordinates: there the gradient with respect to the transform is discontinuous,
and an fp32 implementation may land on the other side of it than this run did.  Every generator forward of a case therefore
records (through a forward hook on the transform Linear; float64) the least distance of a sample coordinate from an integer,
and the case asserts that it is at least its margin, 1e-4.  If that fails, change the case's weight seed.

The default geometry cannot meet 1e-4 under any seed: its seven forwards place 4 x 20 x 256 samples each, some 290 000
coordinates of which about half can reach a patch, and coordinates that are spread evenly between two integers all miss a band
of +-1e-4 around them with probability exp(-290000 * 0.5 * 2e-4) ~ 1e-13 (weight seeds 7..39 gave least distances between
1.7e-7 and 2.0e-5).  What the margin has to exceed is the error of an fp32 coordinate: ix = ((gx + 1) patch - 1) / 2 with
|(gx + 1) patch| <= 2 (patch + 1) = 8 for a sample that can reach a 3-texel patch, four roundings of at most 8 * 2^-24 each on
the way, 2e-6 in all.  That case takes the seed with the largest distance found (35: 2.0e-5) and asserts 1e-5, five times
that error; the other two cases hold the 1e-4.

Usage:  python tests/golden/make_scene_golden.py [case ...]
"""
import contextlib
import copy
import io
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (installs the stand-ins, puts the reference on sys.path)
import torch  # noqa: E402

from oracle.procedural import procedural_state, summarize, synthetic_images  # noqa: E402
from scene_cases import KINK_MARGIN, kink_distance_and_coverage, scene_state  # noqa: E402
from tartangan.models.pluggan import GAN_CONFIGS  # noqa: E402
from tartangan.trainers.scene import SceneTrainer  # noqa: E402

CASES = {
    # name: (config, batch, steps, flags, weight seed, kink margin)
    'scene_c32_s8_p5_b4': ('32', 4, 2, dict(scene_size=8, num_patches=5, patch_size=3, refine_patches=False, patch_noise=False),
                           14, KINK_MARGIN),
    'scene_c64_s16_p20_b4_refine_noise': ('64', 4, 2, dict(scene_size=16, num_patches=20, patch_size=3, refine_patches=True,
                                                           patch_noise=True), 35, 1e-5),
    'scene_c32_s4_p3_k4_b4_refine': ('32', 4, 2, dict(scene_size=4, num_patches=3, patch_size=4, refine_patches=True,
                                                      patch_noise=False), 8, KINK_MARGIN),
}
NOISE_SEED = 555       # the forward pins draw their patch noise from the default generator: seeded right before each


def build_trainer(config, batch, flags, init_seed=0):
    t = object.__new__(SceneTrainer)          # skip Trainer.__init__ (filesystem side effects only)
    t.args = MG.make_args(config, batch)
    for k, v in flags.items():
        setattr(t.args, k, v)
    torch.manual_seed(init_seed)
    with contextlib.redirect_stdout(io.StringIO()):
        t.build_models()
    return t


class KinkWatch:
    """Least distance to a kink over every forward of the generators it watches."""

    def __init__(self):
        self.least, self.forwards = 1.0, 0

    def watch(self, g):
        block = g.structure_generator

        def hook(_module, _inputs, theta):
            B = theta.shape[0]
            dist, _ = kink_distance_and_coverage(theta.detach().reshape(B, -1), B, block.num_patches, block.patch_size,
                                                 block.scene_size)
            self.least, self.forwards = min(self.least, dist), self.forwards + 1
        block.patch_transforms.register_forward_hook(hook)


def run_case(name):
    config, batch, steps, flags, weight_seed, margin = CASES[name]
    t0 = time.time()
    tr = build_trainer(config, batch, flags)
    size = tr.g.max_size
    fixture = dict(
        case=name, config=config, flags=flags, attention=list(GAN_CONFIGS[config].attention or ()), trainer='scene', batch=batch,
        size=size, weight_seed=weight_seed, rng_seed=MG.RNG_SEED, img_seed=MG.IMG_SEED, noise_seed=NOISE_SEED,
        torch_version=torch.__version__, num_threads=torch.get_num_threads(),
        source='reference tartangan v0.4.0 code under torch %s CPU fp32' % torch.__version__,
        blocks=list(tr.gan_config.blocks), latent_dims=tr.gan_config.latent_dims,
    )
    fixture['default_init'] = dict(
        g_l2=MG.total_l2(tr.g), target_g_l2=MG.total_l2(tr.target_g), d_l2=MG.total_l2(tr.d),
        g=MG.net_summary(tr.g, n_samples=2),
        d_last=summarize(list(tr.d.parameters())[-1], 4),
    )
    tr.g.load_state_dict(scene_state(tr.g.state_dict(), weight_seed))
    tr.target_g.load_state_dict(scene_state(tr.target_g.state_dict(), weight_seed + 1))
    tr.d.load_state_dict(procedural_state(tr.d.state_dict(), weight_seed + 2))
    fixture['n_params'] = dict(g=sum(p.numel() for p in tr.g.parameters()), d=sum(p.numel() for p in tr.d.parameters()),
                               g_tensors=len(list(tr.g.parameters())))
    fixture['state_keys'] = dict(g=list(tr.g.state_dict().keys()), d=list(tr.d.state_dict().keys()))
    fixture['param_names'] = dict(g=[n for n, _ in tr.g.named_parameters()])
    watch = KinkWatch()

    with torch.no_grad():
        g2, d2 = copy.deepcopy(tr.g), copy.deepcopy(tr.d)
        watch.watch(g2)
        z = torch.randn(batch, tr.gan_config.latent_dims, generator=torch.Generator().manual_seed(99))
        imgs0 = synthetic_images(batch, size, MG.IMG_SEED)
        torch.manual_seed(NOISE_SEED)
        structure = g2.structure_generator(z)
        torch.manual_seed(NOISE_SEED)
        g_out = g2(z)
        fwd = dict(structure=summarize(structure, 8), g_out=summarize(g_out, 8),
                   d_real=[float(v) for v in d2(imgs0).reshape(-1)], d_fake=[float(v) for v in d2(g_out).reshape(-1)])
        g2.eval()
        torch.manual_seed(NOISE_SEED)
        fwd['g_out_eval'] = summarize(g2(z), 8)
    fixture['forward'] = fwd

    watch.watch(tr.g)
    watch.watch(tr.target_g)
    torch.manual_seed(MG.RNG_SEED)
    fixture['steps'] = []
    for k in range(steps):
        logs = tr.train_batch(synthetic_images(batch, size, MG.IMG_SEED + k))
        entry = dict(logs)
        entry['g_l2'] = MG.total_l2(tr.g)
        entry['d_l2'] = MG.total_l2(tr.d)
        entry['target_g_l2'] = MG.total_l2(tr.target_g)
        entry['g_grad_l2'] = MG.total_l2(tr.g, grads=True)
        entry['d_grad_l2'] = MG.total_l2(tr.d, grads=True)
        fixture['steps'].append(entry)
        print(f'  {name} step {k + 1}: {logs}  ({time.time() - t0:.1f}s)', flush=True)
        if k == 0:
            fixture['after_step1'] = dict(d_grad=MG.net_summary(tr.d, grads=True), g_grad=MG.net_summary(tr.g, grads=True))
    fixture['final'] = dict(g=MG.net_summary(tr.g), d=MG.net_summary(tr.d), target_g=MG.net_summary(tr.target_g))
    fixture['rng_after'] = float(torch.rand(1))
    fixture['kink'] = dict(least_distance=watch.least, forwards=watch.forwards, margin=margin)
    assert watch.forwards == 3 + 2 * steps, watch.forwards
    assert watch.least >= margin, f'{name}: a sample {watch.least:.2e} from a kink; change the weight seed'
    path = os.path.join(HERE, f'{name}.json')
    with open(path, 'w') as f:
        json.dump(fixture, f, indent=None, separators=(',', ':'))
    print(f'wrote {path} ({os.path.getsize(path) / 1024:.0f} KB, kink distance {watch.least:.2e}, {time.time() - t0:.1f}s)')


def main():
    torch.set_num_threads(1)
    for n in sys.argv[1:] or list(CASES):
        run_case(n)


if __name__ == '__main__':
    main()
