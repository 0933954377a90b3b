#!/usr/bin/env python3
"""Generate the shared-filter trainer fixtures (tests/golden/shared_*.json) by running the REFERENCE implementation.

Like make_scene_golden.py (and make_golden.py, whose inert third-party stand-ins, argument namespace and summaries it reuses):
what is executed is the reference's own, unmodified ``tartangan.trainers.shared.cnn.CNNTrainer`` -- ``build_models()`` and
``train_batch()`` -- with ``tartangan.models.shared.pluggan.SharedGenerator`` / ``SharedDiscriminator``; the fixtures hold
recorded numbers only.  The files are named ``shared_*`` so that ``conftest.golden_cases()`` (``c<size>...``) does not pick them up.

The tests hold BOTH steps of a case to 1e-4.  With beta1 = 0 Adam moves every element by lr * sign(gradient) in its first step,
so an element whose step-1 gradient is zero up to rounding may move the other way in another implementation, and LeakyReLU /
BatchNorm have knife edges of their own.  Each case therefore also runs this package's trainer over the CPU emulator
(tests/shared_cases.SharedEmulator), from the same state, with and without its shared passes, and asserts that every loss and L2 of both steps agrees with the
reference's to ROOM (3e-5): if a weight seed lands on an edge, change the seed, not the tolerance.

Usage:  python tests/golden/make_shared_golden.py [case ...]
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

from oracle.procedural import summarize, synthetic_images  # noqa: E402
from shared_cases import SharedEmulator, shared_state  # noqa: E402
from tartangan.models.pluggan import GAN_CONFIGS  # noqa: E402
from tartangan.trainers.shared.cnn import CNNTrainer  # noqa: E402

CASES = {
    # name: (config, batch, steps, flags, weight seed).  Seeds 11..30 were tried per case; the emulated engine's deviation ranged
    # from 2e-7 to 2e-2 (an edge in step 1 shows in step 2's generator gradient); these are the quietest of each case.
    'shared_c16_b4': ('16', 4, 2, {}, 17),
    'shared_c32a2_b4': ('32:2', 4, 2, {}, 27),
    'shared_c64_b2_id': ('64', 2, 2, dict(norm='id'), 27),
}
ROOM = 3e-5            # what the emulated engine may be off from the reference on any recorded loss / L2 (the tests assert 1e-4)


def build_trainer(config, batch, flags, init_seed=0):
    t = object.__new__(CNNTrainer)          # skip Trainer.__init__ (filesystem side effects only)
    t.args = MG.make_args(config, batch, **flags)
    torch.manual_seed(init_seed)
    with contextlib.redirect_stdout(io.StringIO()):
        t.build_models()
    return t


def load_procedural(tr, weight_seed):
    tr.g.load_state_dict(shared_state(tr.g.state_dict(), weight_seed))
    tr.target_g.load_state_dict(shared_state(tr.target_g.state_dict(), weight_seed + 1))
    tr.d.load_state_dict(shared_state(tr.d.state_dict(), weight_seed + 2))


def run_steps(tr, batch, size, steps, name=None, t0=None):
    torch.manual_seed(MG.RNG_SEED)
    out = []
    for k in range(steps):
        logs = tr.train_batch(synthetic_images(batch, size, MG.IMG_SEED + k))
        entry = dict(logs)
        entry['g_l2'] = MG.total_l2(tr.g)
        entry['d_l2'] = MG.total_l2(tr.d)
        entry['target_g_l2'] = MG.total_l2(tr.target_g)
        entry['g_grad_l2'] = MG.total_l2(tr.g, grads=True)
        entry['d_grad_l2'] = MG.total_l2(tr.d, grads=True)
        out.append(entry)
        if name:
            print(f'  {name} step {k + 1}: {logs}  ({time.time() - t0:.1f}s)', flush=True)
        yield k, entry


def emulated_engine_deviation(fixture):
    """Largest relative difference between this package's trainer over the CPU emulator and the recorded reference run."""
    from shared_cases import load_procedural as load_engine, shared_trainer
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(SharedEmulator())
    try:
        worst = (0.0, 'nowhere')
        for pairs in (True, False):          # with and without the shared passes (functional.Pair): other summation orders
            tr = shared_trainer(fixture, 'cpu', pair_d=pairs, pair_g=pairs)
            load_engine(tr, fixture)
            for k, got in run_steps(tr, fixture['batch'], fixture['size'], len(fixture['steps'])):
                for key, ref in fixture['steps'][k].items():
                    dev = abs(got[key] - ref) / max(abs(ref), 1e-12)
                    worst = max(worst, (dev, f'step {k + 1} {key} ({"paired" if pairs else "unpaired"})'))
    finally:
        backend._set_backend_for_testing(prev)
    return worst


def run_case(name, weight_seed=None, write=True):
    """``weight_seed`` / ``write=False``: try another seed without touching the fixture (-> the emulated engine's deviation)."""
    config, batch, steps, flags, case_seed = CASES[name]
    weight_seed = case_seed if weight_seed is None else weight_seed
    t0 = time.time()
    tr = build_trainer(config, batch, flags)
    size = tr.g.max_size
    fixture = dict(
        case=name, config=config.split(':')[0], flags=flags, attention=list(GAN_CONFIGS[config].attention or ()), trainer='shared',
        batch=batch, size=size, weight_seed=weight_seed, rng_seed=MG.RNG_SEED, img_seed=MG.IMG_SEED,
        torch_version=torch.__version__, num_threads=torch.get_num_threads(),
        source='reference tartangan v0.4.0 code under torch %s CPU fp32' % torch.__version__,
        blocks=list(tr.gan_config.blocks), latent_dims=tr.gan_config.latent_dims,
    )
    fixture['default_init'] = dict(
        g_l2=MG.total_l2(tr.g), target_g_l2=MG.total_l2(tr.target_g), d_l2=MG.total_l2(tr.d),
        g=MG.net_summary(tr.g, n_samples=2), d=MG.net_summary(tr.d, n_samples=2),
    )
    load_procedural(tr, weight_seed)
    fixture['n_params'] = dict(g=sum(p.numel() for p in tr.g.parameters()), d=sum(p.numel() for p in tr.d.parameters()),
                               g_tensors=len(list(tr.g.parameters())), d_tensors=len(list(tr.d.parameters())))
    fixture['state_keys'] = dict(g=list(tr.g.state_dict().keys()), d=list(tr.d.state_dict().keys()))
    fixture['param_names'] = dict(g=[n for n, _ in tr.g.named_parameters()], d=[n for n, _ in tr.d.named_parameters()])

    with torch.no_grad():
        g2, d2 = copy.deepcopy(tr.g), copy.deepcopy(tr.d)
        z = torch.randn(batch, tr.gan_config.latent_dims, generator=torch.Generator().manual_seed(99))
        g_out = g2(z)
        fixture['forward'] = dict(g_out=summarize(g_out, 8),
                                  d_real=[float(v) for v in d2(synthetic_images(batch, size, MG.IMG_SEED)).reshape(-1)],
                                  d_fake=[float(v) for v in d2(g_out).reshape(-1)])

    fixture['steps'] = []
    for k, entry in run_steps(tr, batch, size, steps, name, t0):
        fixture['steps'].append(entry)
        if k == 0:
            fixture['after_step1'] = dict(d_grad=MG.net_summary(tr.d, grads=True), g_grad=MG.net_summary(tr.g, grads=True))
    fixture['final'] = dict(g=MG.net_summary(tr.g), d=MG.net_summary(tr.d), target_g=MG.net_summary(tr.target_g))
    fixture['rng_after'] = float(torch.rand(1))
    dev, where = emulated_engine_deviation(fixture)
    fixture['emulated_engine'] = dict(worst_relative_deviation=dev, where=where, room=ROOM)
    if not write:
        return dev, where
    assert dev <= ROOM, f'{name}: the emulated engine is {dev:.2e} off at {where}; change the weight seed'
    path = os.path.join(HERE, f'{name}.json')
    with open(path, 'w') as f:
        json.dump(fixture, f, indent=None, separators=(',', ':'))
    print(f'wrote {path} ({os.path.getsize(path) / 1024:.0f} KB, emulated engine off by {dev:.2e} at {where}, {time.time() - t0:.1f}s)')


def main():
    torch.set_num_threads(1)
    for n in sys.argv[1:] or list(CASES):
        run_case(n)


if __name__ == '__main__':
    main()
