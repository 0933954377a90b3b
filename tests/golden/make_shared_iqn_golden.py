#!/usr/bin/env python3
"""Generate the shared-filter IQN trainer fixtures (tests/golden/shared_iqn_*.json) by running the REFERENCE implementation.

Like make_shared_golden.py (whose helpers it reuses): what is executed is the reference's own, unmodified
``tartangan.trainers.shared.iqn.IQNTrainer`` -- ``build_models()`` and ``train_batch()`` -- with
``tartangan.models.shared.pluggan.SharedGenerator`` / ``SharedIQNDiscriminator``; the fixtures hold recorded numbers only.  The
files are named ``shared_iqn_*`` so that ``conftest.golden_cases()`` (``c<size>...``) does not pick them up.

One quirk of the reference is pinned by the third case: its trainer builds a ``d_output_factory`` bound to ``--norm`` and
``--activation`` and then passes the bare ``IQNDiscriminatorOutput`` (trainers/shared/iqn.py:63-66, 80-84), so the head holds a
BatchNorm2d and a LeakyReLU(0.2) under ``--norm id`` too (state keys ``to_output.activation.0.*``; BatchNorm at batch 2).

The host random stream of a step is z, taus of D(real), taus of D(fake), z, taus of D(fake) in the G phase.  After the run the
stream is replayed from the seed in that order; the replay must leave the generator where the reference's run left it
(``rng_after``), and the heads of the tau draws it made are recorded (``taus``): the taus' share of the stream.

The tests hold BOTH steps of a case to 1e-4.  As for the shared_* fixtures, each case also runs this package's trainer over the
CPU emulator (tests/shared_iqn_cases.SharedIQNEmulator) from the same state -- paired and unpaired, with the fused and with the
composed head -- and asserts that every loss and L2 of both steps agrees with the reference's to ROOM (3e-5): if a weight seed
lands on an edge, change the seed, not the tolerance.

Usage:  python tests/golden/make_shared_iqn_golden.py [case ...]
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

from make_shared_golden import ROOM, load_procedural, run_steps  # noqa: E402
from oracle.procedural import summarize, synthetic_images  # noqa: E402
from shared_iqn_cases import SharedIQNEmulator  # noqa: E402
from tartangan.models.pluggan import GAN_CONFIGS  # noqa: E402
from tartangan.trainers.shared.iqn import IQNTrainer  # noqa: E402

CASES = {
    # name: (config, batch, steps, flags, weight seed).  Seeds 11..30 were tried for the last two cases (--sweep); the emulated
    # engine's deviation ranged from 9e-7 to 1e-2 on '32:2' (an edge in step 1 shows in step 2's generator gradient) and from 9e-7
    # to 5e-4 under norm='id'; these are the quietest of each.  Seed 17 of the first case is shared_c16_b4's; it is quiet here too.
    'shared_iqn_c16_b4': ('16', 4, 2, {}, 17),
    'shared_iqn_c32a2_b4': ('32:2', 4, 2, {}, 12),
    'shared_iqn_c32_b2_id': ('32', 2, 2, dict(norm='id'), 16),
}
SEEDS_TRIED = range(11, 31)


def build_trainer(config, batch, flags, init_seed=0):
    t = object.__new__(IQNTrainer)          # skip Trainer.__init__ (filesystem side effects only)
    t.args = MG.make_args(config, batch, **flags)
    torch.manual_seed(init_seed)
    with contextlib.redirect_stdout(io.StringIO()):
        t.build_models()
    return t


def replay_host_stream(batch, latent_dims, q, steps):
    """The draws of ``steps`` steps from the seed, in the reference's order -> (heads of every tau draw, the next torch.rand(1))."""
    torch.manual_seed(MG.RNG_SEED)
    heads = []
    for _ in range(steps):
        step = []
        for kind in ('z', 'tau', 'tau', 'z', 'tau'):
            if kind == 'z':
                torch.randn(batch, latent_dims)
            else:
                step.append([float(v) for v in torch.rand(q * batch, 1).reshape(-1)[:4]])
        heads.append(step)
    return heads, float(torch.rand(1))


def emulated_engine_deviation(fixture):
    """Largest relative difference between this package's trainer over the CPU emulator and the recorded reference run."""
    from shared_iqn_cases import load_procedural as load_engine, shared_iqn_trainer
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(SharedIQNEmulator())
    before = os.environ.get('TG_IQN_FUSED_HEAD')
    try:
        worst = (0.0, 'nowhere')
        for fused in ('1', '0'):
            os.environ['TG_IQN_FUSED_HEAD'] = fused
            for pairs in (True, False):          # with and without the shared passes (functional.Pair): other summation orders
                tr = shared_iqn_trainer(fixture, 'cpu', pair_d=pairs, pair_g=pairs)
                load_engine(tr, fixture)
                for k, got in run_steps(tr, fixture['batch'], fixture['size'], len(fixture['steps'])):
                    for key, ref in fixture['steps'][k].items():
                        dev = abs(got[key] - ref) / max(abs(ref), 1e-12)
                        worst = max(worst, (dev, f'step {k + 1} {key} ({"paired" if pairs else "unpaired"}, '
                                                 f'{"fused" if fused == "1" else "composed"} head)'))
    finally:
        backend._set_backend_for_testing(prev)
        if before is None:
            os.environ.pop('TG_IQN_FUSED_HEAD', None)
        else:
            os.environ['TG_IQN_FUSED_HEAD'] = before
    return worst


def run_case(name, weight_seed=None, write=True):
    """``weight_seed`` / ``write=False``: try another seed without touching the fixture (-> the emulated engine's deviation)."""
    config, batch, steps, flags, case_seed = CASES[name]
    weight_seed = case_seed if weight_seed is None else weight_seed
    t0 = time.time()
    tr = build_trainer(config, batch, flags)
    size = tr.g.max_size
    fixture = dict(
        case=name, config=config.split(':')[0], flags=flags, attention=list(GAN_CONFIGS[config].attention or ()), trainer='shared_iqn',
        batch=batch, size=size, weight_seed=weight_seed, rng_seed=MG.RNG_SEED, img_seed=MG.IMG_SEED,
        torch_version=torch.__version__, num_threads=torch.get_num_threads(),
        source='reference tartangan v0.4.0 code under torch %s CPU fp32' % torch.__version__,
        blocks=list(tr.gan_config.blocks), latent_dims=tr.gan_config.latent_dims,
        num_quantiles=tr.d.to_output.iqn.num_quantiles,
        head_modules=[type(m).__name__ for m in tr.d.to_output.activation],
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
        fwd = dict(g_out=summarize(g_out, 8))
        torch.manual_seed(555)
        p, loss = d2(synthetic_images(batch, size, MG.IMG_SEED), targets=torch.ones(batch, 1))
        fwd['d_real'], fwd['d_real_loss'] = [float(v) for v in p.reshape(-1)], float(loss)
        p, loss = d2(g_out, targets=torch.zeros(batch, 1))
        fwd['d_fake'], fwd['d_fake_loss'] = [float(v) for v in p.reshape(-1)], float(loss)
        fixture['forward'] = fwd

    fixture['steps'] = []
    for k, entry in run_steps(tr, batch, size, steps, name, t0):
        fixture['steps'].append(entry)
        if k == 0:
            fixture['after_step1'] = dict(d_grad=MG.net_summary(tr.d, grads=True), g_grad=MG.net_summary(tr.g, grads=True))
    fixture['final'] = dict(g=MG.net_summary(tr.g), d=MG.net_summary(tr.d), target_g=MG.net_summary(tr.target_g))
    fixture['rng_after'] = float(torch.rand(1))
    heads, replay_after = replay_host_stream(batch, tr.gan_config.latent_dims, fixture['num_quantiles'], steps)
    assert replay_after == fixture['rng_after'], 'the replayed draw order is not the reference run\'s'
    fixture['taus'] = heads
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
    args = sys.argv[1:]
    if args and args[0] == '--sweep':        # the emulated engine's deviation per seed, nothing written
        for n in args[1:] or list(CASES):
            for seed in SEEDS_TRIED:
                print(n, seed, *run_case(n, seed, write=False), flush=True)
        return
    for n in args or list(CASES):
        run_case(n)


if __name__ == '__main__':
    main()
