#!/usr/bin/env python3
"""Generate the text trainer fixtures (tests/golden/text_*.json) by running the REFERENCE implementation.

Like make_info_golden.py (and make_golden.py, whose inert third-party stand-ins, argument namespace and summaries it reuses, plus
one stand-in for ``torchtext``): what is executed is the reference's own, unmodified ``tartangan.trainers.text_cnn.TextCNNTrainer``
-- ``build_models()`` and ``train_batch()``; the fixtures hold recorded numbers only.  ``prepare_dataset`` (a pickled DataFrame and
torchtext) is bypassed by building what it builds: ``SkipGram(vocab, E, sparse=True, padding_idx=0)`` and its SGD optimiser at
``lr_d``.  Weights come from ``procedural_state`` (the padding row of both tables zeroed, as nn.Embedding initialises it); documents
from a seeded ``RandomState``, with zero tails in some rows so that ``padding_idx`` is hit.

The step draws from TWO host streams: numpy's global generator (window offsets) and torch's default generator (negatives, then the
latents of both phases).  Both are seeded before the steps, both seeds are recorded, and ``rng_after`` holds the next value of each.

Each case also runs this package's trainer over the CPU emulator (tests/text_cases.TextEmulator) from the same state and asserts that
every recorded loss and L2 of every step agrees with the reference's to ROOM (3e-5): if a weight seed lands on an Adam or LeakyReLU
edge, change the seed, not the tolerance (``--search case`` lists the deviation per seed).

Usage:  python tests/golden/make_text_golden.py [case ...]  |  --search case [first_seed end_seed]
"""
import contextlib
import io
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (installs the stand-ins, puts the reference on sys.path)

MG._InertFinder.ROOTS = MG._InertFinder.ROOTS + ('torchtext',)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import text_cases as TC  # noqa: E402
from oracle.procedural import procedural_state  # noqa: E402
from tartangan.models.text import SkipGram  # noqa: E402
from tartangan.trainers.text_cnn import TextCNNTrainer  # noqa: E402

CASES = {
    # name: (config, batch, steps, flags, weight seed)
    'text_c16_e8_b4': ('16', 4, 3, dict(embedding_dims=8, context=3, vocab=23, pretrain_embedding=2), 17),
    'text_c32_e16_b4_id': ('32', 4, 2, dict(embedding_dims=16, context=2, vocab=50, pretrain_embedding=0, norm='id'), 17),
    'text_c16_e64_b2_elu_nogp': ('16', 2, 2, dict(embedding_dims=64, context=1, vocab=12, pretrain_embedding=0, activation='elu',
                                                  grad_penalty=0.), 17),
}
ROOM = 3e-5
NP_SEED = 2468
OWN = ('embedding_dims', 'context', 'vocab', 'pretrain_embedding')


def build_trainer(config, batch, flags, init_seed=0):
    t = object.__new__(TextCNNTrainer)          # skip Trainer.__init__ (filesystem side effects only)
    t.args = MG.make_args(config, batch, **{k: v for k, v in flags.items() if k not in OWN})
    for k in OWN:
        setattr(t.args, k, flags[k])
    torch.manual_seed(init_seed)
    with contextlib.redirect_stdout(io.StringIO()):
        t.build_models()
    # what prepare_dataset builds (text_cnn.py:149-156)
    t.embedding = SkipGram(flags['vocab'], flags['embedding_dims'], sparse=True, padding_idx=0)
    t.optimizer_embedding = torch.optim.SGD(t.embedding.parameters(), lr=t.args.lr_d)
    return t


def load_procedural(tr, weight_seed):
    tr.g.load_state_dict(procedural_state(tr.g.state_dict(), weight_seed))
    tr.target_g.load_state_dict(procedural_state(tr.target_g.state_dict(), weight_seed + 1))
    tr.d.load_state_dict(procedural_state(tr.d.state_dict(), weight_seed + 2))
    state = procedural_state(tr.embedding.state_dict(), weight_seed + 3)
    for v in state.values():
        v[0] = 0.
    tr.embedding.load_state_dict(state)


def run_steps(tr, fixture, name=None, t0=None):
    torch.manual_seed(fixture['rng_seed'])
    np.random.seed(fixture['np_seed'])
    for k in range(fixture['n_steps']):
        logs = tr.train_batch(TC.documents(fixture, k))
        if name:
            print(f'  {name} step {k + 1}: {logs}  ({time.time() - t0:.1f}s)', flush=True)
        yield k, TC.step_entry(tr, logs)


def emulated_engine_deviation(fixture):
    """Largest relative difference between this package's trainer over the CPU emulator and the recorded reference run."""
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(TC.TextEmulator())
    try:
        worst = (0.0, 'nowhere')
        tr = TC.text_trainer(fixture, 'cpu')
        TC.load_procedural(tr, fixture)
        for k, got in run_steps(tr, fixture):
            for key, ref in fixture['steps'][k].items():
                if key in got:
                    dev = abs(got[key] - ref) / max(abs(ref), 1e-12) if ref else abs(got[key])
                    worst = max(worst, (dev, f'step {k + 1} {key}'))
        after = dict(torch=float(torch.rand(1)), numpy=float(np.random.rand()))
        assert after == fixture['rng_after'], (after, fixture['rng_after'])
    finally:
        backend._set_backend_for_testing(prev)
    return worst


def run_case(name, weight_seed=None, write=True):
    config, batch, steps, flags, case_seed = CASES[name]
    weight_seed = case_seed if weight_seed is None else weight_seed
    t0 = time.time()
    tr = build_trainer(config, batch, flags)
    fixture = dict(
        case=name, config=config, flags=flags, trainer='text', batch=batch, size=tr.g.max_size, n_steps=steps,
        weight_seed=weight_seed, rng_seed=MG.RNG_SEED, np_seed=NP_SEED, doc_seed=MG.IMG_SEED,
        torch_version=torch.__version__, numpy_version=np.__version__, num_threads=torch.get_num_threads(),
        source='reference tartangan v0.4.0 code under torch %s CPU fp32' % torch.__version__,
        blocks=list(tr.gan_config.blocks), latent_dims=tr.gan_config.latent_dims,
    )
    load_procedural(tr, weight_seed)
    fixture['state_keys'] = dict(g=list(tr.g.state_dict().keys()), d=list(tr.d.state_dict().keys()),
                                 embedding=list(tr.embedding.state_dict().keys()))
    fixture['steps'] = [entry for _, entry in run_steps(tr, fixture, name, t0)]
    fixture['rng_after'] = dict(torch=float(torch.rand(1)), numpy=float(np.random.rand()))
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
    if sys.argv[1:2] == ['--search']:
        lo, hi = (int(v) for v in sys.argv[3:5]) if len(sys.argv) > 4 else (11, 31)
        for seed in range(lo, hi):
            print(seed, *run_case(sys.argv[2], weight_seed=seed, write=False), flush=True)
        return
    for n in sys.argv[1:] or list(CASES):
        run_case(n)


if __name__ == '__main__':
    main()
