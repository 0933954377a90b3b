"""Time the CNN trainer's step with --spectral-norm gd against the stock step, and the batched kernels against the per-layer one.

    python tools/bench_spectral.py [--steps 20] [--warmup 10] [--rounds 3] [--reps 200] [--out profiles/spectral_step]

Steps (config 128:3, batch 64), each eager and replayed from HIP graphs: the stock step; the step with --spectral-norm gd on the
batched route (spectral scopes: tg_sn_batch_fwd / _bwd); the same step with --spectral-per-layer (no scopes: every forward iterates
and normalises layer by layer, tg_sn_power_iter + its glue).  The trainers are built and warmed up first; then ``--rounds`` rounds
time ``--steps`` steps of each in turn, so that a drifting clock or a busy host hits all alike.  Wall time per step ending in the
step's own loss read-back (a device synchronise); median / min / max over all rounds.

Kernels alone, for the D and G tables of 128:3 and 128big: one tg_sn_batch_fwd (with update) and one tg_sn_batch_bwd per network
against the sum of one tg_sn_power_iter call per layer (which gives sigma only: the per-layer route spends six more launches per
layer on the quotient), device events around ``--reps`` back-to-back calls after a warm-up, median of five such windows."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]


def make(graphs, config='128', attention=(3,), batch=64, **flags):
    from tartangan_amd.models.pluggan import GAN_CONFIGS
    from tartangan_amd.trainers.cnn import CNNTrainer
    cfg = GAN_CONFIGS[config]._replace(attention=attention)
    tr = CNNTrainer(CNNTrainer.default_args(config=cfg, batch_size=batch, device='cuda', **flags))
    torch.manual_seed(0)
    tr.build_models()
    if graphs:
        tr.enable_graphs()
    return tr


def window(fn, reps):
    """ms per call: device events around ``reps`` back-to-back calls; median of five windows after a warm-up window."""
    out = []
    for w in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        if w:
            out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), min(out), max(out)


def kernel_rows(reps):
    from tartangan_amd import backend, functional as TF
    K = backend.get()
    rows = []
    for config, attention in (('128', (3,)), ('128big', ())):
        tr = make(False, config, attention, batch=4, spectral_norm='gd')
        for name in ('d', 'g'):
            store = TF.spectral_store(getattr(tr, name))
            layers = [(m.weight_orig.detach(), m.weight_u, m.weight_v, m.weight_orig.shape[0], m.weight_orig[0].numel()) for m in store.layers]

            def per_layer():
                for W, u, v, r, c in layers:
                    K.sn_power_iter(W, u, v, None, r, c, 1, 1e-12)
            for what, fn in (('tg_sn_batch_fwd', lambda: store.materialize(True)), ('tg_sn_batch_bwd', store.backward),
                             ('tg_sn_power_iter x layers', per_layer)):
                med, lo, hi = window(fn, reps)
                rows.append(dict(config=config, net=name, layers=len(layers), floats=int(store.w_sn.numel()), call=what,
                                 median_ms=med, min_ms=lo, max_ms=hi))
        del tr
        torch.cuda.empty_cache()
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--reps', type=int, default=200)
    p.add_argument('--out', default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), 'bench_spectral needs the GPU (no CPU timing)'
    from oracle.procedural import synthetic_images
    np.random.seed(0)
    kinds = (('stock', {}), ('sn batched', dict(spectral_norm='gd')), ('sn per-layer', dict(spectral_norm='gd', spectral_per_layer=True)))
    arms = {(name, mode): make(mode == 'graph replay', **flags) for mode in ('eager', 'graph replay') for name, flags in kinds}
    imgs = synthetic_images(64, 128, 1).cuda()
    failed = {}
    for key, tr in arms.items():
        try:
            for _ in range(args.warmup):
                tr.train_batch(imgs)
        except Exception as exc:          # (the per-layer route was never replayed from a graph before: report, do not hide)
            failed[key] = repr(exc)[:300]
    torch.cuda.synchronize()
    times, logs = {k: [] for k in arms if k not in failed}, {}
    for _ in range(args.rounds):
        for key in times:
            tr = arms[key]
            for _ in range(args.steps):
                t0 = time.perf_counter()
                logs[key] = tr.train_batch(imgs)               # ends in the loss read-back: a synchronise
                times[key].append((time.perf_counter() - t0) * 1e3)
    result = {'device': torch.cuda.get_device_name(0), 'steps_per_arm': args.steps * args.rounds, 'arms': [], 'failed': {' / '.join(k): v for k, v in failed.items()}}
    lines = []
    for (name, mode), ts in times.items():
        row = dict(trainer=name, mode=mode, median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts),
                   replaying=getattr(arms[(name, mode)], '_graphs', None) is not None, last_losses=logs[(name, mode)])
        result['arms'].append(row)
        lines.append('%-12s 128:3 batch 64  %-12s median %8.3f ms / step (min %8.3f max %8.3f)%s'
                     % (name, mode, row['median_ms'], row['min_ms'], row['max_ms'], '' if mode == 'eager' or row['replaying'] else '  NOT replaying'))
    for key, why in failed.items():
        lines.append('%-12s 128:3 batch 64  %-12s FAILED: %s' % (key[0], key[1], why))
    med = {k: statistics.median(v) for k, v in times.items()}
    for mode in ('eager', 'graph replay'):
        if ('sn batched', mode) in med and ('stock', mode) in med:
            a, b = med[('sn batched', mode)], med[('stock', mode)]
            lines.append('cost of spectral norm (batched - stock), %s: %+.3f ms / step (%.3f x)' % (mode, a - b, a / b))
        if ('sn batched', mode) in med and ('sn per-layer', mode) in med:
            a, b = med[('sn batched', mode)], med[('sn per-layer', mode)]
            lines.append('batched - per-layer, %s: %+.3f ms / step (%.3f x)' % (mode, a - b, a / b))
    arms.clear()
    torch.cuda.empty_cache()
    result['kernels'] = kernel_rows(args.reps)
    for r in result['kernels']:
        lines.append('%-7s %s %2d layers %9d floats  %-26s median %8.4f ms (min %8.4f max %8.4f)'
                     % (r['config'], r['net'], r['layers'], r['floats'], r['call'], r['median_ms'], r['min_ms'], r['max_ms']))
    print('\n'.join(lines))
    if args.out:
        with open(args.out + '.json', 'w') as f:
            json.dump(result, f, indent=1)
        with open(args.out + '.txt', 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
