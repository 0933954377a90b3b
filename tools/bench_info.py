"""Time the InfoGAN trainer's step against the stock CNN step on the GPU.

    python tools/bench_info.py [--steps 30] [--warmup 10] [--rounds 3] [--out profiles/info_step]

``trainers.info.InfoTrainer.train_batch`` (default flags: 10 categorical, 5 continuous codes) and ``trainers.cnn.CNNTrainer.train_batch``
at config 128:3, batch 64, eager and replayed from HIP graphs.  The four trainers are built and warmed up first; then ``--rounds``
rounds time ``--steps`` steps of each in turn, so that a drifting clock or a busy host hits all four alike.  Wall time per step
ending in the step's own loss read-back (a device synchronise); median / min / max over all rounds."""
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


def make(cls, graphs, config='128', attention=(3,), batch=64):
    from tartangan_amd.models.pluggan import GAN_CONFIGS
    cfg = GAN_CONFIGS[config]._replace(attention=attention)
    tr = cls(cls.default_args(config=cfg, batch_size=batch, device='cuda'))
    torch.manual_seed(0)
    tr.build_models()
    if graphs:
        tr.enable_graphs()
    return tr


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--steps', type=int, default=30)
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--out', default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), 'bench_info needs the GPU (no CPU timing)'
    from oracle.procedural import synthetic_images
    from tartangan_amd.trainers.cnn import CNNTrainer
    from tartangan_amd.trainers.info import InfoTrainer
    np.random.seed(0)
    arms = {(name, mode): make(cls, mode == 'graph replay')
            for mode in ('eager', 'graph replay') for name, cls in (('cnn', CNNTrainer), ('info', InfoTrainer))}
    imgs = synthetic_images(64, 128, 1).cuda()
    for tr in arms.values():
        for _ in range(args.warmup):
            tr.train_batch(imgs)
    torch.cuda.synchronize()
    times, logs = {k: [] for k in arms}, {}
    for _ in range(args.rounds):
        for key, tr in arms.items():
            for _ in range(args.steps):
                t0 = time.perf_counter()
                logs[key] = tr.train_batch(imgs)               # ends in the loss read-back: a synchronise
                times[key].append((time.perf_counter() - t0) * 1e3)
    result, lines = {'device': torch.cuda.get_device_name(0), 'steps_per_arm': args.steps * args.rounds, 'arms': []}, []
    for (name, mode), ts in times.items():
        row = dict(trainer=name, mode=mode, median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts),
                   replaying=getattr(arms[(name, mode)], '_graphs', None) is not None, last_losses=logs[(name, mode)])
        result['arms'].append(row)
        lines.append('%-4s 128:3 batch 64  %-12s median %8.3f ms / step (min %8.3f max %8.3f)'
                     % (name, mode, row['median_ms'], row['min_ms'], row['max_ms']))
    for mode in ('eager', 'graph replay'):
        a, b = (statistics.median(times[(n, mode)]) for n in ('info', 'cnn'))
        lines.append('info - cnn, %s: %+.3f ms / step (%.3f x)' % (mode, a - b, a / b))
    print('\n'.join(lines))
    if args.out:
        with open(args.out + '.json', 'w') as f:
            json.dump(result, f, indent=1)
        with open(args.out + '.txt', 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
