"""Time the shared-filter IQN trainer's step with the fused and with the composed head, and the shared CNN step beside them.

    python tools/bench_shared_iqn.py [--steps 30] [--warmup 10] [--rounds 5] [--out profiles/shared_iqn_step]

``trainers.shared.iqn.IQNTrainer.train_batch`` at config 128:3, batch 64, with the fused head (the default) and with
``TG_IQN_FUSED_HEAD=0`` (the parent's composed head), and ``trainers.shared.cnn.CNNTrainer.train_batch``; each arm in a fresh child
process of its own, eager and replayed from HIP graphs.  A child builds and warms up its two trainers, then ``--rounds`` rounds
time ``--steps`` steps of each in turn.  Wall time per step ending in the step's own loss read-back (a device synchronise).
Reported per arm and mode: the median over all steps, min / max, and the spread of the per-round medians (largest - smallest):
two arms whose medians differ by less than that spread are not told apart by this tool.  Also: entry-point calls per eager step
(every ``tg_*`` call that takes a stream; a call may be more than one launch), and how many of them belong to the head."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

ARMS = {'shared iqn, fused head': ('iqn', '1'), 'shared iqn, composed head': ('iqn', '0'), 'shared cnn': ('cnn', '1')}
HEAD_CALLS = ('iqn_head_fwd', 'iqn_head_bwd')
COMPOSED_HEAD_CALLS = ('gemm', 'mul', 'repeat_rows', 'repeat_rows_groups', 'sum_reps', 'sum_reps_groups', 'iqn_cos_embed', 'iqn_loss',
                       'iqn_loss_groups', 'tanh_fwd', 'tanh_bwd', 'scale_dev', 'channel_sum')


class Counting:
    """The HIP backend with every call counted by name."""

    def __init__(self, inner):
        self._inner, self.calls = inner, {}

    def __getattr__(self, name):
        fn = getattr(self._inner, name)
        if not callable(fn):
            return fn

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


def child(kind, args):
    import torch
    from oracle.procedural import synthetic_images
    from tartangan_amd import backend
    from tartangan_amd.models.pluggan import GAN_CONFIGS
    from tartangan_amd.trainers.shared.cnn import CNNTrainer
    from tartangan_amd.trainers.shared.iqn import IQNTrainer
    assert torch.cuda.is_available(), 'bench_shared_iqn needs the GPU (no CPU timing)'
    cls = {'iqn': IQNTrainer, 'cnn': CNNTrainer}[kind]
    cfg = GAN_CONFIGS['128']._replace(attention=(3,))
    trainers = {}
    for mode in ('eager', 'graph replay'):
        tr = cls(cls.default_args(config=cfg, batch_size=64, device='cuda'))
        torch.manual_seed(0)
        tr.build_models()
        if mode == 'graph replay':
            tr.enable_graphs()
        trainers[mode] = tr
    imgs = synthetic_images(64, 128, 1).cuda()
    for tr in trainers.values():
        for _ in range(args.warmup):
            tr.train_batch(imgs)
    counting = Counting(backend.get())          # one eager step with every entry-point call counted
    prev = backend._set_backend_for_testing(counting)
    trainers['eager'].train_batch(imgs)
    backend._set_backend_for_testing(prev)
    streamed = {n[3:] for n, (ret, params) in backend.parse_header().items() if params and params[-1] == ('void*', 'stream')}
    calls = {n: c for n, c in counting.calls.items() if n in streamed}
    torch.cuda.synchronize()
    out = {'calls_per_step': sum(calls.values()), 'head_calls': {n: calls.get(n, 0) for n in HEAD_CALLS + COMPOSED_HEAD_CALLS},
           'device': torch.cuda.get_device_name(0), 'modes': {}}
    times = {mode: [[] for _ in range(args.rounds)] for mode in trainers}
    for r in range(args.rounds):
        for mode, tr in trainers.items():
            for _ in range(args.steps):
                t0 = time.perf_counter()
                logs = tr.train_batch(imgs)               # ends in the loss read-back: a synchronise
                times[mode][r].append((time.perf_counter() - t0) * 1e3)
            out['modes'].setdefault(mode, {})['last_losses'] = logs
    for mode, rounds in times.items():
        flat = [t for r in rounds for t in r]
        medians = [statistics.median(r) for r in rounds]
        out['modes'][mode].update(median_ms=statistics.median(flat), min_ms=min(flat), max_ms=max(flat), round_medians_ms=medians,
                                  spread_ms=max(medians) - min(medians),
                                  replaying=getattr(trainers[mode], '_graphs', None) is not None)
    print('RESULT ' + json.dumps(out))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--steps', type=int, default=30)
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--out', default=None)
    p.add_argument('--child', default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.child:
        return child(args.child, args)
    result, lines = {'steps_per_arm': args.steps * args.rounds, 'warmup': args.warmup, 'rounds': args.rounds, 'arms': {}}, []
    for arm, (kind, fused) in ARMS.items():          # one fresh process per arm, one at a time
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', kind, '--steps', str(args.steps), '--warmup', str(args.warmup),
                            '--rounds', str(args.rounds)], env=dict(os.environ, TG_IQN_FUSED_HEAD=fused), cwd=REPO,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        found = [line for line in r.stdout.splitlines() if line.startswith('RESULT ')]
        if r.returncode != 0 or not found:
            raise SystemExit(f'{arm}: the child process failed ({r.returncode})\n{r.stdout[-3000:]}')
        result['arms'][arm] = json.loads(found[-1][7:])
        print(f'measured {arm}', flush=True)
    for arm, res in result['arms'].items():
        for mode, m in res['modes'].items():
            lines.append('%-26s 128:3 batch 64  %-12s median %8.3f ms / step (min %8.3f max %8.3f; round medians spread %.3f)'
                         % (arm, mode, m['median_ms'], m['min_ms'], m['max_ms'], m['spread_ms']))
    for arm, res in result['arms'].items():
        head = {n: c for n, c in res['head_calls'].items() if c}
        lines.append('%-26s %4d entry-point calls per eager step; of the head\'s kinds: %s' % (arm, res['calls_per_step'], head))
    fused, composed, cnn = (result['arms'][a]['modes'] for a in ARMS)
    for mode in ('eager', 'graph replay'):
        spread = max(fused[mode]['spread_ms'], composed[mode]['spread_ms'])
        d = fused[mode]['median_ms'] - composed[mode]['median_ms']
        lines.append('fused - composed, %s: %+.3f ms / step (spread of the round medians %.3f: %s)'
                     % (mode, d, spread, 'no slower' if d <= spread else 'SLOWER'))
        lines.append('fused iqn - shared cnn, %s: %+.3f ms / step' % (mode, fused[mode]['median_ms'] - cnn[mode]['median_ms']))
    print('\n'.join(lines))
    if args.out:
        with open(args.out + '.json', 'w') as f:
            json.dump(result, f, indent=1)
        with open(args.out + '.txt', 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
