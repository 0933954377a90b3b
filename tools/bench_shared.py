"""Time the shared-filter family on the GPU: the bilinear x2 kernels against ATen, and the shared trainer's step.

    python tools/bench_shared.py [--iters 30] [--warmup 10] [--steps 20] [--out profiles/shared_step]

1. ``tg_bilinear_up2x_fwd`` / ``_bwd`` at (B*C, H) = (64*128, 64) and (64*64, 128) -- the last two generator blocks of a
   128-pixel model at batch 64 -- against ``F.interpolate(scale_factor=2, mode='bilinear', align_corners=True)`` and its
   backward on the same device, the two alternating.  HIP-event time per call, median / min / max, and achieved GB/s over the
   least traffic either direction needs: N floats on the small side, 4N on the large one, 5N * 4 bytes.
2. ``trainers.shared.cnn.CNNTrainer.train_batch`` at config 128:3, batch 64, eager and replayed from HIP graphs: wall time per
   step over ``--steps`` steps ending in the step's own loss read-back (a device synchronise), after warm-up steps.

The shader clock torch reports before and after is noted where the installation can read it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception as exc:          # no amdsmi binding in this installation
        return f'not available ({type(exc).__name__})'


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts, nbytes=None):
    med = statistics.median(ts)
    row = {'median_ms': med, 'min_ms': min(ts), 'max_ms': max(ts)}
    if nbytes is not None:
        row['GBps_at_median'] = nbytes / med / 1e6
    return row


def bench_up2x(K, BC, H, iters, warmup):
    W = H
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(1, BC, H, W, generator=gen).cuda()
    gy = torch.randn(1, BC, 2 * H, 2 * W, generator=gen).cuda()
    y, gx = torch.empty_like(gy), torch.empty_like(x)
    xa = x.clone().requires_grad_(True)
    ya = F.interpolate(xa, scale_factor=2, mode='bilinear', align_corners=True)

    def aten_bwd():
        return torch.autograd.grad(ya, xa, gy, retain_graph=True)[0]
    arms = {
        'native_fwd': lambda: K.bilinear_up2x_fwd(x, None, y, BC, H, W),
        'aten_fwd': lambda: F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True),
        'native_bwd': lambda: K.bilinear_up2x_bwd(gy, None, gx, BC, H, W),
        'aten_bwd': aten_bwd,
    }
    arms['native_fwd'](), arms['native_bwd']()
    diff = (float((y - arms['aten_fwd']()).abs().max() / y.abs().max()), float((gx - aten_bwd()).abs().max() / gx.abs().max()))
    for f in arms.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(iters):
        for k, f in arms.items():
            times[k].append(timed_once(f))
    nbytes = 5 * BC * H * W * 4
    row = {'BC': BC, 'H': H, 'W': W, 'least_traffic_bytes': nbytes, 'max_rel_diff_fwd': diff[0], 'max_rel_diff_bwd': diff[1]}
    row.update({k: stats(t, nbytes) for k, t in times.items()})
    return row


def bench_step(graphs, steps, warmup, config='128', attention=(3,), batch=64):
    from oracle.procedural import synthetic_images
    from tartangan_amd.models.pluggan import GAN_CONFIGS
    from tartangan_amd.trainers.shared.cnn import CNNTrainer
    cfg = GAN_CONFIGS[config]._replace(attention=attention)
    tr = CNNTrainer(CNNTrainer.default_args(config=cfg, batch_size=batch, device='cuda'))
    torch.manual_seed(0)
    tr.build_models()
    if graphs:
        tr.enable_graphs()
    imgs = synthetic_images(batch, tr.g.max_size, 1).cuda()
    for _ in range(warmup):
        logs = tr.train_batch(imgs)
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        logs = tr.train_batch(imgs)               # ends in the loss read-back: a synchronise
        ts.append((time.perf_counter() - t0) * 1e3)
    row = stats(ts)
    row.update(mode='graph replay' if graphs else 'eager', steps=steps, img_per_s_at_median=batch / row['median_ms'] * 1e3,
               replaying=getattr(tr, '_graphs', None) is not None, last_losses=logs)
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=30)
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--out', default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), 'bench_shared needs the GPU (no CPU timing)'
    from tartangan_amd import backend
    K = backend.get()
    result = {'device': torch.cuda.get_device_name(0), 'clock_mhz_before': clock_mhz(), 'up2x': [], 'step': []}
    lines = []
    for BC, H in ((64 * 128, 64), (64 * 64, 128)):
        row = bench_up2x(K, BC, H, args.iters, args.warmup)
        result['up2x'].append(row)
        for k in ('native_fwd', 'aten_fwd', 'native_bwd', 'aten_bwd'):
            lines.append('up2x BC %5d H %3d  %-10s median %7.3f ms (min %7.3f max %7.3f)  %7.0f GB/s of the 5N-float minimum'
                         % (BC, H, k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'], row[k]['GBps_at_median']))
        lines.append('up2x BC %5d H %3d  aten / native time: fwd %.2f  bwd %.2f   max rel diff fwd %.1e bwd %.1e'
                     % (BC, H, row['aten_fwd']['median_ms'] / row['native_fwd']['median_ms'],
                        row['aten_bwd']['median_ms'] / row['native_bwd']['median_ms'], row['max_rel_diff_fwd'], row['max_rel_diff_bwd']))
        print('\n'.join(lines[-5:]), flush=True)
    for graphs in (False, True):
        row = bench_step(graphs, args.steps, args.warmup)
        result['step'].append(row)
        lines.append('shared trainer 128:3 batch 64  %-12s median %8.3f ms / step (min %8.3f max %8.3f)  %7.0f img/s'
                     % (row['mode'], row['median_ms'], row['min_ms'], row['max_ms'], row['img_per_s_at_median']))
        print(lines[-1], flush=True)
    result['clock_mhz_after'] = clock_mhz()
    lines.append('shader clock reported before %s, after %s MHz' % (result['clock_mhz_before'], result['clock_mhz_after']))
    print(lines[-1])
    if args.out:
        with open(args.out + '.json', 'w') as f:
            json.dump(result, f, indent=1)
        with open(args.out + '.txt', 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
