"""Time the scene structure stage, forward + backward, natively and through the reference's ATen composition on the same GPU.

    python tools/bench_scene.py [--batch 64] [--iters 50] [--warmup 10] [--out profiles/scene_structure]

The stage alone (theta and mask logits given; the two Linears in front of it are the same GEMMs either way): native =
``functional.scene_patches`` (tg_scene_patches_fwd + tg_scene_patches_bwd, two launches), aten = the reference's loop over the
patches of F.affine_grid + F.grid_sample + multiply + squeeze, then stack + permute (models/blocks/scene.py:127-155), both
followed by ``backward`` with a given output gradient.  Default geometry (20 patches of 3 x 3 on a 16 x 16 canvas, mask
refinement and noise on).  HIP-event time of every forward + backward (warm-up first, the two alternating), median / min /
max.  The work is latency-bound: what is compared is launch count, not bandwidth."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--patches', type=int, default=20)
    p.add_argument('--patch', type=int, default=3)
    p.add_argument('--scene', type=int, default=16)
    p.add_argument('--iters', type=int, default=50)
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--out', default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), 'bench_scene needs the GPU (no CPU timing)'
    import scene_cases as SC
    from tartangan_amd import functional as TF
    B, P, patch, S = args.batch, args.patches, args.patch, args.scene
    gen = torch.Generator().manual_seed(0)
    theta = (torch.tensor(SC.INIT_THETA).repeat(B, P) + 0.3 * torch.randn(B, P * 6, generator=gen)).cuda().requires_grad_(True)
    logits = torch.randn(B, P * patch * patch, generator=gen).cuda().requires_grad_(True)
    noise = torch.randn(patch, patch, generator=gen).cuda()
    gout = torch.randn(B, P, S, S, generator=gen).cuda()

    def run(f):
        theta.grad = logits.grad = None
        out = f()
        out.backward(gout)
        return out

    native = lambda: run(lambda: TF.scene_patches(theta, logits, noise, patch, S))       # noqa: E731
    aten = lambda: run(lambda: SC.compose(theta, logits, noise, B, P, patch, S))           # noqa: E731
    a = native().detach().clone()
    ga = theta.grad.clone()
    b = aten().detach()
    diff = (float((a - b).abs().max() / b.abs().max()), float((ga - theta.grad).abs().max() / theta.grad.abs().max()))
    for f in (native, aten):
        for _ in range(args.warmup):
            f()
    torch.cuda.synchronize()
    t_native, t_aten = [], []
    for _ in range(args.iters):
        t_native.append(timed_once(native))
        t_aten.append(timed_once(aten))
    row = {'batch': B, 'patches': P, 'patch': patch, 'scene': S, 'iters': args.iters, 'max_rel_diff_out': diff[0],
           'max_rel_diff_gtheta': diff[1]}
    lines = []
    for name, t in (('native', t_native), ('aten', t_aten)):
        med = statistics.median(t)
        row[name] = {'median_ms': med, 'min_ms': min(t), 'max_ms': max(t)}
        lines.append('B %3d P %2d patch %2d S %3d  %-6s fwd+bwd median %8.3f ms (min %8.3f max %8.3f)' % (B, P, patch, S, name, med, min(t), max(t)))
    lines.append('aten / native time %.1f   max rel diff out %.2e gtheta %.2e'
                 % (row['aten']['median_ms'] / row['native']['median_ms'], diff[0], diff[1]))
    print('\n'.join(lines))
    if args.out:
        with open(args.out + '.json', 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'result': row}, f, indent=1)
        with open(args.out + '.txt', 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
