"""Time the explore apps' hot paths on the GPU.

    python tools/bench_explore.py [--steps 200] [--warmup 30] [--rounds 7] [--out profiles/explore_step]

1. The find-image step at config 128:3, batch 2, Adam + MSE: ``explore.find_image.FindImage.step`` eager and replayed from its HIP
   graph, against the loop a user could write without it -- the same generator modules, ATen for the normalisation, the loss, the
   L2 term, the stochastic clip (``randn_like`` on the device) and the statistics, ``torch.optim.Adam`` for the update.  Each arm
   twice: free-running (one synchronise per ``--steps`` steps; the app's ``--log-every 0``) and with the per-step read-back of the
   loss and the three z statistics (``--log-every 1``; the ATen loop reads its four values one by one, as the reference does).
2. ``tg_mosaic_gather`` at 6 x 6 images of 128 x 128, S = 256, against the ATen advanced-indexing gather with prebuilt indexes.
3. ``tg_recon_loss`` (2 x 3 x 128 x 128, with gradient) and ``tg_latent_step`` (Adam, n = 512) alone.

Every figure is the median over ``--rounds`` rounds of the mean over ``--steps`` back-to-back calls, with the rounds' min and max;
the arms take turns inside a round, so that a drifting clock or a busy host hits them alike."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def generator(config='128', attention=(3,)):
    from tartangan_amd.models.pluggan import GAN_CONFIGS, Generator
    torch.manual_seed(0)
    g = Generator(GAN_CONFIGS[config]._replace(attention=attention)).cuda().eval()
    g.requires_grad_(False)
    return g


def fused_arm(g, target, z0, graphs, max_steps):
    from tartangan_amd.explore.find_image import FindImage
    args = FindImage.parse_cli_args(['ckpt', 'out', 'target.png', '--max-steps', str(max_steps), '--save-every', '0', '--log-every', '0'])
    args.device = 'cuda'
    app = FindImage(args)
    app.g, app.target_imgs, app.z = g, target, z0.clone().requires_grad_(True)
    if graphs:
        app.enable_graphs()
    app.prepare_fused()
    assert (app._graph is not None) == graphs
    state = dict(i=0)

    def step(read_back):
        app.step(state['i'])
        state['i'] += 1
        if read_back:
            app._stats.tolist()
    return step


def aten_arm(g, target, z0, lr=0.5, l2=0.):
    z = z0.clone().requires_grad_(True)
    opt = torch.optim.Adam([z], lr)
    mean, std = (torch.tensor(c, device='cuda').view(1, 3, 1, 1) for c in (MEAN, STD))

    def step(read_back):
        with torch.no_grad():
            outside = ((z > 3) | (z < -3)).float()          # the clip as four small ops, a mask multiplied in twice
            noise = torch.randn_like(z)
            z.sub_(z * outside)
            z.add_(noise * outside)
        opt.zero_grad()
        imgs = g(z)
        loss = F.mse_loss(((imgs + 1.) / 2. - mean) / std, target, reduction='sum')
        loss = loss + z.pow(2).mean() * l2
        loss.backward()
        opt.step()
        if read_back:
            float(loss), float(z.min()), float(z.mean()), float(z.max())
    return step


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def summary(name, samples, unit='us'):
    return dict(name=name, unit=unit, median=statistics.median(samples), min=min(samples), max=max(samples), rounds=len(samples))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--steps', type=int, default=200)
    p.add_argument('--warmup', type=int, default=30)
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--out', default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), 'bench_explore needs the GPU (no CPU timing)'
    from tartangan_amd import backend
    K = backend.get()
    total = 2 * (a.warmup + a.steps * a.rounds) + 8
    g = generator()
    torch.manual_seed(1)
    z0 = torch.randn(2, g.config.latent_dims).cuda()
    target = torch.randn(2, 3, g.max_size, g.max_size).cuda()
    steps = {'fused eager': fused_arm(g, target, z0, False, total), 'fused graph replay': fused_arm(g, target, z0, True, total),
             'ATen loop': aten_arm(g, target, z0)}
    arms = {(name, rb): (lambda f=f, rb=rb: f(rb)) for name, f in steps.items() for rb in (False, True)}

    # the kernels alone and the gather
    rows = cols = 6
    grid = torch.randn(rows * cols, 3, 128, 128).cuda()
    S = 256
    out = torch.empty(3, S, S, device='cuda')
    y = torch.arange(S, device='cuda')
    gy, gx, iy, ix = ((y * rows) // S)[:, None], ((y * cols) // S)[None, :], ((y * 128) // S)[:, None], ((y * 128) // S)[None, :]
    grid5 = grid.view(rows, cols, 3, 128, 128)
    imgs, grad, loss = torch.rand(2, 3, 128, 128).cuda() * 2 - 1, torch.empty(2, 3, 128, 128, device='cuda'), torch.zeros(1, device='cuda')
    nbytes = K.recon_loss_workspace(2, 3, 128 * 128)
    ws = torch.empty(max(1, nbytes // 4), device='cuda')
    n = 512
    lz, lg, lm, lv = (torch.randn(n).cuda() for _ in range(4))
    lv.abs_()
    lstep, lstats = torch.zeros(1, dtype=torch.int64, device='cuda'), torch.zeros(4, device='cuda')
    arms[('tg_mosaic_gather 6x6x128^2 -> 256^2', None)] = lambda: K.mosaic_gather(grid, out, rows, cols, 3, 128, 128, S)
    arms[('ATen indexing gather 6x6x128^2 -> 256^2', None)] = lambda: grid5[gy, gx, :, iy, ix].permute(2, 0, 1).contiguous()
    arms[('tg_recon_loss 2x3x128^2', None)] = lambda: K.recon_loss(imgs, target, grad, loss, ws, nbytes, 2, 3, 128 * 128, 0)
    arms[('tg_latent_step adam n=512', None)] = lambda: K.latent_step(lz, lg, lm, lv, lstep, None, lstats, loss, n, 0, 0.5, 0.9, 0.999,
                                                                       1e-8, 0.)
    K.mosaic_gather(grid, out, rows, cols, 3, 128, 128, S)
    assert torch.equal(grid5[gy, gx, :, iy, ix].permute(2, 0, 1), out)

    for fn in arms.values():
        timed(fn, a.warmup)
    samples = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            samples[k].append(timed(fn, a.steps))
    result = dict(device=torch.cuda.get_device_name(0), config='128:3', batch=2, steps_per_round=a.steps, rounds=a.rounds,
                  method='median over rounds of (wall time of steps_per_round back-to-back calls, one synchronise at the end) / steps',
                  arms=[])
    lines = []
    for (name, rb), s in samples.items():
        label = name if rb is None else f'find-image step, {name}, {"per-step read-back" if rb else "free-running"}'
        row = summary(label, s)
        result['arms'].append(row)
        lines.append(f'{label:<72} {row["median"]:10.1f} us   (min {row["min"]:.1f}, max {row["max"]:.1f}, {row["rounds"]} rounds)')
    print('\n'.join(lines))
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out + '.json', 'w') as f:
            json.dump(result, f, indent=1)
        with open(a.out + '.txt', 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
