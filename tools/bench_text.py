"""Time the text kernels on the GPU at the text trainer's CLI defaults (config 64, batch 128, embedding 64, context 3).

    python tools/bench_text.py [--iters 200] [--warmup 20] [--rounds 3] [--vocab 10000] [--out profiles/text_step]

* every k=3 layer shape of G and D (recorded from one forward of ``models.text.build_text_models``) through ``tg_conv1d_fwd`` /
  ``_dgrad`` / ``_wgrad``, against the only route such a layer had before -- ``tg_conv2d_*`` at H = 1 with the filter embedded in the
  middle row of a 3x3 (the embedding copy is timed as its own line) -- and against ATen (``F.conv1d``,
  ``aten.convolution_backward``);
* ``tg_skipgram_step`` against the composed ATen sequence (sparse nn.Embedding tables, the reference's loss, backward, optim.SGD);
* one R1-penalised discriminator pass plus one generator pass over the 1-D models, HIP layers against stock torch.nn layers;
* ``TextCNNTrainer.train_batch``, eager, in its pretraining phase (the skip-gram step and the target EMA) and in its GAN phase.

Method: every arm is warmed up, then ``--rounds`` rounds time back-to-back calls of each arm in turn (so a drifting clock hits all
arms alike).  The conv arms: ``--iters`` x ``--conv-factor`` (2000) calls between two device events, windows of 20-180 ms; the figure
is window / calls, a PER-CALL BACK-TO-BACK time (enqueue and kernel, whichever is longer), not a kernel time.  The skip-gram, model
and step arms end in a read-back and are timed by the host clock around it.  Median / min / max over the rounds."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def layer_shapes(g, d, cfg, batch):
    from tartangan_amd.models.layers import Conv1d
    seen = []

    def hook(m, args, out):
        x = args[0]
        shape = (x.shape[0], x.shape[1], out.shape[1], x.shape[2], m.kernel_size[0])
        if shape[4] == 3 and shape not in seen:
            seen.append(shape)
    hooks = [m.register_forward_hook(hook) for net in (g, d) for m in net.modules() if isinstance(m, Conv1d)]
    with torch.no_grad():
        d(g(torch.randn(batch, cfg.latent_dims, device='cuda')))
    for h in hooks:
        h.remove()
    return seen


def conv_arms(K, shape):
    B, Cin, Cout, L, ks = shape
    x, gy = torch.randn(B, Cin, L, device='cuda'), torch.randn(B, Cout, L, device='cuda')
    w, bias = torch.randn(Cout, Cin, ks, device='cuda') * 0.05, torch.randn(Cout, device='cuda')
    y, gx, gw, gb = torch.empty_like(gy), torch.empty_like(x), torch.empty_like(w), torch.empty_like(bias)
    ws1 = torch.empty(K.conv1d_wgrad_workspace(B, Cin, Cout, L, ks) // 4 + 4, device='cuda')
    w33, gw33 = torch.zeros(Cout, Cin, 3, 3, device='cuda'), torch.empty(Cout, Cin, 3, 3, device='cuda')
    ws2 = torch.empty(K.conv2d_wgrad_workspace(B, Cin, Cout, 1, L, 3) // 4 + 4, device='cuda')
    w33[:, :, 1, :] = w

    def embed():
        w33[:, :, 1, :] = w
    aten_bwd = torch.ops.aten.convolution_backward
    return {
        ('fwd', 'conv1d'): lambda: K.conv1d_fwd(x, w, bias, None, y, B, Cin, Cout, L, ks),
        ('fwd', 'conv2d H=1'): lambda: K.conv2d_fwd(x, w33, bias, None, y, B, Cin, Cout, 1, L, 3),
        ('fwd', 'aten'): lambda: F.conv1d(x, w, bias, padding=1),
        ('dgrad', 'conv1d'): lambda: K.conv1d_dgrad(gy, w, gx, B, Cin, Cout, L, ks),
        ('dgrad', 'conv2d H=1'): lambda: K.conv2d_dgrad(gy, w33, gx, B, Cin, Cout, 1, L, 3),
        ('dgrad', 'aten'): lambda: aten_bwd(gy, x, w, [Cout], [1], [1], [1], False, [0], 1, [True, False, False]),
        ('wgrad', 'conv1d'): lambda: K.conv1d_wgrad(x, gy, gw, gb, ws1, ws1.numel() * 4, B, Cin, Cout, L, ks, 0),
        ('wgrad', 'conv2d H=1'): lambda: K.conv2d_wgrad(x, gy, gw33, gb, ws2, ws2.numel() * 4, B, Cin, Cout, 1, L, 3, 0),
        ('wgrad', 'aten'): lambda: aten_bwd(gy, x, w, [Cout], [1], [1], [1], False, [0], 1, [False, True, True]),
        ('embed filter', 'conv2d H=1'): embed,
    }


def skipgram_arms(B, C2, E, vocab, lr):
    from tartangan_amd.models.text import SkipGram
    g = torch.Generator().manual_seed(0)
    words, contexts = torch.randint(0, vocab, (B,), generator=g).cuda(), torch.randint(0, vocab, (B, C2), generator=g).cuda()
    negatives = torch.randint(0, vocab, (B, C2), generator=g).cuda()
    mine = SkipGram(vocab, E, sparse=True, padding_idx=0).cuda()
    ref_u, ref_v = nn.Embedding(vocab, E, sparse=True, padding_idx=0).cuda(), nn.Embedding(vocab, E, sparse=True, padding_idx=0).cuda()
    opt = torch.optim.SGD(list(ref_u.parameters()) + list(ref_v.parameters()), lr=lr)

    def fused():
        return float(mine.train_step(words, contexts, negatives, lr))

    def aten():
        opt.zero_grad()
        emb_u = ref_u(words)
        pos = torch.bmm(ref_v(contexts), emb_u.unsqueeze(-1)).squeeze(-1)
        neg = torch.bmm(ref_v(negatives), emb_u.unsqueeze(-1)).squeeze(-1)
        loss = -(F.logsigmoid(pos).sum(1) + F.logsigmoid(-neg).sum(1)).mean()
        loss.backward()
        opt.step()
        return float(loss)
    return {('skip-gram step', 'tg_skipgram_step'): fused, ('skip-gram step', 'aten composed'): aten}


def model_arms(cfg, batch):
    from tartangan_amd.models.text import build_text_models
    arms = {}
    for name, layers in (('hip layers', None), ('torch.nn layers', nn)):
        torch.manual_seed(0)
        g, d = build_text_models(cfg, **({} if layers is None else {'layers': layers}))
        g, d = g.cuda(), d.cuda()
        z, real = torch.randn(batch, cfg.latent_dims, device='cuda'), torch.randn(batch, cfg.data_dims, g.max_size, device='cuda')

        def passes(g=g, d=d, z=z, real=real):
            x = real.clone().requires_grad_(True)
            p_real, p_fake = d(x), d(g(z).detach())
            gx, = torch.autograd.grad(p_real.sum(), x, create_graph=True)
            loss = F.softplus(-p_real).mean() + F.softplus(p_fake).mean() + 5.0 * gx.pow(2).flatten(1).sum(1).mean()
            gd = torch.autograd.grad(loss, list(d.parameters()))
            gg = torch.autograd.grad(F.softplus(-d(g(z))).mean(), list(g.parameters()))
            return float(loss) + float(gd[0].sum()) + float(gg[0].sum())
        arms[('D pass with R1 + G pass, eager', name)] = passes
    return arms


def step_arms(batch, E, context, vocab):
    """``TextCNNTrainer.train_batch`` at the CLI defaults, eager: the embedding-only step of the pretraining phase and the full
    step of the GAN phase.  Each call ends in the step's one read-back."""
    from tartangan_amd.trainers.text_cnn import TextCNNTrainer
    arms = {}
    for what, pretrain in (('eager step, pretraining phase', 1 << 30), ('eager step, GAN phase', 0)):
        tr = TextCNNTrainer(TextCNNTrainer.default_args(config='64', batch_size=batch, device='cuda', embedding_dims=E, context=context,
                                                        pretrain_embedding=pretrain))
        torch.manual_seed(0)
        tr.build_models()
        tr.build_embedding(vocab, padding_idx=0)
        docs = torch.randint(1, vocab, (batch, tr.g.max_size), generator=torch.Generator().manual_seed(1))
        arms[(what, 'TextCNNTrainer')] = lambda tr=tr, docs=docs: tr.train_batch(docs)
    return arms


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=200)
    p.add_argument('--warmup', type=int, default=20)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--conv-factor', type=int, default=10, help='the conv arms time iters x this many calls per window')
    p.add_argument('--vocab', type=int, default=10000)
    p.add_argument('--out', default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), 'bench_text needs the GPU (no CPU timing)'
    from tartangan_amd import backend
    from tartangan_amd.models.pluggan import GAN_CONFIGS
    from tartangan_amd.models.text import build_text_models
    K = backend.get()
    batch, E, context = 128, 64, 3
    cfg = GAN_CONFIGS['64']._replace(data_dims=E)
    g, d = build_text_models(cfg)
    shapes = layer_shapes(g.cuda(), d.cuda(), cfg, batch)
    result = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'rounds': args.rounds, 'config': '64', 'batch': batch,
              'embedding_dims': E, 'context': context, 'vocab': args.vocab, 'rows': []}
    lines = []

    def run(label, arms, timer, iters):
        for key in list(arms):
            try:
                for _ in range(args.warmup):
                    arms[key]()
            except backend.KernelError as e:         # a route that refuses the shape is reported, not timed
                lines.append('%-28s %-32s %-18s refused: %s' % (label, key[0], key[1], e))
                result['rows'].append(dict(case=label, what=key[0], arm=key[1], refused=str(e)))
                del arms[key]
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                times[k].append(timer(fn, iters))
        for (what, arm), ts in times.items():
            row = dict(case=label, what=what, arm=arm, median_us=statistics.median(ts), min_us=min(ts), max_us=max(ts))
            result['rows'].append(row)
            lines.append('%-28s %-32s %-18s median %9.1f us (min %9.1f max %9.1f)' % (label, what, arm, row['median_us'], row['min_us'], row['max_us']))

    def host_timer(fn, iters):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()                                     # ends in a read-back
        return (time.perf_counter() - t0) * 1e6 / iters

    for shape in shapes:
        run('B%d Cin%d Cout%d L%d k%d' % shape, conv_arms(K, shape), window, args.iters * args.conv_factor)
    run('B%d C2=%d E%d vocab %d' % (batch, 2 * context, E, args.vocab), skipgram_arms(batch, 2 * context, E, args.vocab, 4e-4), host_timer,
        max(10, args.iters // 4))
    run('config 64 batch %d E%d' % (batch, E), model_arms(cfg, batch), host_timer, max(5, args.iters // 20))
    run('config 64 batch %d E%d' % (batch, E), step_arms(batch, E, context, args.vocab), host_timer, max(20, args.iters // 4))
    print('\n'.join(lines))
    if args.out:
        with open(args.out + '.json', 'w') as f:
            json.dump(result, f, indent=1)
        with open(args.out + '.txt', 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
