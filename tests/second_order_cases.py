"""Per-op first- and second-order checks of ``tartangan_amd.functional`` against stock torch in float64.

Each ``Case`` pairs one public op with the same operation written in stock torch.  ``run_case`` evaluates three levels on
one forward pass:

* ``value``: the op's output(s);
* ``vjp``: the gradient of <y, w> with respect to every differentiable input and parameter;
* ``r1`` (ops on the discriminator's path): g = d<tanh(y), w>/dx with ``create_graph`` (the R1 penalty's first pass, run
  under ``input_grads_only`` as ``models.losses.gradient_penalty`` does), then the gradient of sum(g^2) + <y, w2> with respect
  to x and every parameter.  The tanh gives a linear op a second derivative to carry.

Three evaluations are compared: the op under test (the backend installed by the caller: the HIP library on a GPU, or the
emulator on CPU), the torch reference on the float64 copies of the inputs (the truth), and the torch reference in fp32 on
the CPU on the same fp32 inputs (what plain fp32 arithmetic achieves).  The pass rule is "no worse than plain fp32": for
every output tensor T,  e = |T - T64|_2 / |T64|_2  must satisfy  e_op <= 4 max(e_32, EPS),  and
max|T_op - T64| <= 16 max(max|T_32 - T64|, EPS max|T64|).

Ops with a mask (LeakyReLU, BN + LeakyReLU, ELU/SELU, max-pool, the Huber loss) get inputs redrawn until no float64
pre-activation lies within ``MARGIN`` of the boundary (for max-pool: no window whose runner-up is within MARGIN of its
maximum), so the comparison measures arithmetic, not mask flips; the boundaries are pinned by their own tests."""
import math

import torch
import torch.nn.functional as F

from tartangan_amd import functional as TF

EPS = 2.4e-7           # ~ 2 ulp of fp32 at 1: the floor of the relative error a float32 result can be asked for
RATIO_L2, RATIO_MAX = 4.0, 16.0
MARGIN = 1e-4


class Case:
    """``make(gen) -> {name: fp32 CPU tensor}``; ``diff``: the names that get a gradient; ``data``: the R1 input (None: no R1
    level); ``ours(t)`` / ``ref(t)`` -> tensor or tuple of tensors; ``fix(t, gen)`` redraws inputs off a mask boundary."""

    def __init__(self, name, make, diff, ours, ref, data=None, fix=None, kind=None):
        self.name, self.make, self.diff, self.ours, self.ref, self.data, self.fix = name, make, tuple(diff), ours, ref, data, fix
        self.kind = kind or name.split('[')[0]

    def __repr__(self):
        return self.name


def _t(x):
    return x if isinstance(x, tuple) else (x,)


def _evaluate(fn, base, case, device, dtype, cot, ours):
    """-> {label: tensor (float64, CPU)} for the three levels, on copies of ``base`` moved to (device, dtype)."""
    t = {k: v.to(device=device, dtype=dtype if v.is_floating_point() else v.dtype).clone() for k, v in base.items()}
    for k in case.diff:
        t[k].requires_grad_(True)
    ys = _t(fn(t))
    out = {f'value.y{i}': y.detach() for i, y in enumerate(ys)}
    ws = [c.to(device=device, dtype=dtype) for c in cot['w']]
    wrt = [t[k] for k in case.diff]
    if wrt:
        inner = sum((y * w).sum() for y, w in zip(ys, ws))
        gs = torch.autograd.grad(inner, wrt)
        out.update({f'vjp.{k}': g for k, g in zip(case.diff, gs)})
    if case.data is not None:
        ys = _t(fn(t))               # a fresh graph: the R1 form differentiates the forward once more
        ws2 = [c.to(device=device, dtype=dtype) for c in cot['w2']]
        inner = sum((torch.tanh(y) * w).sum() for y, w in zip(ys, ws))
        if ours:
            with TF.input_grads_only():
                g, = torch.autograd.grad(inner, t[case.data], create_graph=True)
        else:
            g, = torch.autograd.grad(inner, t[case.data], create_graph=True)
        outer = g.pow(2).sum() + sum((y * w).sum() for y, w in zip(ys, ws2))
        gs = torch.autograd.grad(outer, wrt, allow_unused=True)
        out.update({f'r1.{k}': (torch.zeros_like(x) if gr is None else gr) for k, x, gr in zip(case.diff, wrt, gs)})
    return {k: v.detach().to('cpu', torch.float64) for k, v in out.items()}


def inputs_for(case, seed):
    gen = torch.Generator().manual_seed(seed)
    base = case.make(gen)
    if case.fix is not None:
        case.fix(base, gen)
    return base


def references(case, seed=0):
    """(base inputs, cotangents, float64 results, fp32 CPU results) -- computed once, reusable for several backends."""
    base = inputs_for(case, seed)
    with torch.no_grad():
        ys = _t(case.ref({k: v.double() if v.is_floating_point() else v for k, v in base.items()}))
    gen = torch.Generator().manual_seed(seed + 1)
    cot = {'w': [torch.randn(y.shape, generator=gen) for y in ys], 'w2': [torch.randn(y.shape, generator=gen) for y in ys]}
    r64 = _evaluate(case.ref, base, case, 'cpu', torch.float64, cot, False)
    r32 = _evaluate(case.ref, base, case, 'cpu', torch.float32, cot, False)
    return base, cot, r64, r32


def errors(got, r64, r32):
    """-> {label: (e_op, e_32, max_op, max_32, max64)}"""
    out = {}
    for k, T64 in r64.items():
        T, T32 = got[k], r32[k]
        assert T.shape == T64.shape, (k, tuple(T.shape), tuple(T64.shape))
        n = float(T64.norm()) or 1.0
        out[k] = (float((T - T64).norm()) / n, float((T32 - T64).norm()) / n,
                  float((T - T64).abs().max()) if T.numel() else 0.0, float((T32 - T64).abs().max()) if T.numel() else 0.0,
                  float(T64.abs().max()) if T.numel() else 0.0)
    return out


def violations(errs, ratio_l2=RATIO_L2, ratio_max=RATIO_MAX):
    bad = []
    for k, (e, e32, m, m32, m64) in errs.items():
        if not all(math.isfinite(v) for v in (e, m)):
            bad.append(f'{k}: not finite')
        elif e > ratio_l2 * max(e32, EPS) or m > ratio_max * max(m32, EPS * m64):
            bad.append(f'{k}: e_op {e:.2e} e_32 {e32:.2e} | max {m:.2e} max_32 {m32:.2e}')
    return bad


def run_case(case, device, seed=0, refs=None):
    """-> (errors, violations) of the op under test (the installed backend on ``device``) against float64 / fp32 torch."""
    base, cot, r64, r32 = refs if refs is not None else references(case, seed)
    got = _evaluate(case.ours, base, case, device, torch.float32, cot, True)
    assert set(got) == set(r64), (sorted(got), sorted(r64))
    errs = errors(got, r64, r32)
    return errs, violations(errs)


# --------------------------------------------------------------------------- input makers and boundary redraws
def _randn(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def _redraw(x, bad, gen, scale=1.0):
    x[bad] = torch.randn(int(bad.sum()), generator=gen) * scale


def _fix_zero(key):
    def fix(t, gen):
        for _ in range(100):
            bad = t[key].double().abs() < MARGIN
            if not bad.any():
                return
            _redraw(t[key], bad, gen)
        raise AssertionError('could not draw inputs off the boundary')
    return fix


def _fix_bn(t, gen):
    """Redraw elements whose float64 BN output lies within MARGIN of 0 (the LeakyReLU kink); the statistics move with every
    redraw, so until none is left."""
    for _ in range(100):
        x = t['x'].double()
        m, v = x.mean((0, 2, 3), keepdim=True), x.var((0, 2, 3), unbiased=False, keepdim=True)
        y = (x - m) / torch.sqrt(v + 1e-5) * t['gamma'].double().view(1, -1, 1, 1) + t['beta'].double().view(1, -1, 1, 1)
        bad = y.abs() < MARGIN
        if not bad.any():
            return
        fresh = m + torch.sqrt(v) * torch.randn(x.shape, generator=gen, dtype=torch.float64)
        t['x'][bad] = fresh[bad].float()
    raise AssertionError('could not draw BN inputs off the boundary')


def _fix_maxpool(t, gen):
    for _ in range(100):
        x = t['x']
        B, C, H, W = x.shape
        win = x.double().view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
        top = win.topk(2, -1).values
        bad = (top[..., 0] - top[..., 1]) < MARGIN
        if not bad.any():
            return
        mask = bad.repeat_interleave(2, 2).repeat_interleave(2, 3)
        _redraw(x, mask, gen)
    raise AssertionError('could not draw max-pool windows without near ties')


def _fix_huber(k):
    def fix(t, gen):
        for _ in range(100):
            Q = t['preds'].shape[0] // t['target'].shape[0]
            err = t['target'].double().repeat(Q, 1) - t['preds'].double()
            bad = (err.abs() < MARGIN) | ((err.abs() - k).abs() < MARGIN)
            if not bad.any():
                return
            _redraw(t['preds'], bad, gen)
        raise AssertionError('could not draw IQN predictions off the Huber boundaries')
    return fix


def _w(gen, cout, cin, ks):
    return _randn(gen, cout, cin, ks, ks, scale=(1.0 / (cin * ks * ks)) ** 0.5)


# --------------------------------------------------------------------------- the cases
def conv_case(B, Cin, Cout, H, W, ks, residual=False, residual_up=False, tag=''):
    def make(gen):
        t = {'x': _randn(gen, B, Cin, H, W), 'w': _w(gen, Cout, Cin, ks), 'b': _randn(gen, Cout, scale=0.1)}
        if residual:
            t['res'] = _randn(gen, B, Cout, H // 2, W // 2) if residual_up else _randn(gen, B, Cout, H, W)
        return t
    diff = ('x', 'w', 'b') + (('res',) if residual else ())

    def ours(t):
        return TF.conv2d(t['x'], t['w'], t['b'], t.get('res'), residual_up)

    def ref(t):
        y = F.conv2d(t['x'], t['w'], t['b'], padding=ks // 2)
        if residual:
            y = y + (F.interpolate(t['res'], scale_factor=2) if residual_up else t['res'])
        return y
    kind = 'conv2d_1x1' if ks == 1 else 'conv2d_3x3'
    name = f'{kind}{"+res_up" if residual_up else "+res" if residual else ""}{tag}[{B}x{Cin}->{Cout}x{H}x{W}]'
    return Case(name, make, diff, ours, ref, data='x', kind=kind)


def compose_rgb_case(B, C, Cout, H, W, Cimg=3):
    def make(gen):
        return {'img': _randn(gen, B, Cimg, H, W), 'w1': _w(gen, C, Cimg, 1), 'b1': _randn(gen, C, scale=0.1),
                'w3': _w(gen, Cout, C, 3), 'b3': _randn(gen, Cout, scale=0.1)}

    def ours(t):
        wc = TF.compose_rgb_filter(t['w1'], t['b1'], t['w3'])
        return TF.conv2d(TF.copy_channels(t['img'], Cimg + 1, 1.0), wc.view(Cout, Cimg + 1, 3, 3), t['b3'])

    def ref(t):
        return F.conv2d(F.conv2d(t['img'], t['w1'], t['b1']), t['w3'], t['b3'], padding=1)
    return Case(f'compose_rgb[{B}x{Cimg}->{C}->{Cout}x{H}x{W}]', make, ('img', 'w1', 'b1', 'w3', 'b3'), ours, ref, data='img')


def pool_conv_case(B, Cin, Cout, H, W, residual=True):
    """H, W: the OUTPUT plane (the input is 2H x 2W)."""
    def make(gen):
        t = {'x': _randn(gen, B, Cin, 2 * H, 2 * W), 'w': _w(gen, Cout, Cin, 3), 'b': _randn(gen, Cout, scale=0.1)}
        if residual:
            t['res'] = _randn(gen, B, Cout, H, W)
        return t

    def ref(t):
        y = F.avg_pool2d(F.conv2d(t['x'], t['w'], t['b'], padding=1), 2)
        return y + t['res'] if residual else y
    def ours(t):
        # the layer's own routing (models/layers.py): the fused stride-2 kernel where it is supported (enough workgroups),
        # else conv3x3 followed by the pooling pass that carries the shortcut
        if TF.pool_conv3x3_supported(t['x'], t['w']):
            return TF.pool_conv3x3(t['x'], t['w'], t['b'], t.get('res'))
        return TF.avg_pool2(TF.conv2d(t['x'], t['w'], t['b']), t.get('res'))
    return Case(f'pool_conv3x3{"+res" if residual else ""}[{B}x{Cin}->{Cout}x{2 * H}x{2 * W}]', make,
                ('x', 'w', 'b') + (('res',) if residual else ()), ours, ref, data='x', kind='pool_conv3x3')


def avg_pool_case(B, C, H, W, residual=False):
    def make(gen):
        t = {'x': _randn(gen, B, C, H, W)}
        if residual:
            t['res'] = _randn(gen, B, C, H // 2, W // 2)
        return t

    def ref(t):
        y = F.avg_pool2d(t['x'], 2)
        return y + t['res'] if residual else y
    return Case(f'avg_pool2{"+res" if residual else ""}[{B}x{C}x{H}x{W}]', make, ('x',) + (('res',) if residual else ()),
                lambda t: TF.avg_pool2(t['x'], t.get('res')), ref, data='x', kind='avg_pool2')


def upconv_case(B, Cin, Cout, H, W, residual=False):
    """H, W: the INPUT plane (the output is 2H x 2W).  Generator only: first order."""
    def make(gen):
        t = {'a': _randn(gen, B, Cin, H, W), 'w': _w(gen, Cout, Cin, 3), 'b': _randn(gen, Cout, scale=0.1)}
        if residual:
            t['res'] = _randn(gen, B, Cout, 2 * H, 2 * W)
        return t

    def ref(t):
        y = F.conv2d(F.interpolate(t['a'], scale_factor=2), t['w'], t['b'], padding=1)
        return y + t['res'] if residual else y
    return Case(f'upconv3x3{"+res" if residual else ""}[{B}x{Cin}->{Cout}x{H}x{W}]', make,
                ('a', 'w', 'b') + (('res',) if residual else ()),
                lambda t: TF.upconv3x3(t['a'], t['w'], t['b'], t.get('res')), ref, kind='upconv3x3')


def qkv_case(B, Cin, cs, H, W):
    def make(gen):
        ws = torch.cat([_w(gen, c, Cin, 1) for c in cs])           # one storage, as the network's parameter bucket keeps them
        return {'x': _randn(gen, B, Cin, H, W), 'wt': ws[:cs[0]].clone(), 'wp': ws[cs[0]:cs[0] + cs[1]].clone(),
                'wg': ws[cs[0] + cs[1]:].clone()}
    return Case(f'qkv_projections[{B}x{Cin}->{"+".join(map(str, cs))}x{H}x{W}]', make, ('x', 'wt', 'wp', 'wg'),
                lambda t: TF.qkv_projections(t['x'], t['wt'], t['wp'], t['wg']),
                lambda t: tuple(F.conv2d(t['x'], t[k]) for k in ('wt', 'wp', 'wg')), data='x', kind='qkv_projections')


def max_pool_case(B, C, H, W):
    return Case(f'max_pool2[{B}x{C}x{H}x{W}]', lambda gen: {'x': _randn(gen, B, C, H, W)}, ('x',),
                lambda t: TF.max_pool2(t['x']), lambda t: F.max_pool2d(t['x'], 2), data='x', fix=_fix_maxpool)


def attention_case(B, D, DV, N, M):
    def make(gen):
        return {'theta': _randn(gen, B, D, N), 'phi': _randn(gen, B, D, M), 'g': _randn(gen, B, DV, M)}

    def ref(t):
        return torch.bmm(t['g'], torch.softmax(torch.bmm(t['theta'].transpose(1, 2), t['phi']), -1).transpose(1, 2))
    return Case(f'attention_core[{B}x{D}/{DV}x{N}/{M}]', make, ('theta', 'phi', 'g'),
                lambda t: TF.attention_core(t['theta'], t['phi'], t['g']), ref, data='theta')


def scale_add_case(B, C, H, W):
    def make(gen):
        return {'s': _randn(gen, 1).reshape(()), 'a': _randn(gen, B, C, H, W), 'b': _randn(gen, B, C, H, W)}
    return Case(f'scale_add[{B}x{C}x{H}x{W}]', make, ('s', 'a', 'b'), lambda t: TF.scale_add(t['s'], t['a'], t['b']),
                lambda t: t['s'] * t['a'] + t['b'], data='a')


def bn_case(B, C, H, W, slope=0.2, offset=0.0, tag=''):
    """Training-mode BatchNorm2d + LeakyReLU(slope); ``offset``: |mean| / std of every channel."""
    def make(gen):
        x = _randn(gen, B, C, H, W)
        if offset:
            x = x + offset * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).view(1, C, 1, 1)
        return {'x': x, 'gamma': 1 + _randn(gen, C, scale=0.3), 'beta': _randn(gen, C, scale=0.3),
                'rm': torch.zeros(C), 'rv': torch.ones(C)}

    def ours(t):
        return TF.batch_norm_act(t['x'], t['gamma'], t['beta'], t['rm'], t['rv'], True, 0.1, 1e-5, slope)

    def ref(t):
        y = F.batch_norm(t['x'], t['rm'], t['rv'], t['gamma'], t['beta'], training=True, momentum=0.1, eps=1e-5)
        return F.leaky_relu(y, slope) if slope != 1 else y
    return Case(f'batch_norm_act{tag}[s{slope},{B}x{C}x{H}x{W}]', make, ('x', 'gamma', 'beta'), ours, ref, data='x',
                fix=_fix_bn if slope != 1 else None, kind='batch_norm_act')


def unary_case(kind, shape, slope=0.2, data=True):
    ours = {'leaky_relu': lambda t: TF.leaky_relu(t['x'], slope), 'elu': lambda t: TF.elu(t['x']),
            'selu': lambda t: TF.selu(t['x']), 'tanh': lambda t: TF.tanh(t['x'])}[kind]
    ref = {'leaky_relu': lambda t: F.leaky_relu(t['x'], slope), 'elu': lambda t: F.elu(t['x']),
           'selu': lambda t: torch.selu(t['x']), 'tanh': lambda t: torch.tanh(t['x'])}[kind]
    fix = None if kind == 'tanh' else _fix_zero('x')
    return Case(f'{kind}[{"x".join(map(str, shape))}]', lambda gen: {'x': _randn(gen, *shape)}, ('x',), ours, ref,
                data='x' if data else None, fix=fix, kind=kind)


def bilinear_case(B, C, H, W, fork=False):
    def ref_half(x):
        return F.interpolate(x, scale_factor=0.5, mode='bilinear', align_corners=True)
    if fork:
        return Case(f'fork_bilinear_half[{B}x{C}x{H}x{W}]', lambda gen: {'x': _randn(gen, B, C, H, W)}, ('x',),
                    lambda t: TF.fork_bilinear_half(t['x']), lambda t: (ref_half(t['x']), t['x']), data='x',
                    kind='fork_bilinear_half')
    return Case(f'bilinear_half[{B}x{C}x{H}x{W}]', lambda gen: {'x': _randn(gen, B, C, H, W)}, ('x',),
                lambda t: TF.bilinear_half(t['x']), lambda t: ref_half(t['x']), data='x', kind='bilinear_half')


def copy_channels_case(B, C, C2, H, W, fill):
    def ref(t):
        x = t['x']
        if C2 <= C:
            return x[:, :C2]
        return torch.cat([x, torch.full((B, C2 - C, H, W), fill, dtype=x.dtype, device=x.device)], 1)
    return Case(f'copy_channels[{B}x{C}->{C2}x{H}x{W}]', lambda gen: {'x': _randn(gen, B, C, H, W)}, ('x',),
                lambda t: TF.copy_channels(t['x'], C2, fill), ref, data='x', kind='copy_channels')


def sum_hw_case(B, C, H, W):
    # inputs scaled so that the sums are O(1): at |y| ~ sqrt(HW) the R1 probe tanh saturates and its fp32 rounding, not the
    # op, decides the comparison
    return Case(f'sum_hw[{B}x{C}x{H}x{W}]', lambda gen: {'x': _randn(gen, B, C, H, W, scale=(H * W) ** -0.5)}, ('x',),
                lambda t: TF.sum_hw(t['x']),
                lambda t: t['x'].sum((2, 3)), data='x')


def linear_case(B, Cin, Cout):
    def make(gen):
        return {'x': _randn(gen, B, Cin), 'w': _randn(gen, Cout, Cin, scale=Cin ** -0.5), 'b': _randn(gen, Cout, scale=0.1)}
    return Case(f'linear[{B}x{Cin}->{Cout}]', make, ('x', 'w', 'b'), lambda t: TF.linear(t['x'], t['w'], t['b']),
                lambda t: F.linear(t['x'], t['w'], t['b']), data='x')


def binary_case(kind, shape):
    ours = {'add': lambda t: TF.add(t['a'], t['b']), 'mul': lambda t: TF.mul(t['a'], t['b'])}[kind]
    ref = {'add': lambda t: t['a'] + t['b'], 'mul': lambda t: t['a'] * t['b']}[kind]
    return Case(f'{kind}[{"x".join(map(str, shape))}]', lambda gen: {'a': _randn(gen, *shape), 'b': _randn(gen, *shape)},
                ('a', 'b'), ours, ref, data='a', kind=kind)


def iqn_cos_case(n, dims):
    """Value only: no gradient flows into the sampled taus or the embedding range."""
    def make(gen):
        return {'taus': torch.rand(n, 1, generator=gen), 'rng': torch.arange(dims, dtype=torch.float32)}
    return Case(f'iqn_cos_embed[{n}x{dims}]', make, (), lambda t: TF.iqn_cos_embed(t['taus'], t['rng']),
                lambda t: torch.cos(t['taus'].repeat(1, dims) * math.pi * t['rng']), kind='iqn_cos_embed')


def repeat_rows_case(rows, cols, reps):
    return Case(f'repeat_rows[{rows}x{cols}x{reps}]', lambda gen: {'x': _randn(gen, rows, cols)}, ('x',),
                lambda t: TF.repeat_rows(t['x'], reps), lambda t: t['x'].repeat(reps, 1), data='x', kind='repeat_rows')


def mean_reps_case(rows, cols, reps):
    return Case(f'mean_reps[{rows}x{cols}x{reps}]', lambda gen: {'x': _randn(gen, reps * rows, cols)}, ('x',),
                lambda t: TF.mean_reps(t['x'], reps), lambda t: t['x'].reshape(reps, rows, cols).mean(0), kind='mean_reps')


def iqn_ref_loss(preds, target, taus, k):
    """oracle/sagan_cpu.py iqn_loss (models/iqn.py:111-130) for out_dims == 1."""
    B = target.shape[0]
    taus, preds = taus.reshape(-1, B, 1), preds.reshape(-1, B, 1)
    err = target.repeat(preds.shape[0], 1).reshape(-1, B, 1) - preds
    loss = torch.where(err.abs() <= k, 0.5 * err.pow(2), k * (err.abs() - 0.5 * k))
    return ((taus - (err < 0).to(err.dtype)).abs() * loss).sum(0).mean()


def iqn_loss_case(B, Q, k=1.0):
    def make(gen):
        return {'preds': _randn(gen, Q * B, 1, scale=1.5), 'target': (torch.rand(B, 1, generator=gen) < 0.5).float(),
                'taus': torch.rand(Q * B, 1, generator=gen)}
    return Case(f'iqn_quantile_huber_loss[{B}x{Q}]', make, ('preds',),
                lambda t: TF.iqn_quantile_huber_loss(t['preds'], t['target'], t['taus'], Q, k),
                lambda t: iqn_ref_loss(t['preds'], t['target'], t['taus'], k), fix=_fix_huber(k), kind='iqn_quantile_huber_loss')


def bce_case(n):
    def make(gen):
        return {'x': _randn(gen, n, 1, scale=2.0), 't': (torch.rand(n, 1, generator=gen) < 0.5).float()}
    return Case(f'bce_with_logits[{n}]', make, ('x',), lambda t: TF.bce_with_logits(t['x'], t['t']),
                lambda t: F.binary_cross_entropy_with_logits(t['x'], t['t']), kind='bce_with_logits')


def sumsq_case(shape, alpha):
    return Case(f'sumsq[{"x".join(map(str, shape))}]', lambda gen: {'x': _randn(gen, *shape)}, ('x',),
                lambda t: TF.sumsq(t['x'], alpha), lambda t: alpha * t['x'].pow(2).sum(), data='x', kind='sumsq')


def ragged_cases():
    """Small shapes off every alignment the kernels like: B in {1, 3}, channels 3 / 5 / 24 / 100, planes 9x11 and 20x36."""
    return [
        conv_case(1, 3, 5, 9, 11, 3), conv_case(3, 24, 100, 20, 36, 3), conv_case(3, 100, 5, 9, 11, 3),
        conv_case(1, 5, 24, 9, 11, 1), conv_case(3, 100, 5, 20, 36, 1),
        conv_case(3, 5, 24, 9, 11, 3, residual=True), conv_case(1, 24, 5, 20, 36, 1, residual=True),
        conv_case(3, 5, 24, 20, 36, 3, residual=True, residual_up=True),
        # shapes the Winograd kernel is eligible for (8-channel input chunks, W % 32 == 0 with H % 8 == 0, or 16x16 / 8x8 /
        # 4x4 planes; the latter two only under TG_CONV_WINO=2), output channels not a multiple of 16
        conv_case(3, 24, 100, 8, 32, 3), conv_case(1, 16, 5, 16, 16, 3, residual=True), conv_case(3, 32, 24, 8, 8, 3),
        conv_case(1, 48, 100, 4, 4, 3), conv_case(3, 8, 24, 16, 64, 3, residual=True, residual_up=True),
        compose_rgb_case(3, 24, 5, 8, 32),
        compose_rgb_case(3, 24, 5, 9, 11), compose_rgb_case(1, 5, 24, 20, 36),
        pool_conv_case(3, 5, 24, 10, 18), pool_conv_case(1, 24, 100, 5, 6), pool_conv_case(3, 250, 250, 20, 36),
        avg_pool_case(3, 5, 20, 36), avg_pool_case(1, 24, 10, 22, residual=True),
        upconv_case(3, 24, 5, 9, 11), upconv_case(1, 5, 24, 10, 18, residual=True),
        qkv_case(3, 24, (3, 3, 12), 8, 6), qkv_case(1, 5, (1, 1, 4), 16, 9),
        max_pool_case(3, 5, 20, 36), max_pool_case(1, 24, 10, 22),
        attention_case(3, 2, 8, 99, 25), attention_case(1, 4, 16, 180, 45),
        scale_add_case(3, 5, 9, 11),
        bn_case(3, 5, 9, 11, 0.2), bn_case(1, 24, 20, 36, 0.2), bn_case(3, 100, 9, 11, 1.0), bn_case(1, 5, 20, 36, 1.0),
        bn_case(3, 5, 9, 11, 0.2, offset=10.0, tag='+offset10'), bn_case(3, 5, 9, 11, 0.2, offset=1e3, tag='+offset1e3'),
        unary_case('leaky_relu', (3, 5, 9, 11)), unary_case('leaky_relu', (1, 100, 20, 36)),
        unary_case('elu', (3, 5, 9, 11)), unary_case('selu', (1, 24, 20, 36)),
        unary_case('tanh', (3, 5, 9, 11)),
        bilinear_case(3, 5, 20, 36), bilinear_case(1, 24, 10, 22), bilinear_case(3, 3, 20, 36, fork=True),
        copy_channels_case(3, 3, 4, 9, 11, 1.0), copy_channels_case(1, 24, 5, 20, 36, 0.0),
        sum_hw_case(3, 5, 9, 11), sum_hw_case(1, 100, 20, 36),
        linear_case(3, 100, 5), linear_case(1, 24, 1),
        binary_case('add', (3, 5, 9, 11)), binary_case('mul', (3, 24, 20)),
        iqn_cos_case(24, 64), iqn_cos_case(5, 3),
        repeat_rows_case(3, 100, 8), mean_reps_case(3, 24, 8),
        iqn_loss_case(3, 8), iqn_loss_case(1, 5), bce_case(6), bce_case(1),
        sumsq_case((3, 5, 9, 11), 1 / 3),
    ]


# --------------------------------------------------------------------------- the discriminator's own layer shapes
class Recorder:
    """Shapes of every launch of the named backend entry points (integer arguments only) while the block runs."""

    def __init__(self, K, names):
        self.K, self.names, self.seen, self._saved = K, names, {}, {}

    def __enter__(self):
        for n in self.names:
            fn = getattr(self.K, n)
            self._saved[n] = fn
            setattr(self.K, n, self._wrap(n, fn))
        return self

    def _wrap(self, name, fn):
        def rec(*args):
            self.seen.setdefault(name, set()).add(tuple(a for a in args if isinstance(a, int) and not isinstance(a, bool)))
            return fn(*args)
        return rec

    def __exit__(self, *exc):
        for n, fn in self._saved.items():
            setattr(self.K, n, fn)


D_ENTRY_POINTS = ('conv2d_fwd', 'conv2d_fwd_up2res', 'poolconv3x3_fwd', 'conv1x1_multi_fwd', 'attn_fwd', 'bn_train_fwd',
                  'bn_train_fwd_groups', 'maxpool2_fwd', 'bilinear_half_fwd')


def cases_from_launches(seen):
    """One case per distinct launch shape the recorder saw (the batch as launched: 2B for the paired real | fake forward)."""
    out = []
    for B, Cin, Cout, H, W, ks in sorted(seen.get('conv2d_fwd', ())):
        out.append(conv_case(B, Cin, Cout, H, W, ks, tag='@D'))
    for B, Cin, Cout, H, W in sorted(seen.get('conv2d_fwd_up2res', ())):
        out.append(conv_case(B, Cin, Cout, H, W, 3, residual=True, residual_up=True, tag='@D'))
    for B, Cin, Cout, H, W in sorted(seen.get('poolconv3x3_fwd', ())):
        out.append(pool_conv_case(B, Cin, Cout, H, W))
    for c0, c1, c2, B, Cin, H, W in sorted(seen.get('conv1x1_multi_fwd', ())):
        out.append(qkv_case(B, Cin, (c0, c1, c2), H, W))
    for B, D, DV, N, M in sorted(seen.get('attn_fwd', ())):
        out.append(attention_case(B, D, DV, N, M))
    # a grouped launch (the real | fake pair: statistics per half) is one BatchNorm per group of B images; the R1 passes run on
    # the real half alone, at B.  (The grouped kernels themselves are compared with float64 in the D-phase pin.)
    bn = {(B, C, HW) for B, C, HW, *_ in seen.get('bn_train_fwd', ())}
    bn |= {(B, C, HW) for G, B, C, HW, *_ in seen.get('bn_train_fwd_groups', ())}
    for B, C, HW in sorted(bn):
        side = int(round(HW ** 0.5))
        assert side * side == HW, HW
        out.append(bn_case(B, C, side, side, 0.2))
    for BC, H, W in sorted(seen.get('maxpool2_fwd', ())):
        out.append(max_pool_case(1, BC, H, W))
    for BC, H, W in sorted(seen.get('bilinear_half_fwd', ())):
        out.append(bilinear_case(1, BC, H, W))
    return out


# --------------------------------------------------------------------------- exact edges (no redraw: the boundary is the point)
def lrelu_zero_case(slope=0.2):
    """LeakyReLU at exactly +0.0 and -0.0: torch's derivative there is ``slope`` (it tests x > 0)."""
    def make(gen):
        x = _randn(gen, 3, 5, 9, 11)
        pick = torch.rand(x.shape, generator=gen)
        x[pick < 0.2] = 0.0
        x[(pick >= 0.2) & (pick < 0.4)] = -0.0
        return {'x': x}
    return Case(f'leaky_relu@zero[s{slope}]', make, ('x',), lambda t: TF.leaky_relu(t['x'], slope),
                lambda t: F.leaky_relu(t['x'], slope), data='x', kind='leaky_relu')


def bn_zero_case(slope=0.2):
    """Every channel balanced over {-1, 0, 1} and beta = 0: the batch mean is exactly 0, so y is exactly 0 at a third of the
    elements in any arithmetic, and the LeakyReLU derivative there must be torch's (slope)."""
    B, C, H, W = 3, 5, 9, 11
    n = B * H * W

    def make(gen):
        vals = torch.tensor([-1.0, 0.0, 1.0]).repeat_interleave(n // 3)
        x = torch.stack([vals[torch.randperm(n, generator=gen)] for _ in range(C)], 0)
        return {'x': x.view(C, B, H, W).transpose(0, 1).contiguous(), 'gamma': 1 + _randn(gen, C, scale=0.3),
                'beta': torch.zeros(C), 'rm': torch.zeros(C), 'rv': torch.ones(C)}
    base = bn_case(B, C, H, W, slope)
    return Case(f'batch_norm_act@zero[s{slope}]', make, ('x', 'gamma', 'beta'), base.ours, base.ref, data='x',
                kind='batch_norm_act')


def bn_constant_channels_case(B=3, C=6, H=9, W=11, slope=0.2):
    """Every other channel constant (zero variance): outputs and gradients finite and no worse than fp32.  beta is kept off 0,
    so y = beta + (x - mean) * invstd keeps one sign there in any arithmetic."""
    def make(gen):
        x = _randn(gen, B, C, H, W)
        x[:, ::2] = (0.1 + torch.rand(1, C // 2 + C % 2, 1, 1, generator=gen)).expand(B, -1, H, W)
        beta = _randn(gen, C, scale=0.3)
        beta = torch.where(beta.abs() < 0.05, torch.full_like(beta, 0.1), beta)
        return {'x': x, 'gamma': 1 + _randn(gen, C, scale=0.3), 'beta': beta, 'rm': torch.zeros(C), 'rv': torch.ones(C)}
    base = bn_case(B, C, H, W, slope)
    return Case(f'batch_norm_act@zero_var[s{slope},{B}x{C}x{H}x{W}]', make, ('x', 'gamma', 'beta'), base.ours, base.ref,
                data='x', kind='batch_norm_act')


def maxpool_ties_case():
    """Integer-valued windows full of ties: under the R1 form too, the FIRST maximum of a window (row-major) takes it all."""
    def make(gen):
        return {'x': torch.randint(0, 3, (3, 5, 10, 22), generator=gen).float()}
    return Case('max_pool2@ties', make, ('x',), lambda t: TF.max_pool2(t['x']), lambda t: F.max_pool2d(t['x'], 2), data='x',
                kind='max_pool2')


def iqn_edge_case(k=1.0):
    """err == 0 and |err| == k exactly (targets in {0, 1}, predictions at target, target -+ k).  Both Huber branches agree in
    value and slope at |err| == k, and at err == 0 loss and gradient vanish whichever way the quantile indicator goes, so this
    does not tell `<` from `<=`: it checks that values and gradients at the exact edges are finite and match the reference."""
    B, Q = 6, 4

    def make(gen):
        target = torch.tensor([0.0, 1.0, 1.0, 0.0, 1.0, 0.0]).view(B, 1)
        off = torch.tensor([0.0, k, -k])[torch.randint(0, 3, (Q * B,), generator=gen)].view(Q * B, 1)
        return {'preds': target.repeat(Q, 1) + off, 'target': target, 'taus': torch.rand(Q * B, 1, generator=gen)}
    base = iqn_loss_case(B, Q, k)
    return Case('iqn_quantile_huber_loss@edges', make, ('preds',), base.ours, base.ref, kind='iqn_quantile_huber_loss')


def edge_cases():
    return [lrelu_zero_case(0.2), lrelu_zero_case(0.0), bn_zero_case(0.2), bn_constant_channels_case(), maxpool_ties_case(),
            iqn_edge_case(1.0)]
