"""The shared-filter trainer's host logic on the CPU: ``functional.bilinear_up2x`` / ``narrow_filters``, the shared blocks and
models and ``trainers.shared.cnn.CNNTrainer``, run over plain-torch forms of the four new entry points
(shared_cases.SharedEmulator) and compared with the fixtures the reference's own trainer produced
(tests/golden/shared_*.json, made by tests/golden/make_shared_golden.py).

Nothing here says anything about the HIP kernels (tests/test_bilinear_up_gpu.py, test_filter_bank_gpu.py, test_shared_gpu.py)."""
import copy

import pytest
import torch

import shared_cases as SH
from oracle.procedural import summarize, synthetic_images
from tartangan_amd import backend, functional as TF
from tartangan_amd.models import layers
from tartangan_amd.models.shared.blocks import SharedConvBlock, narrow_filters
from tartangan_amd.models.shared.pluggan import SharedDiscriminator, SharedGenerator


@pytest.fixture(autouse=True)
def emulated_backend():
    prev = backend._set_backend_for_testing(SH.SharedEmulator())
    yield
    backend._set_backend_for_testing(prev)


def _close(a, b, rel=1e-4, abs_=1e-6):
    return abs(a - b) <= abs_ + rel * max(abs(a), abs(b))


def _total_l2(module, grads=False):
    s = 0.
    for p in module.parameters():
        t = p.grad if grads else p
        s += float(t.detach().double().pow(2).sum())
    return s ** 0.5


def _unused_bn(model):
    """The BatchNorm tensors of the one block built with apply_norm=False: owned, never run."""
    first = next(m for m in model.modules() if isinstance(m, SharedConvBlock) and not m.apply_norm)
    return [p for p in first.norm_and_activate.parameters()]


# ------------------------------------------------------------------------------------------------- against the fixtures
@pytest.mark.parametrize('case', SH.SHARED_CASES)
def test_models_have_the_reference_keys_counts_and_default_init(case):
    fx = SH.load_shared_fixture(case)
    tr = SH.shared_trainer(fx, 'cpu')
    for net in ('g', 'd'):
        module = getattr(tr, net)
        assert list(module.state_dict().keys()) == fx['state_keys'][net]
        assert [n for n, _ in module.named_parameters()] == fx['param_names'][net]     # the bank once, under its first name
        assert len(list(module.parameters())) == fx['n_params'][net + '_tensors']
        assert sum(p.numel() for p in module.parameters()) == fx['n_params'][net]
    assert list(tr.target_g.state_dict().keys()) == fx['state_keys']['g']
    assert fx['param_names']['g'][0] == 'shared_filters' and sum(k.endswith('shared_filters') for k in fx['state_keys']['g']) > 3
    assert all(m.shared_filters is tr.g.shared_filters for m in tr.g.modules() if hasattr(m, 'shared_filters'))
    di = fx['default_init']
    assert _close(_total_l2(tr.g), di['g_l2'], 1e-6)
    assert _close(_total_l2(tr.target_g), di['target_g_l2'], 1e-6)          # (the second draw of the init stream)
    assert _close(_total_l2(tr.d), di['d_l2'], 1e-6)
    for net in ('g', 'd'):
        for name, v in getattr(tr, net).state_dict().items():
            ref = di[net][name]
            got = summarize(v, len(ref['idx']))
            assert _close(got['l2'], ref['l2'], 1e-6) and _close(got['sum'], ref['sum'], 1e-6, 1e-5), (net, name)
            assert got['samples'] == pytest.approx(ref['samples'], rel=1e-6, abs=1e-7), (net, name)


@pytest.mark.parametrize('case', SH.SHARED_CASES)
def test_forward_pins(case):
    fx = SH.load_shared_fixture(case)
    tr = SH.shared_trainer(fx, 'cpu')
    SH.load_procedural(tr, fx)
    with torch.no_grad():
        g2, d2 = copy.deepcopy(tr.g), copy.deepcopy(tr.d)
        z = torch.randn(fx['batch'], tr.gan_config.latent_dims, generator=torch.Generator().manual_seed(99))
        g_out = g2(z)
        d_real, d_fake = d2(synthetic_images(fx['batch'], fx['size'], fx['img_seed'])), d2(g_out)
    ref = fx['forward']['g_out']
    got = summarize(g_out, len(ref['idx']))
    assert got['numel'] == ref['numel'] and _close(got['l2'], ref['l2'], 1e-5)
    for a, b in zip(got['samples'], ref['samples']):
        assert abs(a - b) <= 1e-5
    for got, name in ((d_real, 'd_real'), (d_fake, 'd_fake')):
        for a, b in zip(got.reshape(-1).tolist(), fx['forward'][name]):
            assert _close(a, b, 1e-5, 1e-5), name


@pytest.mark.parametrize('pairs', [True, False], ids=['paired', 'unpaired'])
@pytest.mark.parametrize('case', SH.SHARED_CASES)
def test_trainer_matches_reference_fixture(case, pairs, single_thread):
    """BOTH steps at 1e-4: losses, parameter and gradient L2s, and the final state tensor by tensor."""
    fx = SH.load_shared_fixture(case)
    tr = SH.shared_trainer(fx, 'cpu', pair_d=pairs, pair_g=pairs)
    SH.load_procedural(tr, fx)
    assert tr._d_pairable() == pairs and tr._g_pairable() == pairs
    torch.manual_seed(fx['rng_seed'])
    for k, ref in enumerate(fx['steps']):
        logs = tr.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + k))
        for name in ('g_loss', 'd_loss', 'gp'):
            assert _close(logs[name], ref[name], 1e-4), (case, k, name, logs[name], ref[name])
        assert _close(_total_l2(tr.g), ref['g_l2'], 1e-4)
        assert _close(_total_l2(tr.d), ref['d_l2'], 1e-4)
        assert _close(_total_l2(tr.target_g), ref['target_g_l2'], 1e-4)
        assert _close(_total_l2(tr.g, True), ref['g_grad_l2'], 1e-4), (case, k)
        assert _close(_total_l2(tr.d, True), ref['d_grad_l2'], 1e-4), (case, k)
        if k == 0:
            for net in ('d', 'g'):
                total = ref[net + '_grad_l2']
                for name, p in getattr(tr, net).named_parameters():
                    ref_s = fx['after_step1'][net + '_grad'][name]
                    got = summarize(p.grad, 4)
                    if ref_s is None:      # the reference never gave it a gradient; here it sits in the bucket with a zero one
                        assert got['max_abs'] == 0.0, (net, name)
                    else:                  # 1e-4 of the tensor, plus rounding at the scale of the whole gradient
                        assert _close(got['l2'], ref_s['l2'], 1e-4, 1e-6 * total), (net, name, got['l2'], ref_s['l2'])
    assert tr.rng_feed.plan == [('z', fx['batch'], tr.gan_config.latent_dims)] * 2
    # Final state, tensor by tensor, at 1e-4.  One kind of tensor cannot be held to that by anybody, the reference against itself
    # under another summation order included: a conv bias in front of a BatchNorm has a gradient that is ZERO in exact arithmetic
    # (the batch mean cancels it); what is computed is rounding noise (recorded: below 1e-8 of the network's gradient per
    # element, everything else above 1e-4), and Adam with beta1 = 0 turns any non-zero gradient into a move of lr per step,
    # in the noise's direction.  Those tensors (step-1 gradient below 1e-6 of the network's) get the Adam bound instead:
    # 2 lr per element and step; the EMA copy lr_target_g times the sum of g's deviations.  The BatchNorm behind such a bias sees its
    # input shifted by the drift so far, which its running mean takes up with the momentum, 0.1: at most 0.1 * 2 lr * (1 + ... +
    # (steps - 1)) per element (running means only; a shift leaves the variance alone).
    steps = len(fx['steps'])
    noise = {net: {n for n, r in fx['after_step1'][net + '_grad'].items() if r is not None and r['l2'] < 1e-6 * fx['steps'][0][net + '_grad_l2']}
             for net in ('g', 'd')}
    assert all(n.endswith('.bias') and '.blocks.' in n for names in noise.values() for n in names)
    assert bool(noise['g']) == (fx['flags'].get('norm') != 'id')
    for net, lr, scale in (('g', tr.args.lr_g, 1.), ('d', tr.args.lr_d, 1.), ('target_g', tr.args.lr_g, tr.args.lr_target_g * steps)):
        for name, v in getattr(tr, net).state_dict().items():
            ref = fx['final'][net][name]
            got = summarize(v, len(ref['idx']))
            if name.rsplit('.', 1)[-1] == 'num_batches_tracked':
                assert got['sum'] == ref['sum'], (net, name)
                continue
            drift = 2 * lr * steps * scale if name in noise['g' if net == 'target_g' else net] else 0.
            if name.endswith('.running_mean') and noise['g' if net == 'target_g' else net]:
                drift = 0.1 * 2 * lr * (steps * (steps - 1) // 2)
            assert _close(got['l2'], ref['l2'], 1e-4, 1e-6 + drift * ref['numel'] ** 0.5), (net, name, got['l2'], ref['l2'])
            assert _close(got['sum'], ref['sum'], 1e-4, 1e-4 * ref['abs_sum'] + 1e-6 + drift * ref['numel']), (net, name, got['sum'], ref['sum'])
    assert float(torch.rand(1)) == fx['rng_after']


# ----------------------------------------------------------------------------------------- what the optimiser must not touch
@pytest.mark.parametrize('case', ['shared_c16_b4', 'shared_c32a2_b4'])
def test_never_read_columns_and_unused_batchnorm_stay_bit_unchanged(case):
    """Config '16' has latent_dims = 100 > max(blocks) = 64: bank columns 64..99 are never read, get an exactly zero gradient
    and keep their bits (g, d and the EMA copy).  The first block's BatchNorm is owned but never run: the reference's Adam skips
    it (grad is None); here it sits in the bucket with a zero gradient, which with beta1 = 0 is a zero update."""
    fx = SH.load_shared_fixture(case)
    tr = SH.shared_trainer(fx, 'cpu')
    SH.load_procedural(tr, fx)
    widest = max(fx['blocks'])
    spare = tr.g.shared_filters.shape[1] > widest
    assert spare == (case == 'shared_c16_b4')
    with torch.no_grad():            # the same non-zero values in g and its EMA copy, so that "unchanged" says something
        tr.target_g.shared_filters[:, widest:].copy_(tr.g.shared_filters[:, widest:])
        for p, q in zip(_unused_bn(tr.g), _unused_bn(tr.target_g)):
            q.copy_(p)
    watched = {}
    for net in ('g', 'd', 'target_g'):
        module = getattr(tr, net)
        if spare:
            watched[(net, 'columns')] = lambda m=module: m.shared_filters[:, widest:]
        for i, p in enumerate(_unused_bn(module)):
            watched[(net, f'unused batchnorm {i}')] = lambda p=p: p
    assert len(watched) == (3 if spare else 0) + 6
    before = {k: get().detach().clone() for k, get in watched.items()}
    assert all(float(v.abs().max()) > 0 for v in before.values())
    torch.manual_seed(fx['rng_seed'])
    for k in range(2):
        tr.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + k))
    for key, get in watched.items():
        assert torch.equal(get().detach().contiguous().view(torch.int32), before[key].contiguous().view(torch.int32)), key
    for net in ('g', 'd'):
        module = getattr(tr, net)
        if spare:
            assert float(module.shared_filters.grad[:, widest:].abs().max()) == 0.0
            assert float(module.shared_filters.grad[:, :widest].abs().min()) > 0.0        # while every column that is read trains
        for p in _unused_bn(module):
            assert float(p.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------ the autograd ops
@pytest.mark.parametrize('shape', [(1, 2, 1, 1), (2, 1, 2, 2), (1, 2, 3, 5)], ids=str)
@pytest.mark.parametrize('residual', [False, True])
def test_bilinear_up2x_gradcheck_and_gradgradcheck(shape, residual):
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, dtype=torch.float64, generator=gen, requires_grad=True)
    B, C, H, W = shape
    args = (x, torch.randn(B, C, 2 * H, 2 * W, dtype=torch.float64, generator=gen, requires_grad=True)) if residual else (x,)
    assert torch.autograd.gradcheck(TF.bilinear_up2x, args)
    assert torch.autograd.gradgradcheck(TF.bilinear_up2x, args)
    want = SH.up(x.detach()) + (args[1].detach() if residual else 0)
    assert torch.equal(TF.bilinear_up2x(*args).detach(), want)


def test_fork_bilinear_up2x_sums_both_gradients_at_the_low_resolution():
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 4, 5, dtype=torch.float64, generator=gen, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: TF.fork_bilinear_up2x(t), (x,))
    a, b = TF.fork_bilinear_up2x(x)
    ga, gb = torch.randn(a.shape, dtype=torch.float64, generator=gen), torch.randn(a.shape, dtype=torch.float64, generator=gen)
    got, = torch.autograd.grad([a, b], x, [ga, gb])
    assert torch.allclose(got, SH.up_transpose(ga + gb), rtol=0, atol=1e-12)
    only_b, = torch.autograd.grad(TF.fork_bilinear_up2x(x)[1], x, gb)
    assert torch.allclose(only_b, SH.up_transpose(gb), rtol=0, atol=1e-12)


def test_bilinear_up2x_of_a_pair_is_one_launch_over_both_halves():
    calls = []

    class Counting(SH.SharedEmulator):
        def bilinear_up2x_fwd(self, x, residual, y, BC, H, W):
            calls.append(('fwd', BC, H, W))
            return super().bilinear_up2x_fwd(x, residual, y, BC, H, W)

        def bilinear_up2x_bwd(self, gy, residual, gx, BC, H, W):
            calls.append(('bwd', BC, H, W))
            return super().bilinear_up2x_bwd(gy, residual, gx, BC, H, W)

    backend._set_backend_for_testing(Counting())
    gen = torch.Generator().manual_seed(5)
    r, f = (torch.randn(2, 3, 4, 4, generator=gen, requires_grad=True) for _ in range(2))
    out = TF.bilinear_up2x(TF.Pair(r, f))
    assert isinstance(out, TF.Pair) and calls == [('fwd', 12, 4, 4)]
    assert torch.allclose(out.r, SH.up(r), rtol=0, atol=1e-6) and torch.allclose(out.f, SH.up(f), rtol=0, atol=1e-6)
    (out.r.sum() + 2 * out.f.sum()).backward()
    assert calls[1:] == [('bwd', 12, 4, 4)]
    assert torch.allclose(f.grad, 2 * r.grad) and torch.allclose(r.grad, SH.up_transpose(torch.ones(2, 3, 8, 8)))
    assert torch.equal(layers.interpolate(r, scale_factor=2, mode='bilinear', align_corners=True), SH.up(r))
    with pytest.raises(NotImplementedError):
        layers.interpolate(r, scale_factor=2, mode='bilinear', align_corners=False)


@pytest.mark.parametrize('corner', [(1, 1), (3, 5), (4, 6)], ids=str)
def test_narrow_filters_gradcheck_and_gradgradcheck(corner):
    O, I = corner
    bank = torch.randn(4, 6, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(6), requires_grad=True)
    fn = lambda b: TF.narrow_filters(b, I, O)          # (in_dims, out_dims): the reference's argument order
    assert torch.equal(fn(bank).detach(), bank.detach()[:O, :I]) and fn(bank).is_contiguous()
    assert torch.autograd.gradcheck(fn, (bank,))
    assert torch.autograd.gradgradcheck(fn, (bank,))
    g, = torch.autograd.grad(fn(bank).sum(), bank)
    assert float(g[:O, :I].min()) == 1.0 and float(g.sum()) == O * I * 9          # exact zeros outside the corner
    for bad in ((5, 1), (1, 7), (0, 1)):
        with pytest.raises(ValueError):
            TF.narrow_filters(bank, bad[1], bad[0])


def test_r1_style_second_order_gradient_reaches_the_bank():
    """conv(x, narrow(bank)): differentiate w.r.t. x with create_graph, then a function of that gradient w.r.t. the bank --
    the path R1's second-order sweep takes through D -- against the same computation in plain float64 torch."""
    gen = torch.Generator().manual_seed(7)
    bank = torch.randn(4, 6, 3, 3, generator=gen).requires_grad_(True)
    x = torch.randn(2, 3, 5, 5, generator=gen).requires_grad_(True)

    def penalty(conv, filt, xin):
        y = conv(xin, filt)
        g, = torch.autograd.grad(y.pow(2).sum(), xin, create_graph=True)
        return g.pow(2).sum() + y.sum()
    got, = torch.autograd.grad(penalty(lambda a, w: TF.conv2d(a, w), narrow_filters(bank, 3, 2), x), bank)
    b64, x64 = bank.detach().double().requires_grad_(True), x.detach().double().requires_grad_(True)
    want, = torch.autograd.grad(penalty(lambda a, w: torch.nn.functional.conv2d(a, w, padding=1), b64[:2, :3], x64), b64)
    assert torch.allclose(got.double(), want, rtol=0, atol=1e-5 * float(want.abs().max()))
    assert float(got[2:].abs().max()) == 0.0 and float(got[:, 3:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------- one view per shape
class _CountingNarrow(SH.SharedEmulator):
    def __init__(self):
        self.fwd, self.bwd = [], []

    def filter_narrow(self, bank, view, O, I, Omax, Imax, taps):
        self.fwd.append((O, I))
        return super().filter_narrow(bank, view, O, I, Omax, Imax, taps)

    def filter_narrow_bwd(self, gview, gbank, O, I, Omax, Imax, taps, accumulate):
        self.bwd.append((O, I, accumulate))
        return super().filter_narrow_bwd(gview, gbank, O, I, Omax, Imax, taps, accumulate)


def _uses(model):
    """(out, in) of every use of the bank in one forward: two convolutions per block, a projection where the width changes."""
    uses = []
    for m in model.modules():
        if isinstance(m, SharedConvBlock):
            uses.append((m.out_dims, m.in_dims))
        elif hasattr(m, 'project_input') and m.in_dims != m.out_dims:
            uses.append((m.out_dims, m.in_dims))
    return uses


@pytest.mark.parametrize('net', ['g', 'd'])
def test_one_view_per_distinct_shape_per_pass(net):
    counting = _CountingNarrow()
    backend._set_backend_for_testing(counting)
    fx = SH.load_shared_fixture('shared_c64_b2_id')
    cfg = SH.shared_config(fx)
    torch.manual_seed(0)
    model = SharedGenerator(cfg) if net == 'g' else SharedDiscriminator(
        cfg, block_factory=SH.shared_trainer(fx, 'cpu')._factories()['d_block'])
    uses = _uses(model)
    distinct = sorted(set(uses))
    assert len(uses) == 10 and len(distinct) == 5           # four blocks: ten uses of five shapes
    x = torch.randn(2, cfg.latent_dims) if net == 'g' else torch.randn(2, 3, 64, 64)
    del counting.fwd[:]
    out = model(x)                                          # the model's own scope: one pass
    assert sorted(counting.fwd) == distinct
    out.sum().backward()
    assert sorted(b[:2] for b in counting.bwd) == distinct  # and one launch per view into the bank on the way back
    del counting.fwd[:]
    with TF.filter_forms(model):                            # a caller's scope spans its passes: still once
        model(x)
        model(x)
        assert sorted(counting.fwd) == distinct
        with torch.no_grad():                               # (a view made without a graph is not one made with)
            model(x)
        assert sorted(counting.fwd) == sorted(distinct * 2)
    del counting.fwd[:]
    for m in model.modules():                               # outside any scope every use materialises
        if isinstance(m, SharedConvBlock):
            m(torch.randn(1, m.in_dims, 4, 4))
    assert len(counting.fwd) == sum(isinstance(m, SharedConvBlock) for m in model.modules())


def test_trainer_step_materialises_each_view_once_per_pass_and_sums_into_the_bucket():
    counting = _CountingNarrow()
    backend._set_backend_for_testing(counting)
    fx = SH.load_shared_fixture('shared_c16_b4')
    tr = SH.shared_trainer(fx, 'cpu')
    SH.load_procedural(tr, fx)
    g_shapes, d_shapes = sorted(set(_uses(tr.g))), sorted(set(_uses(tr.d)))
    torch.manual_seed(fx['rng_seed'])
    tr.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed']))          # records the draw order
    del counting.fwd[:], counting.bwd[:]
    tr.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + 1))
    # one generator pass over both latents, the D phase's pass over real | fake, D(fake) of the G phase
    assert sorted(counting.fwd) == sorted(g_shapes + 2 * d_shapes)
    # backwards every view adds its corner straight into the bank's slot of the gradient bucket (accumulate = 1), once
    assert all(acc == 1 for _, _, acc in counting.bwd)
    assert sorted(b[:2] for b in counting.bwd) == sorted(g_shapes + d_shapes)
    assert tr.g.shared_filters.grad.data_ptr() == tr.optimizer_g.grads.data_ptr()      # the first parameter of the bucket
