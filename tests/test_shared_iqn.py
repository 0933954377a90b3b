"""The shared-filter IQN trainer's host logic on the CPU: ``functional.iqn_head``, ``FusedIQNDiscriminatorOutput``,
``SharedIQNDiscriminator`` and ``trainers.shared.iqn.IQNTrainer``, run over plain-torch forms of the two new entry points
(shared_iqn_cases.SharedIQNEmulator) and compared with a float64 restatement of the head and with the fixtures the reference's own
trainer produced (tests/golden/shared_iqn_*.json, made by tests/golden/make_shared_iqn_golden.py).

Nothing here says anything about the HIP kernels (tests/test_fused_iqn_head_gpu.py, test_shared_iqn_gpu.py).

Tolerance of the emulated entry points against float64: the emulator is fp32 ATen; its longest sums have 16384 terms (rows x
channels at the benched size), a random walk of 128 roundoffs; the bound is 1e-5 of the largest reference value (170 roundoffs),
or 4 x e32 where that is more: e32 is what the restatement itself is off in fp32 on the same inputs, and it shows where a case is
ill-conditioned (err = target - p cancels, and dpreds inherits p's rounding magnified)."""
import pytest
import torch

import shared_iqn_cases as SI
from oracle.procedural import summarize, synthetic_images
from tartangan_amd import backend, functional as TF
from tartangan_amd.models import iqn as iqn_models
from tartangan_amd.models.blocks import FusedIQNDiscriminatorOutput, IQNDiscriminatorOutput
from tartangan_amd.models.layers import BatchNorm2d, LeakyReLU
from tartangan_amd.models.losses import gradient_penalty
from tartangan_amd.models.shared.pluggan import SharedIQNDiscriminator

SHAPES = [(1, 1, 1, 1, 1), (1, 1, 8, 1, 20), (2, 1, 8, 3, 20), (1, 3, 8, 65, 20), (1, 5, 3, 257, 7), (2, 4, 8, 64, 20),
          (2, 64, 8, 128, 20), (2, 8, 8, 1024, 20)]
EMU_TOL = 1e-5
HEAD_CALLS = ('iqn_head_fwd', 'iqn_head_bwd')
COMPOSED_HEAD_CALLS = ('gemm', 'mul', 'repeat_rows', 'repeat_rows_groups', 'sum_reps', 'sum_reps_groups', 'iqn_cos_embed', 'iqn_loss',
                       'iqn_loss_groups', 'tanh_fwd', 'tanh_bwd')


@pytest.fixture(autouse=True)
def emulated_backend(monkeypatch):
    monkeypatch.delenv('TG_IQN_FUSED_HEAD', raising=False)
    prev = backend._set_backend_for_testing(SI.SharedIQNEmulator())
    yield
    backend._set_backend_for_testing(prev)


def _close(a, b, rel=1e-4, abs_=1e-6):
    return abs(a - b) <= abs_ + rel * max(abs(a), abs(b))


def _rel(got, want):
    return SI._rel(got.detach().double().reshape(-1), want.reshape(-1))


def _emu_tol(c, name):
    return max(EMU_TOL, 4 * c['e32'][name])


# ------------------------------------------------------------------------------- the entry points against float64 autograd
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_emulated_entry_points_match_float64_autograd(shape):
    G, B, Q, C, D = shape
    c = SI.head_case(*shape)
    E = backend.get()
    pt, loss, dpreds = torch.zeros(G * B, 1), torch.zeros(()), torch.zeros(G * Q * B)
    E.iqn_head_fwd(c['f'], c['taus'], c['t'], c['W1'], c['b1'], c['w2'], c['b2'], c['range'], c['k'], pt, loss, dpreds, None, *shape)
    outs = dict(pt=pt, loss=loss, dpreds=dpreds)
    grads = dict(df=torch.zeros(G * B, C), dW1=torch.zeros(C, D), db1=torch.zeros(C), dw2=torch.zeros(1, C), db2=torch.zeros(1))
    E.iqn_head_bwd(c['gl'], c['gpt'], dpreds, c['f'], c['taus'], c['W1'], c['b1'], c['w2'], c['range'], *grads.values(), *shape, 0)
    outs.update(grads)
    for name, got in outs.items():
        assert _rel(got, c['want'][name]) <= _emu_tol(c, name), (shape, name)
    again = {n: g.clone() for n, g in grads.items()}          # accumulate: the parameter gradients are added to, df overwritten
    E.iqn_head_bwd(c['gl'], c['gpt'], dpreds, c['f'], c['taus'], c['W1'], c['b1'], c['w2'], c['range'], *again.values(), *shape, 1)
    assert torch.equal(again['df'], grads['df'])
    for name in ('dW1', 'db1', 'dw2', 'db2'):
        assert torch.allclose(again[name], 2 * grads[name], rtol=1e-6, atol=0)


def _through_function(c, paired):
    """pt, loss, first and second order through TF.iqn_head -> dict like head_case's ``want``."""
    G, B, Q, C = c['G'], c['B'], c['Q'], c['C']
    f, W1, b1, w2, b2 = (c[n].clone().requires_grad_(True) for n in ('f', 'W1', 'b1', 'w2', 'b2'))
    gpt = c['gpt'].clone().reshape(G * B, 1).requires_grad_(True)
    t = c['t'].reshape(G * B, 1)
    if paired:
        feats, taus = TF.Pair(f[:B], f[B:]), TF.Pair(c['taus'][:Q * B].reshape(-1, 1), c['taus'][Q * B:].reshape(-1, 1))
        pt, loss = TF.iqn_head(feats, taus, t, W1, b1, w2, b2, c['range'], Q, c['k'])
        assert isinstance(pt, TF.Pair)
        weighted = (gpt[:B] * pt.r).sum() + (gpt[B:] * pt.f).sum()
        pt = torch.cat([pt.r, pt.f])
    else:
        pt, loss = TF.iqn_head(f, c['taus'].reshape(-1, 1), t, W1, b1, w2, b2, c['range'], Q, c['k'])
        weighted = (gpt * pt).sum()
    df, dW1, db1, dw2, db2 = torch.autograd.grad(c['gl'] * loss + weighted, (f, W1, b1, w2, b2), create_graph=True)
    second = torch.autograd.grad((c['v'] * df).sum(), (gpt, W1, b1, w2))
    out = dict(pt=pt, loss=loss, df=df, dW1=dW1, db1=db1, dw2=dw2, db2=db2)
    out.update(zip(SI.OUTPUTS_DBWD, second))
    return out


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_function_first_and_second_order_match_float64_autograd(shape):
    c = SI.head_case(*shape)
    for paired in ([True] if shape[0] == 2 else [False]):          # (G = 2 is the Pair form: its rows are [half][q][b])
        for name, got in _through_function(c, paired).items():
            assert _rel(got, c['want'][name]) <= _emu_tol(c, name), (shape, paired, name)


def test_cotangents_on_the_parameter_gradients_are_refused():
    c = SI.head_case(1, 3, 8, 65, 20)
    f, W1 = c['f'].clone().requires_grad_(True), c['W1'].clone().requires_grad_(True)
    pt, _ = TF.iqn_head(f, c['taus'].reshape(-1, 1), None, W1, c['b1'], c['w2'], c['b2'], c['range'], 8)
    dW1, = torch.autograd.grad(pt.sum(), W1, create_graph=True)
    with pytest.raises(NotImplementedError, match='parameter gradients'):
        torch.autograd.grad(dW1.sum(), f)


def test_mismatched_shapes_are_refused_before_any_launch_in_both_forms():
    c = SI.head_case(2, 4, 8, 64, 20)
    B, Q = 4, 8
    params = (c['W1'], c['b1'], c['w2'], c['b2'], c['range'], Q)
    taus = c['taus'].reshape(-1, 1)
    good = TF.Pair(taus[:Q * B], taus[Q * B:])
    with pytest.raises(ValueError, match='do not fit'):          # a half with too few taus
        TF.iqn_head(TF.Pair(c['f'][:B], c['f'][B:]), TF.Pair(taus[:Q * B - 1], taus[Q * B:2 * Q * B - 1]), None, *params)
    with pytest.raises(ValueError, match='do not fit'):          # features of another width than W1
        TF.iqn_head(TF.Pair(c['f'][:B, :63], c['f'][B:, :63]), good, None, *params)
    with pytest.raises(ValueError, match='do not fit'):
        TF.iqn_head(c['f'][:B], taus[:Q * B - 1], None, *params)
    with pytest.raises(ValueError, match='do not fit'):          # an embedding range of another length than W1's rows
        TF.iqn_head(c['f'][:B], taus[:Q * B], None, c['W1'], c['b1'], c['w2'], c['b2'], c['range'][:19], Q)
    with pytest.raises(TypeError):
        TF.iqn_head(TF.Pair(c['f'][:B], c['f'][B:]), taus, None, *params)


# ----------------------------------------------------------------------------------------- fused head == composed head
def _head(cls, C, taus, **iqn_kw):
    torch.manual_seed(3)
    head = cls(C, 1)
    if iqn_kw:
        head.iqn = iqn_models.IQN(C, **iqn_kw)
    with torch.no_grad():
        for p in head.parameters():
            if p.dim() > 1:
                p.mul_(3.)
    served = iter(taus)
    head.iqn.tau_source = lambda rows, q: next(served).clone()
    return head


def _run_head(head, x, targets, paired, monkeypatch, fused):
    """One D-phase-like use of the head: loss + 5 * R1(p_real) -> (p, loss, gp, parameter gradients, input gradient)."""
    monkeypatch.setenv('TG_IQN_FUSED_HEAD', '1' if fused else '0')
    head.zero_grad()
    B = x.shape[0] // 2
    real = x[:B].clone().requires_grad_(True)
    fake = x[B:].clone().requires_grad_(True)
    if paired:
        p, loss = head(TF.Pair(real, fake), targets=targets)
        p_real, p_all = p.r, torch.cat([p.r, p.f])
    else:
        p_real, loss_r = head(real, targets=targets[:B])
        p_fake, loss_f = head(fake, targets=targets[B:])
        loss, p_all = TF.add(loss_r, loss_f), torch.cat([p_real, p_fake])
    gp = gradient_penalty(p_real, real)
    TF.add(loss, TF.scale(gp, 5.0)).backward()
    return [p_all.detach(), loss.detach(), gp.detach()] + [p.grad.clone() for p in head.parameters()] + [real.grad, fake.grad]


@pytest.mark.parametrize('paired', [True, False], ids=['paired', 'unpaired'])
def test_fused_head_equals_composed_head_forward_gradients_and_r1(paired, monkeypatch):
    B, C, Q = 3, 20, 8
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2 * B, C, 2, 2, generator=gen)
    targets = torch.cat([torch.ones(B, 1), torch.zeros(B, 1)])
    taus = [torch.rand(Q * B, 1, generator=gen) for _ in range(2)]
    runs = []
    for fused in (True, False):
        head = _head(FusedIQNDiscriminatorOutput, C, taus)
        runs.append(_run_head(head, x, targets, paired, monkeypatch, fused))
    names = ['p', 'loss', 'gp'] + [n for n, _ in head.named_parameters()] + ['real.grad', 'fake.grad']
    assert len(names) == len(runs[0])
    for name, a, b in zip(names, *runs):
        assert float(b.abs().max()) > 0, name
        assert _rel(a, b.double()) <= 1e-6, (name, _rel(a, b.double()))
    # the same state_dict keys as the composed head, and a sampling call (no targets) returns the prediction alone
    assert list(head.state_dict()) == list(IQNDiscriminatorOutput(C, 1).state_dict())
    head.iqn.tau_source = lambda rows, q: taus[0]
    monkeypatch.setenv('TG_IQN_FUSED_HEAD', '1')
    assert torch.is_tensor(head(x[:B])) and head(x[:B]).shape == (B, 1)


class _Counting(SI.SharedIQNEmulator):
    """Counts every call by entry-point name."""

    def __init__(self):
        self.calls = {}

    def __getattribute__(self, name):
        value = super().__getattribute__(name)
        if name.startswith('_') or name == 'calls' or not callable(value):
            return value
        calls = super().__getattribute__('calls')

        def counted(*args):
            calls[name] = calls.get(name, 0) + 1
            return value(*args)
        return counted


@pytest.mark.parametrize('why', ['fused', 'env', 'mix', 'embedding', 'out_dims'])
def test_fallback_conditions(why, monkeypatch):
    B, C, Q = 2, 6, 8
    gen = torch.Generator().manual_seed(5)
    taus = [torch.rand(Q * B, 1, generator=gen)] * 4
    kw = {}
    if why == 'mix':
        kw = dict(mix='add')
    if why == 'embedding':
        class Other(iqn_models.CosineQuantileEmbedding):
            pass
        kw = dict(quantile_embedding_factory=Other)
    torch.manual_seed(3)
    head = FusedIQNDiscriminatorOutput(C, 2 if why == 'out_dims' else 1)
    if kw:
        head.iqn = iqn_models.IQN(C, **kw)
    head.iqn.tau_source = lambda rows, q: taus[0]
    if why == 'env':
        monkeypatch.setenv('TG_IQN_FUSED_HEAD', '0')
    counting = _Counting()
    backend._set_backend_for_testing(counting)
    x = torch.randn(B, C, 2, 2, generator=gen)
    if why == 'out_dims':
        assert head(x).shape == (B, 2)
        with pytest.raises(NotImplementedError):
            head(x, targets=torch.ones(B, 1))
    else:
        p, loss = head(x, targets=torch.ones(B, 1))
        assert p.shape == (B, 1) and loss.dim() == 0
    fused_calls = sum(counting.calls.get(n, 0) for n in HEAD_CALLS)
    assert (fused_calls > 0) == (why == 'fused'), counting.calls
    assert (counting.calls.get('iqn_cos_embed', 0) > 0) == (why != 'fused')


# ------------------------------------------------------------------------------------------------- against the fixtures
@pytest.mark.parametrize('case', SI.SHARED_IQN_CASES)
def test_models_have_the_reference_keys_counts_and_default_init(case):
    fx = SI.load_shared_iqn_fixture(case)
    tr = SI.shared_iqn_trainer(fx, 'cpu')
    assert type(tr.d) is SharedIQNDiscriminator and type(tr.d.to_output) is FusedIQNDiscriminatorOutput
    for net in ('g', 'd'):
        module = getattr(tr, net)
        assert list(module.state_dict().keys()) == fx['state_keys'][net]
        assert [n for n, _ in module.named_parameters()] == fx['param_names'][net]
        assert len(list(module.parameters())) == fx['n_params'][net + '_tensors']
        assert sum(p.numel() for p in module.parameters()) == fx['n_params'][net]
    di = fx['default_init']
    assert _close(SI.total_l2(tr.g), di['g_l2'], 1e-6)
    assert _close(SI.total_l2(tr.target_g), di['target_g_l2'], 1e-6)
    assert _close(SI.total_l2(tr.d), di['d_l2'], 1e-6)
    for net in ('g', 'd'):
        for name, v in getattr(tr, net).state_dict().items():
            ref = di[net][name]
            got = summarize(v, len(ref['idx']))
            assert _close(got['l2'], ref['l2'], 1e-6) and _close(got['sum'], ref['sum'], 1e-6, 1e-5), (net, name)
    # the reference's quirk: the head is BatchNorm2d + LeakyReLU(0.2) whatever --norm / --activation say
    assert fx['head_modules'] == ['BatchNorm2d', 'LeakyReLU']
    norm, act = tr.d.to_output.activation
    assert type(norm) is BatchNorm2d and type(act) is LeakyReLU and act.negative_slope == 0.2
    if fx['flags'].get('norm') == 'id':
        assert 'to_output.activation.0.running_var' in fx['state_keys']['d']
        assert not any(isinstance(m, BatchNorm2d) for m in tr.d.blocks.modules())       # ... and nowhere else


@pytest.mark.parametrize('case', SI.SHARED_IQN_CASES)
def test_forward_pins(case):
    import copy
    fx = SI.load_shared_iqn_fixture(case)
    tr = SI.shared_iqn_trainer(fx, 'cpu')
    SI.load_procedural(tr, fx)
    B = fx['batch']
    with torch.no_grad():
        g2, d2 = copy.deepcopy(tr.g), copy.deepcopy(tr.d)
        z = torch.randn(B, tr.gan_config.latent_dims, generator=torch.Generator().manual_seed(99))
        g_out = g2(z)
        torch.manual_seed(555)
        p_real, loss_real = d2(synthetic_images(B, fx['size'], fx['img_seed']), targets=torch.ones(B, 1))
        p_fake, loss_fake = d2(g_out, targets=torch.zeros(B, 1))
    ref = fx['forward']['g_out']
    got = summarize(g_out, len(ref['idx']))
    assert got['numel'] == ref['numel'] and _close(got['l2'], ref['l2'], 1e-5)
    for got, name in ((p_real, 'd_real'), (p_fake, 'd_fake')):
        for a, b in zip(got.reshape(-1).tolist(), fx['forward'][name]):
            assert _close(a, b, 1e-5, 1e-5), name
    assert _close(float(loss_real), fx['forward']['d_real_loss'], 1e-5) and _close(float(loss_fake), fx['forward']['d_fake_loss'], 1e-5)


def _replayed_taus(fx, steps):
    torch.manual_seed(fx['rng_seed'])
    out, rows = [], fx['num_quantiles'] * fx['batch']
    for _ in range(steps):
        for kind in ('z', 'tau', 'tau', 'z', 'tau'):
            if kind == 'z':
                torch.randn(fx['batch'], fx['latent_dims'])
            else:
                out.append(torch.rand(rows, 1))
    return out


@pytest.mark.parametrize('pairs', [True, False], ids=['paired', 'unpaired'])
@pytest.mark.parametrize('case', SI.SHARED_IQN_CASES)
def test_trainer_matches_reference_fixture(case, pairs, single_thread):
    """BOTH steps at 1e-4: losses, parameter and gradient L2s; the taus bit for bit in the reference's draw order."""
    fx = SI.load_shared_iqn_fixture(case)
    tr = SI.shared_iqn_trainer(fx, 'cpu', pair_d=pairs, pair_g=pairs)
    SI.load_procedural(tr, fx)
    assert tr._d_pairable() == pairs and tr._g_pairable() == pairs
    iqn = tr.d.to_output.iqn
    drawn, sample = [], iqn.sample_quantiles
    def sample_quantiles(n=1):          # (a clone: the feed serves later steps from the same buffers)
        taus = sample(n)
        drawn.append(taus.detach().clone())
        return taus
    iqn.sample_quantiles = sample_quantiles
    torch.manual_seed(fx['rng_seed'])
    for k, ref in enumerate(fx['steps']):
        logs = tr.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + k))
        for name in ('g_loss', 'd_loss', 'gp'):
            assert _close(logs[name], ref[name], 1e-4), (case, k, name, logs[name], ref[name])
        assert _close(SI.total_l2(tr.g), ref['g_l2'], 1e-4)
        assert _close(SI.total_l2(tr.d), ref['d_l2'], 1e-4)
        assert _close(SI.total_l2(tr.target_g), ref['target_g_l2'], 1e-4)
        assert _close(SI.total_l2(tr.g, True), ref['g_grad_l2'], 1e-4), (case, k)
        assert _close(SI.total_l2(tr.d, True), ref['d_grad_l2'], 1e-4), (case, k)
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
    assert float(torch.rand(1)) == fx['rng_after']
    z, t = ('z', fx['batch'], fx['latent_dims']), ('tau', fx['num_quantiles'] * fx['batch'], fx['num_quantiles'])
    assert tr.rng_feed.plan == [z, t, t, z, t] == tr._rng_plan(fx['batch'])
    want = _replayed_taus(fx, len(fx['steps']))
    assert len(drawn) == len(want) == 3 * len(fx['steps'])
    for i, (got, ref) in enumerate(zip(drawn, want)):
        assert got.shape == ref.shape and torch.equal(got.view(torch.int32), ref.view(torch.int32)), i
        assert got.reshape(-1)[:4].tolist() == fx['taus'][i // 3][i % 3]


def test_selu_initialises_the_head_too_and_elu_is_unknown():
    fx = SI.load_shared_iqn_fixture('shared_iqn_c16_b4')
    tr = SI.shared_iqn_trainer(fx, 'cpu', activation='selu')
    norm, act = tr.d.to_output.activation
    assert type(norm) is BatchNorm2d and type(act) is LeakyReLU                  # the quirk: not SELU
    assert float(norm.weight.detach().abs().max()) == 0.0                                 # init_params_selu zeroes every vector of d
    assert float(tr.d.to_output.to_output[0].bias.detach().abs().max()) == 0.0
    with pytest.raises(KeyError):
        SI.shared_iqn_trainer(fx, 'cpu', activation='elu')


# -------------------------------------------------------------------------------------------------- launches of the head
def _count_step(fx, fused, monkeypatch):
    monkeypatch.setenv('TG_IQN_FUSED_HEAD', '1' if fused else '0')
    tr = SI.shared_iqn_trainer(fx, 'cpu')
    SI.load_procedural(tr, fx)
    torch.manual_seed(fx['rng_seed'])
    tr.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed']))            # records the draw order
    counting = _Counting()
    prev = backend._set_backend_for_testing(counting)
    tr.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + 1))
    backend._set_backend_for_testing(prev)
    return dict(counting.calls)


def test_head_launches_per_step(monkeypatch):
    """The fused trainer spends at most 10 ``iqn_head_*`` calls per step on the head (D phase: forward, R1's backward, the double
    backward, the loss's backward; G phase: forward + backward; here a forward with targets is one call, two launches on the
    device) and none of the composed head's.  Config '16' has no attention and its generator's input MLP is the only other
    ``gemm`` user, so the composed head's calls are counted as the difference between the two runs."""
    fx = SI.load_shared_iqn_fixture('shared_iqn_c16_b4')
    fused, composed = _count_step(fx, True, monkeypatch), _count_step(fx, False, monkeypatch)
    n_fused = sum(fused.get(n, 0) for n in HEAD_CALLS)
    head_composed = {n: composed.get(n, 0) - fused.get(n, 0) for n in COMPOSED_HEAD_CALLS}
    print(f'HEAD LAUNCHES per step: fused {n_fused} iqn_head_* ({ {n: fused.get(n, 0) for n in HEAD_CALLS} }), '
          f'composed {sum(head_composed.values())} ({head_composed})')
    forwards_with_loss = 2                    # D phase, G phase: each has a one-workgroup finisher on the device
    assert 0 < n_fused + forwards_with_loss <= 10
    assert fused.get('iqn_head_fwd') == 2 and fused.get('iqn_head_bwd') == 4
    for n in ('mul', 'repeat_rows', 'repeat_rows_groups', 'sum_reps', 'sum_reps_groups', 'iqn_cos_embed', 'iqn_loss', 'iqn_loss_groups'):
        assert fused.get(n, 0) == 0, (n, fused.get(n))          # nobody else in this model uses them
    assert fused.get('gemm') == 2          # the generator's input MLP, forward and weight gradient: none of the head's Linear layers
    assert fused.get('tanh_fwd') == 1 and fused.get('tanh_bwd') == 1          # the generator's output stage, once each way
    assert all(v >= 0 for v in head_composed.values()) and sum(head_composed.values()) >= 30
    assert sum(composed.get(n, 0) for n in HEAD_CALLS) == 0
