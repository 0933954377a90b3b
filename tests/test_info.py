"""The InfoGAN trainer's host logic on the CPU: ``functional.info_code_loss``, the two-headed discriminator output, the
code-carrying latent draw of ``RngFeed``, ``trainers.info.InfoTrainer`` and its sampler component, run over a float64 form of the
new entry point (info_cases.InfoEmulator) and compared with the fixtures the reference's own trainer produced
(tests/golden/info_*.json, made by tests/golden/make_info_golden.py).

Nothing here says anything about the HIP kernel (tests/test_code_loss_gpu.py, test_info_gpu.py)."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import info_cases as IC
from oracle.procedural import summarize, synthetic_images
from tartangan_amd import backend, functional as TF
from tartangan_amd.models.blocks import LinearOutput, MultiModelDiscriminatorOutput
from tartangan_amd.models.layers import BatchNorm2d
from tartangan_amd.trainers.cnn import CNNTrainer
from tartangan_amd.trainers.info import InfoTrainer
from tartangan_amd.trainers.trainer import RngFeed

KEYS = ('g_loss', 'g_code_loss', 'd_loss', 'd_code_loss', 'gp')


@pytest.fixture(autouse=True)
def emulated_backend():
    prev = backend._set_backend_for_testing(IC.InfoEmulator())
    yield
    backend._set_backend_for_testing(prev)


def _close(a, b, rel=1e-4, abs_=1e-6):
    return abs(a - b) <= abs_ + rel * max(abs(a), abs(b))


def _np_state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


def _images(fx, k):
    return synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + k)


# ------------------------------------------------------------------------------------------------- against the fixtures
@pytest.mark.parametrize('case', IC.INFO_CASES)
def test_models_have_the_reference_keys_counts_and_default_init(case):
    fx = IC.load_info_fixture(case)
    tr = IC.info_trainer(fx, 'cpu')
    for net in ('g', 'd'):
        module = getattr(tr, net)
        assert list(module.state_dict().keys()) == fx['state_keys'][net]
        assert len(list(module.parameters())) == fx['n_params'][net + '_tensors']
        assert sum(p.numel() for p in module.parameters()) == fx['n_params'][net]
    assert list(tr.target_g.state_dict().keys()) == fx['state_keys']['g']
    tail = [k.split('.', 2)[2] for k in fx['state_keys']['d'][-4:]]
    assert tail == ['output_models.0.xform.0.weight', 'output_models.0.xform.0.bias',
                    'output_models.1.xform.0.weight', 'output_models.1.xform.0.bias']
    codes = fx['flags']['info_cat_dims'] + fx['flags']['info_cont_dims']
    assert tr.d.state_dict()[fx['state_keys']['d'][-2]].shape[0] == codes
    di = fx['default_init']
    assert _close(IC.total_l2(tr.g), di['g_l2'], 1e-6)
    assert _close(IC.total_l2(tr.target_g), di['target_g_l2'], 1e-6)          # (the second draw of the init stream)
    assert _close(IC.total_l2(tr.d), di['d_l2'], 1e-6)
    for name, v in tr.d.state_dict().items():
        ref = di['d'][name]
        got = summarize(v, len(ref['idx']))
        assert _close(got['l2'], ref['l2'], 1e-6) and _close(got['sum'], ref['sum'], 1e-6, 1e-5), name
        assert got['samples'] == pytest.approx(ref['samples'], rel=1e-6, abs=1e-7), name


@pytest.mark.parametrize('pairs', [True, False], ids=['paired', 'unpaired'])
@pytest.mark.parametrize('case', IC.INFO_CASES)
def test_trainer_matches_reference_fixture(case, pairs, single_thread):
    """BOTH steps at 1e-4: the five logs and the parameter and gradient L2s; both host streams end where the reference's did."""
    fx = IC.load_info_fixture(case)
    tr = IC.info_trainer(fx, 'cpu', pair_d=pairs, pair_g=pairs)
    IC.load_procedural(tr, fx)
    assert tr._d_pairable() == pairs and tr._g_pairable() == pairs
    IC.seed_step_streams(fx)
    for k, ref in enumerate(fx['steps']):
        logs = tr.train_batch(_images(fx, k))
        assert tuple(logs) == KEYS
        got = IC.step_entry(tr, logs)
        for name, want in ref.items():
            assert _close(got[name], want, 1e-4), (case, k, name, got[name], want)
    kind = 'zc' if fx['flags']['info_cat_dims'] else 'z'
    assert tr.rng_feed.plan == [(kind, fx['batch'], tr.gan_config.latent_dims)] * 2
    assert dict(torch=float(torch.rand(1)), numpy=float(np.random.rand())) == fx['rng_after']


def test_cont_only_case_never_draws_from_numpy():
    fx = IC.load_info_fixture('info_c16_b2_id_cont')
    tr = IC.info_trainer(fx, 'cpu')
    IC.load_procedural(tr, fx)
    IC.seed_step_streams(fx)
    before = np.random.get_state()
    for k in range(3):                              # recorded plan, refill, prefetch: none of them may touch numpy
        tr.train_batch(_images(fx, k))
    tr.sample_z(5)
    assert _np_state_equal(np.random.get_state(), before)


def test_every_parameter_trains_both_heads_included():
    """The stock blocks own no module that never runs (unlike the shared family's first block): after one step every tensor of
    G and D, the code head's included, has a gradient that is not identically zero."""
    fx = IC.load_info_fixture('info_c16_b4')
    tr = IC.info_trainer(fx, 'cpu')
    IC.load_procedural(tr, fx)
    IC.seed_step_streams(fx)
    tr.train_batch(_images(fx, 0))
    idle = [(net, n) for net in ('g', 'd') for n, p in getattr(tr, net).named_parameters() if float(p.grad.abs().max()) == 0.0]
    assert idle == []
    assert sum('output_models' in n for n, _ in tr.d.named_parameters()) == 4


# ------------------------------------------------------------------------------------------------------ the autograd op
def _case64(B, C, K, ldz=None, seed=0):
    gen = torch.Generator().manual_seed(seed + 100 * B + 10 * C + K)
    ldz = ldz or C + K + 2
    codes = torch.randn(B, C + K, dtype=torch.float64, generator=gen)
    z = torch.randn(B, ldz, dtype=torch.float64, generator=gen)
    if C:
        z[:, :C] = 0.
        z[torch.arange(B), torch.randint(0, C, (B,), generator=gen)] = 1.
    return codes, z


def _truth(codes, z, C, K, w, base):
    code = torch.zeros((), dtype=codes.dtype)
    if C:
        code = code + F.binary_cross_entropy_with_logits(codes[:, :C], z[:, :C])
    if K:
        code = code + F.mse_loss(codes[:, C:], z[:, C:C + K])
    return code, (0. if base is None else base) + w * code


@pytest.mark.parametrize('shape', [(1, 1, 0), (1, 0, 1), (2, 3, 2)], ids=str)
@pytest.mark.parametrize('with_base', [False, True], ids=['no base', 'base'])
def test_info_code_loss_values_and_gradcheck(shape, with_base):
    B, C, K = shape
    codes, z = _case64(B, C, K)
    codes.requires_grad_(True)
    base = torch.tensor(0.75, dtype=torch.float64, requires_grad=True) if with_base else None
    w = 0.5
    code, total = TF.info_code_loss(codes, z, C, K, w, base=base)
    want_code, want_total = _truth(codes.detach(), z, C, K, w, None if base is None else base.detach())
    assert code.shape == total.shape == () and not code.requires_grad and total.requires_grad
    assert abs(float(code) - float(want_code)) <= 1e-12 and abs(float(total.detach()) - float(want_total)) <= 1e-12
    inputs = (codes, base) if with_base else (codes,)
    assert torch.autograd.gradcheck(lambda c, b=None: TF.info_code_loss(c, z, C, K, w, base=b)[1], inputs)


def test_info_code_loss_sends_nothing_to_z_and_rejects_misfits():
    codes, z = _case64(2, 3, 2)
    codes.requires_grad_(True)
    z.requires_grad_(True)
    _, total = TF.info_code_loss(codes, z, 3, 2, 1.0)
    gc, gz = torch.autograd.grad(total, (codes, z), allow_unused=True)
    assert gz is None and gc is not None
    for bad in (lambda: TF.info_code_loss(codes, z, 3, 1, 1.0), lambda: TF.info_code_loss(codes, z[:1], 3, 2, 1.0),
                lambda: TF.info_code_loss(codes.view(-1), z, 3, 2, 1.0)):
        with pytest.raises(ValueError):
            bad()


def test_using_the_reported_value_alone_runs_no_backward():
    calls = collections.Counter()

    class Counting(IC.InfoEmulator):
        def scale_dev(self, *a):
            calls['scale_dev'] += 1
            return super().scale_dev(*a)

    backend._set_backend_for_testing(Counting())
    codes, z = _case64(2, 3, 2)
    codes = codes.float().requires_grad_(True)
    other = codes.sum()
    code, total = TF.info_code_loss(codes, z.float(), 3, 2, 1.0)
    assert not code.requires_grad and code.grad_fn is None
    (other + code).backward()                     # the node of ``total`` is not reached at all
    assert calls['scale_dev'] == 0
    assert torch.equal(codes.grad, torch.ones_like(codes))
    total.backward()
    assert calls['scale_dev'] == 1


# ------------------------------------------------------------------------------------------------------------- the head
def test_head_takes_a_pair_and_the_real_half_codes_get_no_gradient():
    torch.manual_seed(3)
    head = MultiModelDiscriminatorOutput(
        6, 1, [lambda d: LinearOutput(d, out_dims=1), lambda d: LinearOutput(d, out_dims=4)], norm_factory=BatchNorm2d)
    gen = torch.Generator().manual_seed(4)
    r, f = (torch.randn(3, 6, 2, 2, generator=gen, requires_grad=True) for _ in range(2))
    p_labels, p_codes = head(TF.Pair(r, f))
    assert isinstance(p_labels, TF.Pair) and isinstance(p_codes, TF.Pair)
    assert p_labels.r.shape == (3, 1) and p_codes.f.shape == (3, 4)
    # the fake half of the paired head output starts at row B of one (2B, 4) buffer
    assert p_codes.f.data_ptr() == p_codes.r.data_ptr() + 3 * 4 * 4
    p_codes.r.retain_grad()
    (p_labels.r.sum() + 2 * p_labels.f.sum() + p_codes.f.pow(2).sum()).backward()
    assert p_codes.r.grad is None
    # against the two separate evaluations of the reference
    twin = MultiModelDiscriminatorOutput(
        6, 1, [lambda d: LinearOutput(d, out_dims=1), lambda d: LinearOutput(d, out_dims=4)], norm_factory=BatchNorm2d)
    twin.load_state_dict(head.state_dict())
    r2, f2 = r.detach().clone().requires_grad_(True), f.detach().clone().requires_grad_(True)
    lr, _ = twin(r2)
    lf, cf = twin(f2)
    assert isinstance(lr, torch.Tensor)
    (lr.sum() + 2 * lf.sum() + cf.pow(2).sum()).backward()
    assert torch.allclose(r.grad, r2.grad, rtol=1e-5, atol=1e-6) and torch.allclose(f.grad, f2.grad, rtol=1e-5, atol=1e-6)
    for (n, p), (_, q) in zip(head.named_parameters(), twin.named_parameters()):
        assert torch.allclose(p.grad, q.grad, rtol=1e-5, atol=1e-6), n
    assert list(head.state_dict()) == ['activation.0.weight', 'activation.0.bias', 'activation.0.running_mean', 'activation.0.running_var',
                                       'activation.0.num_batches_tracked', 'output_models.0.xform.0.weight', 'output_models.0.xform.0.bias',
                                       'output_models.1.xform.0.weight', 'output_models.1.xform.0.bias']


# ------------------------------------------------------------------------------------------------- launches of the step
COUNTED = ('info_code_loss', 'bce_logits', 'add', 'scale')


def _counting():
    calls = collections.Counter()

    def wrap(name):
        def method(self, *a):
            calls[name] += 1
            return getattr(IC.InfoEmulator, name)(self, *a)
        return method
    return type('Counting', (IC.InfoEmulator,), {n: wrap(n) for n in COUNTED})(), calls


def _second_step_calls(tr, fx, procedural=True):
    counting, calls = _counting()
    backend._set_backend_for_testing(counting)
    if procedural:
        IC.load_procedural(tr, fx)
    IC.seed_step_streams(fx)
    tr.train_batch(_images(fx, 0))
    calls.clear()
    logs = tr.train_batch(_images(fx, 1))
    return dict(calls), logs


@pytest.mark.parametrize('pairs', [True, False], ids=['paired', 'unpaired'])
def test_one_code_loss_launch_per_phase_and_nothing_else_on_top_of_the_stock_step(pairs):
    fx = IC.load_info_fixture('info_c16_b4')
    info, _ = _second_step_calls(IC.info_trainer(fx, 'cpu', pair_d=pairs, pair_g=pairs), fx)
    stock_fx = dict(fx, flags={})
    stock, _ = _second_step_calls(IC.info_trainer(stock_fx, 'cpu', cls=CNNTrainer, pair_d=pairs, pair_g=pairs), stock_fx)
    assert info.pop('info_code_loss') == 2 and 'info_code_loss' not in stock
    assert info == stock and info['bce_logits'] == 2


def test_without_codes_no_code_loss_call_and_zero_entries():
    fx = IC.load_info_fixture('info_c16_b4')
    fx = dict(fx, flags=dict(info_cat_dims=0, info_cont_dims=0, info_w=1.))
    # (default weights: the procedural rules have none for a head of no columns)
    calls, logs = _second_step_calls(IC.info_trainer(fx, 'cpu'), fx, procedural=False)
    assert 'info_code_loss' not in calls
    assert tuple(logs) == KEYS and logs['g_code_loss'] == 0. and logs['d_code_loss'] == 0.
    assert type(logs['g_code_loss']) is float and logs['gp'] > 0 and logs['g_loss'] > 0
    tr = IC.info_trainer(fx, 'cpu')
    state = np.random.get_state()
    tr.sample_z(3)
    assert _np_state_equal(np.random.get_state(), state)


def test_five_losses_come_from_one_read_back():
    fx = IC.load_info_fixture('info_c16_b4')
    tr = IC.info_trainer(fx, 'cpu')
    IC.load_procedural(tr, fx)
    seen = []
    tr._read_back = lambda vals, _rb=tr._read_back: (seen.append(tuple(vals.shape)), _rb(vals))[-1]
    IC.seed_step_streams(fx)
    tr.train_batch(_images(fx, 0))
    assert seen == [(5,)]
    tr.args.grad_penalty = 0.
    logs = tr.train_batch(_images(fx, 1))
    assert seen == [(5,), (4,)] and logs['gp'] == 0. and logs['d_code_loss'] > 0


def test_unknown_activation_and_cli():
    fx = IC.load_info_fixture('info_c16_b4')
    with pytest.raises(KeyError):
        IC.info_trainer(fx, 'cpu', activation='elu')
    args = InfoTrainer.default_args()
    assert (args.info_cat_dims, args.info_cont_dims, args.info_w) == (10, 5, 1.)
    from tartangan_amd.trainers import info
    with pytest.raises(SystemExit):
        info.main()


# ---------------------------------------------------------------------------------------------------------------- latents
def _reference_z(n, latent, C):
    """trainers/info.py:204-213, written out."""
    z = torch.randn(n, latent)
    if C:
        z[..., :C] = 0.
        cats = np.random.randint(0, C, (n,))
        z[np.arange(n), ..., cats] = 1.
    return z


@pytest.mark.parametrize('C', [10, 1, 0])
def test_sample_z_is_byte_equal_to_the_reference_recipe(C):
    fx = IC.load_info_fixture('info_c16_b4')
    tr = IC.info_trainer(dict(fx, flags=dict(fx['flags'], info_cat_dims=C)), 'cpu')
    latent = tr.gan_config.latent_dims
    torch.manual_seed(5)
    np.random.seed(6)
    got = [tr.sample_z(7), tr.sample_z(), tr.sample_g(3)[1]]
    state = np.random.get_state()
    torch.manual_seed(5)
    np.random.seed(6)
    want = [_reference_z(7, latent, C), _reference_z(fx['batch'], latent, C), _reference_z(3, latent, C)]
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert _np_state_equal(np.random.get_state(), state)
    if C:
        assert all(torch.equal(a[:, :C].sum(1), torch.ones(len(a))) and float(a[:, :C].max()) == 1. for a in got)
        assert torch.equal(tr.z_categorical_code(got[0]), got[0][:, :C])
        assert torch.equal(tr.z_continuous_code(got[0]), got[0][:, C:C + 5])
    else:
        np.random.seed(6)
        assert _np_state_equal(np.random.get_state(), state)          # nothing was drawn
    imgs = _images(fx, 0)
    batch, labels, z = tr.make_adversarial_batch(imgs)
    assert batch.shape[0] == 2 * len(imgs) and labels[:len(imgs)].min() == 1 and labels[len(imgs):].max() == 0 and z.shape == (len(imgs), latent)
    gen, ones, z = tr.make_generator_batch(imgs)
    assert gen.shape == imgs.shape and float(ones.min()) == 1. and z.shape == (len(imgs), latent)


def test_ranks_rows_concatenate_to_the_single_process_tensor():
    def draws(rank, world, rows):
        feed = RngFeed('cpu', rank, world)
        feed.cat_dims = 3
        torch.manual_seed(8)
        np.random.seed(9)
        a = feed.draw('zc', rows, 6).clone()               # record mode: inline draws (into what become the static buffers)
        b = feed.draw('zc', rows, 6).clone()
        feed.mode = 'serve'
        feed.refill()                                      # and the same plan drawn into the staging buffers
        return a, b, feed.static[0].clone(), feed.static[1].clone(), np.random.get_state(), torch.get_rng_state()
    whole = draws(0, 1, 4)
    halves = [draws(r, 2, 2) for r in (0, 1)]
    for i in range(4):
        assert torch.equal(torch.cat([halves[0][i], halves[1][i]]), whole[i]), i
    for h in halves:
        assert _np_state_equal(h[4], whole[4]) and torch.equal(h[5], whole[5])
    assert not torch.equal(whole[0], whole[2])             # (the refill drew NEW values)
    assert torch.equal(whole[0][:, :3].sum(1), torch.ones(4))


def _feed_with_plan():
    feed = RngFeed('cpu')
    feed.cat_dims = 4
    feed.adopt([('zc', 3, 8), ('zc', 3, 8)])
    feed.mode = 'serve'
    return feed


def _inline(feed_plan, C):
    out = []
    for _, rows, cols in feed_plan:
        out.append(_reference_z(rows, cols, C))
    return out


def test_a_numpy_draw_between_steps_drops_the_speculation():
    """Only numpy's stream moves between the steps: torch's state alone would say 'adopt'."""
    feed = _feed_with_plan()
    torch.manual_seed(10)
    np.random.seed(11)
    feed.refill()
    feed.prefetch()
    foreign = np.random.randint(0, 4, 2)                   # e.g. a sampler's sample_z in between ... sees the untouched stream
    feed.refill()
    got = [t.clone() for t in feed.static]
    end = (torch.get_rng_state(), np.random.get_state())
    torch.manual_seed(10)
    np.random.seed(11)
    _inline(feed.plan, 4)
    assert np.array_equal(np.random.randint(0, 4, 2), foreign)
    want = _inline(feed.plan, 4)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(end[0], torch.get_rng_state()) and _np_state_equal(end[1], np.random.get_state())


def test_a_torch_draw_between_steps_drops_the_speculation_and_restores_numpy():
    feed = _feed_with_plan()
    torch.manual_seed(10)
    np.random.seed(11)
    feed.refill()
    feed.prefetch()
    foreign = torch.randn(3)
    feed.refill()
    got = [t.clone() for t in feed.static]
    torch.manual_seed(10)
    np.random.seed(11)
    _inline(feed.plan, 4)
    assert torch.equal(torch.randn(3), foreign)
    for a, b in zip(got, _inline(feed.plan, 4)):
        assert torch.equal(a, b)


def test_an_undisturbed_prefetch_ends_where_inline_draws_end():
    feed = _feed_with_plan()
    torch.manual_seed(12)
    np.random.seed(13)
    feed.refill()
    feed.prefetch()
    mid = (torch.get_rng_state(), np.random.get_state())
    feed.refill()
    assert feed._spec is None
    got = [t.clone() for t in feed.static]
    end = (torch.get_rng_state(), np.random.get_state())
    torch.manual_seed(12)
    np.random.seed(13)
    _inline(feed.plan, 4)
    assert torch.equal(mid[0], torch.get_rng_state()) and _np_state_equal(mid[1], np.random.get_state())   # prefetch put both back
    for a, b in zip(got, _inline(feed.plan, 4)):
        assert torch.equal(a, b)
    assert torch.equal(end[0], torch.get_rng_state()) and _np_state_equal(end[1], np.random.get_state())


def test_stock_plans_do_not_look_at_numpy():
    feed = RngFeed('cpu')
    feed.adopt([('z', 3, 8), ('tau', 6, 2), ('z', 3, 8)])
    feed.mode = 'serve'
    assert feed._host_streams()[1] is None
    torch.manual_seed(14)
    feed.refill()
    feed.prefetch()
    np.random.randint(0, 4, 2)                              # numpy is not the stock plans' business
    before = torch.get_rng_state()
    feed.refill()
    assert not torch.equal(before, torch.get_rng_state())   # adopted: the state jumped to the remembered one
    torch.manual_seed(14)
    for _ in range(2):
        want = [torch.randn(3, 8), torch.rand(6, 1), torch.randn(3, 8)]
    for a, b in zip(feed.static, want):
        assert torch.equal(a, b)


def test_trainer_with_and_without_prefetch_and_with_a_sampler_in_between_sees_the_same_values():
    fx = IC.load_info_fixture('info_c16_b4')
    runs = []
    for prefetch in (True, False):
        tr = IC.info_trainer(fx, 'cpu', prefetch_rng=prefetch)
        IC.load_procedural(tr, fx)
        IC.seed_step_streams(fx)
        logs = []
        for k in range(3):
            logs.append(tr.train_batch(_images(fx, k)))
            if k == 1:
                tr.sample_z(2)                             # moves both streams between two steps
        runs.append((logs, float(torch.rand(1)), float(np.random.rand())))
    assert runs[0] == runs[1]


# ---------------------------------------------------------------------------------------------------- sampler component
@pytest.mark.parametrize('C,K', [(3, 5), (0, 2), (2, 0)])
def test_sampler_sweeps_and_pngs(tmp_path, C, K):
    from PIL import Image
    from tartangan_amd.trainers.components import InfoImageSamplerComponent
    fx = IC.load_info_fixture('info_c16_b4')
    fx = dict(fx, flags=dict(info_cat_dims=C, info_cont_dims=K, info_w=1.))
    tr = IC.info_trainer(fx, 'cpu', output=str(tmp_path), run_id='r', gen_freq=2)
    latent = tr.gan_config.latent_dims
    sm = InfoImageSamplerComponent(tr.args)
    tr.attach(sm)
    torch.manual_seed(15)
    np.random.seed(16)
    sm.on_train_begin(0, {})
    after = (float(torch.rand(1)), float(np.random.rand()))
    # the reference's recipe as arithmetic: progress samples, one base latent, the sweeps, two more latents
    torch.manual_seed(15)
    np.random.seed(16)
    progress = _reference_z(32, latent, C)
    base = _reference_z(1, latent, C)
    cols = min(4, K) + 1
    pts = torch.tensor([-2 + 4 * i / 6 for i in range(7)], dtype=torch.float64).float()
    cont = base[0].expand(7, cols, latent).clone()
    for i in range(cols - 1):
        cont[:, i, C + i] = pts
    cont[:, cols - 1, latent - 1] = pts
    assert torch.equal(sm.progress_samples, progress)
    assert sm.continuous_samples.shape == (7, cols, latent)
    assert torch.allclose(sm.continuous_samples, cont, rtol=0, atol=1e-6)
    assert torch.equal(sm.continuous_samples[:, :, :C], cont[:, :, :C])
    if C:
        three = torch.cat([base, _reference_z(2, latent, C)])
        cat = three[:, None, :].expand(3, C, latent).clone()
        for j in range(C):
            cat[:, j, :C] = 0.
            cat[:, j, j] = 1.
        assert torch.equal(sm.categorical_samples, cat)
    else:
        assert sm.categorical_samples is None
    assert after == (float(torch.rand(1)), float(np.random.rand()))
    name = f'{sm.sample_root}/sample_0.png'
    sm.output_samples(name)
    size, pad = fx['size'], 2
    written = sorted(p.name for p in (tmp_path / 'r' / 'samples').iterdir())
    assert written == (['info_cat_sample_0.png'] if C else []) + ['info_cont_sample_0.png']
    with Image.open(tmp_path / 'r' / 'samples' / 'info_cont_sample_0.png') as im:
        assert im.size == (cols * (size + pad) + pad, 7 * (size + pad) + pad)
    if C:
        with Image.open(tmp_path / 'r' / 'samples' / 'info_cat_sample_0.png') as im:
            assert im.size == (C * (size + pad) + pad, 3 * (size + pad) + pad)


def test_only_rank_zero_writes(tmp_path):
    from tartangan_amd.trainers.components import InfoImageSamplerComponent
    fx = IC.load_info_fixture('info_c16_b4')
    tr = IC.info_trainer(fx, 'cpu', output=str(tmp_path), run_id='r', gen_freq=2)
    sm = InfoImageSamplerComponent(tr.args)
    tr.attach(sm)
    sm.on_train_begin(0, {})
    tr.data_parallel = type('DP', (), dict(rank=1, sync_bn=False))()
    sm.output_samples(f'{sm.sample_root}/sample_0.png')
    assert list((tmp_path / 'r' / 'samples').iterdir()) == []
