"""The scene trainer's host logic on the CPU: ``functional.scene_patches``, ``SceneStructureBlock``,
``StructuredSceneGenerator``, ``SceneTrainer`` and the 'noise' kind of ``RngFeed``, run over the float64 restatement of the
structure stage (scene_cases.SceneEmulator) and compared with the fixtures the reference's own SceneTrainer produced
(tests/golden/scene_*.json, made by tests/golden/make_scene_golden.py).

Nothing here says anything about the HIP kernels (tests/test_affine_patches_gpu.py, tests/test_scene_gpu.py)."""
import copy

import pytest
import torch

import scene_cases as SC
from oracle.procedural import summarize, synthetic_images
from tartangan_amd import backend, functional as TF
from tartangan_amd.models.blocks import SceneStructureBlock
from tartangan_amd.trainers.trainer import RngFeed


@pytest.fixture(autouse=True)
def emulated_backend():
    prev = backend._set_backend_for_testing(SC.SceneEmulator())
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


# ------------------------------------------------------------------------------------------------- against the fixtures
@pytest.mark.parametrize('case', SC.SCENE_CASES)
def test_models_have_the_reference_keys_counts_and_default_init(case):
    fx = SC.load_scene_fixture(case)
    tr = SC.scene_trainer(fx, 'cpu')
    assert list(tr.g.state_dict().keys()) == fx['state_keys']['g']
    assert list(tr.target_g.state_dict().keys()) == fx['state_keys']['g']
    assert list(tr.d.state_dict().keys()) == fx['state_keys']['d']
    assert [n for n, _ in tr.g.named_parameters()] == fx['param_names']['g']        # each parameter once, under its first name
    assert len(list(tr.g.parameters())) == fx['n_params']['g_tensors']
    assert sum(p.numel() for p in tr.g.parameters()) == fx['n_params']['g']
    assert sum(p.numel() for p in tr.d.parameters()) == fx['n_params']['d']
    assert tr.g.blocks[0] is tr.g.structure_generator
    di = fx['default_init']
    assert _close(_total_l2(tr.g), di['g_l2'], 1e-6)
    assert _close(_total_l2(tr.target_g), di['target_g_l2'], 1e-6)
    assert _close(_total_l2(tr.d), di['d_l2'], 1e-6)
    for name, v in tr.g.state_dict().items():          # tensor by tensor: zeroed Linears, the transform bias pattern, ones / zeros
        ref = di['g'][name]
        got = summarize(v, len(ref['idx']))
        assert _close(got['l2'], ref['l2'], 1e-6) and _close(got['sum'], ref['sum'], 1e-6, 1e-5), name
        assert got['samples'] == pytest.approx(ref['samples'], rel=1e-6, abs=1e-7), name
    block = tr.g.structure_generator
    assert float(block.masks[0].weight.detach().abs().max()) == 0 and float(block.patch_transforms[0].weight.detach().abs().max()) == 0
    assert block.patch_transforms[0].bias.tolist() == [2., 0., 0., 0., 2., 0.] * block.num_patches
    assert hasattr(block, 'noise_proto') == bool(fx['flags']['patch_noise'])
    assert hasattr(block, 'full_masks') == (not fx['flags']['refine_patches'])
    assert block.output_channels == fx['flags']['num_patches']


@pytest.mark.parametrize('case', SC.SCENE_CASES)
def test_forward_pins(case):
    fx = SC.load_scene_fixture(case)
    tr = SC.scene_trainer(fx, 'cpu')
    SC.load_procedural(tr, fx)
    with torch.no_grad():
        g2, d2 = copy.deepcopy(tr.g), copy.deepcopy(tr.d)
        z = torch.randn(fx['batch'], tr.gan_config.latent_dims, generator=torch.Generator().manual_seed(99))
        torch.manual_seed(fx['noise_seed'])
        structure = g2.structure_generator(z)
        torch.manual_seed(fx['noise_seed'])
        g_out = g2(z)
        outs = dict(structure=structure, g_out=g_out)
        d_real, d_fake = d2(synthetic_images(fx['batch'], fx['size'], fx['img_seed'])), d2(g_out)
        g2.eval()
        torch.manual_seed(fx['noise_seed'])
        outs['g_out_eval'] = g2(z)
    for name, t in outs.items():
        ref = fx['forward'][name]
        got = summarize(t, len(ref['idx']))
        assert got['numel'] == ref['numel']
        assert _close(got['l2'], ref['l2'], 1e-5), name
        for a, b in zip(got['samples'], ref['samples']):
            assert abs(a - b) <= 1e-5, name
    for got, name in ((d_real, 'd_real'), (d_fake, 'd_fake')):
        for a, b in zip(got.reshape(-1).tolist(), fx['forward'][name]):
            assert _close(a, b, 1e-5, 1e-5), name


@pytest.mark.parametrize('case', SC.SCENE_CASES)
def test_trainer_matches_reference_fixture(case, single_thread):
    """The tolerances tests/test_host_logic.py applies to the cnn fixtures: step 1 from identical state at 1e-4 on the losses,
    later steps sanity-bounded; and the random stream (z, noise, z, noise per step) consumed exactly like the reference."""
    fx = SC.load_scene_fixture(case)
    assert fx['kink']['least_distance'] >= fx['kink']['margin']
    tr = SC.scene_trainer(fx, 'cpu')
    SC.load_procedural(tr, fx)
    torch.manual_seed(fx['rng_seed'])
    for k, ref in enumerate(fx['steps']):
        logs = tr.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + k))
        loss_tol, grad_tol = (1e-4, 1e-3) if k == 0 else (1e-1, 1.0)
        for name in ('g_loss', 'd_loss', 'gp'):
            assert _close(logs[name], ref[name], loss_tol), (case, k, name, logs[name], ref[name])
        assert _close(_total_l2(tr.g), ref['g_l2'], 1e-4)
        assert _close(_total_l2(tr.d), ref['d_l2'], 1e-4)
        assert _close(_total_l2(tr.target_g), ref['target_g_l2'], 1e-4)
        assert _close(_total_l2(tr.g, True), ref['g_grad_l2'], grad_tol), (case, k)
        assert _close(_total_l2(tr.d, True), ref['d_grad_l2'], grad_tol), (case, k)
        if k == 0:
            for name, p in tr.d.named_parameters():
                ref_s = fx['after_step1']['d_grad'][name]
                got = summarize(p.grad, len(ref_s['idx']))
                assert _close(got['l2'], ref_s['l2'], 5e-4, 2e-5 * ref['d_grad_l2']), ('d_grad', name, got['l2'], ref_s['l2'])
            for name, p in tr.g.named_parameters():
                ref_s = fx['after_step1']['g_grad'][name]
                got = summarize(p.grad, 4)
                if ref_s is None:          # the reference never gave it a gradient; here it sits in the bucket with a zero one
                    assert got['max_abs'] == 0.0, name
    # final state, tensor by tensor.  A trained tensor may have moved differently where a gradient is zero up to rounding: Adam
    # with beta1 = 0 moves every element by at most ~2 lr per step whatever the gradient's size, so that much per element is
    # the bound on top of the 1e-4; tensors nobody trains are exact
    steps = len(fx['steps'])
    for net, lr in (('g', tr.args.lr_g), ('d', tr.args.lr_d), ('target_g', tr.args.lr_target_g * tr.args.lr_g)):
        module = getattr(tr, net)
        trained = {n for n, _ in module.named_parameters()}
        for name, v in module.state_dict().items():
            ref = fx['final'][net][name]
            got = summarize(v, len(ref['idx']))
            leaf = name.rsplit('.', 1)[-1]
            if leaf in ('full_masks', 'noise_proto', 'num_batches_tracked'):
                assert got['l2'] == ref['l2'] and got['sum'] == ref['sum'], (net, name)
            elif name in trained or name.startswith('blocks.0.'):
                slack = 2 * lr * steps * ref['numel'] ** 0.5
                assert _close(got['l2'], ref['l2'], 1e-4, 1e-6 + slack), (net, name, got['l2'], ref['l2'])
            else:                          # BatchNorm running statistics
                assert _close(got['l2'], ref['l2'], 1e-3, 1e-5), (net, name, got['l2'], ref['l2'])
    assert float(torch.rand(1)) == fx['rng_after']


# ------------------------------------------------------------------------------------------------------ the autograd op
@pytest.mark.parametrize('masks', [True, False])
@pytest.mark.parametrize('noise', [True, False])
def test_scene_patches_gradients_match_float64_autograd(masks, noise):
    B, P, patch, S = 2, 3, 3, 16
    c = SC.kernel_case(B, P, patch, S, masks, noise)
    theta = c['theta'].clone().requires_grad_(True)
    logits = c['logits'].clone().requires_grad_(True) if masks else None
    nz = c['noise'].clone().requires_grad_(True) if noise else None
    out = TF.scene_patches(theta, logits, nz, patch, S)
    assert out.shape == (B, P, S, S)
    out.backward(c['gout'])
    want_out, want_gt, want_gm = c['want']
    assert torch.allclose(out.detach().double(), want_out, rtol=0, atol=1e-6 * float(want_out.abs().max()))
    assert torch.allclose(theta.grad.double(), want_gt, rtol=0, atol=1e-6 * float(want_gt.abs().max()))
    if masks:
        assert torch.allclose(logits.grad.double(), want_gm, rtol=0, atol=1e-6 * float(want_gm.abs().max()))
    if noise:
        assert nz.grad is None           # the noise is a draw, not a parameter


def test_scene_patches_is_once_differentiable():
    c = SC.kernel_case(2, 3, 3, 16)
    theta = c['theta'].clone().requires_grad_(True)
    logits = c['logits'].clone().requires_grad_(True)
    out = TF.scene_patches(theta, logits, c['noise'], 3, 16)
    g_theta, g_logits = torch.autograd.grad(out.pow(2).sum(), (theta, logits), create_graph=True)
    with pytest.raises(NotImplementedError):
        (g_theta.pow(2).sum() + g_logits.pow(2).sum()).backward()


def test_scene_patches_rejects_malformed_arguments():
    with pytest.raises(ValueError):
        TF.scene_patches(torch.zeros(2, 13), None, None, 3, 8)
    with pytest.raises(ValueError):
        TF.scene_patches(torch.zeros(2, 12), torch.zeros(2, 17), None, 3, 8)
    with pytest.raises(ValueError):
        TF.scene_patches(torch.zeros(2, 12), None, torch.zeros(2, 3), 3, 8)


@pytest.mark.parametrize('P', [1, 20])
@pytest.mark.parametrize('refine', [True, False])
def test_structure_block_is_one_launch_each_way(P, refine):
    calls = []

    class Counting(SC.SceneEmulator):
        def scene_patches_fwd(self, *a):
            calls.append('fwd')
            return super().scene_patches_fwd(*a)

        def scene_patches_bwd(self, *a):
            calls.append('bwd')
            return super().scene_patches_bwd(*a)

        def gemm(self, *a):
            calls.append('gemm')
            return super().gemm(*a)

    backend._set_backend_for_testing(Counting())
    torch.manual_seed(0)
    block = SceneStructureBlock(16, P, patch_size=3, scene_size=16, refine_patches=refine, patch_noise=True)
    with torch.no_grad():
        block.patch_transforms[0].weight.normal_(std=0.1)
        block.masks[0].weight.normal_(std=0.1)
    out = block(torch.randn(4, 16))
    assert out.shape == (4, P, 16, 16)
    assert calls == ['gemm'] * (2 if refine else 1) + ['fwd']          # two Linears (one when not refining), one launch
    del calls[:]
    out.sum().backward()
    assert calls.count('fwd') == 0 and calls.count('bwd') == 1
    assert block.patch_transforms[0].weight.grad is not None
    assert (block.masks[0].weight.grad is not None) == refine


def test_structure_block_draws_noise_in_eval_mode_too_and_through_the_hook():
    torch.manual_seed(0)
    block = SceneStructureBlock(8, 2, patch_size=3, scene_size=8, refine_patches=True, patch_noise=True).eval()
    z = torch.randn(2, 8)
    torch.manual_seed(5)
    a = block(z)
    want_next = float(torch.rand(1))
    torch.manual_seed(5)
    torch.randn(3, 3)
    assert float(torch.rand(1)) == want_next                 # exactly one (patch, patch) normal draw per forward
    served = []
    block.noise_source = lambda rows, cols: served.append((rows, cols)) or torch.ones(rows, cols)
    b = block(z)
    assert served == [(3, 3)] and not torch.equal(a, b)
    assert copy.deepcopy(block).noise_source is None         # a trainer's hook does not travel with a copied / pickled model


# ------------------------------------------------------------------------------------------------------------- RngFeed
def test_rng_feed_serves_a_recorded_noise_plan_like_inline_draws():
    plan = [('z', 4, 16), ('noise', 3, 3), ('z', 4, 16), ('noise', 3, 3)]

    def inline():
        return [torch.randn(r, c) for _, r, c in plan]

    torch.manual_seed(11)
    first, second = inline(), inline()
    after = float(torch.rand(1))

    feed = RngFeed('cpu')
    feed.mode = 'record'
    torch.manual_seed(11)
    got = [feed.draw(*p).clone() for p in plan]
    assert feed.plan == plan and all(torch.equal(a, b) for a, b in zip(got, first))
    feed.mode = 'serve'
    feed.refill()
    got = [feed.draw(*p).clone() for p in plan]
    assert all(torch.equal(a, b) for a, b in zip(got, second)) and float(torch.rand(1)) == after

    adopted = RngFeed('cpu')
    adopted.adopt(plan)
    adopted.mode = 'serve'
    torch.manual_seed(11)
    adopted.refill()
    assert all(torch.equal(adopted.draw(*p), b) for p, b in zip(plan, first))
    adopted.prefetch()                                       # the speculative draw of the next step: same values, same stream
    adopted.refill()
    assert all(torch.equal(adopted.draw(*p), b) for p, b in zip(plan, second)) and float(torch.rand(1)) == after


def test_rng_feed_noise_is_the_same_on_every_rank():
    plan = [('z', 2, 16), ('noise', 4, 4)]
    torch.manual_seed(3)
    z_global, noise = torch.randn(4, 16), torch.randn(4, 4)
    got = []
    for rank in (0, 1):
        feed = RngFeed('cpu', rank=rank, world=2)
        feed.mode = 'record'
        torch.manual_seed(3)
        got.append([feed.draw(*p).clone() for p in plan])
        feed.mode = 'serve'
        torch.manual_seed(3)
        feed.refill()
        assert all(torch.equal(feed.draw(*p), g) for p, g in zip(plan, got[-1]))
    assert torch.equal(torch.cat([got[0][0], got[1][0]]), z_global)          # complementary z rows
    assert torch.equal(got[0][1], noise) and torch.equal(got[1][1], noise)   # identical, unsliced noise


def test_served_steps_equal_inline_steps():
    """Step 1 records [z, noise, z, noise]; steps 2 and 3 pre-draw that plan.  A second trainer forgets its plan after every step,
    so each of its steps draws inline: same losses, same generator, same stream."""
    fx = SC.load_scene_fixture('scene_c64_s16_p20_b4_refine_noise')
    runs = []
    for inline in (False, True):
        tr = SC.scene_trainer(fx, 'cpu')
        SC.load_procedural(tr, fx)
        torch.manual_seed(fx['rng_seed'])
        logs = []
        for k in range(3):
            logs.append(tr.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + k)))
            if inline:
                tr.rng_feed = RngFeed(tr.device)
            else:
                latent = tr.gan_config.latent_dims
                assert tr.rng_feed.plan == [('z', 4, latent), ('noise', 3, 3)] * 2
                assert tr.rng_feed.mode == ('record' if k == 0 else 'serve')
        runs.append((logs, tr.optimizer_g.flat.clone(), tr.optimizer_d.flat.clone(), float(torch.rand(1))))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert runs[0][3] == runs[1][3]


# ----------------------------------------------------------------------------------------- what the optimiser must not touch
@pytest.mark.parametrize('case', ['scene_c32_s8_p5_b4', 'scene_c64_s16_p20_b4_refine_noise'])
def test_untrained_tensors_stay_bit_unchanged(case):
    """``full_masks`` / ``noise_proto`` (and, when not refining, the unused ``masks`` Linear) never receive a gradient: the
    reference's Adam skips them (grad is None); here they sit in the flat bucket with a zero gradient, which with beta1 = 0 is a
    zero update, and the EMA of two equal values is that value."""
    fx = SC.load_scene_fixture(case)
    tr = SC.scene_trainer(fx, 'cpu')
    SC.load_procedural(tr, fx)
    names = [n for n in ('full_masks', 'noise_proto') if hasattr(tr.g.structure_generator, n)]
    if not fx['flags']['refine_patches']:
        names += ['masks.0.weight', 'masks.0.bias']
        with torch.no_grad():                    # the same non-zero values on both sides, so that "unchanged" says something
            for n in ('weight', 'bias'):
                getattr(tr.target_g.structure_generator.masks[0], n).copy_(getattr(tr.g.structure_generator.masks[0], n))
    before = {(net, n): getattr(tr, net).structure_generator.get_parameter(n).detach().clone()
              for net in ('g', 'target_g') for n in names}
    assert names and all(float(v.abs().max()) > 0 or k[1] == 'noise_proto' for k, v in before.items())
    torch.manual_seed(fx['rng_seed'])
    for k in range(2):
        tr.train_batch(synthetic_images(fx['batch'], fx['size'], fx['img_seed'] + k))
    for (net, n), v in before.items():
        now = getattr(tr, net).structure_generator.get_parameter(n)
        assert torch.equal(now.view(torch.int32), v.view(torch.int32)), (net, n)
        if net == 'g':
            assert float(now.grad.abs().max()) == 0.0, n
