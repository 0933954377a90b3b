"""The explore apps' host logic on the CPU: ``functional.recon_loss``, the fused latent step, the mosaic index, the three apps
(``tartangan_amd.explore``) run over float64 forms of the new entry points (explore_cases.ExploreEmulator) and compared with the
fixtures the reference's own apps produced (tests/golden/explore_*.json, made by tests/golden/make_explore_golden.py).

Nothing here says anything about the HIP kernels (tests/test_explore_kernels_gpu.py, test_explore_gpu.py)."""
import collections

import numpy as np
import pytest
import torch

import explore_cases as EC
from tartangan_amd import backend, functional as TF


@pytest.fixture(autouse=True)
def emulated_backend():
    prev = backend._set_backend_for_testing(EC.ExploreEmulator())
    yield
    backend._set_backend_for_testing(prev)


# ------------------------------------------------------------------------------------------------- the emulated entry points
@pytest.mark.parametrize('kind', [0, 1], ids=['mse', 'l1'])
def test_recon_loss_against_float64_aten_and_finite_differences(kind):
    c = EC.recon_case(2, 256, kind)
    assert c['planted'] == len(EC.D_PLANTED)
    # through the package's wrapper (shape check, workspace query and size) over the emulated backend, in float64
    x, t = c['imgs'].double().view(2, 3, 16, 16), c['target'].double().view(2, 3, 16, 16)
    loss, grad = torch.zeros(1, dtype=torch.float64), torch.zeros_like(x)
    assert TF.recon_loss_into(x, t, grad, loss, kind) is loss
    assert EC.rel(loss, c['want'][0]) < 1e-12 and EC.rel(grad.view(2, 3, 256), c['want'][1]) < 1e-12
    alone = torch.zeros(1, dtype=torch.float64)
    TF.recon_loss_into(x, t, None, alone, kind)            # the loss alone (an L-BFGS re-evaluation)
    assert torch.equal(alone, loss)
    # central differences on elements away from the planted kinks
    gen = torch.Generator().manual_seed(5)
    flat, checked = x.view(-1), 0
    for i in torch.randperm(flat.numel(), generator=gen)[:40].tolist():
        if i < len(EC.D_PLANTED) * 4:
            continue
        vals = []
        for sign in (1, -1):
            xp = x.clone()
            xp.view(-1)[i] += sign * 1e-6
            vals.append(float(TF.recon_loss_into(xp, t, None, torch.zeros(1, dtype=torch.float64), kind)))
        fd = (vals[0] - vals[1]) / 2e-6
        assert abs(fd - float(grad.view(-1)[i])) <= 1e-6 * max(1.0, abs(fd)), (i, fd, float(grad.view(-1)[i]))
        checked += 1
    assert checked >= 30


@pytest.mark.parametrize('kind', ['mse', 'l1'])
def test_recon_loss_function_is_first_order_only(kind):
    gen = torch.Generator().manual_seed(3)
    x = (torch.rand(2, 3, 4, 4, generator=gen, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    t = torch.randn(2, 3, 4, 4, generator=gen, dtype=torch.float64) + 5          # |d| > 1 everywhere: no kink near a sample
    assert torch.autograd.gradcheck(lambda a: TF.recon_loss(a, t, kind) * 0.37, (x,), eps=1e-6, atol=1e-6)
    g, = torch.autograd.grad(TF.recon_loss(x, t, kind), x, create_graph=True)
    with pytest.raises(NotImplementedError):
        g.sum().backward()
    with pytest.raises(ValueError):
        TF.recon_loss(x, t.clone().requires_grad_(True), kind)
    with pytest.raises(ValueError):
        TF.recon_loss(torch.zeros(2, 4, 4, 4), torch.zeros(2, 4, 4, 4), kind)


@pytest.mark.parametrize('opt,l2', [('adam', 0.), ('adam', 0.1), ('sgd', 0.1)])
def test_latent_step_against_torch_optimisers_for_five_steps(opt, l2):
    n, gen = 203, torch.Generator().manual_seed(11)
    z = torch.randn(n, generator=gen)
    p = z.double().clone().requires_grad_(True)
    lr = 0.5 if opt == 'adam' else 0.01
    ref = (torch.optim.Adam if opt == 'adam' else torch.optim.SGD)([p], lr)
    m, v, step, stats = torch.zeros(n), torch.zeros(n), torch.zeros(1, dtype=torch.int64), torch.zeros(4)
    for k in range(5):
        c = torch.randn(n, generator=gen) * (1 + k)
        recon = torch.rand(1, generator=gen) * 50
        ref.zero_grad()
        want_loss = float(recon.double() + p.detach().pow(2).mean() * l2)
        (p * c.double()).sum().backward()          # gz: what the generator's backward hands over
        gz = p.grad.float().clone()
        (p.pow(2).mean() * l2).backward()          # the L2 term's share, which the kernel adds itself
        ref.step()
        TF.latent_step(z, gz, m, v, step, None, stats, recon, opt, lr=lr, l2=l2)
        q = p.detach()
        assert EC.rel(z, q) < 2e-6, (k, EC.rel(z, q))
        want = torch.tensor([want_loss, float(q.min()), float(q.mean()), float(q.max())], dtype=torch.float64)
        assert EC.rel(stats, want) < 2e-6, (k, stats, want)
    assert int(step) == (5 if opt == 'adam' else 0)
    if opt == 'adam':
        st = ref.state[p]
        assert EC.rel(m, st['exp_avg']) < 2e-6 and EC.rel(v, st['exp_avg_sq']) < 2e-6


@pytest.mark.parametrize('fused', [False, True], ids=['clip-only', 'after-an-update'])
def test_clip_selects_exactly_what_the_reference_sequence_selects(fused):
    z0, noise, selected = EC.planted_clip_inputs(64)
    want, want_sel = EC.reference_clip(z0, noise)
    assert torch.equal(want_sel[:len(selected)], selected)
    z = z0.clone()
    if fused:            # lr 0: the update leaves z as it is, the clip of the same launch follows
        TF.latent_step(z, torch.zeros(64), None, None, None, noise, torch.zeros(4), torch.zeros(1), 'sgd', lr=0.)
        keep = ~torch.isnan(z0) & ~torch.isinf(z0)          # (0 * inf: the update itself turns the infinities into NaN)
    else:
        TF.latent_step(z, None, None, None, None, noise, None, None, 'clip')
        keep = torch.ones(64, dtype=torch.bool)
    got_sel = (z.view(torch.int32) != z0.view(torch.int32))
    assert torch.equal(got_sel[keep], want_sel[keep])
    assert torch.equal(z[want_sel & keep], noise[want_sel & keep])              # the noise itself, bit for bit
    finite = torch.isfinite(z0)
    assert torch.equal(z[finite], want[finite])                                  # where the reference's arithmetic is finite
    assert torch.isnan(z[4]) and torch.isnan(want[4])                            # NaN is not clipped


def test_integer_mosaic_index_equals_the_reference_expression():
    for rows, cols, h, w, S in EC.MOSAIC_SHAPES:
        for a in range(S):
            for b in (rows, cols, h, w):
                assert TF.mosaic_index(a, b, S) == int(a * b / S)
    # and well beyond the test shapes: every a < S <= 512, b <= 512
    b = np.arange(1, 513, dtype=np.int64)[None, :]
    for S in range(1, 513):
        a = np.arange(S, dtype=np.int64)[:, None]
        assert np.array_equal(TF.mosaic_index(a, b, S), (a * b / S).astype(np.int64)), S


@pytest.mark.parametrize('shape', EC.MOSAIC_SHAPES)
def test_mosaic_gather_is_the_reference_loop(shape):
    rows, cols, h, w, S = shape
    imgs = torch.arange(rows * cols * 3 * h * w, dtype=torch.float32).view(rows * cols, 3, h, w)
    got = TF.mosaic_gather(imgs, rows, cols, S)
    grid = imgs.view(rows, cols, 3, h, w)
    want = torch.zeros(3, S, S)
    for y in range(S):              # continuous_interp.py:40-52, its index expressions
        grid_y, img_y = int(y * rows / S), int(y * h / S)
        for x in range(S):
            want[:, y, x] = grid[grid_y, int(x * cols / S), :, img_y, int(x * w / S)]
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        TF.mosaic_gather(imgs, rows + 1, cols, S)


# ------------------------------------------------------------------------------------------------- the apps
class CountingEmulator(EC.ExploreEmulator):
    def __init__(self):
        object.__setattr__(self, 'calls', collections.Counter())

    def __getattribute__(self, name):
        attr = super().__getattribute__(name)
        if callable(attr) and not name.startswith('_'):
            super().__getattribute__('calls')[name] += 1
        return attr


def test_a_find_image_step_launches_no_weight_gradient_and_leaves_g_unchanged(tmp_path):
    fx = EC.load_fixture('explore_find_adam_mse')
    counting = CountingEmulator()
    backend._set_backend_for_testing(counting)
    before = {k: v.clone() for k, v in EC.generator_for(fx).state_dict().items()}
    assert any(k.endswith('num_batches_tracked') for k in before)
    rec = EC.run_app(fx, tmp_path, flags=['--max-steps', '2'])
    app = rec['app']
    assert not app.g.training and not any(p.requires_grad for p in app.g.parameters())
    after = app.g.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert torch.equal(after[k], v) and after[k].dtype == v.dtype, k
    assert not [n for n in counting.calls if 'wgrad' in n], counting.calls
    assert counting.calls['recon_loss'] == 2 and counting.calls['latent_step'] == 4          # a clip and an update per step
    assert counting.calls['bn_eval_stats'] > 0 and not [n for n in counting.calls if n.startswith('bn_train')]


@pytest.mark.parametrize('case', EC.FIND_CASES)
def test_find_image_matches_reference_fixture(case, tmp_path, single_thread):
    fx = EC.load_fixture(case)
    rec = EC.run_app(fx, tmp_path)
    worst = EC.check_against_fixture(rec, fx)
    print(f'EXPLORE {case} (emulated): worst deviation {worst:.2e}')
    assert rec['rng_after'] == fx['rng_after']
    assert [im['filename'].rsplit('_', 1)[1] for im in rec['images']] == [f'{i}.png' for i in range(len(fx['steps']))]


def test_the_adam_fixture_contains_a_clip_and_the_app_takes_it(tmp_path):
    fx = EC.load_fixture('explore_find_adam_mse')
    assert fx['clip_steps']
    k = fx['clip_steps'][0]
    before = torch.tensor(fx['steps'][k - 1]['z'])
    assert bool((before.abs() > 3).any())
    rec = EC.run_app(fx, tmp_path)
    hit = before.abs() > 3
    assert bool((rec['steps'][k]['z'].reshape(-1)[hit].abs() < 3.6).all())          # replaced by noise, then moved by one lr at most


@pytest.mark.parametrize('case', EC.FIND_CASES)
@pytest.mark.parametrize('chunk', [1, 2])
def test_host_draws_do_not_depend_on_the_noise_chunk(case, chunk, tmp_path):
    """One randn(z.shape) per step whether or not anything clips, none beyond the last step: the streams end where the
    reference's did, and the run is the same whatever the chunk."""
    fx = EC.load_fixture(case)
    rec = EC.run_app(fx, tmp_path, noise_chunk=chunk, record_images=False)
    assert rec['rng_after'] == fx['rng_after']
    EC.check_against_fixture(dict(rec, images=[]), dict(fx, images=[]))


def test_save_every_and_log_every_skip_steps(tmp_path):
    fx = EC.load_fixture('explore_find_adam_mse')
    rec = EC.run_app(fx, tmp_path, flags=['--max-steps', '4', '--save-every', '3', '--log-every', '2'], keep_pngs=True)
    assert [im['filename'].rsplit('_', 1)[1] for im in rec['images']] == ['0.png', '3.png']
    assert len(rec['steps']) == 2
    assert EC.close(rec['steps'][1]['loss'], fx['steps'][2]['loss'])
    from PIL import Image
    with Image.open(rec['images'][1]['filename']) as png:
        assert png.size == (2 * 16 + 3 * 2, 16 + 2 * 2)          # two images in make_grid's 2-pixel frame


def test_lbfgs_runs_an_eager_closure_over_the_same_loss(tmp_path):
    fx = EC.load_fixture('explore_find_adam_mse')
    rec = EC.run_app(fx, tmp_path, flags=['--max-steps', '2', '--optimizer', 'lbfgs', '--lr', '0.05'])
    losses = [s['loss'] for s in rec['steps']]
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[1] < losses[0]
    assert EC.close(losses[0], fx['steps'][0]['loss'])           # the first closure evaluation is the first step's loss


def test_refusals(tmp_path):
    fx = EC.load_fixture('explore_find_adam_mse')
    with pytest.raises(NotImplementedError, match='vgg'):
        EC.run_app(fx, tmp_path, flags=['--max-steps', '1', '--vgg'])
    with pytest.raises(ValueError, match='L-BFGS'):
        EC.run_app(fx, tmp_path, flags=['--max-steps', '1', '--optimizer', 'lbfgs'], graphs=True)
    from tartangan_amd.explore.find_image import FindImage
    from tartangan_amd.models.pluggan import GAN_CONFIGS, Discriminator
    for module in (Discriminator(GAN_CONFIGS['16']).state_dict(), torch.nn.Linear(3, 3)):
        path = str(tmp_path / 'other.pt')
        torch.save(module, path)
        app = FindImage(EC.app_args(FindImage, [path, str(tmp_path / 'o'), str(tmp_path / 'target.png'), '--no-cuda']))
        with pytest.raises(ValueError, match='not an image generator'):
            app.run()
    with pytest.raises(ValueError, match='local'):
        app = FindImage(EC.app_args(FindImage, ['s3://bucket/run', 'o', 't.png', '--no-cuda']))
        app.run()


@pytest.mark.parametrize('case', EC.FIND_CASES[:1] + (EC.TOUR_CASE,) + EC.INTERP_CASES[:1])
def test_parsers_have_the_reference_flags_and_defaults(case):
    fx = EC.load_fixture(case)
    mine = EC.parser_spec(EC.my_apps()[fx['app']])
    new = [row for row in mine if row[0] in ('save_every', 'log_every')]
    assert [row for row in mine if row not in new] == fx['parser']
    assert len(new) == (2 if fx['app'] == 'find_image' else 0) and all(row[2] == 1 for row in new)


def test_render_tour_matches_reference_fixture(tmp_path, single_thread):
    fx = EC.load_fixture(EC.TOUR_CASE)
    rec = EC.run_app(fx, tmp_path, keep_pngs=True)
    print(f'EXPLORE tour (emulated): worst deviation {EC.check_against_fixture(rec, fx):.2e}')
    assert rec['rng_after'] == fx['rng_after'] and len(rec['images']) == 6
    from PIL import Image
    with Image.open(rec['images'][5]['filename']) as png:
        assert png.size == (16, 16) and rec['images'][5]['filename'].endswith('frame_5.png')


@pytest.mark.parametrize('case', EC.INTERP_CASES)
def test_continuous_interp_matches_reference_fixture(case, tmp_path, single_thread):
    fx = EC.load_fixture(case)
    counting = CountingEmulator()
    backend._set_backend_for_testing(counting)
    rec = EC.run_app(fx, tmp_path, keep_pngs=True)
    print(f'EXPLORE {case} (emulated): worst deviation {EC.check_against_fixture(rec, fx):.2e}')
    assert rec['rng_after'] == fx['rng_after']
    assert counting.calls['mosaic_gather'] == 1
    assert rec['images'][0]['tensor'].shape == (3, 20, 20) and rec['images'][0]['filename'].endswith('_combined.png')
    assert rec['app'].g.training            # the mode it was pickled in: BatchNorm's running statistics moved, one row per call
    moved = [k for k, v in EC.generator_for(fx).state_dict().items() if k.endswith('num_batches_tracked')
             and int(rec['app'].g.state_dict()[k]) != int(v)]
    assert moved
    tracked = int(rec['app'].g.state_dict()[moved[0]])
    assert tracked == (3 if fx['flags'][-1] == '--tile' else 6)
