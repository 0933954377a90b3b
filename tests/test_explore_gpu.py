"""The explore apps on the GPU, HIP kernels throughout: the fixtures the reference's own apps produced
(tests/golden/explore_*.json) at 1e-4 in eager mode; find-image under HIP-graph replay bit-equal to eager, across noise refills and
the step that clips; a repeated run bit-equal; the generator untouched; PNGs written."""
import pytest
import torch

import explore_cases as EC

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def hip_backend():
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(None)
    backend.get()
    yield
    backend._set_backend_for_testing(prev)


@pytest.mark.parametrize('case', EC.FIND_CASES)
def test_find_image_matches_reference_fixture(case, tmp_path):
    fx = EC.load_fixture(case)
    before = {k: v.clone() for k, v in EC.generator_for(fx).state_dict().items()}
    rec = EC.run_app(fx, tmp_path, device='cuda', keep_pngs=True)
    print(f'EXPLORE {case} (HIP, eager): worst deviation {EC.check_against_fixture(rec, fx):.2e}')
    assert rec['rng_after'] == fx['rng_after']
    after = rec['app'].g.state_dict()
    for k, v in before.items():          # eval mode, frozen: bit-unchanged, num_batches_tracked included
        assert after[k].is_cuda and torch.equal(after[k].cpu(), v), k
    from PIL import Image
    for im in rec['images']:
        with Image.open(im['filename']) as png:
            assert png.size == (2 * 16 + 3 * 2, 16 + 2 * 2) and png.mode == 'RGB'


def _six_steps(tmp_path, sub, **kw):
    fx = EC.load_fixture('explore_find_adam_mse')
    path = tmp_path / sub
    path.mkdir()
    return fx, EC.run_app(fx, path, device='cuda', flags=['--max-steps', '6'], noise_chunk=2, **kw)


def _bits(rec):
    return [torch.cat([s['z'].reshape(-1), torch.tensor([s['loss'], s['z_min'], s['z_mean'], s['z_max']])]).view(torch.int32)
            for s in rec['steps']], [im['tensor'].view(torch.int32) for im in rec['images']]


def test_graph_replay_is_bit_equal_to_eager_across_refills_and_the_clip(tmp_path):
    fx, eager = _six_steps(tmp_path, 'eager')
    _, replay = _six_steps(tmp_path, 'replay', graphs=True)
    assert replay['app']._graph is not None, 'the capture fell back to eager'
    assert fx['clip_steps'] and fx['clip_steps'][0] < 6            # the step that clips is among the six
    assert bool((eager['steps'][fx['clip_steps'][0] - 1]['z'].abs() > 3).any())
    for a, b in zip(_bits(eager), _bits(replay)):
        assert len(a) == len(b) == 6
        for k, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), f'step {k}'
    assert eager['rng_after'] == replay['rng_after']
    EC.check_against_fixture(dict(steps=replay['steps'][:4], images=replay['images'][:4]), fx)


def test_a_repeated_run_is_bit_identical(tmp_path):
    _, first = _six_steps(tmp_path, 'first')
    _, second = _six_steps(tmp_path, 'second')
    for a, b in zip(_bits(first), _bits(second)):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_render_tour_matches_reference_fixture(tmp_path):
    fx = EC.load_fixture(EC.TOUR_CASE)
    rec = EC.run_app(fx, tmp_path, device='cuda', keep_pngs=True)
    print(f'EXPLORE tour (HIP): worst deviation {EC.check_against_fixture(rec, fx):.2e}')
    assert rec['rng_after'] == fx['rng_after']
    from PIL import Image
    assert len(rec['images']) == 6
    for im in rec['images']:
        with Image.open(im['filename']) as png:
            assert png.size == (16, 16)


@pytest.mark.parametrize('case', EC.INTERP_CASES)
def test_continuous_interp_matches_reference_fixture(case, tmp_path):
    fx = EC.load_fixture(case)
    rec = EC.run_app(fx, tmp_path, device='cuda', keep_pngs=True)
    print(f'EXPLORE {case} (HIP): worst deviation {EC.check_against_fixture(rec, fx):.2e}')
    assert rec['rng_after'] == fx['rng_after']
    from PIL import Image
    with Image.open(rec['images'][0]['filename']) as png:
        assert png.size == (20, 20)


@pytest.mark.parametrize('kind', ['mse', 'l1'])
def test_recon_loss_function_forward_and_backward_on_the_device(kind):
    """``functional.recon_loss`` as an autograd op under a scaled upstream gradient (its backward is a ``tg_scale_dev`` launch)
    against the same expression in float64 ATen, by the house rule: e32 is what fp32 ATen makes of it on the CPU."""
    import torch.nn.functional as F
    from tartangan_amd import functional as TF
    c = EC.recon_case(2, 256, TF.RECON_KINDS[kind])
    fn = F.mse_loss if kind == 'mse' else F.smooth_l1_loss

    def aten(dtype):
        x = c['imgs'].to(dtype).clone().requires_grad_(True)
        out = fn(EC.normalise(x), c['target'].to(dtype), reduction='sum') * 0.37
        g, = torch.autograd.grad(out, x)
        return out.detach().double().reshape(1), g.double()
    want, r32 = aten(torch.float64), aten(torch.float32)
    x = c['imgs'].view(2, 3, 16, 16).cuda().requires_grad_(True)
    out = TF.recon_loss(x, c['target'].view(2, 3, 16, 16).cuda(), kind) * 0.37
    g, = torch.autograd.grad(out, x)
    for tag, got, w, r in (('loss', out.detach().reshape(1), want[0], r32[0]), ('grad', g.view(2, 3, 256), want[1], r32[1])):
        e32 = EC.rel(r, w)
        err, lim = EC.rel(got.cpu(), w), EC.limit(e32)
        print(f'EXPLORE recon_loss op {kind} {tag}: e32 {e32:.2e} kernel {err:.2e} limit {lim:.2e}')
        assert err <= lim


def test_wrappers_refuse_other_dtypes_on_the_device():
    from tartangan_amd import functional as TF
    x = torch.zeros(2, 3, 4, 4, device='cuda')
    for bad in (torch.float64, torch.float16):
        with pytest.raises(TypeError):
            TF.recon_loss_into(x.to(bad), x.to(bad), None, torch.zeros(1, device='cuda', dtype=bad), 0)
        with pytest.raises(TypeError):
            TF.mosaic_gather(x.to(bad), 1, 2, 4)
        z = torch.zeros(8, device='cuda', dtype=bad)
        with pytest.raises(TypeError):
            TF.latent_step(z, None, None, None, None, z.clone(), None, None, 'clip')
    with pytest.raises(TypeError):
        z = torch.zeros(8, device='cuda')
        TF.latent_step(z, z.clone(), z.clone(), z.clone(), torch.zeros(1, device='cuda', dtype=torch.int32), None,
                       torch.zeros(4, device='cuda'), torch.zeros(1, device='cuda'), 'adam')


def test_lbfgs_runs_on_the_device(tmp_path):
    """``--optimizer lbfgs``: the eager closure over ``functional.recon_loss`` on HIP.  The loss ``optimizer.step`` returns is its
    FIRST closure evaluation: for step 0 that is the loss at the drawn latents, held at 1e-4 against the run over the CPU emulator
    (and against the adam fixture's first loss, the same quantity).  Step 1's loss comes after 20 quasi-Newton iterations, whose
    amplification of fp32 differences is not bounded by anything written down here: it is printed, and asserted only to be
    finite and lower (measured on the MI355X: 3979.6 on the device against 4492.5 over the emulator, 11 % apart, from first losses
    that agree to 7e-8 -- the iteration is that sensitive, so no parity bound is claimed for it).  Two device runs are
    bit-identical."""
    from tartangan_amd import backend
    fx = EC.load_fixture('explore_find_adam_mse')
    flags = ['--max-steps', '2', '--optimizer', 'lbfgs', '--lr', '0.05']
    runs = []
    for sub in ('a', 'b'):
        (tmp_path / sub).mkdir()
        runs.append(EC.run_app(fx, tmp_path / sub, device='cuda', flags=flags, record_images=False))
    prev = backend._set_backend_for_testing(EC.ExploreEmulator())
    try:
        (tmp_path / 'cpu').mkdir()
        cpu = EC.run_app(fx, tmp_path / 'cpu', device='cpu', flags=flags, record_images=False)
    finally:
        backend._set_backend_for_testing(prev)
    dev, host = [s['loss'] for s in runs[0]['steps']], [s['loss'] for s in cpu['steps']]
    print(f'EXPLORE lbfgs: device {dev} emulated {host} step-1 deviation {abs(dev[1] - host[1]) / abs(host[1]):.2e}')
    assert runs[0]['app'].z.is_cuda
    assert EC.close(dev[0], host[0]) and EC.close(dev[0], fx['steps'][0]['loss'])
    assert dev[1] == dev[1] and abs(dev[1]) != float('inf') and dev[1] < dev[0]
    assert dev == [s['loss'] for s in runs[1]['steps']]
    assert torch.equal(runs[0]['steps'][1]['z'].view(torch.int32), runs[1]['steps'][1]['z'].view(torch.int32))
    assert runs[0]['rng_after'] == cpu['rng_after']
