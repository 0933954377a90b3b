"""tg_recon_loss, tg_latent_step and tg_mosaic_gather (csrc/explore.hip) on the GPU, every call behind guard bands
(guarded.run_both: outputs and workspaces handed over NaN-filled), aligned and one element off, the smallest case with each pointer
shifted alone, against float64 ATen: the normalisation with ``mse_loss`` / ``smooth_l1_loss`` and autograd, ``torch.optim.Adam`` /
``SGD``; the gather bit-exactly.

Tolerance, per case and output: e32 is the error the same ATen ops make in float32 on the CPU on the same inputs against float64
(largest absolute difference over the largest absolute reference value); the kernel may be off by 4 * e32 and never has to beat
2.4e-7 (explore_cases.limit, the rule of shared_cases.limit).  Each case prints its figures (pytest -s).

(This file sorts in front of test_guard_bands_gpu.py on purpose: that file's completeness test wants every entry point with a
pointer parameter to have gone through the guarded harness earlier in the same process.)"""
import pytest
import torch

import explore_cases as EC
import guarded
from guarded import run_both, workspace

pytestmark = pytest.mark.gpu
EMU = EC.ExploreEmulator()
H = EC.HYPER
HYPER_ARGS = [H['lr'], H['beta1'], H['beta2'], H['eps']]


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(None)
    yield backend.get()
    backend._set_backend_for_testing(prev)


def _check(tag, dev, want, e32, failures):
    err, lim = EC.rel(dev.cpu(), want), EC.limit(e32)
    print(f'EXPLORE {tag}: e32 {e32:.2e} kernel {err:.2e} limit {lim:.2e} share {err / lim:.2f}')
    if err > lim:
        failures.append(f'{tag}: {err:.3e} > {lim:.3e} (e32 {e32:.3e})')


# --------------------------------------------------------------------------------------------------------------- recon_loss
@pytest.mark.parametrize('kind', [0, 1], ids=['mse', 'l1'])
@pytest.mark.parametrize('shape', EC.RECON_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_recon_loss(K, shape, kind):
    B, C, HW = shape
    c = EC.recon_case(B, HW, kind)
    assert c['planted'] == min(len(EC.D_PLANTED), B * C * HW)            # d at 0, +-1, +-(1 +- 1 ulp), as many as fit
    nbytes = K.recon_loss_workspace(B, C, HW)
    assert nbytes == EMU.recon_loss_workspace(B, C, HW) and nbytes >= 4
    tol, failures = 2 * max(EC.limit(e) for e in c['e32']), []
    for pl in ['aligned', 'shifted'] + ([0, 1, 2, 3, 4] if shape == EC.RECON_SHAPES[0] else []):
        dev = run_both(K, 'recon_loss', [c['imgs'], c['target'], torch.zeros(B, C, HW), torch.zeros(1), workspace(nbytes), nbytes,
                                         B, C, HW, kind], [2, 3], tol=tol, placement=pl, emulator=EMU)
        _check(f'recon {shape} kind {kind} [{pl}] loss', dev[3], c['want'][0], c['e32'][0], failures)
        _check(f'recon {shape} kind {kind} [{pl}] grad', dev[2], c['want'][1], c['e32'][1], failures)
    for pl in ('aligned', 'shifted'):            # the loss alone
        dev = run_both(K, 'recon_loss', [c['imgs'], c['target'], None, torch.zeros(1), workspace(nbytes), nbytes, B, C, HW, kind], [3],
                       tol=tol, placement=pl, emulator=EMU)
        _check(f'recon {shape} kind {kind} [{pl}] loss alone', dev[3], c['want'][0], c['e32'][0], failures)
    assert not failures, failures


def test_recon_loss_refusals_write_nothing(K):
    B, C, HW = EC.RECON_SHAPES[2]
    c = EC.recon_case(B, HW, 0)
    nbytes = K.recon_loss_workspace(B, C, HW) - 4
    assert nbytes >= 4
    run_both(K, 'recon_loss', [c['imgs'], c['target'], torch.zeros(B, C, HW), torch.zeros(1), workspace(nbytes), nbytes, B, C, HW, 0],
             [2, 3], expect='rejected', emulator=EMU)
    assert K.recon_loss_workspace(2, 4, 16) == 0
    x = guarded.rnd(2, 4, 16)
    run_both(K, 'recon_loss', [x, guarded.rnd(2, 4, 16, seed=1), torch.zeros(2, 4, 16), torch.zeros(1), workspace(64), 64, 2, 4, 16, 0],
             [2, 3], expect='rejected', emulator=EMU)
    run_both(K, 'recon_loss', [x[:, :3].contiguous(), x[:, :3].contiguous(), torch.zeros(2, 3, 16), torch.zeros(1), workspace(64), 64,
                               2, 3, 16, 2], [2, 3], expect='rejected', emulator=EMU)


# -------------------------------------------------------------------------------------------------------------- latent_step
@pytest.mark.parametrize('opt,step0', [(0, 0), (0, 7), (1, 0)], ids=['adam-step0', 'adam-step7', 'sgd'])
@pytest.mark.parametrize('n', EC.LATENT_SIZES)
def test_latent_step(K, n, opt, step0):
    l2 = 0.1
    c = EC.latent_case(n, opt, step0, l2)
    failures = []
    tol = 2 * max(EC.limit(e) for e in c['e32'])
    adam = opt == 0
    m, v, step = (c['m'], c['v'], torch.tensor([step0])) if adam else (None, None, None)
    ptrs = [0, 1, 2, 3, 4, 6, 7] if adam else [0, 1, 6, 7]
    for pl in ['aligned', 'shifted'] + (ptrs if n == 1 else []):
        dev = run_both(K, 'latent_step', [c['z'], c['gz'], m, v, step, None, torch.zeros(4), c['recon'], n, opt] + HYPER_ARGS + [l2],
                       [0, 2, 3, 4, 6] if adam else [0, 6], tol=tol, accum=[0, 2, 3, 4] if adam else [0], placement=pl, emulator=EMU)
        tag = f'latent n={n} opt {opt} step {step0} [{pl}]'
        _check(tag + ' z', dev[0], c['want'][0], c['e32'][0], failures)
        _check(tag + ' stats', dev[6], c['want'][3], c['e32'][3], failures)
        if adam:
            _check(tag + ' m', dev[2], c['want'][1], c['e32'][1], failures)
            _check(tag + ' v', dev[3], c['want'][2], c['e32'][2], failures)
            assert int(dev[4]) == step0 + 1
    assert not failures, failures


@pytest.mark.parametrize('n', EC.LATENT_SIZES)
def test_clip_selection_is_exact(K, n):
    """Clip only, and the clip behind an update (lr 0, so that the update leaves finite values alone), with 3, -3, their
    neighbours outside, NaN and the infinities planted.  z is not compared by run_both (NaN in it): bit for bit here."""
    z0, noise, _ = EC.planted_clip_inputs(n)
    want = z0.clone()
    EMU.latent_step(want, None, None, None, None, noise, None, None, n, 2, 0., 0., 0., 0., 0.)
    ref, ref_sel = EC.reference_clip(z0, noise)
    finite = torch.isfinite(z0)
    assert torch.equal(want[finite], ref[finite]) and bool(ref_sel.any()) == (n > 2)
    for pl in ['aligned', 'shifted'] + ([0, 5] if n == 1 else []):
        dev = run_both(K, 'latent_step', [z0, None, None, None, None, noise, None, None, n, 2] + HYPER_ARGS + [0.], [], scratch=[0],
                       accum=[0], placement=pl, emulator=EMU)
        assert torch.equal(dev[0].cpu().view(torch.int32), want.view(torch.int32)), pl
    # behind an SGD update with lr 0 and a zero gradient: finite values pass through the update unchanged
    zf, nf = z0[finite].contiguous(), noise[finite].contiguous()
    k = zf.numel()
    if k:
        wantf = want[finite]
        for pl in ('aligned', 'shifted'):
            dev = run_both(K, 'latent_step', [zf, torch.zeros(k), None, None, None, nf, torch.zeros(4), torch.zeros(1), k, 1, 0., 0.9,
                                              0.999, 1e-8, 0.], [6], scratch=[0], accum=[0], placement=pl, emulator=EMU)
            assert torch.equal(dev[0].cpu().view(torch.int32), wantf.view(torch.int32)), pl


def test_latent_step_refusals_write_nothing(K):
    c = EC.latent_case(256, 0, 0, 0.1)
    base = [c['z'], c['gz'], c['m'], c['v'], torch.tensor([0]), None, torch.zeros(4), c['recon']]
    for n, opt, beta1 in ((0, 0, 0.9), (256, 3, 0.9), (256, 0, 1.0)):
        run_both(K, 'latent_step', base + [n, opt, 0.5, beta1, 0.999, 1e-8, 0.], [0, 2, 3, 4, 6], accum=[0, 2, 3, 4], expect='rejected',
                 emulator=EMU)
    run_both(K, 'latent_step', [c['z'], None, None, None, None, None, None, None, 256, 2, 0.5, 0.9, 0.999, 1e-8, 0.], [0], accum=[0],
             expect='rejected', emulator=EMU)            # clip only without noise
    run_both(K, 'latent_step', [c['z'], c['gz'], None, c['v'], torch.tensor([0]), None, torch.zeros(4), c['recon'], 256, 0, 0.5, 0.9,
                                0.999, 1e-8, 0.], [0, 3, 4, 6], accum=[0, 3, 4], expect='rejected', emulator=EMU)


# ------------------------------------------------------------------------------------------------------------ mosaic_gather
@pytest.mark.parametrize('shape', EC.MOSAIC_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_mosaic_gather_is_bit_exact(K, shape):
    rows, cols, h, w, S = shape
    imgs = guarded.rnd(rows * cols, 3, h, w, seed=4)
    pls = ['aligned', 'shifted'] + ([0, 1] if shape == EC.MOSAIC_SHAPES[3] else [])
    dev = run_both(K, 'mosaic_gather', [imgs, torch.zeros(3, S, S), rows, cols, 3, h, w, S], [1], atol=0.0, placement=pls, emulator=EMU)
    grid = imgs.view(rows, cols, 3, h, w)
    y = torch.arange(S)
    want = grid[(y * rows // S)[:, None], (y * cols // S)[None, :], :, (y * h // S)[:, None], (y * w // S)[None, :]].permute(2, 0, 1)
    assert torch.equal(dev[1].cpu(), want)
    run_both(K, 'mosaic_gather', [imgs, torch.zeros(3, S, S), rows, cols, 3, h, w, 0], [1], expect='rejected', emulator=EMU)


# ----------------------------------------------------------------------------------------------------------------- twice
def test_two_runs_are_bit_identical(K):
    B, C, HW = EC.RECON_SHAPES[2]
    n = EC.LATENT_SIZES[2]
    rc, lc = EC.recon_case(B, HW, 1), EC.latent_case(n, 0, 7, 0.1)
    rows, cols, h, w, S = EC.MOSAIC_SHAPES[2]
    grid_imgs = guarded.rnd(rows * cols, 3, h, w, seed=4).cuda()
    nbytes = K.recon_loss_workspace(B, C, HW)
    runs = []
    for _ in range(2):
        nan = lambda *s: torch.full(s, float('nan'), device='cuda')
        grad, loss, ws, stats, out = nan(B, C, HW), nan(1), nan((nbytes + 3) // 4), nan(4), nan(3, S, S)
        z, m, v, step = lc['z'].cuda(), lc['m'].cuda(), lc['v'].cuda(), torch.tensor([7], device='cuda')
        K.recon_loss(rc['imgs'].cuda(), rc['target'].cuda(), grad, loss, ws, nbytes, B, C, HW, 1)
        K.latent_step(z, lc['gz'].cuda(), m, v, step, None, stats, loss, n, 0, *HYPER_ARGS, 0.1)
        K.mosaic_gather(grid_imgs, out, rows, cols, 3, h, w, S)
        torch.cuda.synchronize()
        assert int(step) == 8
        runs.append(torch.cat([t.view(-1) for t in (grad, loss, z, m, v, stats, out)]).cpu().view(torch.int32))
    assert torch.equal(*runs) and not bool(torch.isnan(runs[0].view(torch.float32)).any())


def test_the_entry_points_went_through_the_guarded_harness():
    assert {'recon_loss', 'latent_step', 'mosaic_gather'} <= guarded.SEEN
