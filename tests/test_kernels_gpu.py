"""Per-entry-point parity: every HIP kernel behind include/tartangan_amd.h against the
reference semantics in tests/emulator.py, on identical seeded inputs, through the C ABI."""
import pytest
import torch

from emulator import Emulator
from guarded import rnd, run_both, workspace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    backend._set_backend_for_testing(None)
    return backend.get()


E = Emulator()


CONV_SHAPES = [
    # B, Cin, Cout, H, W, ks
    (3, 3, 16, 32, 32, 3), (2, 16, 16, 64, 64, 3), (5, 32, 16, 32, 32, 3), (2, 64, 32, 16, 16, 3),
    (20, 128, 128, 4, 4, 3), (6, 128, 64, 8, 8, 3), (2, 128, 128, 16, 16, 3), (1, 16, 3, 64, 64, 1),
    (2, 3, 16, 40, 24, 1), (3, 128, 16, 16, 16, 1), (2, 100, 120, 8, 8, 3), (2, 8, 4, 32, 32, 3),
    (1, 4, 1, 16, 16, 1), (2, 16, 3, 20, 36, 3), (2, 32, 64, 32, 32, 1), (1, 64, 128, 16, 16, 1),
    (17, 16, 48, 4, 4, 1), (2, 32, 32, 128, 128, 3),
    # many pixel tiles with a short reduction, ragged and aligned
    (8, 16, 16, 128, 128, 3), (3, 5, 7, 250, 200, 3), (2, 32, 32, 256, 256, 3), (9, 20, 40, 96, 128, 3), (5, 24, 12, 130, 127, 3),
    (8, 3, 16, 128, 128, 1), (8, 16, 3, 128, 128, 1), (4, 100, 33, 192, 128, 1), (33, 32, 16, 64, 64, 1),
    # direct few-channel 1x1 kernel: every accumulator width, vector and scalar pixel paths, both filter orientations
    (3, 32, 4, 32, 32, 1), (2, 5, 7, 9, 11, 1), (2, 64, 8, 16, 16, 1), (2, 128, 6, 20, 20, 1), (3, 200, 3, 8, 8, 1), (2, 8, 84, 8, 8, 1),
]


@pytest.mark.parametrize('shape', CONV_SHAPES)
def test_conv_fwd(K, shape):
    B, Cin, Cout, H, W, ks = shape
    x, w, b = rnd(B, Cin, H, W), rnd(Cout, Cin, ks, ks, scale=0.2), rnd(Cout)
    run_both(K, 'conv2d_fwd', [x, w, b, None, torch.zeros(B, Cout, H, W), B, Cin, Cout, H, W, ks], [4], tol=2e-5)
    run_both(K, 'conv2d_fwd', [x, w, None, None, torch.zeros(B, Cout, H, W), B, Cin, Cout, H, W, ks], [4], tol=2e-5)
    run_both(K, 'conv2d_fwd', [x, w, b, rnd(B, Cout, H, W, seed=7), torch.zeros(B, Cout, H, W), B, Cin, Cout, H, W, ks], [4], tol=2e-5)


# The step's own 3x3 layers AT THE BENCHED BATCH (64): the launch heuristics pick other tile / chunk / K-split variants here
# than on the small cases above (e.g. conv_dma_kernel<G16, 32, 1, 8> needs >= 64 images of 16x16).
STEP_CONV_SHAPES = [(64, 128, 128, 16, 16, 3), (64, 64, 128, 16, 16, 3), (64, 128, 64, 16, 16, 3), (64, 128, 64, 32, 32, 3), (64, 64, 64, 32, 32, 3),
                    (64, 32, 64, 32, 32, 3), (64, 32, 32, 64, 64, 3), (64, 64, 32, 64, 64, 3), (64, 16, 16, 128, 128, 3), (64, 32, 16, 128, 128, 3),
                    (64, 4, 16, 128, 128, 3), (64, 128, 128, 8, 8, 3), (64, 128, 128, 4, 4, 3), (64, 256, 256, 8, 8, 3),
                    # the discriminator's real | fake pass: its forward and final-backward layers at 2 x 64 images
                    (128, 4, 16, 128, 128, 3), (128, 16, 32, 64, 64, 3), (128, 32, 64, 32, 32, 3), (128, 64, 128, 16, 16, 3),
                    (128, 128, 128, 8, 8, 3),
                    # ... and the generator's forward at 2 x 64 latents (its backward stays at 64)
                    (128, 128, 128, 16, 16, 3), (128, 64, 64, 32, 32, 3), (128, 32, 32, 64, 64, 3), (128, 16, 16, 128, 128, 3)]


def poison_lds(K):
    """Leave NaNs in the LDS of every CU: LDS is not cleared between kernels, so a kernel that reads a cell it did not write
    (a lane that skipped its LDS-DMA, a pad it assumed zero) computes NaN afterwards instead of passing by luck."""
    nan = torch.full((64, 32, 64, 64), float('nan'), device='cuda')
    w = torch.full((32, 32, 3, 3), float('nan'), device='cuda')
    y = torch.empty(64, 32, 64, 64, device='cuda')
    K.conv2d_fwd(nan, w, None, None, y, 64, 32, 32, 64, 64, 3)
    gw = torch.empty_like(w)
    ws = torch.empty((K.conv2d_wgrad_workspace(64, 32, 32, 64, 64, 3) + 3) // 4, device='cuda')
    K.conv2d_wgrad(nan, nan, gw, None, ws, ws.numel() * 4, 64, 32, 32, 64, 64, 3, 0)
    nan8 = torch.full((64, 128, 8, 8), float('nan'), device='cuda')
    w8 = torch.full((128, 128, 3, 3), float('nan'), device='cuda')
    K.conv2d_fwd(nan8, w8, None, None, torch.empty_like(nan8), 64, 128, 128, 8, 8, 3)
    hi = torch.full((64, 32, 64, 64), float('nan'), device='cuda'); lo = torch.empty(64, 32, 32, 32, device='cuda')
    K.poolconv3x3_fwd(hi, torch.full((32, 32, 4, 4), float('nan'), device='cuda'), None, None, lo, 64, 32, 32, 32, 32)
    K.upconv3x3_fwd(lo.fill_(float('nan')), torch.full((4, 32, 32, 2, 2), float('nan'), device='cuda'), None, None, hi, 64, 32, 32, 32, 32)
    torch.cuda.synchronize()


@pytest.mark.parametrize('shape', STEP_CONV_SHAPES)
def test_conv_step_shapes_full_batch_after_lds_poison(K, shape):
    B, Cin, Cout, H, W, ks = shape
    x, w, b = rnd(B, Cin, H, W), rnd(Cout, Cin, ks, ks, scale=0.2), rnd(Cout)
    gy = rnd(B, Cout, H, W, seed=3)
    poison_lds(K)
    run_both(K, 'conv2d_fwd', [x, w, b, None, torch.zeros(B, Cout, H, W), B, Cin, Cout, H, W, ks], [4], tol=2e-5)
    poison_lds(K)
    run_both(K, 'conv2d_dgrad', [gy, w, torch.zeros(B, Cin, H, W), B, Cin, Cout, H, W, ks], [2], tol=2e-5)
    ws = workspace(K.conv2d_wgrad_workspace(B, Cin, Cout, H, W, ks))
    poison_lds(K)
    run_both(K, 'conv2d_wgrad', [x, gy, torch.zeros(Cout, Cin, ks, ks), torch.zeros(Cout), ws, ws.numel() * 4, B, Cin, Cout, H, W, ks, 0],
             [2, 3], tol=5e-5, scratch=[4])


STEP_S2_SHAPES = [(64, 128, 128, 8, 8), (64, 128, 64, 16, 16), (64, 64, 32, 32, 32), (64, 32, 16, 64, 64),
                  # pooled convolutions of the paired discriminator pass (2 x 64 images)
                  (128, 16, 16, 64, 64), (128, 32, 32, 32, 32), (128, 64, 64, 16, 16), (128, 128, 128, 8, 8), (128, 128, 128, 4, 4),
                  # up-convolutions of the generator's shared pass (2 x 64 latents)
                  (128, 128, 64, 16, 16), (128, 64, 32, 32, 32), (128, 32, 16, 64, 64)]


@pytest.mark.parametrize('shape', STEP_S2_SHAPES)
def test_stride2_step_shapes_full_batch_after_lds_poison(K, shape):
    B, Cin, Cout, H, W = shape                     # H x W: the low-resolution plane
    a, w, b = rnd(B, Cin, H, W), rnd(Cout, Cin, 3, 3, scale=0.2), rnd(Cout)
    wp, w4t = torch.zeros(4, Cout, Cin, 2, 2), torch.zeros(Cin, Cout, 4, 4)
    E.upconv3x3_weights(w, wp, Cout, Cin)
    E.upconv3x3_weights_t(w, w4t, Cout, Cin)
    gyh = rnd(B, Cout, 2 * H, 2 * W, seed=3)
    poison_lds(K)
    run_both(K, 'upconv3x3_fwd', [a, wp, b, None, torch.zeros(B, Cout, 2 * H, 2 * W), B, Cin, Cout, H, W], [4], tol=3e-5)
    if K.upconv3x3_dgrad_supported(B, Cin, Cout, H, W):        # (4x4 source planes take the composed path in the layer)
        poison_lds(K)
        run_both(K, 'upconv3x3_dgrad', [gyh, w4t, torch.zeros(B, Cin, H, W), B, Cin, Cout, H, W], [2], tol=5e-5)
        ws = workspace(K.upconv3x3_wgrad_workspace(B, Cin, Cout, H, W))
        poison_lds(K)
        run_both(K, 'upconv3x3_wgrad', [a, gyh, torch.zeros(Cout, Cin, 3, 3), ws, ws.numel() * 4, B, Cin, Cout, H, W, 0, torch.zeros(Cout)], [2, 11],
                 tol=1e-4, scratch=[3])
    x, gy = rnd(B, Cin, 2 * H, 2 * W, seed=5), rnd(B, Cout, H, W, seed=6)
    w4, wpp = torch.zeros(Cout, Cin, 4, 4), torch.zeros(4, Cin, Cout, 2, 2)
    E.poolconv3x3_weights(w, w4, wpp, Cout, Cin)
    if K.poolconv3x3_supported(B, Cin, Cout, H, W):
        poison_lds(K)
        run_both(K, 'poolconv3x3_fwd', [x, w4, b, None, torch.zeros(B, Cout, H, W), B, Cin, Cout, H, W], [4], tol=5e-5)
        poison_lds(K)
        run_both(K, 'poolconv3x3_dgrad', [gy, wpp, torch.zeros(B, Cin, 2 * H, 2 * W), B, Cin, Cout, H, W], [2], tol=5e-5)
        ws = workspace(K.poolconv3x3_wgrad_workspace(B, Cin, Cout, H, W))
        poison_lds(K)
        run_both(K, 'poolconv3x3_wgrad', [x, gy, torch.zeros(Cout, Cin, 3, 3), ws, ws.numel() * 4, B, Cin, Cout, H, W, 0, torch.zeros(Cout)], [2, 11],
                 tol=1e-4, scratch=[3])


@pytest.mark.parametrize('shape', [(2, 16, 16, 64, 64), (3, 32, 16, 32, 32), (2, 64, 32, 16, 16), (5, 128, 128, 8, 8), (20, 128, 128, 4, 4),
                                   (2, 8, 12, 20, 36), (2, 20, 24, 10, 6), (3, 5, 7, 34, 18), (64, 16, 16, 128, 128), (64, 64, 64, 32, 32), (64, 128, 128, 16, 16),
                                   (64, 128, 128, 8, 8)])
def test_conv_fwd_with_half_resolution_residual(K, shape):
    """y = conv3x3(x) + bias + up2x(residual_lo): the generator block's shortcut added from the low resolution."""
    B, Cin, Cout, H, W = shape
    x, w, b = rnd(B, Cin, H, W), rnd(Cout, Cin, 3, 3, scale=0.2), rnd(Cout)
    r = rnd(B, Cout, H // 2, W // 2, seed=7)
    poison_lds(K)
    run_both(K, 'conv2d_fwd_up2res', [x, w, b, r, torch.zeros(B, Cout, H, W), B, Cin, Cout, H, W], [4], tol=2e-5)
    run_both(K, 'conv2d_fwd_up2res', [x, w, None, r, torch.zeros(B, Cout, H, W), B, Cin, Cout, H, W], [4], tol=2e-5)
    # the same bits as the materialised form: up2x, then the plain fused-residual kernel
    xd, wd, bd, rd = x.cuda(), w.cuda(), b.cuda(), r.cuda()
    y1, y2, ru = torch.empty(B, Cout, H, W, device='cuda'), torch.empty(B, Cout, H, W, device='cuda'), torch.empty(B, Cout, H, W, device='cuda')
    K.conv2d_fwd_up2res(xd, wd, bd, rd, y1, B, Cin, Cout, H, W)
    K.up2x(rd, ru, 1.0, B * Cout, H // 2, W // 2)
    K.conv2d_fwd(xd, wd, bd, ru, y2, B, Cin, Cout, H, W, 3)
    assert torch.equal(y1, y2)


UPCONV_SHAPES = [(2, 16, 16, 16, 16), (3, 8, 20, 8, 8), (2, 32, 16, 64, 64), (4, 128, 128, 4, 4), (2, 128, 64, 16, 16), (2, 5, 7, 6, 10),
                 (8, 64, 32, 32, 32), (1, 16, 3, 33, 20), (64, 128, 128, 4, 4),
                 # enough low-resolution tiles for the all-phases-in-one kernel (aligned, 16x16 planes, ragged)
                 (16, 32, 16, 64, 64), (128, 8, 24, 16, 16), (20, 12, 10, 70, 50), (64, 64, 32, 32, 32),
                 # 8x8 source planes: 4 images per tile (full and ragged batch)
                 (64, 128, 128, 8, 8), (258, 24, 40, 8, 8), (520, 24, 20, 8, 8)]


@pytest.mark.parametrize('shape', UPCONV_SHAPES)
def test_upconv3x3(K, shape):
    """conv3x3(up2x(a)) as four low-resolution 2x2-tap phases == the reference's formulation."""
    B, Cin, Cout, H, W = shape
    a, w, b = rnd(B, Cin, H, W), rnd(Cout, Cin, 3, 3, scale=0.2), rnd(Cout)
    wp = torch.zeros(4, Cout, Cin, 2, 2)
    run_both(K, 'upconv3x3_weights', [w, wp, Cout, Cin], [1], tol=1e-6)
    E.upconv3x3_weights(w, wp, Cout, Cin)
    y = torch.zeros(B, Cout, 2 * H, 2 * W)
    run_both(K, 'upconv3x3_fwd', [a, wp, b, None, y, B, Cin, Cout, H, W], [4], tol=3e-5)
    run_both(K, 'upconv3x3_fwd', [a, wp, None, rnd(B, Cout, 2 * H, 2 * W, seed=7), y, B, Cin, Cout, H, W], [4], tol=3e-5)
    # and against the textbook formulation
    E.upconv3x3_fwd(a, wp, b, None, y, B, Cin, Cout, H, W)
    want = torch.nn.functional.conv2d(torch.nn.functional.interpolate(a, scale_factor=2), w, b, padding=1)
    assert torch.allclose(y, want, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize('shape', [(16, 32, 16, 64, 64), (128, 32, 24, 16, 16), (20, 20, 10, 70, 50), (64, 64, 32, 32, 32), (8, 70, 9, 128, 32),
                                   (64, 128, 128, 8, 8), (258, 40, 24, 8, 8), (520, 24, 20, 8, 8)])
def test_upconv3x3_dgrad(K, shape):
    """stride-2 4x4 transpose kernel == pool2x2sum(dgrad3x3(gy)) == autograd's gradient of conv3x3(up2x(a))."""
    B, Cin, Cout, H, W = shape
    assert K.upconv3x3_dgrad_supported(B, Cin, Cout, H, W)
    w, gy = rnd(Cout, Cin, 3, 3, scale=0.2), rnd(B, Cout, 2 * H, 2 * W, seed=3)
    w4t = torch.zeros(Cin, Cout, 4, 4)
    run_both(K, 'upconv3x3_weights_t', [w, w4t, Cout, Cin], [1], tol=1e-6)
    E.upconv3x3_weights_t(w, w4t, Cout, Cin)
    ga = torch.zeros(B, Cin, H, W)
    run_both(K, 'upconv3x3_dgrad', [gy, w4t, ga, B, Cin, Cout, H, W], [2], tol=5e-5)
    E.upconv3x3_dgrad(gy, w4t, ga, B, Cin, Cout, H, W)
    a = torch.zeros(B, Cin, H, W, requires_grad=True)
    y = torch.nn.functional.conv2d(torch.nn.functional.interpolate(a, scale_factor=2), w, None, padding=1)
    want, = torch.autograd.grad(y, a, gy)
    assert torch.allclose(ga, want, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize('shape', [(16, 16, 16, 64, 64), (128, 32, 24, 16, 16), (20, 20, 18, 70, 50), (64, 64, 64, 16, 16), (8, 40, 33, 128, 32),
                                   (64, 128, 128, 8, 8), (258, 40, 36, 8, 8), (520, 24, 20, 8, 8)])
def test_poolconv3x3(K, shape):
    """AvgPool2d(2) o conv3x3 as one stride-2 kernel, and its input gradient as the four-phase kernel."""
    B, Cin, Cout, H, W = shape            # H x W = pooled output plane
    assert K.poolconv3x3_supported(B, Cin, Cout, H, W)
    x, w, b = rnd(B, Cin, 2 * H, 2 * W), rnd(Cout, Cin, 3, 3, scale=0.2), rnd(Cout)
    w4, wp = torch.zeros(Cout, Cin, 4, 4), torch.zeros(4, Cin, Cout, 2, 2)
    run_both(K, 'poolconv3x3_weights', [w, w4, wp, Cout, Cin], [1, 2], tol=1e-6)
    E.poolconv3x3_weights(w, w4, wp, Cout, Cin)
    y = torch.zeros(B, Cout, H, W)
    run_both(K, 'poolconv3x3_fwd', [x, w4, b, None, y, B, Cin, Cout, H, W], [4], tol=5e-5)
    run_both(K, 'poolconv3x3_fwd', [x, w4, None, rnd(B, Cout, H, W, seed=7), y, B, Cin, Cout, H, W], [4], tol=5e-5)
    gy, gx = rnd(B, Cout, H, W, seed=3), torch.zeros(B, Cin, 2 * H, 2 * W)
    run_both(K, 'poolconv3x3_dgrad', [gy, wp, gx, B, Cin, Cout, H, W], [2], tol=5e-5)
    # and against the textbook formulation
    E.poolconv3x3_fwd(x, w4, b, None, y, B, Cin, Cout, H, W)
    E.poolconv3x3_dgrad(gy, wp, gx, B, Cin, Cout, H, W)
    xr = x.clone().requires_grad_()
    want = torch.nn.functional.avg_pool2d(torch.nn.functional.conv2d(xr, w, b, padding=1), 2)
    assert torch.allclose(y, want, rtol=1e-4, atol=1e-4)
    gwant, = torch.autograd.grad(want, xr, gy)
    assert torch.allclose(gx, gwant, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize('shape', [(16, 16, 16, 64, 64), (32, 32, 24, 16, 16), (10, 20, 18, 70, 50), (64, 64, 64, 16, 16), (4, 40, 33, 64, 32),
                                   (64, 128, 128, 8, 8), (30, 40, 24, 8, 8)])
def test_stride2_weight_gradients(K, shape):
    """16-tap stride-2 weight gradients of the pooled conv and of the up-conv == the 3x3 weight gradient on the
    materialised high-resolution pair."""
    B, Cin, Cout, H, W = shape
    w0 = rnd(Cout, Cin, 3, 3, seed=9)
    # pooled conv: x high resolution (Cin), gy low resolution (Cout)
    x, gy = rnd(B, Cin, 2 * H, 2 * W), rnd(B, Cout, H, W, seed=3)
    ws = workspace(K.poolconv3x3_wgrad_workspace(B, Cin, Cout, H, W))
    b0 = rnd(Cout, seed=10)
    for acc in (0, 1):       # with the bias gradient riding along (sum of gy), and without
        run_both(K, 'poolconv3x3_wgrad', [x, gy, w0.clone(), ws, ws.numel() * 4, B, Cin, Cout, H, W, acc, b0.clone()], [2, 11], tol=1e-4, scratch=[3])
    run_both(K, 'poolconv3x3_wgrad', [x, gy, w0.clone(), ws, ws.numel() * 4, B, Cin, Cout, H, W, 0, None], [2], tol=1e-4, scratch=[3])
    # up-conv: a low resolution (Cin), gy high resolution (Cout)
    a, gyh = rnd(B, Cin, H, W, seed=4), rnd(B, Cout, 2 * H, 2 * W, seed=5)
    ws = workspace(K.upconv3x3_wgrad_workspace(B, Cin, Cout, H, W))
    for acc in (0, 1):
        run_both(K, 'upconv3x3_wgrad', [a, gyh, w0.clone(), ws, ws.numel() * 4, B, Cin, Cout, H, W, acc, b0.clone()], [2, 11], tol=1e-4, scratch=[3])
    run_both(K, 'upconv3x3_wgrad', [a, gyh, w0.clone(), ws, ws.numel() * 4, B, Cin, Cout, H, W, 0, None], [2], tol=1e-4, scratch=[3])


@pytest.mark.parametrize('shape', [(16, 16, 16, 64, 64), (32, 32, 24, 16, 16), (10, 20, 18, 70, 50), (64, 128, 128, 8, 8)])
def test_stride2_weight_gradients_in_two_steps_are_bit_identical(K, shape):
    """tg_*_wgrad_partials + ONE tg_s2_wgrad_reduce_batch for several layers == the one-call forms, bit for bit, incl. the bias
    gradients and accumulation into an existing gradient."""
    B, Cin, Cout, H, W = shape
    x, gy = rnd(B, Cin, 2 * H, 2 * W).cuda(), rnd(B, Cout, H, W, seed=3).cuda()
    a, gyh = rnd(B, Cin, H, W, seed=4).cuda(), rnd(B, Cout, 2 * H, 2 * W, seed=5).cuda()
    w0, b0 = rnd(Cout, Cin, 3, 3, seed=9).cuda(), rnd(Cout, seed=10).cuda()
    want = []
    for name, lo, hi in (('poolconv3x3', x, gy), ('upconv3x3', a, gyh)):
        ws = workspace(getattr(K, name + '_wgrad_workspace')(B, Cin, Cout, H, W)).cuda()
        gw, gb = w0.clone(), b0.clone()
        getattr(K, name + '_wgrad')(lo, hi, gw, ws, ws.numel() * 4, B, Cin, Cout, H, W, 1, gb)
        gw2 = w0.clone()
        getattr(K, name + '_wgrad')(lo, hi, gw2, ws, ws.numel() * 4, B, Cin, Cout, H, W, 0, None)
        want.append((gw, gb, gw2))
    rows, got, keep = [], [], []
    for mode, (name, lo, hi) in enumerate((('poolconv3x3', x, gy), ('upconv3x3', a, gyh))):
        for with_bias, acc in ((1, 1), (0, 0)):
            ws = workspace(getattr(K, name + '_wgrad_workspace')(B, Cin, Cout, H, W)).cuda()
            getattr(K, name + '_wgrad_partials')(lo, hi, ws, ws.numel() * 4, B, Cin, Cout, H, W, with_bias)
            gw, gb = w0.clone(), b0.clone()
            rows.append([ws.data_ptr(), gw.data_ptr(), gb.data_ptr() if with_bias else 0, B, Cin, Cout, H, W, mode, acc])
            got.append((gw, gb))
            keep.append(ws)
    K.s2_wgrad_reduce_batch(torch.tensor(rows, dtype=torch.int64), len(rows))
    torch.cuda.synchronize()
    for mode in (0, 1):
        gw, gb, gw2 = want[mode]
        assert torch.equal(got[2 * mode][0], gw) and torch.equal(got[2 * mode][1], gb)
        assert torch.equal(got[2 * mode + 1][0], gw2) and torch.equal(got[2 * mode + 1][1], b0)


def _s2_table(K, n=18):
    """``n`` rows of tg_s2_wgrad_reduce_batch (more than the 16 one launch holds), stage 1 done: small 8x8, odd and 16x16 planes, the
    modes alternating, with and without bias, overwriting and accumulating -> rows, [(gw, gb)], [(wanted gw, wanted gb)] from the
    one-call forms, and what must stay alive."""
    shapes = [(3, 5, 7, 8, 8), (2, 5, 7, 12, 10), (2, 16, 8, 16, 16)]
    rows, got, want, keep = [], [], [], []
    for i in range(n):
        B, Cin, Cout, H, W = shapes[i % 3]
        mode, with_bias, acc = i % 2, (i // 2) % 2, (i // 3) % 2
        name = 'upconv3x3' if mode else 'poolconv3x3'
        lo = rnd(B, Cin, *((H, W) if mode else (2 * H, 2 * W)), seed=i).cuda()
        hi = rnd(B, Cout, *((2 * H, 2 * W) if mode else (H, W)), seed=50 + i).cuda()
        w0, b0 = rnd(Cout, Cin, 3, 3, seed=100 + i).cuda(), rnd(Cout, seed=150 + i).cuda()
        nbytes = getattr(K, name + '_wgrad_workspace')(B, Cin, Cout, H, W)
        ws = workspace(nbytes).cuda()
        a, ab = w0.clone(), b0.clone()
        getattr(K, name + '_wgrad')(lo, hi, a, ws, ws.numel() * 4, B, Cin, Cout, H, W, acc, ab if with_bias else None)
        want.append((a, ab))
        ws2 = workspace(nbytes).cuda()
        getattr(K, name + '_wgrad_partials')(lo, hi, ws2, ws2.numel() * 4, B, Cin, Cout, H, W, with_bias)
        gw, gb = w0.clone(), b0.clone()
        rows.append([ws2.data_ptr(), gw.data_ptr(), gb.data_ptr() if with_bias else 0, B, Cin, Cout, H, W, mode, acc])
        got.append((gw, gb))
        keep.append(ws2)
    return rows, got, want, keep


def test_stride2_batched_reduce_is_bit_identical_across_launches(K):
    """18 rows: tg_s2_wgrad_reduce_batch cuts them into two launches (16 items per argument block); each row == its one-call form."""
    rows, got, want, keep = _s2_table(K)
    assert {(r[8], bool(r[2]), r[9]) for r in rows} == {(m, b, a) for m in (0, 1) for b in (False, True) for a in (0, 1)}
    K.s2_wgrad_reduce_batch(torch.tensor(rows, dtype=torch.int64), len(rows))
    torch.cuda.synchronize()
    for (gw, gb), (a, ab) in zip(got, want):
        assert torch.equal(gw, a) and torch.equal(gb, ab)


def _forms_table(n=18):
    """``n`` rows of tg_poolconv3x3_weights_batch: Cout*Cin below one 256-thread workgroup, no multiple of 256, and several of them."""
    pairs = [(5, 7), (20, 18), (16, 16), (33, 40)]
    assert 5 * 7 < 256 and (20 * 18) % 256 and (33 * 40) % 256
    rows, ws, outs = [], [], []
    for i in range(n):
        Cout, Cin = pairs[i % len(pairs)]
        w = rnd(Cout, Cin, 3, 3, seed=i).cuda()
        w4, wp = rnd(Cout, Cin, 4, 4, seed=30 + i).cuda(), rnd(4, Cin, Cout, 2, 2, seed=60 + i).cuda()
        rows.append([w.data_ptr(), w4.data_ptr(), wp.data_ptr(), Cout, Cin])
        ws.append(w)
        outs.append((w4, wp))
    return rows, ws, outs


def test_poolconv_weights_batch_is_bit_identical_across_launches(K):
    """18 rows (two launches of at most 16 items) == 18 single tg_poolconv3x3_weights calls, bit for bit."""
    rows, ws, outs = _forms_table()
    K.poolconv3x3_weights_batch(torch.tensor(rows, dtype=torch.int64), len(rows))
    torch.cuda.synchronize()
    for (w, w4, wp, Cout, Cin), src, (got4, gotp) in zip(rows, ws, outs):
        one4, onep = torch.zeros_like(got4), torch.zeros_like(gotp)
        K.poolconv3x3_weights(src, one4, onep, Cout, Cin)
        assert torch.equal(got4, one4) and torch.equal(gotp, onep)


def _rejected_unwritten(call, rows, outs, code):
    """``call(table, n)`` fails with ``code`` and no tensor of ``outs`` changed: every row is checked before the first launch."""
    from tartangan_amd import backend
    before = [t.clone() for t in outs]
    torch.cuda.synchronize()
    with pytest.raises(backend.KernelError, match=f'code {code}$'):
        call(torch.tensor(rows, dtype=torch.int64), len(rows))
    torch.cuda.synchronize()
    for t, t0 in zip(outs, before):
        assert torch.equal(t, t0)


def test_a_bad_row_behind_the_first_launch_leaves_nothing_written(K):
    """A table longer than one argument block whose bad row sits in the SECOND launch's share: the error comes back and not even
    the first launch has run -- no output, no accumulating gradient has changed.  (Every address in the tables is live device
    memory or 0.)"""
    # tg_s2_wgrad_reduce_batch: the 17th of 18 rows without a gw (-1), then on a 4x4 plane, which the stride-2 kernels do not take (-2)
    rows, got, _, keep = _s2_table(K)
    outs = [t for pair in got for t in pair]
    bad = [list(r) for r in rows]
    bad[16][1] = 0
    _rejected_unwritten(K.s2_wgrad_reduce_batch, bad, outs, -1)
    bad = [list(r) for r in rows]
    bad[16][6:8] = [4, 4]
    _rejected_unwritten(K.s2_wgrad_reduce_batch, bad, outs, -2)
    # tg_poolconv3x3_weights_batch: the 17th of 18 rows without a w4
    rows, ws, forms = _forms_table()
    rows[16][1] = 0
    _rejected_unwritten(K.poolconv3x3_weights_batch, rows, [t for pair in forms for t in pair], -1)
    # tg_conv2d_wgrad_reduce_batch (40 items per launch): the 41st of 45 rows without a gw, then with a 5x5 filter (-2)
    rows, outs, keep = [], [], []
    for i in range(45):
        B, Cin, Cout, H, W, ks = [(3, 5, 7, 20, 12, 3), (2, 8, 4, 8, 8, 1), (2, 16, 16, 4, 4, 3)][i % 3]
        x, gy = rnd(B, Cin, H, W, seed=i).cuda(), rnd(B, Cout, H, W, seed=100 + i).cuda()
        ws = workspace(K.conv2d_wgrad_workspace(B, Cin, Cout, H, W, ks)).cuda()
        K.conv2d_wgrad_partials(x, gy, ws, ws.numel() * 4, B, Cin, Cout, H, W, ks, 1)
        gw, gb = rnd(Cout, Cin, ks, ks, seed=200 + i).cuda(), rnd(Cout, seed=300 + i).cuda()
        rows.append([ws.data_ptr(), gw.data_ptr(), gb.data_ptr(), B, Cin, Cout, H, W, ks, i % 2])
        outs += [gw, gb]
        keep.append(ws)
    bad = [list(r) for r in rows]
    bad[40][1] = 0
    _rejected_unwritten(K.conv2d_wgrad_reduce_batch, bad, outs, -1)
    bad = [list(r) for r in rows]
    bad[40][8] = 5
    _rejected_unwritten(K.conv2d_wgrad_reduce_batch, bad, outs, -2)


@pytest.mark.parametrize('op', ['pool_conv', 'up_conv'])
def test_stride2_functions_under_autograd(K, op):
    """The Functions built on the stride-2 kernels, on the GPU, against plain torch on the CPU: values, first-order
    gradients and (pooled conv, which sits under the R1 penalty) the gradient of a gradient-norm penalty."""
    from tartangan_amd import functional as TF
    F = torch.nn.functional
    B, Cin, Cout, S = 128, 32, 24, 16                     # enough 16x16 planes for the one-kernel forms
    x0, w0, b0 = rnd(B, Cin, 2 * S if op == 'pool_conv' else S, 2 * S if op == 'pool_conv' else S), rnd(Cout, Cin, 3, 3, scale=0.2), rnd(Cout, scale=0.1)
    assert TF.pool_conv3x3_supported(x0.cuda(), w0.cuda()) if op == 'pool_conv' else TF.upconv3x3_pays(x0, w0)

    def run(dev, second_order):
        x, w, b = (t.detach().clone().to(dev).requires_grad_() for t in (x0, w0, b0))
        if dev == 'cuda':
            y = TF.pool_conv3x3(x, w, b) if op == 'pool_conv' else TF.upconv3x3(x, w, b)
        else:
            y = F.avg_pool2d(F.conv2d(x, w, b, padding=1), 2) if op == 'pool_conv' else \
                F.conv2d(F.interpolate(x, scale_factor=2), w, b, padding=1)
        if second_order:
            g, = torch.autograd.grad(y.tanh().sum(), x, create_graph=True)
            (g.pow(2).sum() + y.sum()).backward()
        else:
            y.pow(2).sum().backward()
        return [t.detach().cpu() for t in (y, x.grad, w.grad, b.grad)]

    for second_order in ((False, True) if op == 'pool_conv' else (False,)):
        got, want = run('cuda', second_order), run('cpu', second_order)
        for a_, b_ in zip(got, want):
            scale = float(b_.abs().max())
            assert float((a_ - b_).abs().max()) <= 2e-4 * scale + 1e-5, (op, second_order)


def test_conv_fwd_exact_integer_layout(K):
    """Asymmetric small-integer data: any A/B/C fragment transposition shows up as an exact mismatch."""
    B, Cin, Cout, H, W = 2, 8, 32, 32, 32
    x = (torch.arange(B * Cin * H * W) % 7 - 3).float().view(B, Cin, H, W)
    w = (torch.arange(Cout * Cin * 9) % 5 - 2).float().view(Cout, Cin, 3, 3)
    run_both(K, 'conv2d_fwd', [x, w, None, None, torch.zeros(B, Cout, H, W), B, Cin, Cout, H, W, 3], [4], atol=0.0)
    run_both(K, 'conv2d_dgrad', [torch.round(rnd(B, Cout, H, W) * 2), w, torch.zeros(B, Cin, H, W), B, Cin, Cout, H, W, 3],
             [2], atol=0.0)


@pytest.mark.parametrize('shape', CONV_SHAPES)
def test_conv_dgrad(K, shape):
    B, Cin, Cout, H, W, ks = shape
    gy, w = rnd(B, Cout, H, W), rnd(Cout, Cin, ks, ks, scale=0.2)
    run_both(K, 'conv2d_dgrad', [gy, w, torch.zeros(B, Cin, H, W), B, Cin, Cout, H, W, ks], [2], tol=2e-5)


@pytest.mark.parametrize('shape', CONV_SHAPES)
def test_conv_wgrad(K, shape):
    B, Cin, Cout, H, W, ks = shape
    x, gy = rnd(B, Cin, H, W), rnd(B, Cout, H, W, seed=3)
    nbytes = K.conv2d_wgrad_workspace(B, Cin, Cout, H, W, ks)
    assert nbytes > 0
    ws = workspace(nbytes)
    run_both(K, 'conv2d_wgrad', [x, gy, torch.zeros(Cout, Cin, ks, ks), None, ws, ws.numel() * 4, B, Cin, Cout, H, W, ks, 0],
             [2], tol=5e-5, scratch=[4])
    # fused bias gradient + accumulate-into-existing (the flat .grad bucket path)
    run_both(K, 'conv2d_wgrad', [x, gy, rnd(Cout, Cin, ks, ks, seed=9), rnd(Cout, seed=10), ws, ws.numel() * 4,
                                 B, Cin, Cout, H, W, ks, 1], [2, 3], tol=5e-5, scratch=[4])
    run_both(K, 'conv2d_wgrad', [x, gy, rnd(Cout, Cin, ks, ks, seed=9), rnd(Cout, seed=10), ws, ws.numel() * 4,
                                 B, Cin, Cout, H, W, ks, 0], [2, 3], tol=5e-5, scratch=[4])


def test_conv_wgrad_is_deterministic(K):
    B, Cin, Cout, H, W, ks = 4, 32, 32, 32, 32, 3
    x, gy = rnd(B, Cin, H, W).cuda(), rnd(B, Cout, H, W, seed=3).cuda()
    ws = workspace(K.conv2d_wgrad_workspace(B, Cin, Cout, H, W, ks)).cuda()
    outs = []
    for _ in range(3):
        gw = torch.zeros(Cout, Cin, ks, ks).cuda()
        K.conv2d_wgrad(x, gy, gw, None, ws, ws.numel() * 4, B, Cin, Cout, H, W, ks, 0)
        outs.append(gw.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


def test_conv_wgrad_batched_reduce_is_bit_identical(K):
    """stage 1 + one batched stage 2 over many layers == the per-layer call, bit for bit (also across the
    kernel-argument chunking at 40 items)."""
    shapes = [(4, 16, 16, 32, 32, 3), (2, 128, 128, 8, 8, 3), (3, 5, 7, 20, 12, 3), (4, 32, 4, 32, 32, 1), (2, 3, 16, 64, 64, 1)] * 9
    want, got, items, keep = [], [], [], []
    for i, (B, Cin, Cout, H, W, ks) in enumerate(shapes):
        x, gy = rnd(B, Cin, H, W, seed=i).cuda(), rnd(B, Cout, H, W, seed=100 + i).cuda()
        bias = i % 2 == 0
        gw0, gb0 = rnd(Cout, Cin, ks, ks, seed=200 + i).cuda(), rnd(Cout, seed=300 + i).cuda()
        nbytes = K.conv2d_wgrad_workspace(B, Cin, Cout, H, W, ks)
        ws = workspace(nbytes).cuda()
        a, ab = gw0.clone(), gb0.clone()
        K.conv2d_wgrad(x, gy, a, ab if bias else None, ws, ws.numel() * 4, B, Cin, Cout, H, W, ks, 1)
        want.append((a, ab))
        b, bb = gw0.clone(), gb0.clone()
        ws2 = workspace(nbytes).cuda()
        K.conv2d_wgrad_partials(x, gy, ws2, ws2.numel() * 4, B, Cin, Cout, H, W, ks, int(bias))
        items.append([ws2.data_ptr(), b.data_ptr(), bb.data_ptr() if bias else 0, B, Cin, Cout, H, W, ks, 1])
        got.append((b, bb))
        keep.append(ws2)
    K.conv2d_wgrad_reduce_batch(torch.tensor(items, dtype=torch.int64), len(items))
    torch.cuda.synchronize()
    for (a, ab), (b, bb) in zip(want, got):
        assert torch.equal(a, b) and torch.equal(ab, bb)
    with pytest.raises(RuntimeError):
        K.conv2d_wgrad_reduce_batch(torch.tensor(items, dtype=torch.int64).cuda(), len(items))    # table must be host memory


def test_conv_rejects_unsupported(K):
    x = torch.zeros(1, 4, 8, 8).cuda()
    with pytest.raises(RuntimeError):
        K.conv2d_fwd(x, torch.zeros(4, 4, 5, 5).cuda(), None, None, torch.zeros(1, 4, 8, 8).cuda(), 1, 4, 4, 8, 8, 5)


@pytest.mark.parametrize('shape', [(64, 32, 4, 4, 16, 64, 64), (128, 32, 4, 4, 16, 32, 32), (3, 32, 4, 4, 16, 8, 8), (2, 64, 8, 8, 32, 8, 8),
                                   (5, 48, 6, 6, 24, 16, 16), (2, 20, 2, 2, 10, 12, 12), (2, 16, 2, 2, 8, 4, 4)])
def test_fused_attention_projections(K, shape):
    """tg_conv1x1_multi_{fwd,dgrad,wgrad}: theta | phi | g of SelfAttention2d in one pass each way, against three convolutions."""
    B, Cin, c0, c1, c2, H, W = shape
    assert K.conv1x1_multi_supported(c0, c1, c2, B, Cin, H, W)
    C = c0 + c1 + c2
    x, w = rnd(B, Cin, H, W), rnd(C, Cin, scale=0.2)
    outs = [torch.zeros(B, c, H, W) for c in (c0, c1, c2)]
    run_both(K, 'conv1x1_multi_fwd', [x, w, outs[0], outs[1], outs[2], c0, c1, c2, B, Cin, H, W], [2, 3, 4], tol=2e-5)
    gys = [rnd(B, c, H, W, seed=3 + k) for k, c in enumerate((c0, c1, c2))]
    run_both(K, 'conv1x1_multi_dgrad', [gys[0], gys[1], gys[2], w, torch.zeros(B, Cin, H, W), c0, c1, c2, B, Cin, H, W], [4], tol=3e-5)
    ws = workspace(K.conv1x1_multi_wgrad_workspace(c0, c1, c2, B, Cin, H, W))
    for acc in (0, 1):
        run_both(K, 'conv1x1_multi_wgrad', [x, gys[0], gys[1], gys[2], rnd(C, Cin, seed=9), ws, ws.numel() * 4, c0, c1, c2, B, Cin, H, W, acc],
                 [4], tol=5e-5, scratch=[5])
    assert not K.conv1x1_multi_supported(c0, c1, c2, B, Cin, 5, 7) and not K.conv1x1_multi_supported(c0, c1, c2, B, 128, H, W)
    with pytest.raises(RuntimeError):
        K.conv1x1_multi_fwd(torch.zeros(B, Cin, 5, 7).cuda(), w.cuda(), *[torch.zeros(B, c, 5, 7).cuda() for c in (c0, c1, c2)],
                            c0, c1, c2, B, Cin, 5, 7)


BN_SHAPES = [(4, 16, 64 * 64), (8, 128, 16), (3, 3, 32 * 32), (2, 32, 128 * 128), (5, 100, 8 * 8), (64, 128, 1), (2, 7, 12 * 10),
             (64, 128, 64), (64, 128, 256), (16, 64, 1024), (64, 128, 16)]


@pytest.mark.parametrize('shape', BN_SHAPES)
def test_batchnorm_all_passes(K, shape):
    B, C, HW = shape
    x = rnd(B, C, HW) * 1.5 + 0.3
    gamma, beta = 1 + 0.1 * rnd(C), 0.1 * rnd(C, seed=1)
    rm, rv = 0.05 * rnd(C, seed=2), 1 + 0.1 * torch.rand(C)
    ws = workspace(K.bn_workspace(B, C, HW))
    mean, invstd = torch.zeros(C), torch.zeros(C)
    nbt = torch.tensor(41, dtype=torch.int64)
    run_both(K, 'bn_train_stats', [x, mean, invstd, rm, rv, nbt, 0.1, 1e-5, ws, B, C, HW, 1], [1, 2, 3, 4, 5], tol=1e-5)
    run_both(K, 'bn_train_stats', [x, mean, invstd, rm, rv, nbt, 0.1, 1e-5, ws, B, C, HW, 4], [1, 2, 3, 4, 5], tol=1e-5)
    run_both(K, 'bn_train_fwd', [x, torch.zeros(C), torch.zeros(C), rm, rv, nbt, gamma, beta, 0.2, 0.1, 1e-5,
                                 torch.zeros(B, C, HW), ws, B, C, HW, 1], [1, 2, 3, 4, 5, 11], tol=1e-5)
    run_both(K, 'bn_train_fwd', [x, torch.zeros(C), torch.zeros(C), rm, rv, nbt, gamma, beta, 0.2, 0.1, 1e-5,
                                 torch.zeros(B, C, HW), ws, B, C, HW, 4], [1, 2, 3, 4, 5, 11], tol=1e-5)
    E.bn_train_stats(x, mean, invstd, None, None, None, 0.1, 1e-5, None, B, C, HW, 1)
    run_both(K, 'bn_eval_stats', [rm, rv, torch.zeros(C), torch.zeros(C), 1e-5, C], [2, 3], tol=1e-6)
    for slope in (0.2, 1.0):
        run_both(K, 'bn_act_fwd', [x, mean, invstd, gamma, beta, slope, torch.zeros(B, C, HW), B, C, HW], [6], tol=1e-5)
        gz = rnd(B, C, HW, seed=5)
        for training in (1, 0):
            run_both(K, 'bn_act_bwd', [gz, x, mean, invstd, gamma, beta, slope, training, torch.zeros(B, C, HW),
                                       torch.zeros(C), torch.zeros(C), ws, B, C, HW, 0, None], [8, 9, 10], tol=3e-5)
        run_both(K, 'bn_act_bwd', [gz, x, mean, invstd, gamma, beta, slope, 1, None, rnd(C, seed=11), rnd(C, seed=12),
                                   ws, B, C, HW, 1, None], [9, 10], tol=3e-5)
        run_both(K, 'bn_act_bwd', [gz, x, mean, invstd, gamma, beta, slope, 1, torch.zeros(B, C, HW), torch.zeros(C), torch.zeros(C),
                                   ws, B, C, HW, 0, rnd(B, C, HW, seed=14)], [8, 9, 10], tol=3e-5)       # gx = ... + gx_add
        v = rnd(B, C, HW, seed=6)
        for vg, vb in ((rnd(C, seed=7), rnd(C, seed=8)), (None, None)):
            run_both(K, 'bn_act_dbwd', [v, vg, vb, gz, x, mean, invstd, gamma, beta, slope, torch.zeros(B, C, HW),
                                        torch.zeros(B, C, HW), torch.zeros(C), ws, B, C, HW, 0], [10, 11, 12], tol=5e-5)
        run_both(K, 'bn_act_dbwd', [v, None, None, gz, x, mean, invstd, gamma, beta, slope, torch.zeros(B, C, HW),
                                    torch.zeros(B, C, HW), rnd(C, seed=13), ws, B, C, HW, 1], [10, 11, 12], tol=5e-5)    # adj_gamma +=


# grouped BatchNorm (the discriminator's real and fake batch as one tensor): every code path -- one workgroup per channel
# (<= 16384 elements per group and channel), the two-launch big-plane path, the generic three-launch path (small planes,
# many images; odd sizes) -- and the D layers of the benched step (64 + 64 images)
BN_GROUP_SHAPES = [(2, 4, 16, 64 * 64), (2, 8, 128, 16), (2, 3, 3, 32 * 32), (3, 2, 32, 128 * 128), (2, 5, 100, 8 * 8), (2, 7, 12, 12 * 10),
                   (2, 130, 24, 16 * 16), (2, 40, 7, 30 * 30), (2, 64, 16, 64 * 64), (2, 64, 32, 32 * 32), (2, 64, 64, 16 * 16),
                   (2, 64, 128, 8 * 8), (2, 64, 128, 4 * 4), (2, 64, 16, 128 * 128)]


@pytest.mark.parametrize('shape', BN_GROUP_SHAPES)
def test_batchnorm_groups(K, shape):
    G, B, C, HW = shape
    x = rnd(G * B, C, HW) * 1.5 + 0.3
    x[B:] = x[B:] * 0.5 - 1.0                      # the groups' statistics differ
    gamma, beta = 1 + 0.1 * rnd(C), 0.1 * rnd(C, seed=1)
    rm, rv = 0.05 * rnd(C, seed=2), 1 + 0.1 * torch.rand(C)
    ws = workspace(K.bn_workspace(B, G * C, HW))
    nbt = torch.tensor(41, dtype=torch.int64)
    for replicate in (1, 4):
        run_both(K, 'bn_train_fwd_groups', [x, torch.zeros(G * C), torch.zeros(G * C), rm, rv, nbt, gamma, beta, 0.2, 0.1, 1e-5,
                                            torch.zeros(G * B, C, HW), ws, G, B, C, HW, replicate], [1, 2, 3, 4, 5, 11], tol=1e-5)
    mean, invstd = torch.zeros(G * C), torch.zeros(G * C)
    E.bn_train_fwd_groups(x, mean, invstd, None, None, None, gamma, beta, 0.2, 0.1, 1e-5, torch.zeros(G * B, C, HW), None, G, B, C, HW, 1)
    gz = rnd(G * B, C, HW, seed=5)
    for slope in (0.2, 1.0):
        for training in (1, 0):
            run_both(K, 'bn_act_bwd_groups', [gz, x, mean, invstd, gamma, beta, slope, training, torch.zeros(G * B, C, HW),
                                              torch.zeros(C), torch.zeros(C), ws, G, B, C, HW, 0, None, 1], [8, 9, 10], tol=3e-5)
        run_both(K, 'bn_act_bwd_groups', [gz, x, mean, invstd, gamma, beta, slope, 1, None, rnd(C, seed=11), rnd(C, seed=12),
                                          ws, G, B, C, HW, 1, None, 1], [9, 10], tol=3e-5)
        # the R1 second-order gradient of the first group's images only, folded into the pass
        run_both(K, 'bn_act_bwd_groups', [gz, x, mean, invstd, gamma, beta, slope, 1, torch.zeros(G * B, C, HW), torch.zeros(C),
                                          torch.zeros(C), ws, G, B, C, HW, 0, rnd(B, C, HW, seed=14), 1], [8, 9, 10], tol=3e-5)
    with pytest.raises(RuntimeError):
        K.bn_act_bwd_groups(*[a.cuda() if torch.is_tensor(a) else a for a in
                              [gz, x, mean, invstd, gamma, beta, 0.2, 1, torch.zeros(G * B, C, HW), torch.zeros(C), torch.zeros(C), ws,
                               G, B, C, HW, 0, rnd(B, C, HW), G + 1]])


def test_batchnorm_groups_equal_two_separate_calls(K):
    """One grouped call == the real call followed by the fake call (statistics, outputs, running statistics, in that order)."""
    for (B, C, HW) in [(64, 32, 32 * 32), (64, 128, 8 * 8), (40, 24, 16 * 16)]:
        x = (rnd(2 * B, C, HW) * 1.3 + 0.2).cuda()
        gamma, beta = (1 + 0.1 * rnd(C)).cuda(), (0.1 * rnd(C, seed=1)).cuda()
        ws = workspace(K.bn_workspace(B, 2 * C, HW)).cuda()
        rm1, rv1, n1 = torch.zeros(C).cuda(), torch.ones(C).cuda(), torch.tensor(0).cuda()
        rm2, rv2, n2 = torch.zeros(C).cuda(), torch.ones(C).cuda(), torch.tensor(0).cuda()
        m1, i1, z1 = torch.zeros(2 * C).cuda(), torch.zeros(2 * C).cuda(), torch.zeros(2 * B, C, HW).cuda()
        m2, i2, z2 = torch.zeros(2 * C).cuda(), torch.zeros(2 * C).cuda(), torch.zeros(2 * B, C, HW).cuda()
        K.bn_train_fwd_groups(x, m1, i1, rm1, rv1, n1, gamma, beta, 0.2, 0.1, 1e-5, z1, ws, 2, B, C, HW, 1)
        for g in range(2):
            K.bn_train_fwd(x[g * B:(g + 1) * B], m2[g * C:(g + 1) * C], i2[g * C:(g + 1) * C], rm2, rv2, n2, gamma, beta, 0.2, 0.1, 1e-5,
                           z2[g * B:(g + 1) * B], ws, B, C, HW, 1)
        # planes of >= 1024 elements: the same partial sums in the same order -> bit-identical; the one-workgroup-per-channel
        # kernels split a channel's elements over 512 (two groups) instead of 1024 threads: last-bit differences
        exact = HW >= 1024
        for a, b in ((m1, m2), (i1, i2), (z1, z2), (rm1, rm2), (rv1, rv2)):
            assert torch.equal(a, b) if exact else torch.allclose(a, b, rtol=2e-6, atol=1e-7), (B, C, HW)
        assert int(n1) == int(n2) == 2


@pytest.mark.parametrize('shape', [(6, 4, 4), (8, 16, 16), (3, 64, 64), (5, 10, 6), (4, 128, 128), (3, 34, 20), (2, 256, 64), (5000, 16, 16)])
def test_resample(K, shape):
    BC, H, W = shape
    x = rnd(BC, H, W)
    for alpha in (1.0, 0.25):
        run_both(K, 'up2x', [x, torch.zeros(BC, 2 * H, 2 * W), alpha, BC, H, W], [1], tol=1e-6)
        run_both(K, 'pool2', [x, None, torch.zeros(BC, H // 2, W // 2), alpha, BC, H, W], [2], tol=1e-6)
        run_both(K, 'pool2', [x, rnd(BC, H // 2, W // 2, seed=3), torch.zeros(BC, H // 2, W // 2), alpha, BC, H, W], [2], tol=1e-6)
    run_both(K, 'bilinear_half_fwd', [x, torch.zeros(BC, H // 2, W // 2), BC, H, W], [1], tol=1e-5)   # lambda = r - floor(r) carries ulp(r)
    run_both(K, 'bilinear_half_bwd', [rnd(BC, H // 2, W // 2), None, torch.zeros(BC, H, W), BC, H, W], [2], tol=1e-5)
    run_both(K, 'bilinear_half_bwd', [rnd(BC, H // 2, W // 2), rnd(BC, H, W, seed=5), torch.zeros(BC, H, W), BC, H, W], [2], tol=1e-5)
    idx = torch.zeros(BC, H // 2, W // 2, dtype=torch.uint8)
    run_both(K, 'maxpool2_fwd', [x, torch.zeros(BC, H // 2, W // 2), idx, BC, H, W], [1, 2], atol=0.0)
    E.maxpool2_fwd(x, torch.zeros(BC, H // 2, W // 2), idx, BC, H, W)
    run_both(K, 'maxpool2_bwd', [rnd(BC, H // 2, W // 2), idx, torch.zeros(BC, H, W), BC, H, W], [2], atol=0.0)
    run_both(K, 'maxpool2_gather', [x, idx, torch.zeros(BC, H // 2, W // 2), BC, H, W], [2], atol=0.0)


def test_maxpool_ties_pick_first(K):
    x = torch.ones(2, 4, 4)
    idx = torch.zeros(2, 2, 2, dtype=torch.uint8)
    run_both(K, 'maxpool2_fwd', [x, torch.zeros(2, 2, 2), idx, 2, 4, 4], [1, 2], atol=0.0)


GEMM_CASES = [
    # M, N, K, ta, tb, batch
    (64, 2048, 256, 0, 1, 1), (64, 1, 128, 0, 1, 1), (512, 128, 20, 0, 1, 1), (256, 64, 16, 1, 0, 3),
    (16, 256, 64, 0, 1, 3), (4096, 1024, 4, 1, 0, 2), (100, 37, 19, 1, 1, 2), (33, 65, 17, 0, 0, 1),
    (4, 256, 1024, 0, 0, 3), (16, 256, 1024, 0, 0, 2), (3, 70, 300, 0, 0, 2), (9, 130, 513, 0, 0, 1),
    # skinny, B transposed (matrix-core path): aligned, ragged N, M not a multiple of 4
    (16, 1024, 256, 0, 1, 3), (4, 1024, 256, 0, 1, 2), (5, 100, 64, 0, 1, 2), (1, 77, 32, 0, 1, 1), (13, 4096, 96, 0, 1, 1),
]


@pytest.mark.parametrize('case', GEMM_CASES)
def test_gemm(K, case):
    M, N, Kd, ta, tb, batch = case
    A = rnd(batch, Kd, M) if ta else rnd(batch, M, Kd)
    Bm = rnd(batch, N, Kd, seed=1) if tb else rnd(batch, Kd, N, seed=1)
    lda, ldb = A.shape[-1], Bm.shape[-1]
    for bias in (None, rnd(N, seed=2)):
        run_both(K, 'gemm', [A, Bm, torch.zeros(batch, M, N), bias, M, N, Kd, lda, ldb, N, ta, tb, batch,
                             A[0].numel(), Bm[0].numel(), M * N, 0.0], [2], tol=2e-5)
    run_both(K, 'gemm', [A, Bm, rnd(batch, M, N, seed=5), None, M, N, Kd, lda, ldb, N, ta, tb, batch,
                         A[0].numel(), Bm[0].numel(), M * N, 1.0], [2], tol=2e-5)


def test_row_and_channel_ops(K):
    B, C, HW = 5, 12, 48
    x = rnd(B, C, HW)
    ws = workspace(K.bn_workspace(B, C, HW))
    run_both(K, 'channel_sum', [x, torch.zeros(C), ws, B, C, HW, 0], [1], tol=1e-5)
    run_both(K, 'channel_sum', [x, rnd(C, seed=4), ws, B, C, HW, 1], [1], tol=1e-5)
    xb = rnd(3, 16, 64 * 64)
    wsb = workspace(K.bn_workspace(3, 16, 64 * 64))
    run_both(K, 'channel_sum', [xb, torch.zeros(16), wsb, 3, 16, 64 * 64, 0], [1], tol=1e-5)
    run_both(K, 'channel_bcast', [rnd(C), torch.zeros(B, C, HW), B, C, HW], [1], atol=0.0)
    run_both(K, 'channel_bcast', [rnd(16), torch.zeros(3, 16, 64 * 64), 3, 16, 64 * 64], [1], atol=0.0)
    run_both(K, 'row_sum', [x, torch.zeros(B * C), 1.0, B * C, HW], [1], tol=1e-5)
    run_both(K, 'row_sum', [rnd(1, 300), torch.zeros(1), 0.5, 1, 300], [1], tol=1e-5)
    run_both(K, 'row_bcast', [rnd(B * C), torch.zeros(B * C, HW), 0.5, B * C, HW], [1], tol=1e-6)
    run_both(K, 'repeat_rows', [rnd(7, 9), torch.zeros(8 * 7, 9), 1.0, 7, 9, 8], [1], atol=0.0)
    run_both(K, 'sum_reps', [rnd(8 * 7, 9), torch.zeros(7, 9), 0.125, 7, 9, 8], [1], tol=1e-6)
    # two row blocks back to back, each repeated / averaged on its own (the real and the fake half through the IQN head)
    run_both(K, 'repeat_rows_groups', [rnd(2 * 7, 9), torch.zeros(2 * 8 * 7, 9), 1.0, 7, 9, 8, 2], [1], atol=0.0)
    run_both(K, 'sum_reps_groups', [rnd(2 * 8 * 7, 9), torch.zeros(2 * 7, 9), 0.125, 7, 9, 8, 2], [1], tol=1e-6)


def test_elementwise(K):
    for n in (1, 5, 1024, 4099):
        a, b = rnd(n), rnd(n, seed=1)
        run_both(K, 'add', [a, b, torch.zeros(n), n], [2], atol=0.0)
        run_both(K, 'mul', [a, b, torch.zeros(n), n], [2], atol=0.0)
        run_both(K, 'scale', [a, 0.3, torch.zeros(n), n], [2], tol=1e-7)
        s = torch.tensor(1.7)
        run_both(K, 'scale_dev', [s, 0.5, a, torch.zeros(n), n], [3], tol=1e-6)
        run_both(K, 'scale_add_dev', [s, a, b, torch.zeros(n), n], [3], tol=1e-6)
        ws = workspace(K.reduce_workspace(n))
        run_both(K, 'dot', [a, b, 0.5, torch.zeros(()), ws, n, 0], [3], tol=1e-5, atol=1e-5 * n ** 0.5)
        run_both(K, 'dot', [a, b, 0.5, torch.tensor(3.0), ws, n, 1], [3], tol=1e-5, atol=1e-5 * n ** 0.5)
        run_both(K, 'sumsq', [a, 0.25, torch.zeros(()), ws, n], [2], tol=1e-5)
        run_both(K, 'lrelu_bwd', [a, b, 0.2, torch.zeros(n), n], [3], atol=0.0)
        y = torch.tanh(a)
        run_both(K, 'tanh_fwd', [a, torch.zeros(n), n], [1], tol=1e-6)
        run_both(K, 'tanh_bwd', [b, y, torch.zeros(n), n], [2], tol=1e-6)
        run_both(K, 'fill', [torch.ones(n), 2.5, n], [0], atol=0.0)


def test_unaligned_views(K):
    base = rnd(1030).cuda()
    a, b = base[1:1025], base[3:1027]
    out = torch.zeros(1030).cuda()
    K.add(a, b, out[5:1029], 1024)
    assert torch.allclose(out[5:1029].cpu(), (a + b).cpu())


@pytest.mark.parametrize('shape', [(7, 16), (64, 64), (33, 1024), (5, 300)])
def test_softmax(K, shape):
    rows, cols = shape
    s = rnd(rows, cols) * 3
    y = torch.softmax(s, -1)
    run_both(K, 'softmax_fwd', [s, torch.zeros(rows, cols), rows, cols], [1], tol=2e-6)
    gy, v = rnd(rows, cols, seed=1), rnd(rows, cols, seed=2)
    run_both(K, 'softmax_bwd', [gy, y, torch.zeros(rows, cols), rows, cols], [2], tol=1e-5)
    run_both(K, 'softmax_dbwd', [v, gy, y, torch.zeros(rows, cols), rows, cols], [3], tol=1e-5)


@pytest.mark.parametrize('dims', [(3, 4, 16, 1024, 256), (2, 16, 64, 256, 64), (2, 16, 64, 64, 16), (2, 1, 4, 1024, 256),
                                  (1, 4, 16, 4096, 1024), (2, 8, 32, 300, 75), (1, 2, 8, 64, 16),
                                  # batches large enough for the 4-tiles-per-wave variants (aligned and ragged)
                                  (256, 4, 16, 1024, 256), (256, 4, 16, 1000, 250), (128, 8, 32, 2048, 512), (260, 1, 4, 1020, 255)])
def test_fused_attention(K, dims):
    B, D, DV, N, M = dims
    assert K.attn_supported(D, DV)
    theta, phi, g = rnd(B, D, N), rnd(B, D, M, seed=1), rnd(B, DV, M, seed=2)
    o, lse = torch.zeros(B, DV, N), torch.zeros(B, N)
    run_both(K, 'attn_fwd', [theta, phi, g, o, lse, B, D, DV, N, M], [3, 4], tol=6e-6)   # online softmax + v_exp_f32
    E.attn_fwd(theta, phi, g, o, lse, B, D, DV, N, M)
    go = rnd(B, DV, N, seed=3)
    ws = workspace(K.attn_bwd_workspace(B, D, DV, N, M))
    run_both(K, 'attn_bwd', [go, theta, phi, g, o, lse, torch.zeros(B, D, N), torch.zeros(B, D, M), torch.zeros(B, DV, M),
                             ws, B, D, DV, N, M], [6, 7, 8], tol=2e-5)


@pytest.mark.parametrize('dims', [(3, 4, 16, 1024, 256), (256, 4, 16, 1024, 256), (2, 16, 64, 256, 64), (260, 1, 4, 1020, 255)])
def test_fused_attention_wide_score_range(K, dims):
    """The forward kernel keeps a per-query reference score that it raises lazily (only past a slack): keys whose scores
    keep growing along the row force many raises, and a large common negative offset would underflow a reference that is
    not a score of the row."""
    B, D, DV, N, M = dims
    ramp = torch.linspace(0.1, 3.0, M)
    theta, phi, g = rnd(B, D, N) * 4, rnd(B, D, M, seed=1) * 4 * ramp, rnd(B, DV, M, seed=2)
    theta[:, 0, :] = -40.
    phi[:, 0, :] = 8. + 0.01 * ramp                    # every score carries about -320
    o, lse = torch.zeros(B, DV, N), torch.zeros(B, N)
    run_both(K, 'attn_fwd', [theta, phi, g, o, lse, B, D, DV, N, M], [3, 4], tol=2e-4)      # (NaN / inf fail the comparison)


@pytest.mark.parametrize('shape', [(3 * 1024, 256), (2 * 300, 75), (70, 1024), (5, 6)])
def test_attention_second_order_rows(K, shape):
    """The row-wise middle of the differentiated attention backward; every output overwrites an input."""
    rows, cols = shape
    s, gp, u, v = (rnd(rows, cols, seed=i) for i in range(4))
    lse = torch.logsumexp(s, -1)
    run_both(K, 'attn_dbwd_rows', [s, lse, gp, u, v, rows, cols], [0, 2, 3, 4], tol=2e-5)


@pytest.mark.parametrize('dims', [(3, 4, 16, 1024, 256), (2, 8, 32, 300, 75), (2, 16, 64, 70, 17), (65, 4, 16, 1000, 250), (2, 1, 4, 200, 130),
                                  (2, 2, 8, 64, 256)])
def test_attention_second_order_fused(K, dims):
    """Adjoints of (go, theta, phi, g) through the first-order backward, one kernel, against autograd of autograd."""
    B, D, DV, N, M = dims
    assert K.attn_dbwd_supported(D, DV, M)
    assert not K.attn_dbwd_supported(D, DV, 64 * 4 + 1) and not K.attn_dbwd_supported(3, 12, M)
    theta, phi, g, go = rnd(B, D, N), rnd(B, D, M, seed=1), rnd(B, DV, M, seed=2), rnd(B, DV, N, seed=3)
    a, b, c = rnd(B, D, N, seed=4), rnd(B, D, M, seed=5), rnd(B, DV, M, seed=6)
    lse = torch.logsumexp(torch.bmm(theta.transpose(1, 2), phi), -1)
    ws = workspace(K.attn_dbwd_workspace(B, D, DV, N, M))
    run_both(K, 'attn_dbwd', [go, theta, phi, g, lse, a, b, c, torch.zeros(B, DV, N), torch.zeros(B, D, N), torch.zeros(B, D, M),
                              torch.zeros(B, DV, M), ws, B, D, DV, N, M], [8, 9, 10, 11], tol=3e-5)


@pytest.mark.parametrize('dims', [(3, 4, 16, 1024, 256), (2, 8, 32, 300, 75), (1, 4, 16, 2048, 512)])
def test_attention_double_backward_matches_composed(K, dims):
    """Gradient of a gradient-norm penalty through the fused core == the same through the twice-differentiable primitives."""
    from tartangan_amd import functional as TF
    B, D, DV, N, M = dims
    theta, phi, g = (t.cuda().requires_grad_() for t in (rnd(B, D, N), rnd(B, D, M, seed=1), rnd(B, DV, M, seed=2)))

    def run(f):
        for t in (theta, phi, g):
            t.grad = None
        y = f(theta, phi, g)
        grads = torch.autograd.grad(y.tanh().sum(), (theta, phi, g), create_graph=True)
        (sum(q.pow(2).sum() for q in grads) + y.pow(2).sum()).backward()
        return [y.detach()] + [t.grad.clone() for t in (theta, phi, g)]

    for got, want in zip(run(TF.attention_core), run(TF.attention_composed)):
        assert float((got - want).abs().max()) <= 1e-4 * max(float(want.abs().max()), 1e-3)


def test_fused_attention_unsupported_dims(K):
    assert not K.attn_supported(3, 12)
    with pytest.raises(RuntimeError):
        K.attn_fwd(rnd(1, 3, 16).cuda(), rnd(1, 3, 4).cuda(), rnd(1, 12, 4).cuda(), torch.zeros(1, 12, 16).cuda(),
                   torch.zeros(1, 16).cuda(), 1, 3, 12, 16, 4)


@pytest.mark.parametrize('dims', [(16, 16, 3), (32, 16, 3), (5, 7, 2)])
def test_composed_from_rgb_filter(K, dims):
    Cout, C, Cimg = dims
    w1, b1, w3 = rnd(C, Cimg), rnd(C, seed=1), rnd(Cout, C, 3, 3, seed=2)
    run_both(K, 'rgb_compose_fwd', [w1, b1, w3, torch.zeros(Cout, Cimg + 1, 3, 3), Cout, C, Cimg], [3], tol=2e-6)
    gwc = rnd(Cout, Cimg + 1, 3, 3, seed=3)
    for acc in (0, 1):
        run_both(K, 'rgb_compose_bwd', [gwc, w1, b1, w3, rnd(C, Cimg, seed=4), rnd(C, seed=5), rnd(Cout, C, 3, 3, seed=6), Cout, C, Cimg, acc],
                 [4, 5, 6], tol=5e-6)


def test_iqn_and_losses(K):
    Q, B = 8, 24
    taus = torch.rand(Q * B, 1)
    rng = torch.arange(1, 21).float()
    run_both(K, 'iqn_cos_embed', [taus, rng, torch.zeros(Q * B, 20), Q * B, 20], [2], atol=2e-5)
    preds = rnd(Q * B, 1) * 2
    preds[3] = 1.0                       # err == 0 for a target of 1: indicator and Huber branch edge
    preds[5] = 3.0                       # |err| = 2 > k: linear branch
    target = (torch.arange(B) % 2).float().view(B, 1)
    ws = workspace(K.reduce_workspace(Q * B))
    run_both(K, 'iqn_loss', [preds, target, taus, 1.0, torch.zeros(()), torch.zeros(Q * B, 1), ws, Q, B], [4, 5], tol=2e-6)
    # two evaluations back to back: the sum of their losses, each over its own rows / targets / taus
    preds2, taus2 = torch.cat([preds, rnd(Q * B, 1, seed=7) * 2]), torch.cat([taus, torch.rand(Q * B, 1)])
    target2 = torch.cat([target, 1 - target])
    run_both(K, 'iqn_loss_groups', [preds2, target2, taus2, 1.0, torch.zeros(()), torch.zeros(2 * Q * B, 1), ws, Q, B, 2], [4, 5], tol=2e-6)
    logits, t = rnd(48, 1) * 4, (torch.arange(48) % 2).float().view(48, 1)
    run_both(K, 'bce_logits', [logits, t, torch.zeros(()), torch.zeros(48, 1), ws, 48], [2, 3], tol=2e-6)
    # more than one block of partials (the one-block case above is finished by its own kernel)
    logits, t = rnd(5000, 1, seed=3) * 4, (torch.arange(5000) % 2).float().view(5000, 1)
    run_both(K, 'bce_logits', [logits, t, torch.zeros(()), torch.zeros(5000, 1), ws, 5000], [2, 3], tol=2e-6)


def test_adam_and_ema(K):
    n = 5000
    p, g, m, v = rnd(n), rnd(n, seed=1) * 1e-2, torch.zeros(n), torch.zeros(n)
    g[:10] = 0.0
    for step in (1, 2, 7):
        b1, b2 = 0.0, 0.999
        hyper = torch.tensor([4e-4 / (1 - b1 ** step), (1 - b2 ** step) ** 0.5, b1, b2, 1 - b1, 1 - b2])
        run_both(K, 'adam_step', [p, g, m, v, hyper, 1e-8, n], [0, 2, 3], tol=1e-6)
        E.adam_step(p, g, m, v, hyper, 1e-8, n)
    hyper = torch.tensor([1e-3 / (1 - 0.9 ** 3), (1 - 0.999 ** 3) ** 0.5, 0.9, 0.999, 1 - 0.9, 1 - 0.999])
    run_both(K, 'adam_step', [p, g, rnd(n, seed=4) * 1e-2, v, hyper, 1e-8, n], [0, 2, 3], tol=1e-6)
    run_both(K, 'ema', [rnd(n, seed=2), p, 1e-3, n], [0], tol=1e-7)
