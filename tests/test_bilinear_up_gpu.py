"""tg_bilinear_up2x_fwd / tg_bilinear_up2x_bwd (csrc/resample.hip) on the GPU, every call behind guard bands
(guarded.run_both), aligned and one element off, against float64 ``F.interpolate(scale_factor=2, mode='bilinear',
align_corners=True)`` and its autograd.

Tolerance, per case and per direction: let e32 be the error the SAME ATen op makes in float32 on the CPU against the float64
result (largest absolute difference over the largest absolute reference value).  The kernel may be off by at most 4 * e32 and
never has to beat 2.4e-7, four fp32 roundoffs (shared_cases.limit, the rule of scene_cases.limit).  Each case prints e32 and the
kernel's error (pytest -s; the table is in DESIGN.md section 9).

(This file sorts in front of test_guard_bands_gpu.py on purpose: that file's completeness test wants every entry point with a
pointer parameter to have gone through the guarded harness earlier in the same process.)"""
import pytest
import torch

import guarded
import shared_cases as SH
from guarded import run_both

pytestmark = pytest.mark.gpu
EMU = SH.SharedEmulator()

SHAPES = [(1, 1, 1),          # scale 0: every output reads the one input
          (1, 2, 2),          # the six-candidate window (clipped by the four outputs there are)
          (3, 1, 5),
          (3, 2, 3),          # non-square
          (2, 3, 7),          # odd sizes
          (6, 4, 4),          # the base size
          (5, 16, 16),
          (2, 64, 64),        # an output plane of 16384 floats: more than a workgroup's threads; eight slabs
          (1, 2, 130),        # one element off: rows of 260 single-element units, more than a workgroup's threads
          (140000, 2, 3),     # more slabs than the grid has workgroups, both ways: every workgroup stages a second slab
          (1, 1, 516),        # past the forward's 512-column table and the transpose's 256: the direct kernels
          (1, 516, 1)]        # (the transpose alone: 516 rows)
SMALLEST = SHAPES[0]


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(None)
    yield backend.get()
    backend._set_backend_for_testing(prev)


def _args(c, BC, H, W):
    fwd = [c['x'], c['res_y'], torch.zeros(BC, 2 * H, 2 * W), BC, H, W]
    bwd = [c['gy'], c['res_x'], torch.zeros(BC, H, W), BC, H, W]
    return fwd, bwd


def _errors(dev_y, dev_gx, c):
    out = []
    for label, got, want, e32 in (('fwd', dev_y, c['want'][0], c['e32'][0]), ('bwd', dev_gx, c['want'][1], c['e32'][1])):
        got = got.cpu().double().reshape(want.shape)
        out.append((label, float((got - want).abs().max()) / float(want.abs().max()), e32))
    return out


@pytest.mark.parametrize('placement', ['aligned', 'shifted'])
@pytest.mark.parametrize('residual', [False, True], ids=['plain', 'residual'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bilinear_up2x_and_its_transpose(K, shape, residual, placement):
    BC, H, W = shape
    c = SH.up_case(BC, H, W, residual)
    fwd, bwd = _args(c, BC, H, W)
    loosest = max(SH.limit(e) for e in c['e32'])
    dev_y = run_both(K, 'bilinear_up2x_fwd', fwd, [2], tol=loosest, placement=placement, emulator=EMU)[2]
    dev_gx = run_both(K, 'bilinear_up2x_bwd', bwd, [2], tol=loosest, placement=placement, emulator=EMU)[2]
    for label, err, e32 in _errors(dev_y, dev_gx, c):
        print(f'UP2X {shape} {"residual" if residual else "plain"} [{placement}] {label}: e32 {e32:.2e} kernel {err:.2e} limit {SH.limit(e32):.2e}')
        assert err <= SH.limit(e32), f'{shape} {label} [{placement}]: {err:.3e} > {SH.limit(e32):.3e} (e32 {e32:.3e})'


@pytest.mark.parametrize('which', ['fwd', 'bwd'])
def test_smallest_shape_with_each_pointer_shifted_alone(K, which):
    BC, H, W = SMALLEST
    c = SH.up_case(BC, H, W, True)
    fwd, bwd = _args(c, BC, H, W)
    tol = max(SH.limit(e) for e in c['e32'])
    run_both(K, 'bilinear_up2x_' + which, fwd if which == 'fwd' else bwd, [2], tol=tol, placement=[0, 1, 2], emulator=EMU)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_transpose_identity(K, shape):
    """<up(x), g> = <x, up^T(g)>, both sides accumulated in float64 from the kernels' fp32 results; the two sides differ by the
    kernels' own errors, so by at most limit(fwd) |up(x)|max |g|_1 + limit(bwd) |up^T(g)|max |x|_1."""
    BC, H, W = shape
    c = SH.up_case(BC, H, W, False)
    x, g = c['x'].cuda(), c['gy'].cuda()
    y, gx = torch.empty(BC, 2 * H, 2 * W, device='cuda'), torch.empty(BC, H, W, device='cuda')
    K.bilinear_up2x_fwd(x, None, y, BC, H, W)
    K.bilinear_up2x_bwd(g, None, gx, BC, H, W)
    lhs = float((y.double() * g.double()).sum())
    rhs = float((x.double() * gx.double()).sum())
    bound = (SH.limit(c['e32'][0]) * float(c['want'][0].abs().max()) * float(c['gy'].double().abs().sum())
             + SH.limit(c['e32'][1]) * float(c['want'][1].abs().max()) * float(c['x'].double().abs().sum()))
    print(f'UP2X {shape} transpose identity: {lhs:.9g} vs {rhs:.9g}, difference {abs(lhs - rhs):.2e}, bound {bound:.2e}')
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize('shape', [(1, 2, 2), (2, 3, 7), (5, 16, 16), (2, 64, 64), (1, 1, 516)], ids=lambda s: 'x'.join(map(str, s)))
def test_two_runs_of_the_transpose_are_bit_identical(K, shape):
    BC, H, W = shape
    c = SH.up_case(BC, H, W, True)
    g, res = c['gy'].cuda(), c['res_x'].cuda()
    runs = []
    for _ in range(2):
        gx = torch.full((BC, H, W), float('nan'), device='cuda')
        K.bilinear_up2x_bwd(g, res, gx, BC, H, W)
        torch.cuda.synchronize()
        runs.append(gx.cpu().view(torch.int32))
    assert torch.equal(*runs)


@pytest.mark.parametrize('form', ['BC0', 'H0', 'W-1', 'null x', 'null y'])
def test_bad_arguments_are_rejected_with_nothing_written(K, form):
    BC, H, W = 2, 3, 4
    x, y = torch.ones(BC, H, W), torch.zeros(BC, 2 * H, 2 * W)
    dims = dict(BC0=(0, H, W), H0=(BC, 0, W)).get(form, (BC, H, -1) if form == 'W-1' else (BC, H, W))
    fwd = [None if form == 'null x' else x, None, None if form == 'null y' else y, *dims]
    bwd = [None if form == 'null x' else y.clone(), None, None if form == 'null y' else x.clone(), *dims]
    run_both(K, 'bilinear_up2x_fwd', fwd, [2] if fwd[2] is not None else [], expect='rejected', emulator=EMU)
    run_both(K, 'bilinear_up2x_bwd', bwd, [2] if bwd[2] is not None else [], expect='rejected', emulator=EMU)


def test_autograd_function_on_the_device_matches_aten_twice_differentiated(K):
    """functional.bilinear_up2x on the device: forward, gradient and the gradient of a function of the gradient against ATen."""
    from tartangan_amd import functional as TF
    gen = torch.Generator().manual_seed(2)
    x0 = torch.randn(2, 3, 5, 6, generator=gen)

    def chain(fn, x):
        x = x.clone().requires_grad_(True)
        y = fn(x)
        g, = torch.autograd.grad(y.pow(2).sum(), x, create_graph=True)
        gg, = torch.autograd.grad(g.pow(2).sum(), x)
        return y.detach().double().cpu(), g.detach().double().cpu(), gg.double().cpu()
    got = chain(TF.bilinear_up2x, x0.cuda())
    want = chain(SH.up, x0.double())
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


def test_both_entry_points_went_through_the_guarded_harness():
    assert {'bilinear_up2x_fwd', 'bilinear_up2x_bwd'} <= guarded.SEEN
