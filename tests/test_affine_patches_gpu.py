"""tg_scene_patches_fwd / tg_scene_patches_bwd (csrc/scene.hip) on the GPU, every call behind guard bands
(guarded.run_both), against the float64 composition of F.affine_grid + F.grid_sample the reference runs
(scene_cases.SceneEmulator).

Tolerance, per case and per output: let e32 be the error the SAME ATen composition makes in float32 on the CPU against the
float64 result (largest absolute difference over the largest absolute reference value).  The kernel may be off by at most
4 * e32 -- the factor covers another summation order over S*S terms and another sigmoid evaluation -- and never has to beat
2.4e-7, four fp32 roundoffs.  Each case prints e32 and the kernel's error (pytest -s; the table is in DESIGN.md section 9).

(This file sorts in front of test_guard_bands_gpu.py on purpose: that file's completeness test wants every entry point with a
pointer parameter to have gone through the guarded harness earlier in the same process.)"""
import pytest
import torch

import guarded
import scene_cases as SC
from guarded import run_both

pytestmark = pytest.mark.gpu
EMU = SC.SceneEmulator()

SHAPES = [(1, 1, 1, 4),        # a single texel: every corner is at an edge
          (1, 2, 2, 4),
          (2, 3, 3, 16),
          (3, 20, 3, 16),      # the default geometry
          (2, 5, 4, 8),
          (2, 2, 7, 32),       # more pixels than a workgroup has threads
          (2, 3, 16, 64)]      # the largest patch, 4096 pixels: 16 staging rounds
SMALLEST = SHAPES[0]


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(None)
    yield backend.get()
    backend._set_backend_for_testing(prev)


def _args(c, B, P, patch, S):
    fwd = [c['theta'], c['logits'], c['noise'], torch.zeros(B, P, S, S), B, P, patch, S]
    bwd = [c['gout'], c['theta'], c['logits'], c['noise'], torch.zeros(B, P * 6),
           torch.zeros(B, P * patch * patch) if c['logits'] is not None else None, B, P, patch, S]
    return fwd, bwd


def _check(K, shape, placement, masks=True, noise=True, theta='random'):
    B, P, patch, S = shape
    c = SC.kernel_case(B, P, patch, S, masks, noise, theta)
    fwd, bwd = _args(c, B, P, patch, S)
    want_out, want_gt, want_gm = c['want']
    e_out, e_gt, e_gm = c['e32']
    loosest = max(SC.limit(e) for e in c['e32'] if e is not None)
    exact = dict(atol=0.0) if theta == 'off' else {}               # everything off the canvas: exact zeros, not small numbers
    dev = run_both(K, 'scene_patches_fwd', fwd, [3], tol=loosest, placement=placement, emulator=EMU, **exact)
    checks = [('out', dev[3], want_out, e_out)]
    dev = run_both(K, 'scene_patches_bwd', bwd, [4, 5] if masks else [4], tol=loosest, placement=placement, emulator=EMU, **exact)
    checks.append(('gtheta', dev[4], want_gt, e_gt))
    if masks:
        checks.append(('gmask_logits', dev[5], want_gm, e_gm))
    where = f'{shape} masks={masks} noise={noise} theta={theta} [{placement}] seed {c["seed"]}'
    for label, got, want, e32 in checks:
        got = got.cpu().double().reshape(want.shape)
        scale = float(want.abs().max())
        err = float((got - want).abs().max()) / scale if scale > 0 else float(got.abs().max())
        print(f'SCENE {where} {label}: e32 {e32:.2e} kernel {err:.2e} limit {SC.limit(e32):.2e}')
        if theta == 'off':
            assert scale == 0.0 and float(got.abs().max()) == 0.0, f'{where} {label}: not exactly zero'
        else:
            assert err <= SC.limit(e32), f'{where} {label}: {err:.3e} > {SC.limit(e32):.3e} (e32 {e32:.3e})'


@pytest.mark.parametrize('placement', ['aligned', 'shifted'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_scene_patches(K, shape, placement):
    _check(K, shape, placement)


@pytest.mark.parametrize('which', ['fwd', 'bwd'])
def test_smallest_shape_with_each_pointer_shifted_alone(K, which):
    B, P, patch, S = SMALLEST
    c = SC.kernel_case(B, P, patch, S)
    fwd, bwd = _args(c, B, P, patch, S)
    tol = max(SC.limit(e) for e in c['e32'])
    if which == 'fwd':
        run_both(K, 'scene_patches_fwd', fwd, [3], tol=tol, placement=[0, 1, 2, 3], emulator=EMU)
    else:
        run_both(K, 'scene_patches_bwd', bwd, [4, 5], tol=tol, placement=[0, 1, 2, 3, 4, 5], emulator=EMU)


@pytest.mark.parametrize('placement', ['aligned', 'shifted'])
@pytest.mark.parametrize('masks,noise', [(True, False), (False, True), (False, False)])      # (True, True) is in test_scene_patches
def test_null_mask_logits_and_null_noise(K, masks, noise, placement):
    _check(K, (2, 3, 3, 16), placement, masks, noise)


@pytest.mark.parametrize('placement', ['aligned', 'shifted'])
def test_exact_initial_transform(K, placement):
    """theta = [2, 0, 0, 0, 2, 0]: the samples sit at 3 (2j + 1) / 16 - 2, never on an integer."""
    _check(K, (2, 3, 3, 16), placement, theta='init')


@pytest.mark.parametrize('placement', ['aligned', 'shifted'])
def test_patches_off_the_canvas_give_exact_zeros(K, placement):
    _check(K, (2, 3, 3, 16), placement, theta='off')


@pytest.mark.parametrize('form', ['patch0', 'patch17', 'gmask_without_mask', 'mask_without_gmask'])
def test_rejected_forms_write_nothing(K, form):
    B, P, S = 2, 3, 8
    patch = {'patch0': 0, 'patch17': 17}.get(form, 3)
    theta = torch.tensor(SC.INIT_THETA).repeat(B, P)
    T = max(patch * patch, 1)
    logits, noise = torch.zeros(B, P * T), torch.ones(max(patch, 1), max(patch, 1))
    if form in ('patch0', 'patch17'):
        run_both(K, 'scene_patches_fwd', [theta, logits, noise, torch.zeros(B, P, S, S), B, P, patch, S], [3], expect='rejected',
                 emulator=EMU)
    given = None if form == 'gmask_without_mask' else logits
    gmask = None if form == 'mask_without_gmask' else torch.zeros(B, P * T)
    run_both(K, 'scene_patches_bwd', [torch.ones(B, P, S, S), theta, given, noise, torch.zeros(B, P * 6), gmask, B, P, patch, S],
             [4, 5] if gmask is not None else [4], expect='rejected', emulator=EMU)


@pytest.mark.parametrize('shape', [(3, 20, 3, 16), (2, 3, 16, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_two_runs_are_bit_identical(K, shape):
    B, P, patch, S = shape
    c = SC.kernel_case(B, P, patch, S)
    theta, logits, noise, gout = (c[k].cuda() for k in ('theta', 'logits', 'noise', 'gout'))
    runs = []
    for _ in range(2):
        out = torch.full((B, P, S, S), float('nan'), device='cuda')
        gtheta = torch.full((B, P * 6), float('nan'), device='cuda')
        gmask = torch.full((B, P * patch * patch), float('nan'), device='cuda')
        K.scene_patches_fwd(theta, logits, noise, out, B, P, patch, S)
        K.scene_patches_bwd(gout, theta, logits, noise, gtheta, gmask, B, P, patch, S)
        torch.cuda.synchronize()
        runs.append([t.cpu().view(torch.int32) for t in (out, gtheta, gmask)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_both_entry_points_went_through_the_guarded_harness():
    assert {'scene_patches_fwd', 'scene_patches_bwd'} <= guarded.SEEN
