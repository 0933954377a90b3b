"""tg_info_code_loss (csrc/elementwise.hip) on the GPU, every call behind guard bands (guarded.run_both), aligned and one element
off, against float64 ``F.binary_cross_entropy_with_logits`` + ``F.mse_loss`` and their autograd.

Tolerance, per case and per output (``out[0]``, ``out[1]``, ``dcodes``): let e32 be the error the SAME ATen ops make in float32 on
the CPU against the float64 result (largest absolute difference over the largest absolute reference value).  The kernel may be
off by at most 4 * e32 and never has to beat 2.4e-7, four fp32 roundoffs (info_cases.limit, the rule of shared_cases.limit).  Each
case prints e32, the kernel's error and its share of the limit (pytest -s; the table is in DESIGN.md, f7).

(This file sorts in front of test_guard_bands_gpu.py on purpose: that file's completeness test wants every entry point with a
pointer parameter to have gone through the guarded harness earlier in the same process.)"""
import pytest
import torch

import guarded
import info_cases as IC
from guarded import run_both

pytestmark = pytest.mark.gpu
EMU = IC.InfoEmulator()

SHAPES = [(1, 1, 0, 1),          # smallest, BCE only
          (1, 0, 1, 1),          # smallest, MSE only
          (1, 1, 1, 2),          # both terms at the smallest size
          (3, 3, 0, 7),          # ldz > C + K, BCE only
          (4, 0, 2, 5),          # ldz > C + K, MSE only
          (2, 10, 5, 100),       # the default flags on config '16'
          (64, 10, 5, 256),      # the benched batch
          (300, 40, 24, 64)]     # codes fill every column of z; 19200 elements: every thread of the one workgroup sums several
VARIANTS = [(True, 1.0), (False, 0.5), (True, 0.5)]          # (base present, w)
OUTPUTS = ('out[0]', 'out[1]', 'dcodes')


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(None)
    yield backend.get()
    backend._set_backend_for_testing(prev)


def _args(K, c, B, C, Kc, ldz, w):
    return [c['codes'], c['z'], c['base'], w, torch.zeros(2), torch.zeros(B, C + Kc),
            guarded.workspace(K.reduce_workspace(B * (C + Kc))), B, C, Kc, ldz]


def _errors(dev, c):
    out, dcodes = dev[4].cpu().double(), dev[5].cpu().double()
    got = (out[0:1], out[1:2], dcodes)
    return [(label, float((g - want).abs().max()) / float(want.abs().max()), e32)
            for label, g, want, e32 in zip(OUTPUTS, got, c['want'], c['e32'])]


@pytest.mark.parametrize('placement', ['aligned', 'shifted'])
@pytest.mark.parametrize('variant', VARIANTS, ids=lambda v: f'{"base" if v[0] else "nobase"}-w{v[1]}')
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_code_loss_and_its_gradient(K, shape, variant, placement):
    B, C, Kc, ldz = shape
    with_base, w = variant
    c = IC.code_case(B, C, Kc, ldz, w, with_base)
    loosest = max(IC.limit(e) for e in c['e32'])
    dev = run_both(K, 'info_code_loss', _args(K, c, B, C, Kc, ldz, w), [4, 5], tol=2 * loosest, placement=placement, emulator=EMU)
    failures = []
    for label, err, e32 in _errors(dev, c):
        lim = IC.limit(e32)
        print(f'CODELOSS {shape} {"base" if with_base else "nobase"} w={w} [{placement}] {label}: e32 {e32:.2e} kernel {err:.2e} '
              f'limit {lim:.2e} share {err / lim:.2f}')
        if err > lim:
            failures.append(f'{label}: {err:.3e} > {lim:.3e} (e32 {e32:.3e})')
    assert not failures, (shape, variant, placement, failures)


@pytest.mark.parametrize('shape', SHAPES[:3], ids=lambda s: 'x'.join(map(str, s)))
def test_smallest_shapes_with_each_pointer_shifted_alone(K, shape):
    B, C, Kc, ldz = shape
    c = IC.code_case(B, C, Kc, ldz, 1.0, True)
    tol = 2 * max(IC.limit(e) for e in c['e32'])
    run_both(K, 'info_code_loss', _args(K, c, B, C, Kc, ldz, 1.0), [4, 5], tol=tol, placement=[0, 1, 2, 4, 5, 6], emulator=EMU)


def test_two_runs_are_bit_identical(K):
    B, C, Kc, ldz = SHAPES[-1]
    c = IC.code_case(B, C, Kc, ldz, 0.5, True)
    codes, z, base = c['codes'].cuda(), c['z'].cuda(), c['base'].cuda()
    runs = []
    for _ in range(2):
        out = torch.full((2,), float('nan'), device='cuda')
        dcodes = torch.full((B, C + Kc), float('nan'), device='cuda')
        K.info_code_loss(codes, z, base, 0.5, out, dcodes, None, B, C, Kc, ldz)
        torch.cuda.synchronize()
        runs.append(torch.cat([out, dcodes.view(-1)]).cpu().view(torch.int32))
    assert torch.equal(*runs)


@pytest.mark.parametrize('form', ['B0', 'C-1', 'K-1', 'C+K=0', 'ldz<C+K', 'null codes', 'null z', 'null out', 'null dcodes'])
def test_bad_arguments_are_rejected_with_nothing_written(K, form):
    B, C, Kc, ldz = 2, 3, 2, 6
    codes, z = torch.ones(B, C + Kc), torch.ones(B, ldz)
    dims = {'B0': (0, C, Kc, ldz), 'C-1': (B, -1, Kc + C + 1, ldz), 'K-1': (B, C + Kc + 1, -1, ldz), 'C+K=0': (B, 0, 0, ldz),
            'ldz<C+K': (B, C, Kc, C + Kc - 1)}.get(form, (B, C, Kc, ldz))
    args = [None if form == 'null codes' else codes, None if form == 'null z' else z, torch.ones(()), 1.0,
            None if form == 'null out' else torch.zeros(2), None if form == 'null dcodes' else torch.zeros(B, C + Kc),
            guarded.workspace(K.reduce_workspace(B * (C + Kc))), *dims]
    run_both(K, 'info_code_loss', args, [i for i in (4, 5) if args[i] is not None], expect='rejected', emulator=EMU)


def test_autograd_function_on_the_device_reads_the_fake_half_in_place(K):
    """functional.info_code_loss on rows B.. of a (2B, C + K) buffer (4 bytes off a 16-byte boundary) and a (B, latent) z."""
    from tartangan_amd import functional as TF
    B, C, Kc, ldz, w = 3, 2, 1, 9, 0.5
    c = IC.code_case(B, C, Kc, ldz, w, True)
    both = torch.zeros(2 * B, C + Kc, device='cuda')
    both[B:] = c['codes'].cuda()
    codes = both[B:].requires_grad_(True)
    assert codes.data_ptr() % 16 != 0
    base = c['base'].cuda().requires_grad_(True)
    code, total = TF.info_code_loss(codes, c['z'].cuda(), C, Kc, w, base=base)
    g_codes, g_base = torch.autograd.grad(total * 3, (codes, base))
    want = c['want']
    assert abs(float(code) - float(want[0])) <= 1e-6 * float(want[0]) and abs(float(total.detach()) - float(want[1])) <= 1e-6 * float(want[1])
    assert float((g_codes.double().cpu() - 3 * want[2]).abs().max()) <= 1e-6 * 3 * float(want[2].abs().max())
    assert float(g_base) == 3.0 and not code.requires_grad


def test_the_entry_point_went_through_the_guarded_harness():
    assert 'info_code_loss' in guarded.SEEN
