"""tg_conv1d_* and the 1-D resampling pair (csrc/conv1d.hip) on the GPU, every call behind guard bands (guarded.run_both: outputs
and workspaces handed over NaN-filled), aligned and one element off, the smallest case with each pointer shifted alone, against
float64 ``F.conv1d`` and its autograd.

Tolerance, per case and output: e32 is the error ``F.conv1d`` / its backward make in float32 on the CPU on the same inputs against
float64 (largest absolute difference over the largest absolute reference value); the kernel may be off by 4 * e32 and never has to
beat 2.4e-7 (text_cases.limit, the rule of shared_cases.limit).  Each case prints its figures (pytest -s).

(This file sorts in front of test_guard_bands_gpu.py on purpose: that file's completeness test wants every entry point with a
pointer parameter to have gone through the guarded harness earlier in the same process.)"""
import pytest
import torch
import torch.nn.functional as F

import guarded
import text_cases as TC
from guarded import run_both, workspace

pytestmark = pytest.mark.gpu
EMU = TC.TextEmulator()
CASES = [(s, ks) for s in TC.CONV_SHAPES for ks in (1, 3)]
SMALLEST = TC.CONV_SHAPES[0]


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(None)
    yield backend.get()
    backend._set_backend_for_testing(prev)


def _placements(shape, ptrs):
    return ['aligned', 'shifted'] + (list(ptrs) if shape == SMALLEST else [])


def _check(tag, dev, want, e32, failures):
    err, lim = TC.rel(dev.cpu(), want), TC.limit(e32)
    print(f'CONV1D {tag}: e32 {e32:.2e} kernel {err:.2e} limit {lim:.2e} share {err / lim:.2f}')
    if err > lim:
        failures.append(f'{tag}: {err:.3e} > {lim:.3e} (e32 {e32:.3e})')


@pytest.mark.parametrize('shape,ks', CASES, ids=[f'{"x".join(map(str, s))}-k{k}' for s, k in CASES])
def test_forward_and_input_gradient(K, shape, ks):
    B, Cin, Cout, L = shape
    assert K.conv1d_supported(B, Cin, Cout, L, ks) == 1
    c = TC.conv_case(B, Cin, Cout, L, ks)
    dims, failures = [B, Cin, Cout, L, ks], []
    for pl in _placements(shape, (0, 1, 2, 3, 4)):
        tag = f'{shape} k{ks} [{pl}]'
        dev = run_both(K, 'conv1d_fwd', [c['x'], c['w'], c['bias'], c['residual'], torch.zeros(B, Cout, L)] + dims, [4],
                       tol=2 * TC.limit(c['e32']['full']), placement=pl, emulator=EMU)
        _check(tag + ' fwd bias residual', dev[4], c['want']['full'], c['e32']['full'], failures)
    for pl in _placements(shape, (0, 1, 4)):
        dev = run_both(K, 'conv1d_fwd', [c['x'], c['w'], None, None, torch.zeros(B, Cout, L)] + dims, [4],
                       tol=2 * TC.limit(c['e32']['plain']), placement=pl, emulator=EMU)
        _check(f'{shape} k{ks} [{pl}] fwd plain', dev[4], c['want']['plain'], c['e32']['plain'], failures)
    for pl in _placements(shape, (0, 1, 2)):
        dev = run_both(K, 'conv1d_dgrad', [c['gy'], c['w'], torch.zeros(B, Cin, L)] + dims, [2], tol=2 * TC.limit(c['e32']['gx']),
                       placement=pl, emulator=EMU)
        _check(f'{shape} k{ks} [{pl}] dgrad', dev[2], c['want']['gx'], c['e32']['gx'], failures)
    assert not failures, failures


@pytest.mark.parametrize('shape,ks', CASES, ids=[f'{"x".join(map(str, s))}-k{k}' for s, k in CASES])
def test_weight_and_bias_gradient(K, shape, ks):
    B, Cin, Cout, L = shape
    c = TC.conv_case(B, Cin, Cout, L, ks)
    nbytes = K.conv1d_wgrad_workspace(B, Cin, Cout, L, ks)
    assert nbytes >= 4 * Cout * (Cin * ks + 1)
    dims, failures = [B, Cin, Cout, L, ks], []
    tol = 2 * max(TC.limit(c['e32'][k]) for k in ('gw', 'gb', 'gw_acc', 'gb_acc'))
    for acc, kw, kb in ((0, 'gw', 'gb'), (1, 'gw_acc', 'gb_acc')):
        for pl in _placements(shape, (0, 1, 2, 3, 4)):
            dev = run_both(K, 'conv1d_wgrad', [c['x'], c['gy'], c['gw0'], c['gb0'], workspace(nbytes), nbytes] + dims + [acc], [2, 3],
                           tol=tol, accum=[2, 3] if acc else [], placement=pl, emulator=EMU)
            _check(f'{shape} k{ks} [{pl}] wgrad acc={acc} gw', dev[2], c['want'][kw], c['e32'][kw], failures)
            _check(f'{shape} k{ks} [{pl}] wgrad acc={acc} gbias', dev[3], c['want'][kb], c['e32'][kb], failures)
    for pl in ('aligned', 'shifted'):
        dev = run_both(K, 'conv1d_wgrad', [c['x'], c['gy'], torch.zeros(Cout, Cin, ks), None, workspace(nbytes), nbytes] + dims + [0], [2],
                       tol=tol, placement=pl, emulator=EMU)
        _check(f'{shape} k{ks} [{pl}] wgrad no gbias', dev[2], c['want']['gw'], c['e32']['gw'], failures)
    assert not failures, failures


@pytest.mark.parametrize('L', [3, 5, 64])
def test_a_sequence_never_sees_its_neighbours_tokens(K, L):
    """x is zero except the LAST token of every sequence: the k=3 output at the FIRST token of every sequence (whose left tap is
    its own zero padding, not the previous sequence's last token) is exactly 0; mirrored for the first token / last output.
    Tiles of 64 columns span 64 / L sequences here."""
    B, Cin, Cout = 9, 6, 10
    w, dims = torch.ones(Cout, Cin, 3), [B, Cin, Cout, L, 3]
    for hot, cold in ((L - 1, 0), (0, L - 1)):
        x = torch.zeros(B, Cin, L)
        x[:, :, hot] = 1 + torch.arange(B * Cin, dtype=torch.float32).view(B, Cin)
        y = run_both(K, 'conv1d_fwd', [x, w, None, None, torch.zeros(B, Cout, L)] + dims, [4], placement=['aligned', 'shifted'], emulator=EMU)[4]
        assert float(y[:, :, cold].abs().max()) == 0.0 and float(y[:, :, hot].abs().min()) > 0
        gy = torch.zeros(B, Cout, L)
        gy[:, :, hot] = 1 + torch.arange(B * Cout, dtype=torch.float32).view(B, Cout)
        gx = run_both(K, 'conv1d_dgrad', [gy, w, torch.zeros(B, Cin, L)] + dims, [2], placement=['aligned', 'shifted'], emulator=EMU)[2]
        assert float(gx[:, :, cold].abs().max()) == 0.0 and float(gx[:, :, hot].abs().min()) > 0


def test_other_kernel_sizes_are_refused_with_nothing_written(K):
    B, Cin, Cout, L, ks = 2, 3, 4, 6, 5
    assert K.conv1d_supported(B, Cin, Cout, L, ks) == 0 and K.conv1d_wgrad_workspace(B, Cin, Cout, L, ks) == 0
    x, w, gy = guarded.rnd(B, Cin, L), guarded.rnd(Cout, Cin, ks), guarded.rnd(B, Cout, L)
    dims = [B, Cin, Cout, L, ks]
    run_both(K, 'conv1d_fwd', [x, w, guarded.rnd(Cout), None, torch.zeros(B, Cout, L)] + dims, [4], expect='rejected', emulator=EMU)
    run_both(K, 'conv1d_dgrad', [gy, w, torch.zeros(B, Cin, L)] + dims, [2], expect='rejected', emulator=EMU)
    run_both(K, 'conv1d_wgrad', [x, gy, guarded.rnd(Cout, Cin, ks), guarded.rnd(Cout), workspace(4096), 4096] + dims + [0], [2, 3],
             expect='rejected', emulator=EMU)


@pytest.mark.parametrize('shape,ks', [((5, 33, 17, 5), 3), ((3, 5, 7, 1), 1)])
def test_an_undersized_workspace_is_refused_with_nothing_written(K, shape, ks):
    B, Cin, Cout, L = shape
    c = TC.conv_case(B, Cin, Cout, L, ks)
    nbytes = K.conv1d_wgrad_workspace(B, Cin, Cout, L, ks) - 4
    run_both(K, 'conv1d_wgrad', [c['x'], c['gy'], c['gw0'], c['gb0'], workspace(nbytes), nbytes, B, Cin, Cout, L, ks, 1], [2, 3],
             expect='rejected', emulator=EMU)


def test_two_runs_are_bit_identical(K):
    B, Cin, Cout, L, ks = 5, 33, 17, 5, 3
    c = TC.conv_case(B, Cin, Cout, L, ks)
    x, w, gy, bias = (c[k].cuda() for k in ('x', 'w', 'gy', 'bias'))
    nbytes = K.conv1d_wgrad_workspace(B, Cin, Cout, L, ks)
    runs = []
    for _ in range(2):
        nan = lambda *s: torch.full(s, float('nan'), device='cuda')
        y, gx, gw, gb, ws = nan(B, Cout, L), nan(B, Cin, L), nan(Cout, Cin, ks), nan(Cout), nan((nbytes + 3) // 4)
        K.conv1d_fwd(x, w, bias, None, y, B, Cin, Cout, L, ks)
        K.conv1d_dgrad(gy, w, gx, B, Cin, Cout, L, ks)
        K.conv1d_wgrad(x, gy, gw, gb, ws, nbytes, B, Cin, Cout, L, ks, 0)
        torch.cuda.synchronize()
        runs.append(torch.cat([t.view(-1) for t in (y, gx, gw, gb)]).cpu().view(torch.int32))
    assert torch.equal(*runs) and not bool(torch.isnan(runs[0].view(torch.float32)).any())


@pytest.mark.parametrize('BC,L', [(1, 1), (15, 6), (256, 64)])
def test_resampling_pair(K, BC, L):
    """up2x1d bit-exactly; pool2_1d by the house rule against float64 (e32: F.avg_pool1d + the add in float32)."""
    x, res = guarded.rnd(BC, L, seed=1), guarded.rnd(BC, L, seed=2)
    pls = ['aligned', 'shifted'] + ([0, 1] if (BC, L) == (1, 1) else [])
    for alpha in (1.0, 0.5, 0.3):
        run_both(K, 'up2x1d', [x, torch.zeros(BC, 2 * L), alpha, BC, L], [1], atol=0.0, placement=pls, emulator=EMU)
    big = guarded.rnd(BC, 2 * L, seed=3)
    for residual in (None, res):
        want = F.avg_pool1d(big.double()[None], 2)[0] + (0 if residual is None else residual.double())
        got32 = F.avg_pool1d(big[None], 2)[0] + (0 if residual is None else residual)
        lim = TC.limit(TC.rel(got32, want))
        alone = ([0, 2] + ([1] if residual is not None else [])) if (BC, L) == (1, 1) else []
        for p in ['aligned', 'shifted'] + alone:
            dev = run_both(K, 'pool2_1d', [big, residual, torch.zeros(BC, L), BC, L], [2], tol=2 * lim, placement=p, emulator=EMU)
            err = TC.rel(dev[2].cpu(), want)
            print(f'POOL1D ({BC}, {L}) residual={residual is not None} [{p}]: kernel {err:.2e} limit {lim:.2e}')
            assert err <= lim


def test_autograd_double_backward_on_the_device(K):
    """The R1-style double backward of tests/test_text.py on the device against float64 torch."""
    import test_text
    test_text.check_r1_double_backward('cuda', torch.float32)


def test_the_entry_points_went_through_the_guarded_harness():
    assert {'conv1d_fwd', 'conv1d_dgrad', 'conv1d_wgrad', 'up2x1d', 'pool2_1d'} <= guarded.SEEN
