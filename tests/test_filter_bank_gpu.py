"""tg_filter_narrow / tg_filter_narrow_bwd (csrc/rowops.hip) on the GPU, every call behind guard bands (guarded.run_both),
aligned and one element off.  Copies and single adds: everything is compared BIT-exactly.

(This file sorts in front of test_guard_bands_gpu.py on purpose: that file's completeness test wants every entry point with a
pointer parameter to have gone through the guarded harness earlier in the same process.)"""
import pytest
import torch

import guarded
import shared_cases as SH
from guarded import rnd, run_both

pytestmark = pytest.mark.gpu
EMU = SH.SharedEmulator()
POISON = 12345.678          # finite (the harness compares values), never produced by the inputs

# (Omax, Imax, O, I, taps)
SHAPES = [(1, 1, 1, 1, 9),
          (4, 6, 4, 6, 9),          # the full bank
          (4, 6, 1, 6, 9),
          (4, 6, 4, 1, 9),
          (5, 7, 3, 2, 9),
          (64, 100, 32, 64, 9),     # the config-16 bank
          (64, 100, 64, 64, 9),
          (5, 7, 3, 2, 1)]          # taps = 1
SMALLEST = SHAPES[0]


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(None)
    yield backend.get()
    backend._set_backend_for_testing(prev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize('placement', ['aligned', 'shifted'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_narrow_and_its_transpose_are_bit_exact(K, shape, placement):
    Omax, Imax, O, I, taps = shape
    dims = [O, I, Omax, Imax, taps]
    bank, gview = rnd(Omax, Imax, taps), rnd(O, I, taps, seed=1)
    view = run_both(K, 'filter_narrow', [bank, torch.zeros(O, I, taps)] + dims, [1], atol=0.0, placement=placement, emulator=EMU)[1]
    assert torch.equal(_bits(view), _bits(bank[:O, :I].contiguous()))
    # accumulate = 0: the whole bank is written -- the corner, and exact (positive) zeros everywhere else
    gbank = run_both(K, 'filter_narrow_bwd', [gview, torch.zeros(Omax, Imax, taps)] + dims + [0], [1], atol=0.0, placement=placement,
                     emulator=EMU)[1]
    want = torch.zeros(Omax, Imax, taps)
    want[:O, :I] = gview
    assert torch.equal(_bits(gbank), _bits(want))
    # accumulate = 1: corner += gview; poisoned elements outside the corner keep their bits
    start = rnd(Omax, Imax, taps, seed=2)
    outside = torch.ones(Omax, Imax, dtype=torch.bool)
    outside[:O, :I] = False
    start[outside] = POISON
    gbank = run_both(K, 'filter_narrow_bwd', [gview, start] + dims + [1], [1], atol=0.0, accum=[1], placement=placement, emulator=EMU)[1]
    want = start.clone()
    want[:O, :I] += gview
    assert torch.equal(_bits(gbank), _bits(want))
    assert bool((gbank.cpu()[outside] == start[outside]).all())


@pytest.mark.parametrize('which', ['narrow', 'bwd0', 'bwd1'])
def test_smallest_shape_with_each_pointer_shifted_alone(K, which):
    Omax, Imax, O, I, taps = SMALLEST
    dims = [O, I, Omax, Imax, taps]
    if which == 'narrow':
        run_both(K, 'filter_narrow', [rnd(Omax, Imax, taps), torch.zeros(O, I, taps)] + dims, [1], atol=0.0, placement=[0, 1], emulator=EMU)
    else:
        acc = int(which == 'bwd1')
        run_both(K, 'filter_narrow_bwd', [rnd(O, I, taps), rnd(Omax, Imax, taps, seed=2)] + dims + [acc], [1], atol=0.0,
                 accum=[1] if acc else [], placement=[0, 1], emulator=EMU)


@pytest.mark.parametrize('form', ['O > Omax', 'I > Imax', 'O = 0', 'I = 0', 'Omax = 0', 'Imax = -1', 'taps = 0', 'null in', 'null out'])
def test_bad_arguments_are_rejected_with_nothing_written(K, form):
    Omax, Imax, O, I, taps = 4, 6, 3, 2, 9
    bank, view = rnd(Omax, Imax, taps), rnd(O, I, taps, seed=1)
    dims = {'O > Omax': [5, I, Omax, Imax, taps], 'I > Imax': [O, 7, Omax, Imax, taps], 'O = 0': [0, I, Omax, Imax, taps],
            'I = 0': [O, 0, Omax, Imax, taps], 'Omax = 0': [O, I, 0, Imax, taps], 'Imax = -1': [O, I, Omax, -1, taps],
            'taps = 0': [O, I, Omax, Imax, 0]}.get(form, [O, I, Omax, Imax, taps])
    src = None if form == 'null in' else bank
    dst = None if form == 'null out' else view
    run_both(K, 'filter_narrow', [src, dst] + dims, [1] if dst is not None else [], expect='rejected', emulator=EMU)
    src = None if form == 'null in' else view
    dst = None if form == 'null out' else bank
    for acc in (0, 1):
        run_both(K, 'filter_narrow_bwd', [src, dst] + dims + [acc], [1] if dst is not None else [], expect='rejected', emulator=EMU)


def test_sum_over_views_is_the_same_in_every_run(K):
    """Five views of one bank added in a fixed order on one stream, twice: bit-identical, and what float32 adds in that order give."""
    Omax, Imax, taps = 64, 100, 9
    corners = [(64, 64), (32, 64), (32, 32), (64, 64), (16, 8)]
    views = [rnd(O, I, taps, seed=k).cuda() for k, (O, I) in enumerate(corners)]
    runs = []
    for _ in range(2):
        gbank = torch.zeros(Omax, Imax, taps, device='cuda')
        for (O, I), v in zip(corners, views):
            K.filter_narrow_bwd(v, gbank, O, I, Omax, Imax, taps, 1)
        torch.cuda.synchronize()
        runs.append(_bits(gbank))
    assert torch.equal(*runs)
    want = torch.zeros(Omax, Imax, taps)
    for (O, I), v in zip(corners, views):
        want[:O, :I] += v.cpu()
    assert torch.equal(runs[0], _bits(want))
    assert float(want[:, 64:].abs().max()) == 0.0


def test_both_entry_points_went_through_the_guarded_harness():
    assert {'filter_narrow', 'filter_narrow_bwd'} <= guarded.SEEN
