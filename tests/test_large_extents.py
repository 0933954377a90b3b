"""The large-extent helper (tests/large_extent.py) shown to catch what it claims, on the CPU: its boundaries are scaled down to
2^12 elements and 300 "images", the emulator stands in for the device -- once unmodified (must pass) and once per defect
(must be flagged, by the periodic path AND by the probe path).  The defective stand-ins are Python stubs over CPU tensors;
nothing here runs a faulty kernel.  The period and 2^24 assertions of the real case table are arithmetic and run here too."""
import pytest
import torch
import torch.nn.functional as F

import large_extent as LE
from emulator import Emulator
from large_extent import Check, Out, Small, Sparse, Tiled

WRAP = 1 << 12
SHIFTS = (1 << 10, 1 << 11, 1 << 12, 1 << 13)
OFFSETS = (1 << 10, 1 << 11, 1 << 12)
B, CIN, COUT, H = 300, 2, 2, 4                     # 300 images of 32 elements: 9600 > 2^13
BLOCK = 64
N = B * BLOCK + 5                                  # a flat extent with a ragged tail, in blocks of 64: 301 of them
NBLK = (N + BLOCK - 1) // BLOCK
REF = Emulator()                                   # the reference side is always the unmodified emulator, in float64


def _wrapped(t):
    return t.reshape(-1)[torch.arange(t.numel()) % WRAP].view(t.shape)


class WrapsIndex(Emulator):
    """Reads every large operand at its flat element index modulo 2^12: a 32-bit offset that wrapped."""

    def add(self, a, b, out, n):
        return super().add(_wrapped(a), _wrapped(b), out, n)

    def dot(self, a, b, alpha, out, ws, n, accumulate):
        return super().dot(_wrapped(a), _wrapped(b), alpha, out, ws, n, accumulate)

    def conv2d_fwd(self, x, w, bias, residual, y, B, Cin, Cout, H, W, ks):
        return super().conv2d_fwd(_wrapped(x), w, bias, residual, y, B, Cin, Cout, H, W, ks)

    def conv2d_wgrad(self, x, gy, gw, gbias, ws, ws_bytes, B, Cin, Cout, H, W, ks, accumulate):
        return super().conv2d_wgrad(_wrapped(x), _wrapped(gy), gw, gbias, ws, ws_bytes, B, Cin, Cout, H, W, ks, accumulate)


class MasksBatch(Emulator):
    """Works on B & 0xFF images: an image count that went through a narrow field."""

    def conv2d_fwd(self, x, w, bias, residual, y, B, Cin, Cout, H, W, ks):
        m = B & 0xFF
        return super().conv2d_fwd(x[:m], w, bias, residual, y[:m], m, Cin, Cout, H, W, ks)

    def conv2d_wgrad(self, x, gy, gw, gbias, ws, ws_bytes, B, Cin, Cout, H, W, ks, accumulate):
        m = B & 0xFF
        return super().conv2d_wgrad(x[:m], gy[:m], gw, gbias, ws, ws_bytes, m, Cin, Cout, H, W, ks, accumulate)


class DropsTail(Emulator):
    """Leaves out the n % 4 elements behind the last whole vector."""

    def add(self, a, b, out, n):
        m = n - n % 4
        return super().add(a[:m], b[:m], out[:m], m)

    def dot(self, a, b, alpha, out, ws, n, accumulate):
        m = n - n % 4
        return super().dot(a[:m], b[:m], alpha, out, ws, m, accumulate)


# ------------------------------------------------------------------ the four scaled-down cases, written as the GPU file writes them
def periodic_elementwise(K):
    LE.check_period(BLOCK, SHIFTS)
    a, b = LE.base(BLOCK, seed=1), LE.base(BLOCK, seed=2)
    want = (a.double() + b.double()).float().double()          # one fp32 rounding: the sum itself is the kernel's only operation
    LE.run(K, 'add', [Tiled(a, NBLK, N), Tiled(b, NBLK, N), Out(N), N], [Check(2, want, atol=0.0)], device='cpu')


def periodic_per_image(K):
    LE.check_period(CIN * H * H, SHIFTS)
    LE.check_period(COUT * H * H, SHIFTS)
    x, w, bias = LE.base(CIN, H, H, seed=3), torch.randn(COUT, CIN, 3, 3, generator=torch.Generator().manual_seed(4)) * 0.2, torch.randn(COUT)
    n = LE.images(B)
    args = [Tiled(x, B), Small(w), Small(bias), None, Out(n, COUT, H, H), n, CIN, COUT, H, H, 3]
    assert torch.equal(LE.reference(REF, 'conv2d_fwd', args)[4], F.conv2d(x.double(), w.double(), bias.double(), padding=1))
    LE.run_against(K, REF, 'conv2d_fwd', args, {4: dict(tol=2e-5)}, device='cpu')


def probe_flat(K):
    case = LE.Case(NBLK, [BLOCK], terms=(BLOCK, 4))
    case.check(SHIFTS, OFFSETS)
    pr = case.probes(OFFSETS)
    assert pr == [0, 15, 16, 31, 32, 63, 64, NBLK - 1]
    a, b = LE.base(BLOCK, seed=5, integer=True), LE.base(BLOCK, seed=6, integer=True, nonzero=True)
    want = torch.zeros((), dtype=torch.float64)
    for p in pr:
        k = min(BLOCK, N - p * BLOCK)
        want += (a[p % LE.P, :k].double() * b[p % LE.P, :k].double()).sum()
    LE.run(K, 'dot', [Tiled(a, NBLK, N), Sparse(b, NBLK, pr, N), 1.0, Out(1), Out(4), N, 0], [Check(3, want, exact=True, tiled=False)], device='cpu')


def probe_per_image(K):
    case = LE.Case(B, [CIN * H * H, COUT * H * H], terms=(H * H, 4))
    case.check(SHIFTS, OFFSETS)
    pr = case.probes(OFFSETS)
    assert pr[0] == 0 and pr[-1] == B - 1 and {31, 32, 63, 64, 127, 128} <= set(pr)
    x, gy = LE.base(CIN, H, H, seed=7, integer=True), LE.base(COUT, H, H, seed=8, integer=True, nonzero=True)
    counts = torch.tensor(LE.probe_counts(pr), dtype=torch.float64)
    per = torch.stack([torch.nn.grad.conv2d_weight(x[r:r + 1].double(), (COUT, CIN, 3, 3), gy[r:r + 1].double(), padding=1) for r in range(LE.P)])
    want_w = (per * counts.view(-1, 1, 1, 1, 1)).sum(0)
    want_b = (gy.double().sum((2, 3)) * counts.view(-1, 1)).sum(0)
    n = LE.images(B)
    args = [Tiled(x, B), Sparse(gy, B, pr), Out(COUT, CIN, 3, 3), Out(COUT), Out(64), 256, n, CIN, COUT, H, H, 3, 0]
    want = LE.probe_want(REF, 'conv2d_wgrad', args, [2, 3], pr)
    assert torch.equal(want[2], want_w) and torch.equal(want[3], want_b)
    LE.run_probe(K, REF, 'conv2d_wgrad', args, [2, 3], pr, device='cpu')
    g0, b0 = torch.full((COUT, CIN, 3, 3), 3.0), torch.full((COUT,), -5.0)         # accumulate: on top of what the outputs held
    args = args[:2] + [Small(g0), Small(b0)] + args[4:-1] + [1]
    want = LE.probe_want(REF, 'conv2d_wgrad', args, [2, 3], pr)
    assert torch.equal(want[2], want_w + 3.0) and torch.equal(want[3], want_b - 5.0)
    LE.run_probe(K, REF, 'conv2d_wgrad', args, [2, 3], pr, device='cpu')


PATHS = {'periodic elementwise': periodic_elementwise, 'periodic per image': periodic_per_image, 'probe flat': probe_flat,
         'probe per image': probe_per_image}


@pytest.mark.parametrize('path', sorted(PATHS))
def test_clean_emulator_passes(path):
    PATHS[path](Emulator())


@pytest.mark.parametrize('defect,path', [
    (WrapsIndex, 'periodic elementwise'), (WrapsIndex, 'periodic per image'), (WrapsIndex, 'probe flat'), (WrapsIndex, 'probe per image'),
    (MasksBatch, 'periodic per image'), (MasksBatch, 'probe per image'),
    (DropsTail, 'periodic elementwise'), (DropsTail, 'probe flat'),
])
def test_each_defect_is_flagged_by_the_periodic_and_by_the_probe_path(defect, path):
    with pytest.raises(AssertionError) as e:
        PATHS[path](defect())
    assert 'max err' in str(e.value), str(e.value)


def test_comparison_reads_every_element_and_sees_non_finite_values():
    want = LE.base(5, seed=9).double()
    got = LE.tile(want.float(), 1003, 'cpu').double()
    for chunk in (1 << 26, 1000, 35):                          # one chunk, ragged chunks, one period per chunk
        assert LE.max_err(got, want.float(), chunk=chunk) == 0.0
        for at in (0, 34, 35, got.numel() - 1):
            bad = got.clone()
            bad.view(-1)[at] += 0.5
            assert LE.max_err(bad, want.float(), chunk=chunk) == 0.5
            bad.view(-1)[at] = float('nan')
            assert LE.max_err(bad, want.float(), chunk=chunk) == float('inf')
    idx = LE.fresh(7, 3, device='cpu', dtype=torch.uint8)       # an integer output nobody wrote differs from any 0..3 index
    assert LE.max_err(idx, torch.zeros(3)) > 3


def test_period_and_exactness_assertions_reject_what_they_should():
    LE.check_period(1 << 15)
    LE.check_period(3 << 15)
    with pytest.raises(AssertionError):
        LE.check_period(1 << 15, period=8)                    # a power-of-two period: every shift is a whole number of periods
    with pytest.raises(AssertionError):
        LE.check_period(1 << 15, shifts=(7 << 15,))
    with pytest.raises(AssertionError):
        LE.check_period(3 << 10, shifts=(3 << 12,))           # whole images of a size that is no power of two
    LE.check_exact(14 * 4096, 4)
    with pytest.raises(AssertionError):
        LE.check_exact(1 << 22, 4)
    assert LE.probes(10, [4], offsets=(16,)) == [0, 3, 4, 9]


@pytest.mark.parametrize('name', sorted(LE.CASES))
def test_real_case_table_period_and_exactness(name):
    case = LE.CASES[name]
    case.check()
    if case.terms is not None:
        pr = case.probes()
        assert len(pr) >= 2 and pr[0] == 0 and pr[-1] == case.count - 1
    total = max(case.count * per for per in case.sizes)
    assert total * 4 >= (1 << 31) - max(case.sizes) * 4 or name.startswith('attention'), f'{name} reaches no boundary'
