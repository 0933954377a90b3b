"""Every kernel family across the 2 GiB, 4 GiB and 2^31-element boundaries (and above 65535 images), against float64.

The inputs are 7-periodic along the leading dimension and built on the device; the reference is the emulator in float64 on
the 7 base images, tiled; reductions over the batch run on integer probe data and must be exact (tests/large_extent.py, shown
to catch wrapped offsets, masked image counts and dropped tails in tests/test_large_extents.py).  Per-image operations keep
the tolerance of their parity test in tests/test_kernels_gpu.py: a large batch lengthens none of their sums.

The knobs TG_CONV_WINO / TG_CONV_DMA are read once per process: the convolution cases run again in child processes with
either kernel switched off (``test_convolutions_with_a_fast_path_switched_off``)."""
import os
import subprocess
import sys

import pytest
import torch

import large_extent as LE
from emulator import Emulator
from large_extent import CASES, Dim, Out, Small, Sparse, Tiled, images

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB = LE.GIB


class Emulator64(Emulator):
    """The emulator where it builds float32 tensors of its own: the same formulas in the dtype of the arguments."""

    @staticmethod
    def _half_matrix(size, dtype):
        """(size // 2, size) interpolation matrix of F.interpolate(scale .5, bilinear, align_corners=True) with ATen's weights:
        the source index scale * o and its fractional part are fp32 values BY DEFINITION of the operation (ATen computes them
        in fp32, and so does the kernel, on purpose); a float64 index would be another operation, off by ulp(127) x |dx|.
        Everything after the weights -- the products and sums over the pixels -- is in `dtype`."""
        out = size // 2
        scale = torch.tensor((size - 1) / (out - 1), dtype=torch.float32)
        r = scale * torch.arange(out, dtype=torch.float32)
        i0 = r.to(torch.int64).clamp(max=size - 1)
        i1 = (i0 + 1).clamp(max=size - 1)
        l1 = r - i0.to(torch.float32)
        l0 = 1 - l1
        m = torch.zeros(out, size, dtype=dtype)
        m[torch.arange(out), i0] += l0.to(dtype)
        m[torch.arange(out), i1] += l1.to(dtype)
        return m

    def bilinear_half_fwd(self, x, y, BC, H, W):
        mh, mw = self._half_matrix(H, x.dtype), self._half_matrix(W, x.dtype)
        y.view(BC, H // 2, W // 2).copy_(mh @ x.view(BC, H, W) @ mw.t())
        return 0

    def bilinear_half_bwd(self, gy, residual, gx, BC, H, W):
        mh, mw = self._half_matrix(H, gy.dtype), self._half_matrix(W, gy.dtype)
        g = mh.t() @ gy.view(BC, H // 2, W // 2) @ mw
        gx.view(BC, H, W).copy_(g if residual is None else residual.view(BC, H, W) + g)
        return 0

    def bilinear_up2x_fwd(self, x, residual, y, BC, H, W):
        import shared_cases as SH
        r = SH.up(x.reshape(1, BC, H, W))[0]
        y.copy_((r if residual is None else residual.reshape(BC, 2 * H, 2 * W) + r).reshape(y.shape))
        return 0

    def bilinear_up2x_bwd(self, gy, residual, gx, BC, H, W):
        import shared_cases as SH
        g = SH.up_transpose(gy.reshape(1, BC, 2 * H, 2 * W))[0]
        gx.copy_((g if residual is None else residual.reshape(BC, H, W) + g).reshape(gx.shape))
        return 0


E = Emulator64()


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    backend._set_backend_for_testing(None)
    return backend.get()


def against(K, name, args, outs, **kw):
    LE.need(LE.device_bytes(LE._device_args(args)))
    return LE.run_against(K, E, name, args, outs, **kw)


def probe(K, name, args, outs, pr, **kw):
    LE.need(LE.device_bytes(LE._device_args(args)))
    return LE.run_probe(K, E, name, args, outs, pr, **kw)


def filt(*shape, seed=0, scale=0.2):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(4000 + seed)) * scale


# =========================================================================================== elementwise, n = 2^31 + 5
N, L = LE.N_EW, LE.EW_BLOCK
NB = CASES['elementwise'].count
n_ = Dim(N, LE.P * L)


def flat(seed, **kw):
    return Tiled(LE.base(L, seed=seed, **kw), NB, N)


def positive(seed):
    return Tiled(LE.base(L, seed=seed).abs() + 0.5, NB, N)


EXACT32 = dict(atol=0.0)           # one correctly rounded fp32 operation per element (or a copy): the fp32 emulator is the truth
ELEMENTWISE = {
    'add': (lambda: [flat(1), flat(2), Out(n_), n_], {2: EXACT32}, torch.float32),
    'add4': (lambda: [flat(1), flat(2), flat(3), None, Out(n_), n_], {4: EXACT32}, torch.float32),
    'mul': (lambda: [flat(1), flat(2), Out(n_), n_], {2: EXACT32}, torch.float32),
    'scale': (lambda: [flat(1), 0.375, Out(n_), n_], {2: dict(tol=1e-7)}, torch.float64),
    'scale_dev': (lambda: [Small(torch.tensor(1.7)), 0.5, flat(1), Out(n_), n_], {3: dict(tol=1e-6)}, torch.float64),
    'scale_add_dev': (lambda: [Small(torch.tensor(1.7)), flat(1), flat(2), Out(n_), n_], {3: dict(tol=1e-6)}, torch.float64),
    'lrelu_bwd': (lambda: [flat(1), flat(2), 0.2, Out(n_), n_], {3: EXACT32}, torch.float32),
    'tanh_fwd': (lambda: [flat(1), Out(n_), n_], {1: dict(tol=1e-6)}, torch.float64),
    'tanh_bwd': (lambda: [flat(1), Tiled(torch.tanh(LE.base(L, seed=2)), NB, N), Out(n_), n_], {2: dict(tol=1e-6)}, torch.float64),
    'elu_fwd': (lambda: [flat(1), 1.0, 1.0, Out(n_), n_], {3: dict(tol=1e-6)}, torch.float64),
    'elu_bwd order 1': (lambda: [flat(2), flat(1), 1.6733, 1.0507, 1, Out(n_), n_], {5: dict(tol=1e-6)}, torch.float64),
    'elu_bwd order 2': (lambda: [flat(2), flat(1), 1.6733, 1.0507, 2, Out(n_), n_], {5: dict(tol=1e-6)}, torch.float64),
    'recip': (lambda: [positive(1), Out(n_), n_], {1: dict(tol=1e-6)}, torch.float64),
    'fill': (lambda: [Out(n_), 2.5, n_], {0: EXACT32}, torch.float32),
    'ema': (lambda: [flat(1), flat(2), 0.01, n_], {0: dict(tol=1e-7)}, torch.float64),
    'adam_step': (lambda: [flat(1), flat(2), flat(3, scale=0.1), positive(4),
                           Small(torch.tensor([1e-3 / 0.1, 0.001 ** 0.5, 0.9, 0.999, 0.1, 0.001])), 1e-8, n_],
                  {0: dict(tol=1e-6), 2: dict(tol=1e-6), 3: dict(tol=1e-6)}, torch.float64),
}


@pytest.mark.parametrize('op', sorted(ELEMENTWISE))
def test_elementwise(K, op):
    CASES['elementwise'].check()
    make, outs, dtype = ELEMENTWISE[op]
    against(K, op.split()[0], make(), outs, dtype=dtype, label=op)


@pytest.mark.parametrize('op', ['dot', 'sumsq'])
def test_scalar_reductions_on_probe_data(K, op):
    case = CASES['dot sumsq']
    case.check()
    pr = case.probes()
    a, b = LE.base(L, seed=5, integer=True, nonzero=True), LE.base(L, seed=6, integer=True, nonzero=True)
    want = torch.zeros((), dtype=torch.float64)
    for p in pr:
        k = min(L, N - p * L)
        ar, br = a[p % LE.P, :k].double(), b[p % LE.P, :k].double()
        want += (ar * br).sum() if op == 'dot' else (br * br).sum()
    ws = Out((K.reduce_workspace(N) + 3) // 4)
    if op == 'dot':
        args = [Tiled(a, NB, N), Sparse(b, NB, pr, N), 1.0, Out(1), ws, N, 0]
    else:
        args = [Sparse(b, NB, pr, N), 1.0, Out(1), ws, N]
    LE.need(LE.device_bytes(args))
    LE.run(K, op, args, [LE.Check(3 if op == 'dot' else 2, want, exact=True, tiled=False)], label=op)


# =========================================================================================== row operations
ROWS, ROWS_A, COLS = LE.ROWS_SM, LE.ROWS_ATTN, LE.COLS


def rows(seed, count=ROWS, **kw):
    return Tiled(LE.base(COLS, seed=seed, **kw), count)


def softmax_rows(seed, count=ROWS):
    return Tiled(torch.softmax(LE.base(COLS, seed=seed), -1), count)


r_, ra_ = images(ROWS), images(ROWS_A)
RC = 1 << 18                       # repeat_rows / sum_reps: 8200 repetitions of 256 x 1024
reps_ = images(CASES['repeat sum_reps'].count)
ROW_OPS = {
    'row_sum': (lambda: [rows(1, integer=True), Out(r_), 0.5, r_, COLS], {1: EXACT32}, torch.float32, 'rows 2^21+3 x 1024'),
    'row_bcast': (lambda: [Tiled(LE.base(1, seed=2), ROWS), Out(r_, COLS), 0.5, r_, COLS], {1: dict(tol=1e-6)}, torch.float64, 'rows 2^21+3 x 1024'),
    'softmax_fwd': (lambda: [rows(1), Out(r_, COLS), r_, COLS], {1: dict(tol=2e-6)}, torch.float64, 'rows 2^21+3 x 1024'),
    'softmax_bwd': (lambda: [rows(1), softmax_rows(2), Out(r_, COLS), r_, COLS], {2: dict(tol=1e-5)}, torch.float64, 'rows 2^21+3 x 1024'),
    'softmax_dbwd': (lambda: [rows(3), rows(1), softmax_rows(2), Out(r_, COLS), r_, COLS], {3: dict(tol=1e-5)}, torch.float64, 'rows 2^21+3 x 1024'),
    'attn_dbwd_rows': (lambda: [rows(1, ROWS_A), Tiled(torch.logsumexp(LE.base(COLS, seed=1), -1, keepdim=True), ROWS_A), rows(2, ROWS_A),
                                rows(3, ROWS_A), rows(4, ROWS_A), ra_, COLS],
                       {0: dict(tol=2e-5), 2: dict(tol=2e-5), 3: dict(tol=2e-5), 4: dict(tol=2e-5)}, torch.float64, 'rows 2^20+3 x 1024'),
    'channel_bcast': (lambda: [Small(torch.arange(8.0) - 3.5), Out(images(LE.B_31E), 8, 4096), images(LE.B_31E), 8, 4096],
                      {1: EXACT32}, torch.float32, 'channel_bcast'),
}


@pytest.mark.parametrize('op', sorted(ROW_OPS))
def test_row_operations(K, op):
    make, outs, dtype, case = ROW_OPS[op]
    CASES[case].check()
    against(K, op, make(), outs, dtype=dtype, label=op)


def test_repeat_rows_and_sum_reps(K):
    """out (reps, rows, cols) = alpha x, and its transpose; 8200 repetitions of 2^18 elements.  Integer data: 8200 terms of
    magnitude <= 2 stay far below 2^24, so the sum over the repetitions is exact whatever its order."""
    case = CASES['repeat sum_reps']
    case.check()
    reps = case.count
    LE.check_exact(reps, 2)
    x = LE.base(256, COLS, seed=1, integer=True, period=1)
    LE.need(LE.device_bytes([Tiled(x, reps)]))
    LE.run(K, 'repeat_rows', [Small(x[0]), Out(reps, 256, COLS), 0.5, 256, COLS, reps], [LE.Check(1, 0.5 * x[0].double(), atol=0.0)])
    out = LE.fresh(2, reps // 2, 256, COLS, device='cuda')        # two groups: x and -x, each repeated 4100 times
    K.repeat_rows_groups(torch.stack([x[0], -x[0]]).cuda(), out, 1.0, 256, COLS, reps // 2, 2)
    torch.cuda.synchronize()
    LE.check_tiled(out[0], x[0].double(), atol=0.0, label='repeat_rows_groups group 0')
    LE.check_tiled(out[1], -x[0].double(), atol=0.0, label='repeat_rows_groups group 1')
    del out
    xs = LE.base(256, COLS, seed=2, integer=True)
    counts = torch.tensor(LE.probe_counts(range(reps)), dtype=torch.float64)
    want = 0.5 * (xs.double() * counts.view(-1, 1, 1)).sum(0)
    LE.run(K, 'sum_reps', [Tiled(xs, reps), Out(256, COLS), 0.5, 256, COLS, reps], [LE.Check(1, want, exact=True, tiled=False)])
    half = reps // 2                                             # two groups of 4100 repetitions: group g sums images [g * 4100, (g + 1) * 4100)
    wants = []
    for g in range(2):
        c = torch.tensor(LE.probe_counts(range(g * half, (g + 1) * half)), dtype=torch.float64)
        wants.append((xs.double() * c.view(-1, 1, 1)).sum(0))
    LE.run(K, 'sum_reps_groups', [Tiled(xs, reps), Out(2, 256, COLS), 1.0, 256, COLS, half, 2],
           [LE.Check(1, torch.stack(wants), exact=True, tiled=False)])


def test_channel_sum_on_probe_data(K):
    case = CASES['channel_sum']
    case.check()
    pr, B = case.probes(), case.count
    x = LE.base(8, 4096, seed=3, integer=True, nonzero=True)
    ws = Out((K.bn_workspace(B, 8, 4096) + 3) // 4)
    n = images(B)
    probe(K, 'channel_sum', [Sparse(x, B, pr), Out(8), ws, n, 8, 4096, 0], [1], pr)
    probe(K, 'channel_sum', [Sparse(x, B, pr), Small(torch.arange(8.0)), ws, n, 8, 4096, 1], [1], pr, label='channel_sum accumulate')


@pytest.mark.parametrize('ta', [0, 1])
def test_batched_gemm_past_2_31_elements_of_c(K, ta):
    """The composed attention path's maps: s = theta^T phi (transA) and its plain counterpart, C = 2052 x 1024 x 1024."""
    case = CASES['gemm batched']
    case.check()
    batch, M, Nn, Kd = case.count, 1024, 1024, 4
    A = LE.base(Kd, M, seed=1) if ta else LE.base(M, Kd, seed=1)
    Bm = LE.base(Kd, Nn, seed=2)
    n = images(batch)
    lda = M if ta else Kd
    against(K, 'gemm', [Tiled(A, batch), Tiled(Bm, batch), Out(n, M, Nn), None, M, Nn, Kd, lda, Nn, Nn, ta, 0, n, M * Kd, Kd * Nn, M * Nn, 0.0],
            {2: dict(tol=2e-5)}, label=f'gemm transA={ta}')


# =========================================================================================== resampling
BC = LE.BC_RS
bc_ = images(BC)


def planes(h, w, seed, **kw):
    return Tiled(LE.base(h, w, seed=seed, **kw), BC)


def _up2x_limits():
    import shared_cases as SH
    x, gy = LE.base(64, 64, seed=1), LE.base(128, 128, seed=2)
    ry, rx = LE.base(128, 128, seed=3), LE.base(64, 64, seed=4)
    f = lambda d: (ry.to(d) + SH.up(x.to(d)[None])[0]).double()
    b = lambda d: (rx.to(d) + SH.up_transpose(gy[None], d)[0]).double()
    return SH.limit(SH._rel(f(torch.float32), f(torch.float64))), SH.limit(SH._rel(b(torch.float32), b(torch.float64)))


def _maxpool_idx():
    idx = torch.zeros(LE.P, 64, 64, dtype=torch.uint8)
    Emulator().maxpool2_fwd(LE.base(128, 128, seed=1), torch.zeros(LE.P, 64, 64), idx, LE.P, 128, 128)
    return Tiled(idx, BC)


RESAMPLE = {
    'up2x': (lambda: [planes(64, 64, 1), Out(bc_, 128, 128), 0.25, bc_, 64, 64], {1: dict(tol=1e-6)}),
    'pool2': (lambda: [planes(128, 128, 1), planes(64, 64, 2), Out(bc_, 64, 64), 0.25, bc_, 128, 128], {2: dict(tol=1e-6)}),
    'bilinear_half_fwd': (lambda: [planes(128, 128, 1), Out(bc_, 64, 64), bc_, 128, 128], {1: dict(tol=1e-5)}),
    'bilinear_half_bwd': (lambda: [planes(64, 64, 1), planes(128, 128, 2), Out(bc_, 128, 128), bc_, 128, 128], {2: dict(tol=1e-5)}),
    'bilinear_up2x_fwd': (lambda: [planes(64, 64, 1), planes(128, 128, 3), Out(bc_, 128, 128), bc_, 64, 64], {2: dict(tol=_up2x_limits()[0])}),
    'bilinear_up2x_bwd': (lambda: [planes(128, 128, 2), planes(64, 64, 4), Out(bc_, 64, 64), bc_, 64, 64], {2: dict(tol=_up2x_limits()[1])}),
    'maxpool2_fwd': (lambda: [planes(128, 128, 1), Out(bc_, 64, 64), Out(bc_, 64, 64, dtype=torch.uint8), bc_, 128, 128], {1: EXACT32, 2: EXACT32}),
    'maxpool2_bwd': (lambda: [planes(64, 64, 2), _maxpool_idx(), Out(bc_, 128, 128), bc_, 128, 128], {2: EXACT32}),
    'maxpool2_gather': (lambda: [planes(128, 128, 3), _maxpool_idx(), Out(bc_, 64, 64), bc_, 128, 128], {2: EXACT32}),
}


@pytest.mark.parametrize('op', sorted(RESAMPLE))
def test_resampling(K, op):
    CASES['resample'].check()
    make, outs = RESAMPLE[op]
    exact = any(o is EXACT32 for o in outs.values())
    against(K, op, make(), outs, dtype=torch.float32 if exact else torch.float64, label=op)


@pytest.mark.parametrize('cs,cd', [(7, 8), (8, 7)])
def test_copy_channels(K, cs, cd):
    case = CASES['copy_channels']
    case.check()
    n = images(case.count)
    against(K, 'copy_channels', [Tiled(LE.base(cs, 4096, seed=1), case.count), Out(n, cd, 4096), n, cs, cd, 4096, 1.5], {1: EXACT32},
            dtype=torch.float32, label=f'copy_channels {cs}->{cd}')


# =========================================================================================== 3x3 convolutions
def conv3x3_cases(K, which):
    """fwd (bias, bias + residual) and dgrad, 8 -> 8 at 64 x 64, for one of the batches B-, B+, B31e."""
    case = CASES[f'conv3x3 {which}']
    case.check()
    B, n = case.count, images(case.count)
    x, w, b = LE.base(8, 64, 64, seed=1), filt(8, 8, 3, 3), filt(8, seed=1, scale=1.0)
    against(K, 'conv2d_fwd', [Tiled(x, B), Small(w), Small(b), None, Out(n, 8, 64, 64), n, 8, 8, 64, 64, 3], {4: dict(tol=2e-5)},
            label=f'conv2d_fwd bias {which}')
    against(K, 'conv2d_fwd', [Tiled(x, B), Small(w), Small(b), Tiled(LE.base(8, 64, 64, seed=7), B), Out(n, 8, 64, 64), n, 8, 8, 64, 64, 3],
            {4: dict(tol=2e-5)}, label=f'conv2d_fwd bias+residual {which}')
    against(K, 'conv2d_dgrad', [Tiled(LE.base(8, 64, 64, seed=3), B), Small(w), Out(n, 8, 64, 64), n, 8, 8, 64, 64, 3], {2: dict(tol=2e-5)},
            label=f'conv2d_dgrad {which}')


@pytest.mark.parametrize('which', ['B-', 'B+', 'B31e'])
def test_conv3x3(K, which):
    conv3x3_cases(K, which)


def test_conv3x3_wide_output_behind_a_fast_path_input(K):
    """8 -> 24: the input stays under 2 GiB (fast path) while the output passes 2^32 bytes; and the mirror case for dgrad."""
    case = CASES['conv3x3 8->24 B-']
    case.check()
    B, n = case.count, images(case.count)
    w = filt(24, 8, 3, 3)
    against(K, 'conv2d_fwd', [Tiled(LE.base(8, 64, 64, seed=1), B), Small(w), Small(filt(24, seed=1)), None, Out(n, 24, 64, 64), n, 8, 24, 64, 64, 3],
            {4: dict(tol=2e-5)}, label='conv2d_fwd 8->24 B-')
    wd = filt(8, 24, 3, 3, seed=2)                             # forward 24 -> 8: its gradient takes gy of 8 channels to gx of 24
    against(K, 'conv2d_dgrad', [Tiled(LE.base(8, 64, 64, seed=3), B), Small(wd), Out(n, 24, 64, 64), n, 24, 8, 64, 64, 3], {2: dict(tol=2e-5)},
            label='conv2d_dgrad gy 8 -> gx 24 B-')


def test_conv3x3_with_half_resolution_residual(K):
    case = CASES['conv3x3 up2res B+']
    case.check()
    B, n = case.count, images(case.count)
    against(K, 'conv2d_fwd_up2res', [Tiled(LE.base(8, 64, 64, seed=1), B), Small(filt(8, 8, 3, 3)), Small(filt(8, seed=1)),
                                     Tiled(LE.base(8, 32, 32, seed=7), B), Out(n, 8, 64, 64), n, 8, 8, 64, 64], {4: dict(tol=2e-5)})


def _wgrad_both_forms(K, name, partials, reduce, x, gy, shape, dims, row_tail, bias_last, pr, label):
    """One weight gradient on probe data, four ways: overwrite, accumulate, and the two-step form (stage-1 partials, then the
    batched reduction) for both -- which must leave the same BITS as the one-call form."""
    Cout, Cin = shape
    E_ = Emulator()
    ws_bytes = getattr(K, name + '_workspace')(*dims)
    dev_x, dev_gy = LE._materialise(x, 'cuda'), LE._materialise(gy, 'cuda')
    ws = LE.fresh((ws_bytes + 3) // 4, device='cuda')
    ks = 3
    g0, b0 = torch.full((Cout, Cin, ks, ks), 3.0), torch.arange(float(Cout))
    got = {}
    for acc in (0, 1):
        gw = g0.clone().cuda() if acc else LE.fresh(Cout, Cin, ks, ks, device='cuda')
        gb = b0.clone().cuda() if acc else LE.fresh(Cout, device='cuda')
        if bias_last:
            getattr(K, name)(dev_x, dev_gy, gw, ws, ws.numel() * 4, *dims, acc, gb)
        else:
            getattr(K, name)(dev_x, dev_gy, gw, gb, ws, ws.numel() * 4, *dims, acc)
        torch.cuda.synchronize()
        got[acc] = (gw, gb)
        gw2 = g0.clone().cuda() if acc else LE.fresh(Cout, Cin, ks, ks, device='cuda')
        gb2 = b0.clone().cuda() if acc else LE.fresh(Cout, device='cuda')
        ws.fill_(float('nan'))
        getattr(K, partials)(dev_x, dev_gy, ws, ws.numel() * 4, *dims, 1)
        items = torch.tensor([[ws.data_ptr(), gw2.data_ptr(), gb2.data_ptr(), *dims[:5], row_tail[0] if row_tail else dims[5], acc]], dtype=torch.int64)
        getattr(K, reduce)(items, 1)
        torch.cuda.synchronize()
        assert torch.equal(gw, gw2) and torch.equal(gb, gb2), f'{label}: two-step form differs from the one-call form (accumulate={acc})'
    del dev_x, dev_gy, ws
    torch.cuda.empty_cache()
    return got, g0, b0


@pytest.mark.parametrize('which', ['B+', 'B31e'])
def test_conv3x3_wgrad_on_probe_data(K, which):
    case = CASES[f'conv3x3 wgrad {which}']
    case.check()
    B, pr = case.count, case.probes()
    xb, gb_ = LE.base(8, 64, 64, seed=1, integer=True), LE.base(8, 64, 64, seed=2, integer=True, nonzero=True)
    x, gy = Tiled(xb, B), Sparse(gb_, B, pr)
    LE.need(LE.device_bytes([x, gy]))
    dims = (B, 8, 8, 64, 64, 3)
    got, g0, b0 = _wgrad_both_forms(K, 'conv2d_wgrad', 'conv2d_wgrad_partials', 'conv2d_wgrad_reduce_batch', x, gy, (8, 8), dims, (), False, pr,
                                    f'conv2d_wgrad {which}')
    n = images(B)
    want = LE.probe_want(Emulator(), 'conv2d_wgrad', [x, gy, Out(8, 8, 3, 3), Out(8), None, 0, n, 8, 8, 64, 64, 3, 0], [2, 3], pr)
    for acc in (0, 1):
        LE.check_equal(got[acc][0], want[2] + (g0.double() if acc else 0), f'conv2d_wgrad {which} gw accumulate={acc}')
        LE.check_equal(got[acc][1], want[3] + (b0.double() if acc else 0), f'conv2d_wgrad {which} gbias accumulate={acc}')


# =========================================================================================== 1x1 convolutions
def conv1x1_cases(K):
    case = CASES['conv1x1 direct 8->4']
    case.check()
    B, n = case.count, images(case.count)
    against(K, 'conv2d_fwd', [Tiled(LE.base(8, 64, 64, seed=1), B), Small(filt(4, 8, 1, 1)), Small(filt(4, seed=1)), None, Out(n, 4, 64, 64),
                              n, 8, 4, 64, 64, 1], {4: dict(tol=2e-5)}, label='conv1x1 direct 8->4 B=65535')
    case = CASES['conv1x1 streaming 8->8']
    case.check()
    B, n = case.count, images(case.count)
    against(K, 'conv2d_fwd', [Tiled(LE.base(8, 64, 64, seed=1), B), Small(filt(8, 8, 1, 1)), Small(filt(8, seed=1)), None, Out(n, 8, 64, 64),
                              n, 8, 8, 64, 64, 1], {4: dict(tol=2e-5)}, label='conv1x1 streaming 8->8 B31e')
    against(K, 'conv2d_dgrad', [Tiled(LE.base(8, 64, 64, seed=3), B), Small(filt(8, 8, 1, 1)), Out(n, 8, 64, 64), n, 8, 8, 64, 64, 1],
            {2: dict(tol=2e-5)}, label='conv1x1 dgrad 8->8 B31e')
    case = CASES['conv1x1 tiled 63x63']
    case.check()
    B, n = case.count, images(case.count)
    against(K, 'conv2d_fwd', [Tiled(LE.base(8, 63, 63, seed=1), B), Small(filt(16, 8, 1, 1)), Small(filt(16, seed=1)), None, Out(n, 16, 63, 63),
                              n, 8, 16, 63, 63, 1], {4: dict(tol=2e-5)}, label='conv1x1 tiled 8->16 at 63x63')


def test_conv1x1(K):
    conv1x1_cases(K)


def test_conv1x1_wgrad_on_probe_data(K):
    case = CASES['conv1x1 wgrad B+']
    case.check()
    B, pr, n = case.count, case.probes(), images(case.count)
    x, gy = Tiled(LE.base(8, 64, 64, seed=1, integer=True), B), Sparse(LE.base(8, 64, 64, seed=2, integer=True, nonzero=True), B, pr)
    ws = Out((K.conv2d_wgrad_workspace(B, 8, 8, 64, 64, 1) + 3) // 4)
    wsb = Dim(ws.shape[0] * 4, 0, 0)
    probe(K, 'conv2d_wgrad', [x, gy, Out(8, 8, 1, 1), Out(8), ws, wsb, n, 8, 8, 64, 64, 1, 0], [2, 3], pr, label='conv1x1 wgrad B+')
    probe(K, 'conv2d_wgrad', [x, gy, Small(torch.full((8, 8, 1, 1), 3.0)), Small(torch.arange(8.0)), ws, wsb, n, 8, 8, 64, 64, 1, 1], [2, 3], pr,
          label='conv1x1 wgrad B+ accumulate')


def test_conv1x1_multi(K):
    case = CASES['conv1x1 multi B+']
    case.check()
    B, n = case.count, images(case.count)
    assert K.conv1x1_multi_supported(8, 8, 8, B, 8, 64, 64)
    w = filt(24, 8)
    y = lambda: Out(n, 8, 64, 64)
    against(K, 'conv1x1_multi_fwd', [Tiled(LE.base(8, 64, 64, seed=1), B), Small(w), y(), y(), y(), 8, 8, 8, n, 8, 64, 64],
            {2: dict(tol=2e-5), 3: dict(tol=2e-5), 4: dict(tol=2e-5)})
    g = lambda s: Tiled(LE.base(8, 64, 64, seed=s), B)
    against(K, 'conv1x1_multi_dgrad', [g(2), g(3), g(4), Small(w), y(), 8, 8, 8, n, 8, 64, 64], {4: dict(tol=3e-5)})
    pr = CASES['conv1x1 multi wgrad B+'].probes()
    CASES['conv1x1 multi wgrad B+'].check()
    s = lambda sd: Sparse(LE.base(8, 64, 64, seed=sd, integer=True, nonzero=True), B, pr)
    ws = Out((K.conv1x1_multi_wgrad_workspace(8, 8, 8, B, 8, 64, 64) + 3) // 4)
    probe(K, 'conv1x1_multi_wgrad', [Tiled(LE.base(8, 64, 64, seed=1, integer=True), B), s(2), s(3), s(4), Out(24, 8), ws,
                                     Dim(ws.shape[0] * 4, 0, 0), 8, 8, 8, n, 8, 64, 64, 0], [4], pr)


# =========================================================================================== stride-2 forms
def _s2_weights(Cout, Cin, seed):
    w = filt(Cout, Cin, 3, 3, seed=seed)
    wp, w4t = torch.zeros(4, Cout, Cin, 2, 2), torch.zeros(Cin, Cout, 4, 4)
    w4, wpp = torch.zeros(Cout, Cin, 4, 4), torch.zeros(4, Cin, Cout, 2, 2)
    Emulator().upconv3x3_weights(w, wp, Cout, Cin)
    Emulator().upconv3x3_weights_t(w, w4t, Cout, Cin)
    Emulator().poolconv3x3_weights(w, w4, wpp, Cout, Cin)
    return wp, w4t, w4, wpp


def stride2_cases(K, which):
    """upconv3x3 8 -> 8 and poolconv3x3 8 -> 16, forward and input gradient: low plane 32 x 32, high plane 64 x 64."""
    case = CASES[f'upconv {which}']
    case.check()
    CASES[f'poolconv {which}'].check()
    B, n = case.count, images(case.count)
    wp, w4t, _, _ = _s2_weights(8, 8, 1)
    against(K, 'upconv3x3_fwd', [Tiled(LE.base(8, 32, 32, seed=1), B), Small(wp), Small(filt(8, seed=1)), None, Out(n, 8, 64, 64), n, 8, 8, 32, 32],
            {4: dict(tol=3e-5)}, label=f'upconv3x3_fwd {which}')
    assert K.upconv3x3_dgrad_supported(B, 8, 8, 32, 32)
    against(K, 'upconv3x3_dgrad', [Tiled(LE.base(8, 64, 64, seed=3), B), Small(w4t), Out(n, 8, 32, 32), n, 8, 8, 32, 32], {2: dict(tol=5e-5)},
            label=f'upconv3x3_dgrad {which}')
    _, _, w4, wpp = _s2_weights(16, 8, 2)
    assert K.poolconv3x3_supported(B, 8, 16, 32, 32)
    against(K, 'poolconv3x3_fwd', [Tiled(LE.base(8, 64, 64, seed=5), B), Small(w4), Small(filt(16, seed=1)), None, Out(n, 16, 32, 32), n, 8, 16, 32, 32],
            {4: dict(tol=5e-5)}, label=f'poolconv3x3_fwd {which}')
    against(K, 'poolconv3x3_dgrad', [Tiled(LE.base(16, 32, 32, seed=6), B), Small(wpp), Out(n, 8, 64, 64), n, 8, 16, 32, 32], {2: dict(tol=5e-5)},
            label=f'poolconv3x3_dgrad {which}')


@pytest.mark.parametrize('which', ['B-', 'B+', 'B32'])
def test_stride2(K, which):
    stride2_cases(K, which)


@pytest.mark.parametrize('kind', ['upconv', 'poolconv'])
def test_stride2_wgrad_on_probe_data(K, kind):
    case = CASES[f'{kind} wgrad B+']
    case.check()
    B, pr, n = case.count, case.probes(), images(case.count)
    if kind == 'upconv':                                         # a (B, 8, 32, 32), gy (B, 8, 64, 64): the sparse operand is gy
        first, second, Cin, Cout = Tiled(LE.base(8, 32, 32, seed=1, integer=True), B), Sparse(LE.base(8, 64, 64, seed=2, integer=True, nonzero=True), B, pr), 8, 8
    else:                                                        # x (B, 8, 64, 64), gy (B, 16, 32, 32); the 1/4 of the pooling keeps quarters exact
        first, second, Cin, Cout = Tiled(LE.base(8, 64, 64, seed=1, integer=True), B), Sparse(LE.base(16, 32, 32, seed=2, integer=True, nonzero=True), B, pr), 8, 16
    LE.need(LE.device_bytes([first, second]))
    dims = (B, Cin, Cout, 32, 32)
    got, g0, b0 = _wgrad_both_forms(K, f'{kind}3x3_wgrad', f'{kind}3x3_wgrad_partials', 's2_wgrad_reduce_batch', first, second, (Cout, Cin), dims,
                                    (1 if kind == 'upconv' else 0,), True, pr, f'{kind}3x3_wgrad B+')
    want = LE.probe_want(Emulator(), f'{kind}3x3_wgrad', [first, second, Out(Cout, Cin, 3, 3), None, 0, n, Cin, Cout, 32, 32, 0, Out(Cout)], [2, 11], pr)
    for acc in (0, 1):
        LE.check_equal(got[acc][0], want[2] + (g0.double() if acc else 0), f'{kind}3x3_wgrad B+ gw accumulate={acc}')
        LE.check_equal(got[acc][1], want[11] + (b0.double() if acc else 0), f'{kind}3x3_wgrad B+ gbias accumulate={acc}')


# =========================================================================================== BatchNorm
class WeightedBN:
    """tests/emulator.py's BatchNorm formulas in float64 over the 7 base images, image r counting `counts[r]` times: what the
    statistics and backward sums of the tiled tensor are, exactly (the sums are linear in the images)."""

    def __init__(self, counts, C, HW):
        self.c = torch.tensor(counts, dtype=torch.float64).view(-1, 1, 1)
        self.n = float(sum(counts)) * HW
        self.C = C

    def wsum(self, t):
        return (t * self.c).sum((0, 2))

    def ch(self, t):
        return t.view(1, self.C, 1)

    def stats(self, x, eps):
        mean = self.wsum(x) / self.n
        var = self.wsum((x - self.ch(mean)) ** 2) / self.n
        return mean, 1 / torch.sqrt(var + eps), var

    def parts(self, x, mean, invstd, gamma, beta, slope):
        xhat = (x - self.ch(mean)) * self.ch(invstd)
        y = xhat * self.ch(gamma) + self.ch(beta)
        return xhat, y, torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))

    def bwd(self, gz, x, mean, invstd, gamma, beta, slope, gx_add):
        xhat, y, s = self.parts(x, mean, invstd, gamma, beta, slope)
        gyh = gz * s
        sb, sg = self.wsum(gyh), self.wsum(gyh * xhat)
        gx = self.ch(gamma * invstd) * (gyh - self.ch(sb) / self.n - xhat * self.ch(sg) / self.n) + gx_add
        return gx, sg, sb

    def dbwd(self, v, vg, vb, gz, x, mean, invstd, gamma, beta, slope):
        xhat, y, s = self.parts(x, mean, invstd, gamma, beta, slope)
        n, c, r = self.n, self.ch, invstd
        gyh = gz * s
        S1, S2, S3, S4, S5 = self.wsum(v), self.wsum(v * xhat), self.wsum(gyh), self.wsum(gyh * xhat), self.wsum(v * gyh)
        a_gz = (c(gamma * r) * (v - c(S1) / n - xhat * c(S2) / n) + c(vg) * xhat + c(vb)) * s
        A = S5 - S1 * S3 / n - S2 * S4 / n
        q = -c(gamma * r) * (c(S4 / n) * v + c(S2 / n) * gyh) + c(vg) * gyh
        a_x = c(r) * (q - c(self.wsum(q) / n) - xhat * c(self.wsum(q * xhat) / n)) - c(gamma * A * r * r / n) * xhat
        return a_gz, a_x, r * A


BN_C, BN_HW, BN_EPS, BN_MOM, BN_SLOPE = LE.BN_C, LE.BN_HW, 1e-5, 0.1, 0.2
BN_MEASURED = {}                   # label -> (kernel error, ATen fp32 error), relative to max|want|: printed, and copied into DESIGN.md


def _rel(got, want):
    return float((got.detach().reshape(-1).cpu().double() - want.reshape(-1)).abs().max() / want.abs().max())


def _bn_bound(label, got, want, parity_tol, aten):
    """Statistics and backward sums are the one place where a sum grows with the extent (2^27 terms per channel): the bound
    is the larger of the parity tolerance and 4 x what ATen's own fp32 kernel is off on the same device tensor (4 x: another
    summation order, not another algorithm)."""
    err, e_aten = _rel(got, want), _rel(aten, want)
    BN_MEASURED[label] = (err, e_aten)
    lim = max(parity_tol, 4 * e_aten)
    print(f'LARGE bn {label}: kernel {err:.3e}, ATen fp32 {e_aten:.3e}, limit {lim:.3e}')
    assert err <= lim, f'bn {label}: {err:.3e} > {lim:.3e} (ATen fp32 on the same tensor: {e_aten:.3e})'


def _bn_params():
    g = torch.Generator().manual_seed(77)
    return 1 + 0.3 * torch.randn(BN_C, generator=g), 0.3 * torch.randn(BN_C, generator=g), torch.randn(BN_C, generator=g), 1 + torch.rand(BN_C, generator=g)


def test_batchnorm_forward_at_2_31_elements(K):
    """bn_train_fwd, bn_train_fwd_groups (2 groups) and bn_act_fwd on 8200 x 16 x 128 x 128; statistics and running statistics
    against float64 and against ATen's fp32 native_batch_norm on the same device tensor."""
    case = CASES['bn 2^31']
    case.check()
    B, C, HW = case.count, BN_C, BN_HW
    LE.need(3 * B * C * HW * 4 + 2 * LE.CHUNK * 8)
    xb = LE.base(C, HW, seed=1) * 1.5 + 0.7
    gamma, beta, rm0, rv0 = _bn_params()
    ref = WeightedBN(LE.probe_counts(range(B)), C, HW)
    mean, invstd, var = ref.stats(xb.double(), BN_EPS)
    n = ref.n
    want_rm = (1 - BN_MOM) * rm0.double() + BN_MOM * mean
    want_rv = (1 - BN_MOM) * rv0.double() + BN_MOM * var * (n / (n - 1))
    xhat, y, s = ref.parts(xb.double(), mean, invstd, gamma.double(), beta.double(), BN_SLOPE)
    x = LE.tile(xb, B, 'cuda')
    # ATen's own fp32 kernel on the same tensor (the native kernel, not a library's)
    with torch.backends.cudnn.flags(enabled=False):
        a_rm, a_rv = rm0.clone().cuda(), rv0.clone().cuda()
        a_out, a_mean, a_invstd = torch.native_batch_norm(x.view(B, C, 128, 128), gamma.cuda(), beta.cuda(), a_rm, a_rv, True, BN_MOM, BN_EPS)
        del a_out
    torch.cuda.empty_cache()
    d = lambda t: t.clone().cuda()
    m_, i_, rm, rv, nbt = LE.fresh(C, device='cuda'), LE.fresh(C, device='cuda'), d(rm0), d(rv0), torch.tensor(41).cuda()
    z = LE.fresh(B, C, HW, device='cuda')
    ws = LE.fresh((K.bn_workspace(B, C, HW) + 3) // 4, device='cuda')
    K.bn_train_fwd(x, m_, i_, rm, rv, nbt, d(gamma), d(beta), BN_SLOPE, BN_MOM, BN_EPS, z, ws, B, C, HW, 1)
    torch.cuda.synchronize()
    assert int(nbt) == 42
    _bn_bound('mean', m_, mean, 1e-5, a_mean)
    _bn_bound('invstd', i_, invstd, 1e-5, a_invstd)
    _bn_bound('running_mean', rm, want_rm, 1e-5, a_rm)
    _bn_bound('running_var', rv, want_rv, 1e-5, a_rv)
    LE.check_tiled(z, y * s, tol=1e-5, label='bn_train_fwd z')
    assert LE.max_err(x, xb) == 0.0
    # bn_act_fwd with the float64 statistics rounded to fp32
    z.fill_(float('nan'))
    K.bn_act_fwd(x, mean.float().cuda(), invstd.float().cuda(), d(gamma), d(beta), BN_SLOPE, z, B, C, HW)
    torch.cuda.synchronize()
    LE.check_tiled(z, y * s, tol=1e-5, label='bn_act_fwd z')
    # two groups of 4100 images: statistics per half, running statistics updated once per group, in group order
    half = B // 2
    refs = [WeightedBN(LE.probe_counts(range(g * half, (g + 1) * half)), C, HW) for g in range(2)]
    st = [r.stats(xb.double(), BN_EPS) for r in refs]
    w_rm, w_rv = rm0.double(), rv0.double()
    for r, (m, _, v) in zip(refs, st):
        w_rm = (1 - BN_MOM) * w_rm + BN_MOM * m
        w_rv = (1 - BN_MOM) * w_rv + BN_MOM * v * (r.n / (r.n - 1))
    mg, ig, rm, rv = LE.fresh(2 * C, device='cuda'), LE.fresh(2 * C, device='cuda'), d(rm0), d(rv0)
    ws = LE.fresh((K.bn_workspace(half, 2 * C, HW) + 3) // 4, device='cuda')
    z.fill_(float('nan'))
    K.bn_train_fwd_groups(x, mg, ig, rm, rv, nbt, d(gamma), d(beta), BN_SLOPE, BN_MOM, BN_EPS, z, ws, 2, half, C, HW, 1)
    torch.cuda.synchronize()
    assert int(nbt) == 44
    with torch.backends.cudnn.flags(enabled=False):
        a_rm, a_rv, a_stats = rm0.clone().cuda(), rv0.clone().cuda(), []
        for g in range(2):
            _, am, ai = torch.native_batch_norm(x[g * half:(g + 1) * half].view(half, C, 128, 128), gamma.cuda(), beta.cuda(), a_rm, a_rv, True, BN_MOM, BN_EPS)
            a_stats.append((am, ai))
            del _
    _bn_bound('groups mean', mg, torch.cat([s_[0] for s_ in st]), 1e-5, torch.cat([a[0] for a in a_stats]))
    _bn_bound('groups invstd', ig, torch.cat([s_[1] for s_ in st]), 1e-5, torch.cat([a[1] for a in a_stats]))
    _bn_bound('groups running_mean', rm, w_rm, 1e-5, a_rm)
    _bn_bound('groups running_var', rv, w_rv, 1e-5, a_rv)
    for g in range(2):
        # group g starts at image g * 4100 = residue (g * 4100) % 7 of the period: compare against the rolled reference
        xh, yy, ss = refs[g].parts(xb.double(), st[g][0], st[g][1], gamma.double(), beta.double(), BN_SLOPE)
        LE.check_tiled(z[g * half:(g + 1) * half], torch.roll(yy * ss, -((g * half) % LE.P), 0), tol=1e-5, label=f'bn_train_fwd_groups z group {g}')
    del x, z
    torch.cuda.empty_cache()


def test_batchnorm_backward_at_2_31_elements(K):
    """bn_act_bwd (training, with gx_add): gx against float64, ggamma / gbeta against float64 and ATen's fp32 autograd."""
    case = CASES['bn 2^31']
    B, C, HW = case.count, BN_C, BN_HW
    LE.need(4 * B * C * HW * 4 + 2 * LE.CHUNK * 8)
    xb, gzb, addb = LE.base(C, HW, seed=1) * 1.5 + 0.7, LE.base(C, HW, seed=2), LE.base(C, HW, seed=3)
    gamma, beta, _, _ = _bn_params()
    ref = WeightedBN(LE.probe_counts(range(B)), C, HW)
    mean, invstd, _ = ref.stats(xb.double(), BN_EPS)
    want_gx, want_gg, want_gb = ref.bwd(gzb.double(), xb.double(), mean, invstd, gamma.double(), beta.double(), BN_SLOPE, addb.double())
    x, gz = LE.tile(xb, B, 'cuda'), LE.tile(gzb, B, 'cuda')
    # ATen in fp32 on the same tensors: native_batch_norm_backward o leaky_relu_backward, what autograd runs
    with torch.backends.cudnn.flags(enabled=False):
        xv = x.view(B, C, 128, 128)
        out, sm, si = torch.native_batch_norm(xv, gamma.cuda(), beta.cuda(), None, None, True, BN_MOM, BN_EPS)
        gyh = torch.ops.aten.leaky_relu_backward(gz.view(B, C, 128, 128), out, BN_SLOPE, False)
        del out
        a_gx, a_gg, a_gb = torch.ops.aten.native_batch_norm_backward(gyh, xv, gamma.cuda(), None, None, sm, si, True, BN_EPS, [False, True, True])
        del gyh, a_gx
    torch.cuda.empty_cache()
    add = LE.tile(addb, B, 'cuda')
    gx, gg, gb = LE.fresh(B, C, HW, device='cuda'), LE.fresh(C, device='cuda'), LE.fresh(C, device='cuda')
    ws = LE.fresh((K.bn_workspace(B, C, HW) + 3) // 4, device='cuda')
    K.bn_act_bwd(gz, x, mean.float().cuda(), invstd.float().cuda(), gamma.cuda(), beta.cuda(), BN_SLOPE, 1, gx, gg, gb, ws, B, C, HW, 0, add)
    torch.cuda.synchronize()
    _bn_bound('ggamma', gg, want_gg, 3e-5, a_gg)
    _bn_bound('gbeta', gb, want_gb, 3e-5, a_gb)
    LE.check_tiled(gx, want_gx, tol=3e-5, label='bn_act_bwd gx')
    del x, gz, add, gx
    torch.cuda.empty_cache()


def test_batchnorm_second_backward_at_2_30_elements(K):
    """bn_act_dbwd has five large operands: 4100 x 16 x 128 x 128 each."""
    case = CASES['bn dbwd 2^30']
    case.check()
    B, C, HW = case.count, BN_C, BN_HW
    LE.need(5 * B * C * HW * 4 + 2 * LE.CHUNK * 8)
    xb, gzb, vb_ = LE.base(C, HW, seed=1) * 1.5 + 0.7, LE.base(C, HW, seed=2), LE.base(C, HW, seed=6)
    gamma, beta, vg, vbeta = _bn_params()
    ref = WeightedBN(LE.probe_counts(range(B)), C, HW)
    mean, invstd, _ = ref.stats(xb.double(), BN_EPS)
    w_gz, w_x, w_gamma = ref.dbwd(vb_.double(), vg.double(), vbeta.double(), gzb.double(), xb.double(), mean, invstd, gamma.double(), beta.double(), BN_SLOPE)
    v, gz, x = LE.tile(vb_, B, 'cuda'), LE.tile(gzb, B, 'cuda'), LE.tile(xb, B, 'cuda')
    a_gz, a_x, a_gamma = LE.fresh(B, C, HW, device='cuda'), LE.fresh(B, C, HW, device='cuda'), LE.fresh(C, device='cuda')
    ws = LE.fresh((K.bn_workspace(B, C, HW) + 3) // 4, device='cuda')
    K.bn_act_dbwd(v, vg.cuda(), vbeta.cuda(), gz, x, mean.float().cuda(), invstd.float().cuda(), gamma.cuda(), beta.cuda(), BN_SLOPE,
                  a_gz, a_x, a_gamma, ws, B, C, HW, 0)
    torch.cuda.synchronize()
    LE.check_tiled(a_gz, w_gz, tol=5e-5, label='bn_act_dbwd adj_gz')
    LE.check_tiled(a_x, w_x, tol=5e-5, label='bn_act_dbwd adj_x')
    err = _rel(a_gamma, w_gamma)
    print(f'LARGE bn_act_dbwd adj_gamma: {err:.3e} (limit 5e-05)')
    assert err <= 5e-5
    del v, gz, x, a_gz, a_x
    torch.cuda.empty_cache()


# =========================================================================================== image count
def test_attention_above_65535_images(K):
    """65540 images put the batch past what a grid's second dimension holds: the fused kernels must refuse with nothing
    written, and the layer must take the composed path, whose result is checked against float64."""
    from tartangan_amd import functional as TF
    case = CASES['attention B=65540']
    case.check()
    B, D, DV, Nq, M = case.count, 1, 4, 64, 16
    n = images(B)
    th, ph, g = LE.base(D, Nq, seed=1), LE.base(D, M, seed=2), LE.base(DV, M, seed=3)
    T = lambda t: Tiled(t, B)
    LE.run(K, 'attn_fwd', LE._device_args([T(th), T(ph), T(g), Out(n, DV, Nq), Out(n, Nq), n, D, DV, Nq, M]), [], expect='rejected')
    ws = Out((K.attn_bwd_workspace(B, D, DV, Nq, M) + 3) // 4)
    go, o, lse = LE.base(DV, Nq, seed=4), LE.base(DV, Nq, seed=5), LE.base(Nq, seed=6)
    LE.run(K, 'attn_bwd', LE._device_args([T(go), T(th), T(ph), T(g), T(o), T(lse), Out(n, D, Nq), Out(n, D, M), Out(n, DV, M), ws, n, D, DV, Nq, M]),
           [], expect='rejected')
    assert K.attn_dbwd_supported(D, DV, M)
    ws = Out((K.attn_dbwd_workspace(B, D, DV, Nq, M) + 3) // 4)
    LE.run(K, 'attn_dbwd', LE._device_args([T(go), T(th), T(ph), T(g), T(lse), T(th), T(ph), T(g), Out(n, DV, Nq), Out(n, D, Nq), Out(n, D, M),
                                            Out(n, DV, M), ws, n, D, DV, Nq, M]), [], expect='rejected')
    # the layer: forward, first and second derivative through the composed path
    ref = [t.double().requires_grad_() for t in (th, ph, g)]
    dev = [LE.tile(t, B, 'cuda').requires_grad_() for t in (th, ph, g)]

    def second_order(theta, phi, gg, core, cot, cot2):
        out = core(theta, phi, gg)
        first = torch.autograd.grad(out, (theta, phi, gg), cot, create_graph=True)
        second = torch.autograd.grad(first, (theta, phi, gg), cot2)
        return [out] + list(first) + list(second)

    composed = lambda t, p, q: torch.bmm(q, torch.softmax(torch.bmm(t.transpose(1, 2), p), -1).transpose(1, 2))
    cot2 = [LE.base(D, Nq, seed=7), LE.base(D, M, seed=8), LE.base(DV, M, seed=9)]
    want = second_order(*ref, composed, go.double(), [c.double() for c in cot2])
    got = second_order(*dev, TF.attention_core, LE.tile(go, B, 'cuda'), [LE.tile(c, B, 'cuda') for c in cot2])
    for name, w_, g_, tol in zip(('o', 'dtheta', 'dphi', 'dg', 'ddtheta', 'ddphi', 'ddg'), want, got, (2e-4, 2e-5, 2e-5, 2e-5, 3e-5, 3e-5, 3e-5)):
        LE.check_tiled(g_.detach(), w_.detach(), tol=tol, label=f'attention_core B=65540 {name}')


# =========================================================================================== the fast paths switched off
@pytest.mark.parametrize('knob', ['TG_CONV_WINO', 'TG_CONV_DMA'])
def test_convolutions_with_a_fast_path_switched_off(knob):
    """TG_CONV_WINO=0 hands the 3x3 layers under 2 GiB to the LDS-DMA kernel, TG_CONV_DMA=0 takes that away too (and the DMA
    forms of the stride-2 and weight-gradient kernels): the convolution cases again, in a child process (the knobs are read once)."""
    sel = 'test_conv3x3 or test_conv1x1 or test_stride2'
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-x', '-q', '-s', '-k', sel, '-p', 'no:cacheprovider'],
                       env=dict(os.environ, **{knob: '0'}), cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert ' passed' in r.stdout and ' skipped' not in r.stdout
