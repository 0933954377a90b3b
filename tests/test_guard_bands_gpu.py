"""Every entry point with a device-pointer parameter through the guard-banded harness (tests/guarded.py), at the aligned
and at the one-element-shifted placement, the smallest case of each also with every pointer argument shifted alone.
Tolerances are those of the entry point's own parity test.  Placements an entry point documents as unsupported must be
rejected with nothing written; every other placement must be accepted and correct."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import guarded
from emulator import Emulator
from guarded import HostTable, Per, rnd, run_both, workspace

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Reference(Emulator):
    """The emulator plus plain-torch forms of the three Inception-v3 forward entry points (packed filter as the header lays it out)."""

    def inception_conv_fwd(self, x, wp, bias, y, B, Cin, Cout, H, W, KH, KW, stride, ph, pw, relu, x_ctot, x_coff, y_ctot, y_coff):
        kk, coutp = Cin * KH * KW, (Cout + 127) // 128 * 128
        w = wp.view(-1, coutp)[:kk, :Cout].t().reshape(Cout, Cin, KH, KW)
        r = F.conv2d(x.view(B, x_ctot, H, W)[:, x_coff:x_coff + Cin], w, bias, stride=stride, padding=(ph, pw))
        y.view(B, y_ctot, r.shape[2], r.shape[3])[:, y_coff:y_coff + Cout].copy_(F.relu(r) if relu else r)

    def inception_maxpool3s2(self, x, y, B, C, H, W, x_ctot, x_coff, y_ctot, y_coff):
        r = F.max_pool2d(x.view(B, x_ctot, H, W)[:, x_coff:x_coff + C], 3, stride=2)
        y.view(B, y_ctot, r.shape[2], r.shape[3])[:, y_coff:y_coff + C].copy_(r)

    def inception_avgpool3(self, x, y, B, C, H, W, x_ctot, x_coff, y_ctot, y_coff):
        y.view(B, y_ctot, H, W)[:, y_coff:y_coff + C].copy_(F.avg_pool2d(x.view(B, x_ctot, H, W)[:, x_coff:x_coff + C], 3, stride=1, padding=1))


R = Reference()


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    backend._set_backend_for_testing(None)
    return backend.get()


# Entry points that document a 16-byte alignment requirement: the pointer arguments whose misalignment must be rejected (pinned here).
REJECTS = {
    'conv1x1_multi_fwd': ('x', 'w', 'y0', 'y1', 'y2'), 'conv1x1_multi_dgrad': ('gy0', 'gy1', 'gy2', 'w', 'gx'),
    'conv1x1_multi_wgrad': ('x', 'gy0', 'gy1', 'gy2', 'gw', 'workspace'),
    'gemm_big': ('A', 'Bm'), 'inception_conv_fwd': ('wp',), 'image_bytes_batch': ('out',),
}


def call(name, args, outs, **kw):
    return dict(name=name, args=args, outs=outs, kw=kw)


# ------------------------------------------------------------------------------------------------ case builders
def conv_calls(K, shape):
    B, Cin, Cout, H, W, ks = shape
    x, w, b, gy = rnd(B, Cin, H, W), rnd(Cout, Cin, ks, ks, scale=0.2), rnd(Cout), rnd(B, Cout, H, W, seed=3)
    dims = [B, Cin, Cout, H, W, ks]
    yield call('conv2d_fwd', [x, w, b, None, torch.zeros(B, Cout, H, W)] + dims, [4], tol=2e-5)
    yield call('conv2d_fwd', [x, w, None, rnd(B, Cout, H, W, seed=7), torch.zeros(B, Cout, H, W)] + dims, [4], tol=2e-5)
    yield call('conv2d_dgrad', [gy, w, torch.zeros(B, Cin, H, W)] + dims, [2], tol=2e-5)
    if ks == 3 and H % 2 == 0 and W % 2 == 0:
        yield call('conv2d_fwd_up2res', [x, w, b, rnd(B, Cout, H // 2, W // 2, seed=7), torch.zeros(B, Cout, H, W)] + dims[:5], [4], tol=2e-5)
    nbytes = K.conv2d_wgrad_workspace(*dims)
    ws = workspace(nbytes)
    for acc in (0, 1):
        yield call('conv2d_wgrad', [x, gy, rnd(Cout, Cin, ks, ks, seed=9), rnd(Cout, seed=10), ws, nbytes] + dims + [acc], [2, 3], tol=5e-5)
    yield call('conv2d_wgrad', [x, gy, torch.zeros(Cout, Cin, ks, ks), None, ws, nbytes] + dims + [0], [2], tol=5e-5)
    yield call('conv2d_wgrad_partials+conv2d_wgrad_reduce_batch', dims, [], tol=5e-5)


def wgrad_two_steps(K, kind, dims, tol, placements):
    """Stage 1 into an exact guarded workspace, then the batched stage 2 over a host table of guarded tensors (with and without bias,
    accumulating and overwriting), against the emulator's finished gradients."""
    if kind == 'conv2d':
        B, Cin, Cout, H, W, ks = dims
        lo, hi, last = rnd(B, Cin, H, W), rnd(B, Cout, H, W, seed=3), ks
        reduce = 'conv2d_wgrad_reduce_batch'
    else:
        B, Cin, Cout, H, W = dims
        ks = 3
        lo, hi = (rnd(B, Cin, 2 * H, 2 * W), rnd(B, Cout, H, W, seed=3)) if kind == 'poolconv3x3' else (rnd(B, Cin, H, W, seed=4), rnd(B, Cout, 2 * H, 2 * W, seed=5))
        last, reduce = (0 if kind == 'poolconv3x3' else 1), 's2_wgrad_reduce_batch'
    nbytes = getattr(K, kind + '_wgrad_workspace')(*dims)
    for pl in placements:
        if not isinstance(pl, str):
            continue                     # (single-pointer shifts: through the one-call forms and the partials below)
        rows, outs, accum = [], [], []
        for r, (want_bias, acc) in enumerate(((1, 1), (0, 0))):
            ws_e = workspace(getattr(R, kind + '_wgrad_workspace')(*dims))
            getattr(R, kind + '_wgrad_partials')(lo, hi, ws_e, ws_e.numel() * 4, *dims, want_bias)
            dev = run_both(K, kind + '_wgrad_partials', [lo, hi, workspace(nbytes), nbytes, *dims, want_bias], [], placement=pl)
            rows.append([Per(ws_e, dev[2].cpu()), rnd(Cout, Cin, ks, ks, seed=9), rnd(Cout, seed=10) if want_bias else None,
                         B, Cin, Cout, H, W, last, acc])
            outs += [(r, 1)] + ([(r, 2)] if want_bias else [])
            accum += ([(r, 1), (r, 2)] if acc else [])
        run_both(K, reduce, [HostTable(rows, outs=outs, accum=accum), len(rows)], [], tol=tol, placement=pl, emulator=R)
    ptrs = [p for p in placements if not isinstance(p, str)]
    if ptrs:
        run_both(K, kind + '_wgrad_partials', [lo, hi, workspace(nbytes), nbytes, *dims, 1], [], placement=[0, 1, 2])
    return {kind + '_wgrad_partials': [str(p) for p in placements if isinstance(p, str)] + (['0', '1', '2'] if ptrs else []),
            reduce: [str(p) for p in placements if isinstance(p, str)]}


# the up-conv shapes whose low-resolution plane gives the one-kernel input gradient enough workgroups (asserted, not assumed)
UPCONV_DGRAD = {(128, 32, 24, 16, 16), (520, 24, 20, 8, 8), (258, 24, 40, 8, 8)}


def upconv_calls(K, shape):
    B, Cin, Cout, H, W = shape
    a, w, b = rnd(B, Cin, H, W), rnd(Cout, Cin, 3, 3, scale=0.2), rnd(Cout)
    wp, w4t = torch.zeros(4, Cout, Cin, 2, 2), torch.zeros(Cin, Cout, 4, 4)
    yield call('upconv3x3_weights', [w, wp, Cout, Cin], [1], tol=1e-6)
    yield call('upconv3x3_weights_t', [w, w4t, Cout, Cin], [1], tol=1e-6)
    yield call('upconv3x3_weights_pair', [w, wp.clone(), w4t.clone(), Cout, Cin], [1, 2], tol=1e-6)
    R.upconv3x3_weights(w, wp, Cout, Cin)
    R.upconv3x3_weights_t(w, w4t, Cout, Cin)
    dims = [B, Cin, Cout, H, W]
    yield call('upconv3x3_fwd', [a, wp, b, None, torch.zeros(B, Cout, 2 * H, 2 * W)] + dims, [4], tol=3e-5)
    yield call('upconv3x3_fwd', [a, wp, None, rnd(B, Cout, 2 * H, 2 * W, seed=7), torch.zeros(B, Cout, 2 * H, 2 * W)] + dims, [4], tol=3e-5)
    gyh = rnd(B, Cout, 2 * H, 2 * W, seed=3)
    assert bool(K.upconv3x3_dgrad_supported(*dims)) == (tuple(shape) in UPCONV_DGRAD), shape
    if tuple(shape) in UPCONV_DGRAD:
        yield call('upconv3x3_dgrad', [gyh, w4t, torch.zeros(B, Cin, H, W)] + dims, [2], tol=5e-5)
    if H >= 8 and W >= 8 and K.upconv3x3_wgrad_workspace(*dims) > 0:
        nbytes = K.upconv3x3_wgrad_workspace(*dims)
        for acc in (0, 1):
            yield call('upconv3x3_wgrad', [a, gyh, rnd(Cout, Cin, 3, 3, seed=9), workspace(nbytes), nbytes] + dims + [acc, rnd(Cout, seed=10)], [2, 11], tol=1e-4)
        yield call('upconv3x3_wgrad', [a, gyh, torch.zeros(Cout, Cin, 3, 3), workspace(nbytes), nbytes] + dims + [0, None], [2], tol=1e-4)
        yield call('upconv3x3_wgrad_partials+s2_wgrad_reduce_batch', dims, [], tol=1e-4)


def poolconv_calls(K, shape):
    B, Cin, Cout, H, W = shape
    assert K.poolconv3x3_supported(B, Cin, Cout, H, W)
    x, w, b = rnd(B, Cin, 2 * H, 2 * W), rnd(Cout, Cin, 3, 3, scale=0.2), rnd(Cout)
    w4, wp = torch.zeros(Cout, Cin, 4, 4), torch.zeros(4, Cin, Cout, 2, 2)
    yield call('poolconv3x3_weights', [w, w4, wp, Cout, Cin], [1, 2], tol=1e-6)
    w2 = rnd(Cin, Cout, 3, 3, seed=8, scale=0.2)
    rows = [[w, torch.zeros(Cout, Cin, 4, 4), torch.zeros(4, Cin, Cout, 2, 2), Cout, Cin], [w2, torch.zeros(Cin, Cout, 4, 4), torch.zeros(4, Cout, Cin, 2, 2), Cin, Cout]]
    yield call('poolconv3x3_weights_batch', [HostTable(rows, outs=[(0, 1), (0, 2), (1, 1), (1, 2)]), 2], [], tol=1e-6)
    R.poolconv3x3_weights(w, w4, wp, Cout, Cin)
    dims = [B, Cin, Cout, H, W]
    yield call('poolconv3x3_fwd', [x, w4, b, None, torch.zeros(B, Cout, H, W)] + dims, [4], tol=5e-5)
    yield call('poolconv3x3_fwd', [x, w4, None, rnd(B, Cout, H, W, seed=7), torch.zeros(B, Cout, H, W)] + dims, [4], tol=5e-5)
    gy = rnd(B, Cout, H, W, seed=3)
    yield call('poolconv3x3_dgrad', [gy, wp, torch.zeros(B, Cin, 2 * H, 2 * W)] + dims, [2], tol=5e-5)
    nbytes = K.poolconv3x3_wgrad_workspace(*dims)
    for acc in (0, 1):
        yield call('poolconv3x3_wgrad', [x, gy, rnd(Cout, Cin, 3, 3, seed=9), workspace(nbytes), nbytes] + dims + [acc, rnd(Cout, seed=10)], [2, 11], tol=1e-4)
    yield call('poolconv3x3_wgrad', [x, gy, torch.zeros(Cout, Cin, 3, 3), workspace(nbytes), nbytes] + dims + [0, None], [2], tol=1e-4)
    yield call('poolconv3x3_wgrad_partials+s2_wgrad_reduce_batch', dims, [], tol=1e-4)


def multi_calls(K, shape):
    B, Cin, c0, c1, c2, H, W = shape
    assert K.conv1x1_multi_supported(c0, c1, c2, B, Cin, H, W)
    C = c0 + c1 + c2
    x, w = rnd(B, Cin, H, W), rnd(C, Cin, scale=0.2)
    dims = [c0, c1, c2, B, Cin, H, W]
    yield call('conv1x1_multi_fwd', [x, w] + [torch.zeros(B, c, H, W) for c in (c0, c1, c2)] + dims, [2, 3, 4], tol=2e-5)
    gys = [rnd(B, c, H, W, seed=3 + k) for k, c in enumerate((c0, c1, c2))]
    yield call('conv1x1_multi_dgrad', gys + [w, torch.zeros(B, Cin, H, W)] + dims, [4], tol=3e-5)
    nbytes = K.conv1x1_multi_wgrad_workspace(*dims)
    for acc in (0, 1):
        yield call('conv1x1_multi_wgrad', [x] + gys + [rnd(C, Cin, seed=9), workspace(nbytes), nbytes] + dims + [acc], [4], tol=5e-5)


def rgb_calls(K, dims):
    Cout, C, Cimg = dims
    w1, b1, w3 = rnd(C, Cimg), rnd(C, seed=1), rnd(Cout, C, 3, 3, seed=2)
    yield call('rgb_compose_fwd', [w1, b1, w3, torch.zeros(Cout, Cimg + 1, 3, 3), Cout, C, Cimg], [3], tol=2e-6)
    for acc in (0, 1):
        yield call('rgb_compose_bwd', [rnd(Cout, Cimg + 1, 3, 3, seed=3), w1, b1, w3, rnd(C, Cimg, seed=4), rnd(C, seed=5), rnd(Cout, C, 3, 3, seed=6),
                                       Cout, C, Cimg, acc], [4, 5, 6], tol=5e-6)


def bn_calls(K, shape):
    B, C, HW = shape
    x = rnd(B, C, HW) * 1.5 + 0.3
    gamma, beta = 1 + 0.1 * rnd(C), 0.1 * rnd(C, seed=1)
    rm, rv = 0.05 * rnd(C, seed=2), 1 + 0.1 * torch.rand(C, generator=torch.Generator().manual_seed(5))
    ws = workspace(K.bn_workspace(B, C, HW))
    nbt = torch.tensor(41, dtype=torch.int64)
    z = lambda *s: torch.zeros(*s)
    for rep in (1, 4):
        yield call('bn_train_stats', [x, z(C), z(C), rm, rv, nbt, 0.1, 1e-5, ws, B, C, HW, rep], [1, 2, 3, 4, 5], tol=1e-5)
        yield call('bn_train_fwd', [x, z(C), z(C), rm, rv, nbt, gamma, beta, 0.2, 0.1, 1e-5, z(B, C, HW), ws, B, C, HW, rep], [1, 2, 3, 4, 5, 11], tol=1e-5)
    yield call('bn_train_stats', [x, z(C), z(C), None, None, None, 0.1, 1e-5, ws, B, C, HW, 1], [1, 2], tol=1e-5)
    mean, invstd = z(C), z(C)
    R.bn_train_stats(x, mean, invstd, None, None, None, 0.1, 1e-5, None, B, C, HW, 1)
    yield call('bn_eval_stats', [rm, rv, z(C), z(C), 1e-5, C], [2, 3], tol=1e-6)
    gz, v = rnd(B, C, HW, seed=5), rnd(B, C, HW, seed=6)
    for slope in (0.2, 1.0):
        yield call('bn_act_fwd', [x, mean, invstd, gamma, beta, slope, z(B, C, HW), B, C, HW], [6], tol=1e-5)
        for training in (1, 0):
            yield call('bn_act_bwd', [gz, x, mean, invstd, gamma, beta, slope, training, z(B, C, HW), z(C), z(C), ws, B, C, HW, 0, None], [8, 9, 10], tol=3e-5)
        yield call('bn_act_bwd', [gz, x, mean, invstd, gamma, beta, slope, 1, None, rnd(C, seed=11), rnd(C, seed=12), ws, B, C, HW, 1, None], [9, 10], tol=3e-5)
        yield call('bn_act_bwd', [gz, x, mean, invstd, gamma, beta, slope, 1, z(B, C, HW), z(C), z(C), ws, B, C, HW, 0, rnd(B, C, HW, seed=14)], [8, 9, 10], tol=3e-5)
        yield call('bn_act_dbwd', [v, rnd(C, seed=7), rnd(C, seed=8), gz, x, mean, invstd, gamma, beta, slope, z(B, C, HW), z(B, C, HW), z(C), ws, B, C, HW, 0],
                   [10, 11, 12], tol=5e-5)
        yield call('bn_act_dbwd', [v, None, None, gz, x, mean, invstd, gamma, beta, slope, z(B, C, HW), z(B, C, HW), rnd(C, seed=13), ws, B, C, HW, 1],
                   [10, 11, 12], tol=5e-5)
    # the data-parallel protocol, one rank: local sums (float64), finish
    d = lambda k: torch.zeros(C * k, dtype=torch.float64)
    s3, s2, s5 = d(3), d(2), d(5)
    yield call('bn_sync_stats_local', [x, d(3), ws, B, C, HW], [1], tol=1e-5)
    R.bn_sync_stats_local(x, s3, None, B, C, HW)
    yield call('bn_sync_stats_finish', [s3, 1, z(C), z(C), rm, rv, nbt, 0.1, 1e-5, B * HW, 1, C], [2, 3, 4, 5, 6], tol=1e-5)
    yield call('bn_sync_bwd_local', [gz, x, mean, invstd, gamma, beta, 0.2, d(2), ws, B, C, HW], [7], tol=3e-5)
    R.bn_sync_bwd_local(gz, x, mean, invstd, gamma, beta, 0.2, s2, None, B, C, HW)
    yield call('bn_sync_bwd_finish', [gz, x, mean, invstd, gamma, beta, 0.2, s2, s2.clone(), B * HW, z(B, C, HW), z(C), z(C), ws, B, C, HW, 0, None],
               [10, 11, 12], tol=3e-5)
    yield call('bn_sync_bwd_finish', [gz, x, mean, invstd, gamma, beta, 0.2, s2, s2.clone(), B * HW, z(B, C, HW), rnd(C, seed=11), rnd(C, seed=12), ws, B, C, HW, 1,
                                      rnd(B, C, HW, seed=14)], [10, 11, 12], tol=3e-5)
    yield call('bn_sync_dbwd_local', [v, gz, x, mean, invstd, gamma, beta, 0.2, d(5), ws, B, C, HW], [8], tol=5e-5)
    R.bn_sync_dbwd_local(v, gz, x, mean, invstd, gamma, beta, 0.2, s5, None, B, C, HW)
    for acc in (0, 1):
        yield call('bn_sync_dbwd_finish', [v, gz, x, mean, invstd, gamma, beta, 0.2, s5, B * HW, 1, z(B, C, HW), z(B, C, HW), rnd(C, seed=13), ws, B, C, HW, acc],
                   [11, 12, 13], tol=5e-5)
    yield call('channel_sum', [x, z(C), ws, B, C, HW, 0], [1], tol=1e-5)
    yield call('channel_sum', [x, rnd(C, seed=4), ws, B, C, HW, 1], [1], tol=1e-5)
    yield call('channel_bcast', [rnd(C), z(B, C, HW), B, C, HW], [1], atol=0.0)


def bn_group_calls(K, shape):
    G, B, C, HW = shape
    x = rnd(G * B, C, HW) * 1.5 + 0.3
    x[B:] = x[B:] * 0.5 - 1.0
    gamma, beta = 1 + 0.1 * rnd(C), 0.1 * rnd(C, seed=1)
    rm, rv = 0.05 * rnd(C, seed=2), 1 + 0.1 * torch.rand(C, generator=torch.Generator().manual_seed(5))
    ws = workspace(K.bn_workspace(B, G * C, HW))
    nbt = torch.tensor(41, dtype=torch.int64)
    z = lambda *s: torch.zeros(*s)
    for rep in (1, 4):
        yield call('bn_train_fwd_groups', [x, z(G * C), z(G * C), rm, rv, nbt, gamma, beta, 0.2, 0.1, 1e-5, z(G * B, C, HW), ws, G, B, C, HW, rep],
                   [1, 2, 3, 4, 5, 11], tol=1e-5)
    mean, invstd = z(G * C), z(G * C)
    R.bn_train_fwd_groups(x, mean, invstd, None, None, None, gamma, beta, 0.2, 0.1, 1e-5, z(G * B, C, HW), None, G, B, C, HW, 1)
    gz = rnd(G * B, C, HW, seed=5)
    for training in (1, 0):
        yield call('bn_act_bwd_groups', [gz, x, mean, invstd, gamma, beta, 0.2, training, z(G * B, C, HW), z(C), z(C), ws, G, B, C, HW, 0, None, 1], [8, 9, 10], tol=3e-5)
    yield call('bn_act_bwd_groups', [gz, x, mean, invstd, gamma, beta, 0.2, 1, None, rnd(C, seed=11), rnd(C, seed=12), ws, G, B, C, HW, 1, None, 1], [9, 10], tol=3e-5)
    yield call('bn_act_bwd_groups', [gz, x, mean, invstd, gamma, beta, 0.2, 1, z(G * B, C, HW), z(C), z(C), ws, G, B, C, HW, 0, rnd(B, C, HW, seed=14), 1],
               [8, 9, 10], tol=3e-5)


def resample_calls(K, shape):
    BC, H, W = shape
    x = rnd(BC, H, W)
    h, w = H // 2, W // 2
    for alpha in (1.0, 0.25):
        yield call('up2x', [x, torch.zeros(BC, 2 * H, 2 * W), alpha, BC, H, W], [1], tol=1e-6)
        yield call('pool2', [x, None, torch.zeros(BC, h, w), alpha, BC, H, W], [2], tol=1e-6)
        yield call('pool2', [x, rnd(BC, h, w, seed=3), torch.zeros(BC, h, w), alpha, BC, H, W], [2], tol=1e-6)
    yield call('bilinear_half_fwd', [x, torch.zeros(BC, h, w), BC, H, W], [1], tol=1e-5)
    yield call('bilinear_half_bwd', [rnd(BC, h, w), None, torch.zeros(BC, H, W), BC, H, W], [2], tol=1e-5)
    yield call('bilinear_half_bwd', [rnd(BC, h, w), rnd(BC, H, W, seed=5), torch.zeros(BC, H, W), BC, H, W], [2], tol=1e-5)
    idx = torch.zeros(BC, h, w, dtype=torch.uint8)
    yield call('maxpool2_fwd', [x, torch.zeros(BC, h, w), idx.clone(), BC, H, W], [1, 2], atol=0.0)
    R.maxpool2_fwd(x, torch.zeros(BC, h, w), idx, BC, H, W)
    yield call('maxpool2_bwd', [rnd(BC, h, w), idx, torch.zeros(BC, H, W), BC, H, W], [2], atol=0.0)
    yield call('maxpool2_gather', [x, idx, torch.zeros(BC, h, w), BC, H, W], [2], atol=0.0)
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    B = max(1, BC // 3)
    xi = rnd(B, 3, H, W)
    for stages, (OH, OW) in ((2, (H + 3, W + 5)), (1, (H, W)), (0, (2 * H - 1, W + 1))):
        yield call('inception_preprocess', [xi, mean, std, torch.zeros(B, 3, OH, OW), B, 3, H, W, OH, OW, stages], [3], tol=1e-5)


def gemm_calls(K, case):
    M, N, Kd, ta, tb, batch = case
    A = rnd(batch, Kd, M) if ta else rnd(batch, M, Kd)
    Bm = rnd(batch, N, Kd, seed=1) if tb else rnd(batch, Kd, N, seed=1)
    tail = [M, N, Kd, A.shape[-1], Bm.shape[-1], N, ta, tb, batch, A[0].numel(), Bm[0].numel(), M * N]
    yield call('gemm', [A, Bm, torch.zeros(batch, M, N), None] + tail + [0.0], [2], tol=2e-5)
    yield call('gemm', [A, Bm, torch.zeros(batch, M, N), rnd(N, seed=2)] + tail + [0.0], [2], tol=2e-5)
    yield call('gemm', [A, Bm, rnd(batch, M, N, seed=5), None] + tail + [1.0], [2], tol=2e-5)


def rows_calls(K, shape):
    B, C, HW = shape
    x = rnd(B, C, HW)
    yield call('row_sum', [x, torch.zeros(B * C), 1.0, B * C, HW], [1], tol=1e-5)
    yield call('row_bcast', [rnd(B * C), torch.zeros(B * C, HW), 0.5, B * C, HW], [1], tol=1e-6)
    yield call('repeat_rows', [rnd(C, HW), torch.zeros(8 * C, HW), 1.0, C, HW, 8], [1], atol=0.0)
    yield call('sum_reps', [rnd(8 * C, HW), torch.zeros(C, HW), 0.125, C, HW, 8], [1], tol=1e-6)
    yield call('repeat_rows_groups', [rnd(2 * C, HW), torch.zeros(2 * 8 * C, HW), 1.0, C, HW, 8, 2], [1], atol=0.0)
    yield call('sum_reps_groups', [rnd(2 * 8 * C, HW), torch.zeros(2 * C, HW), 0.125, C, HW, 8, 2], [1], tol=1e-6)
    rows, cols = B * C, HW
    s = rnd(rows, cols) * 3
    y = torch.softmax(s, -1)
    gy, v = rnd(rows, cols, seed=1), rnd(rows, cols, seed=2)
    yield call('softmax_fwd', [s, torch.zeros(rows, cols), rows, cols], [1], tol=2e-6)
    yield call('softmax_bwd', [gy, y, torch.zeros(rows, cols), rows, cols], [2], tol=1e-5)
    yield call('softmax_dbwd', [v, gy, y, torch.zeros(rows, cols), rows, cols], [3], tol=1e-5)
    yield call('attn_dbwd_rows', [s, torch.logsumexp(s, -1), gy, v, rnd(rows, cols, seed=3), rows, cols], [0, 2, 3, 4], tol=2e-5)
    yield call('copy_channels', [x, torch.zeros(B, C + 1, HW), B, C, C + 1, HW, 1.0], [1], atol=0.0)
    yield call('copy_channels', [x, torch.zeros(B, C - 1, HW), B, C, C - 1, HW, 0.0], [1], atol=0.0)
    yield call('center_rows', [rnd(rows, cols), rnd(cols, seed=1), rows, cols], [0], tol=1e-6)
    yield call('trace', [rnd(cols, cols + 3), torch.zeros(()), cols, cols + 3], [1], tol=1e-5)
    p = torch.softmax(rnd(rows, cols), -1)
    yield call('is_kl_rows', [p, p.mean(0), torch.zeros(rows), rows, cols], [2], tol=1e-5, atol=1e-6)
    taus = torch.rand(rows, 1, generator=torch.Generator().manual_seed(3))
    yield call('iqn_cos_embed', [taus, torch.arange(1, 21).float(), torch.zeros(rows, 20), rows, 20], [2], atol=2e-5)
    W_ = rnd(rows, cols)
    yield call('sn_power_iter', [W_, F.normalize(rnd(rows, seed=1), dim=0), F.normalize(rnd(cols, seed=2), dim=0), torch.zeros(()), rows, cols, 2, 1e-12],
               [1, 2, 3], tol=1e-5)


def elementwise_calls(K, n):
    a, b = rnd(n), rnd(n, seed=1)
    z = lambda: torch.zeros(n)
    yield call('add', [a, b, z(), n], [2], atol=0.0)
    yield call('add4', [a, b, rnd(n, seed=2), rnd(n, seed=3), z(), n], [4], atol=0.0)
    yield call('add4', [a, b, rnd(n, seed=2), None, z(), n], [4], atol=0.0)
    yield call('mul', [a, b, z(), n], [2], atol=0.0)
    yield call('scale', [a, 0.3, z(), n], [2], tol=1e-7)
    s = torch.tensor(1.7)
    yield call('scale_dev', [s, 0.5, a, z(), n], [3], tol=1e-6)
    yield call('scale_add_dev', [s, a, b, z(), n], [3], tol=1e-6)
    ws = workspace(K.reduce_workspace(n))
    yield call('dot', [a, b, 0.5, torch.zeros(()), ws, n, 0], [3], tol=1e-5, atol=1e-5 * n ** 0.5)
    yield call('dot', [a, b, 0.5, torch.tensor(3.0), ws, n, 1], [3], tol=1e-5, atol=1e-5 * n ** 0.5)
    yield call('sumsq', [a, 0.25, torch.zeros(()), ws, n], [2], tol=1e-5)
    yield call('lrelu_bwd', [a, b, 0.2, z(), n], [3], atol=0.0)
    yield call('tanh_fwd', [a, z(), n], [1], tol=1e-6)
    yield call('tanh_bwd', [b, torch.tanh(a), z(), n], [2], tol=1e-6)
    yield call('elu_fwd', [a, 1.0, 1.0, z(), n], [3], tol=1e-6)
    for order in (1, 2):
        yield call('elu_bwd', [b, a, 1.6733, 1.0507, order, z(), n], [5], tol=1e-6)
    yield call('recip', [a.abs() + 0.5, z(), n], [1], tol=1e-6)
    yield call('fill', [torch.ones(n), 2.5, n], [0], atol=0.0)
    hyper = torch.tensor([1e-3 / (1 - 0.9 ** 3), (1 - 0.999 ** 3) ** 0.5, 0.9, 0.999, 1 - 0.9, 1 - 0.999])
    yield call('adam_step', [a, b * 1e-2, rnd(n, seed=4) * 1e-2, rnd(n, seed=5).abs() * 1e-4, hyper, 1e-8, n], [0, 2, 3], tol=1e-6)
    yield call('ema', [rnd(n, seed=2), a, 1e-3, n], [0], tol=1e-7)
    Q, B = 3, max(1, n // 3)
    taus = torch.rand(Q * B, 1, generator=torch.Generator().manual_seed(3))
    preds, target = rnd(Q * B, 1) * 2, (torch.arange(B) % 2).float().view(B, 1)
    wsl = workspace(K.reduce_workspace(2 * Q * B))
    yield call('iqn_loss', [preds, target, taus, 1.0, torch.zeros(()), torch.zeros(Q * B, 1), wsl, Q, B], [4, 5], tol=2e-6)
    yield call('iqn_loss_groups', [torch.cat([preds, preds * 0.5]), torch.cat([target, 1 - target]), torch.cat([taus, 1 - taus]), 1.0, torch.zeros(()),
                                   torch.zeros(2 * Q * B, 1), wsl, Q, B, 2], [4, 5], tol=2e-6)
    # (few rows: logits of order 1, so that the mean stays of order 1 -- torch's own formula log(exp(-m) + exp(-x - m)) carries ulp(1)
    # per row, which a mean of 1e-3 over one row would turn into 1e-4 relative, a property of the reference and not of the kernel)
    yield call('bce_logits', [rnd(n, 1) * (4 if n >= 48 else 1), (torch.arange(n) % 2).float().view(n, 1), torch.zeros(()), torch.zeros(n, 1), ws, n], [2, 3], tol=2e-6)


def attn_calls(K, dims):
    B, D, DV, N, M = dims
    assert K.attn_supported(D, DV)
    theta, phi, g = rnd(B, D, N), rnd(B, D, M, seed=1), rnd(B, DV, M, seed=2)
    o, lse = torch.zeros(B, DV, N), torch.zeros(B, N)
    yield call('attn_fwd', [theta, phi, g, o.clone(), lse.clone(), B, D, DV, N, M], [3, 4], tol=6e-6)
    R.attn_fwd(theta, phi, g, o, lse, B, D, DV, N, M)
    go = rnd(B, DV, N, seed=3)
    yield call('attn_bwd', [go, theta, phi, g, o, lse, torch.zeros(B, D, N), torch.zeros(B, D, M), torch.zeros(B, DV, M),
                            workspace(K.attn_bwd_workspace(B, D, DV, N, M)), B, D, DV, N, M], [6, 7, 8], tol=2e-5)
    if K.attn_dbwd_supported(D, DV, M):
        a, b, c = rnd(B, D, N, seed=4), rnd(B, D, M, seed=5), rnd(B, DV, M, seed=6)
        yield call('attn_dbwd', [go, theta, phi, g, lse, a, b, c, torch.zeros(B, DV, N), torch.zeros(B, D, N), torch.zeros(B, D, M), torch.zeros(B, DV, M),
                                 workspace(K.attn_dbwd_workspace(B, D, DV, N, M)), B, D, DV, N, M], [8, 9, 10, 11], tol=3e-5)


def fid_calls(K, case):
    M, N, Kd, ta = case
    assert K.gemm_big_supported(M, N, Kd, M if ta else Kd, N, ta)
    A = rnd(Kd, M) if ta else rnd(M, Kd)
    yield call('gemm_big', [A, rnd(Kd, N, seed=1), torch.zeros(M, N), M, N, Kd, A.shape[1], N, N, ta, -0.5, 1.5], [2], tol=2e-5)
    yield call('gemm_big', [A, rnd(Kd, N, seed=1), torch.zeros(M, N), M, N, Kd, A.shape[1], N, N, ta, 1.0, 0.0], [2], tol=2e-5)


def inception_calls(K, case):
    B, Cin, Cout, H, W, KH, KW, stride, ph, pw, x_ctot, x_coff, y_ctot, y_coff = case
    assert K.inception_conv_supported(B, Cin, Cout, H, W, KH, KW, stride, ph, pw, x_ctot, y_ctot) == 1
    w = rnd(Cout, Cin, KH, KW, scale=(2.0 / (Cin * KH * KW)) ** 0.5)
    kk, coutp = Cin * KH * KW, (Cout + 127) // 128 * 128
    wp = torch.zeros((kk + 15) // 16 * 16, coutp)
    wp[:kk, :Cout] = w.reshape(Cout, kk).t()
    assert wp.numel() == K.inception_conv_weight_floats(Cin, Cout, KH, KW)
    x = rnd(B, x_ctot, H, W)
    OH, OW = (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1
    for relu, bias in ((1, rnd(Cout, seed=2) * 0.2), (0, None)):
        yield call('inception_conv_fwd', [x, wp, bias, rnd(B, y_ctot, OH, OW, seed=4), B, Cin, Cout, H, W, KH, KW, stride, ph, pw, relu, x_ctot, x_coff, y_ctot, y_coff],
                   [3], tol=2e-5)          # fp32 matrix-core accumulation over K <= 63 products, as tg_conv2d_fwd
    xc = rnd(B, x_ctot, H, W, seed=5)
    C = min(Cin, Cout)
    yield call('inception_maxpool3s2', [xc, rnd(B, y_ctot, (H - 3) // 2 + 1, (W - 3) // 2 + 1, seed=6), B, C, H, W, x_ctot, x_coff, y_ctot, y_coff], [1], atol=0.0)
    yield call('inception_avgpool3', [xc, rnd(B, y_ctot, H, W, seed=7), B, C, H, W, x_ctot, x_coff, y_ctot, y_coff], [1], tol=1e-6)


def image_calls(K, case):
    B, n_images, H, W, ch, size = case
    g = torch.Generator().manual_seed(7)
    archive = torch.randint(0, 256, (n_images, H, W, ch), generator=g, dtype=torch.uint8)
    index = torch.randint(0, n_images, (B,), generator=g, dtype=torch.int64)
    cy = torch.randint(0, H - size + 1, (B,), generator=g, dtype=torch.int32)
    cx = torch.randint(0, W - size + 1, (B,), generator=g, dtype=torch.int32)
    yield call('image_bytes_batch', [archive, index, cy, cx, torch.zeros(B, ch, size, size), B, n_images, H, W, ch, size], [4], atol=0.0)
    yield call('image_bytes_batch', [archive[:, :size, :size].contiguous(), index, None, None, torch.zeros(B, ch, size, size), B, n_images, size, size, ch, size],
               [4], atol=0.0)


# family: (builder, shapes -- the FIRST is the smallest: it also runs with every pointer shifted alone --, entry points it must reach)
FAMILIES = {
    'conv2d': (conv_calls, [(2, 5, 7, 9, 11, 1), (3, 5, 7, 20, 12, 3),      # smallest ragged 1x1 (direct few-channel kernel, scalar pixels) and 3x3
                          (3, 32, 4, 32, 32, 1),                          # few-channel direct 1x1, vector pixels
                          (2, 16, 16, 32, 32, 3), (2, 128, 128, 8, 8, 3),  # aligned 3x3 (Winograd-eligible); long reduction: K-split weight gradient
                          # 64 planes of 16 x 16, Cin > 16 (8-channel chunks), 64 * ceil(Cout / 32) = 256 workgroups: conv_dma_kernel<G16, 32, 1, 8>
                          # (below the 512 the Winograd form asks for at 16 x 16, so TG_CONV_WINO = 0 and the default both take it)
                          (64, 32, 128, 16, 16, 3)],
             ['conv2d_fwd', 'conv2d_fwd_up2res', 'conv2d_dgrad', 'conv2d_wgrad', 'conv2d_wgrad_partials', 'conv2d_wgrad_reduce_batch']),
    'upconv': (upconv_calls, [(2, 5, 7, 6, 10), (2, 16, 16, 16, 16), (128, 32, 24, 16, 16),     # ragged; aligned; all phases in one kernel
                              # 8 x 8 planes, 4 images per tile, all phases in one kernel: ceil(B / 4) * ceil(C / 16) = 260 either way (G8),
                              # and 65 * 3 = 195 forward / 65 * 2 = 130 backward, in [128, 256): the K-split form (G8k)
                              (520, 24, 20, 8, 8), (258, 24, 40, 8, 8)],
               ['upconv3x3_weights', 'upconv3x3_weights_t', 'upconv3x3_weights_pair', 'upconv3x3_fwd', 'upconv3x3_dgrad', 'upconv3x3_wgrad',
                'upconv3x3_wgrad_partials', 's2_wgrad_reduce_batch']),
    'poolconv': (poolconv_calls, [(20, 20, 18, 70, 50), (128, 32, 24, 16, 16)],        # ragged; 16 x 16 planes, one-kernel forms
                 ['poolconv3x3_weights', 'poolconv3x3_weights_batch', 'poolconv3x3_fwd', 'poolconv3x3_dgrad', 'poolconv3x3_wgrad',
                  'poolconv3x3_wgrad_partials', 's2_wgrad_reduce_batch']),
    'multi': (multi_calls, [(2, 16, 2, 2, 8, 4, 4), (2, 20, 2, 2, 10, 12, 12)], ['conv1x1_multi_fwd', 'conv1x1_multi_dgrad', 'conv1x1_multi_wgrad']),
    'rgb': (rgb_calls, [(5, 7, 2), (16, 16, 3)], ['rgb_compose_fwd', 'rgb_compose_bwd']),
    'bn': (bn_calls, [(2, 7, 12 * 10), (8, 128, 16),         # ragged; one workgroup per channel
                      (2, 4, 128 * 128), (64, 128, 1)],      # big planes (two launches); the generic three-launch path
           ['bn_train_stats', 'bn_train_fwd', 'bn_eval_stats', 'bn_act_fwd', 'bn_act_bwd', 'bn_act_dbwd', 'bn_sync_stats_local', 'bn_sync_stats_finish',
            'bn_sync_bwd_local', 'bn_sync_bwd_finish', 'bn_sync_dbwd_local', 'bn_sync_dbwd_finish', 'channel_sum', 'channel_bcast']),
    'bn_groups': (bn_group_calls, [(2, 7, 12, 12 * 10), (2, 8, 128, 16), (3, 2, 4, 128 * 128), (2, 130, 24, 16 * 16)],
                  ['bn_train_fwd_groups', 'bn_act_bwd_groups']),
    'resample': (resample_calls, [(5, 10, 6), (3, 34, 20), (6, 16, 16)],
                 ['up2x', 'pool2', 'bilinear_half_fwd', 'bilinear_half_bwd', 'maxpool2_fwd', 'maxpool2_bwd', 'maxpool2_gather', 'inception_preprocess']),
    'gemm': (gemm_calls, [(1, 77, 32, 0, 1, 1), (3, 70, 300, 0, 0, 2), (16, 1024, 256, 0, 1, 3),        # ragged skinny; ragged; skinny matrix-core
                          (100, 37, 19, 1, 1, 2), (256, 64, 16, 1, 0, 3)], ['gemm']),
    'rows': (rows_calls, [(5, 12, 47), (3, 8, 64), (2, 3, 300)],
             ['row_sum', 'row_bcast', 'repeat_rows', 'sum_reps', 'repeat_rows_groups', 'sum_reps_groups', 'softmax_fwd', 'softmax_bwd', 'softmax_dbwd',
              'attn_dbwd_rows', 'copy_channels', 'center_rows', 'trace', 'is_kl_rows', 'iqn_cos_embed', 'sn_power_iter']),
    'elementwise': (elementwise_calls, [5, 1, 1024, 4099],
                    ['add', 'add4', 'mul', 'scale', 'scale_dev', 'scale_add_dev', 'dot', 'sumsq', 'lrelu_bwd', 'tanh_fwd', 'tanh_bwd', 'elu_fwd', 'elu_bwd',
                     'recip', 'fill', 'adam_step', 'ema', 'iqn_loss', 'iqn_loss_groups', 'bce_logits']),
    'attention': (attn_calls, [(1, 2, 8, 64, 16), (2, 8, 32, 300, 75),
                               # 4 tiles per wave on both sides: B * ceil(N / 64) = 4096 query-side, B * ceil(M / 64) = 1024 key-side
                               # (the thresholds of attn_rt / attn_rt_keys), whole tiles and ragged ones
                               (256, 1, 4, 1024, 256), (1024, 1, 4, 250, 63)],
                  ['attn_fwd', 'attn_bwd', 'attn_dbwd']),
    'fid': (fid_calls, [(33, 40, 20, 0), (132, 136, 64, 1)], ['gemm_big']),
    'inception': (inception_calls, [(2, 7, 9, 6, 5, 1, 7, 1, 0, 3, 10, 2, 12, 1), (1, 3, 80, 37, 41, 3, 3, 2, 0, 0, 3, 0, 80, 0),
                                    (2, 5, 130, 24, 27, 3, 3, 1, 1, 1, 5, 0, 130, 0)],
                  ['inception_conv_fwd', 'inception_maxpool3s2', 'inception_avgpool3']),
    'input': (image_calls, [(3, 5, 9, 11, 3, 7), (4, 6, 16, 16, 3, 16)], ['image_bytes_batch']),
}
# entry points with a device-pointer parameter that are left out, by name, each with its reason (at most 6)
EXCLUDED = {}
WINO_FAMILIES = ('conv2d', 'upconv', 'poolconv')
CASES = [(fam, i) for fam, (_, shapes, _) in FAMILIES.items() for i in range(len(shapes))]


def expectation(name, args, pl):
    names = [p[1] for p in guarded.params_of(name)]
    shifted = [n for i, (n, a) in enumerate(zip(names, args)) if torch.is_tensor(a) and (pl == 'shifted' or pl == i)]
    return 'rejected' if any(n in REJECTS.get(name, ()) for n in shifted) else 'ok'


_FIRST = {}


def first_case(K, fam):
    """{entry point: index of the first (smallest) case of the family that reaches it}: that case also shifts every pointer alone."""
    if fam not in _FIRST:
        builder, shapes, _ = FAMILIES[fam]
        _FIRST[fam] = {}
        for i, shape in enumerate(shapes):
            for c in builder(K, shape):
                for n in c['name'].split('+'):
                    _FIRST[fam].setdefault(n, i)
    return _FIRST[fam]


@pytest.mark.parametrize('fam,i', CASES, ids=[f'{f}-{FAMILIES[f][1][i]}'.replace(' ', '') for f, i in CASES])
def test_sweep(K, fam, i):
    builder, shapes, names = FAMILIES[fam]
    first = first_case(K, fam)
    assert set(first) == set(names), f'{fam}: declared {sorted(names)}, reached {sorted(first)}'
    ran = {}
    for c in builder(K, shapes[i]):
        name, args = c['name'], c['args']
        if '+' in name:                                        # stage 1 + batched stage 2
            kind = name.split('_wgrad')[0]
            pls = ['aligned', 'shifted'] + ([0] if first[kind + '_wgrad_partials'] == i else [])
            for k, v in wgrad_two_steps(K, kind, args, c['kw']['tol'], pls).items():
                ran.setdefault(k, {'ok': [], 'rejected': []})['ok'] += v
            continue
        ptrs = [j for j, a in enumerate(args) if torch.is_tensor(a)]
        pls = ['aligned', 'shifted'] + (ptrs if first[name] == i else [])
        by = {'ok': [p for p in pls if expectation(name, args, p) == 'ok'], 'rejected': [p for p in pls if expectation(name, args, p) == 'rejected']}
        for expect, group in by.items():
            if group:
                run_both(K, name, args, c['outs'], placement=group, expect=expect, emulator=R, **c['kw'])
                ran.setdefault(name, {'ok': [], 'rejected': []})[expect] += [str(p) for p in group]
    for name, r in sorted(ran.items()):
        print(f'GUARD {name}: {len(r["ok"]) + len(r["rejected"])} placements, accepted [{" ".join(r["ok"])}] rejected [{" ".join(r["rejected"])}]')


@pytest.mark.parametrize('kind,dims', [('conv2d', (3, 5, 7, 20, 12, 3)), ('poolconv3x3', (32, 32, 24, 16, 16)), ('upconv3x3', (32, 32, 24, 16, 16)),
                                       ('conv1x1_multi', (2, 2, 8, 2, 16, 4, 4))])
def test_undersized_workspace_is_rejected(K, kind, dims):
    """nbytes - 4 declared (and allocated): TG_EWORKSPACE, nothing written."""
    nbytes = getattr(K, kind + '_wgrad_workspace')(*dims) - 4
    ws = workspace(nbytes)
    if kind == 'conv1x1_multi':
        c0, c1, c2, B, Cin, H, W = dims
        args = [rnd(B, Cin, H, W)] + [rnd(B, c, H, W, seed=k) for k, c in enumerate((c0, c1, c2))] + [rnd(c0 + c1 + c2, Cin), ws, nbytes, *dims, 0]
        run_both(K, 'conv1x1_multi_wgrad', args, [4], expect='rejected')
        return
    B, Cin, Cout, H, W = dims[:5]
    if kind == 'conv2d':
        x, gy = rnd(B, Cin, H, W), rnd(B, Cout, H, W, seed=3)
        run_both(K, 'conv2d_wgrad', [x, gy, rnd(Cout, Cin, 3, 3), rnd(Cout), ws, nbytes, *dims, 0], [2, 3], expect='rejected')
    else:
        lo, hi = (rnd(B, Cin, 2 * H, 2 * W), rnd(B, Cout, H, W)) if kind == 'poolconv3x3' else (rnd(B, Cin, H, W), rnd(B, Cout, 2 * H, 2 * W))
        run_both(K, kind + '_wgrad', [lo, hi, rnd(Cout, Cin, 3, 3), ws, nbytes, *dims, 0, rnd(Cout)], [2, 11], expect='rejected')
    run_both(K, kind + '_wgrad_partials', [lo if kind != 'conv2d' else x, hi if kind != 'conv2d' else gy, ws, nbytes, *dims, 1], [], expect='rejected')
    print(f'GUARD {kind}_wgrad / _wgrad_partials: workspace of nbytes - 4 rejected')


@pytest.mark.parametrize('mode', ['0', '2'])
@pytest.mark.parametrize('fam', WINO_FAMILIES)
def test_convolution_families_under_each_winograd_mode(fam, mode):
    """TG_CONV_WINO is read once per process: the convolution families again in a fresh child with Winograd off / on every eligible shape."""
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-s', '-k', f'test_sweep and {fam}-', '-p', 'no:cacheprovider'],
                       env=dict(os.environ, TG_CONV_WINO=mode), cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    lines = [line[line.index('GUARD'):] for line in r.stdout.splitlines() if 'GUARD' in line]
    print(f'wino={mode} {fam}: {len(lines)} entry-point lines')
    assert r.returncode == 0, r.stdout[-4000:]
    assert ' passed' in r.stdout and ' deselected' in r.stdout and lines


def test_every_entry_point_with_a_device_pointer_is_covered():
    """Against what the harness actually ran in this process (guarded.SEEN, filled by run_both): a deselected, skipped or failed
    sweep case leaves its entry points uncovered here.  Runs after the sweep, in this file's order; alone it has nothing to count."""
    from tartangan_amd import backend
    need = {n[3:] for n, (ret, params) in backend.parse_header().items()
            if any(t.endswith('*') and t not in ('const char*',) and a != 'stream' for t, a in params)}
    here = {n for _, _, names in FAMILIES.values() for n in names}
    assert len(EXCLUDED) <= 6 and not (set(EXCLUDED) & here)
    assert not (here - need), sorted(here - need)
    ran = set(guarded.SEEN)
    uncovered = need - ran - set(EXCLUDED)
    print(f'GUARD coverage: {len(need)} entry points with pointer parameters, {len(need & ran)} ran through the guarded harness in this process, '
          f'excluded {sorted(EXCLUDED)}, uncovered {sorted(uncovered)}')
    assert not uncovered, f'not run through the guarded harness in this process (run the whole file): {sorted(uncovered)}'
