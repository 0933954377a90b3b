"""Parity for every row of the dispatch ledger (tests/conv_dispatch_cases.py): each distinct answer of conv.hip's dispatch code,
at the smallest call the search found for it, against the emulator -- once on random data after NaN-poisoning the LDS (the
tolerance of the entry point's own parity test), once on small integers, bit for bit.

A row first asks tg_conv_dispatch, with the switches THIS process read from its environment, whether the call still gets the
row's record: the run below it is then known to be a run of those kernels.  Rows of a knob set other than the default run in one
child process per set (the switches are read once per process)."""
import os
import re
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import conv_dispatch_search as S  # noqa: E402
from conv_dispatch_cases import CASES  # noqa: E402
from grouped_wgrad_cases import GroupedEmulator  # noqa: E402
from guarded import HostTable, Per, rnd, run_both, workspace  # noqa: E402
from test_kernels_gpu import poison_lds  # noqa: E402

pytestmark = pytest.mark.gpu
E = GroupedEmulator()


class Bounded:
    """The emulator for the exact runs: after each of its calls every floating-point tensor it was handed -- operands and the
    reference result alike -- must lie below 2^24 in float64, so that the exactness of the reference rests on the reference alone
    and not on the kernel under test.  (Tensors behind a host table are checked through the device-side copy that matched them
    bit for bit, see test_row.)"""

    def __getattr__(self, name):
        fn = getattr(E, name)

        def call(*args):
            r = fn(*args)
            for a in args:
                if torch.is_tensor(a) and a.is_floating_point() and a.numel():
                    assert float(a.double().abs().max()) < EXACT, f'{name}: the reference leaves the exact integer range'
            return r
        return call if callable(fn) else fn


ENV_KEYS = ('TG_CONV_WINO', 'TG_CONV_DMA', 'TG_DMA_PRIO')
# the knob set this process runs under: the one whose three variables are set as tools/conv_dispatch_search.KNOB_ENV spells them
ACTIVE = next((k for k, env in S.KNOB_ENV.items() if all(os.environ.get(v) == env[v] for v in ENV_KEYS)), 'default')
ROWS = [i for i, (case, _, _) in enumerate(CASES) if case[5] == ACTIVE]
# tolerances of the existing parity tests of the same entry points (tests/test_kernels_gpu.py, tests/test_guard_bands_gpu.py)
TOL = {'conv2d_fwd': 2e-5, 'conv2d_fwd_up2res': 2e-5, 'conv2d_dgrad': 2e-5, 'conv2d_wgrad': 5e-5, 'conv2d_wgrad_partials': 5e-5,
       'conv2d_wgrad_reduce_batch': 5e-5, 'conv1x1_wgrad_partials_batch': 5e-5, 'upconv3x3_fwd': 3e-5, 'upconv3x3_dgrad': 5e-5,
       'poolconv3x3_fwd': 5e-5, 'poolconv3x3_dgrad': 5e-5, 'upconv3x3_wgrad': 1e-4, 'poolconv3x3_wgrad': 1e-4,
       'upconv3x3_wgrad_partials': 1e-4, 'poolconv3x3_wgrad_partials': 1e-4, 's2_wgrad_reduce_batch': 1e-4,
       'upconv3x3_weights': 1e-6, 'upconv3x3_weights_t': 1e-6, 'upconv3x3_weights_pair': 1e-6, 'poolconv3x3_weights': 1e-6,
       'poolconv3x3_weights_batch': 1e-6, 'rgb_compose_fwd': 2e-6, 'rgb_compose_bwd': 5e-6, 'conv1x1_multi_fwd': 2e-5,
       'conv1x1_multi_dgrad': 3e-5, 'conv1x1_multi_wgrad': 5e-5}
EXACT = 1 << 24                      # integers up to here are exact in fp32


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    backend._set_backend_for_testing(None)
    return backend.get()


class Data:
    """Operands of one run.  Random: guarded.rnd (filters at ``scale``).  Exact: integers in [-m, m] in an asymmetric pattern (a
    transposed fragment or a swapped tap shows), m chosen by ``fit`` so that the largest sum of products stays below 2^24."""

    def __init__(self, exact):
        self.exact, self.m = exact, (3, 2)

    def fit(self, terms, extra=0, headroom=1):
        """terms: products per output element; extra: what bias / residual / a folded tap add; headroom: power of two the kernel may scale
        by on the way (derived filters in quarters, Winograd transforms that halve twice each way).  The bound is on every partial sum of
        the float64 reference, whatever the order, so both sides are exact by construction."""
        if not self.exact:
            return
        for m in ((3, 2), (2, 1), (1, 1)):
            self.m = m
            if (m[0] * m[1] * terms + extra) * headroom < EXACT:
                return
        raise AssertionError(f'no integer range keeps {terms} products below 2^24')

    def __call__(self, *shape, seed=0, scale=1.0, filt=False):
        if not self.exact:
            return rnd(*shape, seed=seed, scale=scale)
        m = self.m[1 if filt else 0]
        n = 1
        for s in shape:
            n *= s
        i = torch.arange(n)
        return ((i + i // 17 + seed) % (2 * m + 1) - m).float().view(*shape)


def two_steps(K, kind, lo, hi, dims, last, bias, pl1, pl2, tol, atol, D):
    """Stage 1 into a guarded workspace, then the batched stage 2 over a one-row host table, against the emulator's finished gradients."""
    B, Cin, Cout = dims[:3]
    ks = dims[5] if kind == 'conv2d' else 3
    nbytes = getattr(K, kind + '_wgrad_workspace')(*dims)
    ws_e = workspace(getattr(E, kind + '_wgrad_workspace')(*dims))
    getattr(E, kind + '_wgrad_partials')(lo, hi, ws_e, ws_e.numel() * 4, *dims, bias)
    dev = run_both(K, kind + '_wgrad_partials', [lo, hi, workspace(nbytes), nbytes, *dims, bias], [], placement=pl1, emulator=E)
    row = [Per(ws_e, dev[2].cpu()), torch.zeros(Cout, Cin, ks, ks), torch.zeros(Cout) if bias else None, *dims[:5], last, 0]
    outs = [(0, 1)] + ([(0, 2)] if bias else [])
    reduce = 'conv2d_wgrad_reduce_batch' if kind == 'conv2d' else 's2_wgrad_reduce_batch'
    got = run_both(K, reduce, [HostTable([row], outs=outs), 1], [], tol=tol, atol=atol, placement=pl2, emulator=E)
    return [got[0][pos] for pos in outs]


def run_row(K, case, exact):
    """One run of the row's call through the guarded harness -> the device-side outputs."""
    op, (B, Cin, Cout, H, W, ks, c1, c2), pl, bias, res, _ = case
    D = Data(exact)
    tol, atol = TOL[op], (0.0 if exact else None)
    ref = Bounded() if exact else E
    go = lambda args, outs: [run_both(K, op, args, outs, tol=tol, atol=atol, placement=pl, emulator=ref)[i] for i in outs]
    d5 = [B, Cin, Cout, H, W]
    if op in ('conv2d_fwd', 'conv2d_fwd_up2res'):
        D.fit(Cin * ks * ks, extra=6, headroom=64)
        x, w = D(B, Cin, H, W), D(Cout, Cin, ks, ks, scale=0.2, filt=True)
        b = D(Cout, seed=1) if bias else None
        if op == 'conv2d_fwd':
            return go([x, w, b, D(B, Cout, H, W, seed=7) if res else None, torch.zeros(B, Cout, H, W)] + d5 + [ks], [4])
        return go([x, w, b, D(B, Cout, H // 2, W // 2, seed=7), torch.zeros(B, Cout, H, W)] + d5, [4])
    if op == 'conv2d_dgrad':
        D.fit(Cout * ks * ks, headroom=64)
        return go([D(B, Cout, H, W, seed=3), D(Cout, Cin, ks, ks, scale=0.2, filt=True), torch.zeros(B, Cin, H, W)] + d5 + [ks], [2])
    if op.startswith('conv2d_wgrad'):
        D.fit(B * H * W)
        x, gy = D(B, Cin, H, W), D(B, Cout, H, W, seed=3, filt=True)
        if op == 'conv2d_wgrad':
            nbytes = K.conv2d_wgrad_workspace(*d5, ks)
            return go([x, gy, torch.zeros(Cout, Cin, ks, ks), torch.zeros(Cout) if bias else None, workspace(nbytes), nbytes] + d5 + [ks, 0],
                      [2, 3] if bias else [2])
        first = op == 'conv2d_wgrad_partials'
        return two_steps(K, 'conv2d', x, gy, d5 + [ks], ks, bias, pl if first else 'aligned', 'aligned' if first else pl, tol, atol, D)
    if op in ('upconv3x3_fwd', 'upconv3x3_dgrad', 'poolconv3x3_fwd', 'poolconv3x3_dgrad'):
        # derived filters: sums of up to 4 taps (in quarters for the pooled form), 4 x 4 or 2 x 2 of them per channel pair
        D.fit((Cout if op.endswith('dgrad') else Cin) * 36, extra=6, headroom=64)
        w = D(Cout, Cin, 3, 3, scale=0.2, filt=True)
        b = D(Cout, seed=1) if bias else None
        if op.startswith('upconv'):
            wp, w4t = torch.zeros(4, Cout, Cin, 2, 2), torch.zeros(Cin, Cout, 4, 4)
            E.upconv3x3_weights_pair(w, wp, w4t, Cout, Cin)
            if op == 'upconv3x3_fwd':
                return go([D(B, Cin, H, W), wp, b, D(B, Cout, 2 * H, 2 * W, seed=7) if res else None, torch.zeros(B, Cout, 2 * H, 2 * W)] + d5, [4])
            return go([D(B, Cout, 2 * H, 2 * W, seed=3), w4t, torch.zeros(B, Cin, H, W)] + d5, [2])
        w4, wp = torch.zeros(Cout, Cin, 4, 4), torch.zeros(4, Cin, Cout, 2, 2)
        E.poolconv3x3_weights(w, w4, wp, Cout, Cin)
        if op == 'poolconv3x3_fwd':
            return go([D(B, Cin, 2 * H, 2 * W), w4, b, D(B, Cout, H, W, seed=7) if res else None, torch.zeros(B, Cout, H, W)] + d5, [4])
        return go([D(B, Cout, H, W, seed=3), wp, torch.zeros(B, Cin, 2 * H, 2 * W)] + d5, [2])
    if op in ('upconv3x3_wgrad', 'poolconv3x3_wgrad', 'upconv3x3_wgrad_partials', 'poolconv3x3_wgrad_partials', 's2_wgrad_reduce_batch'):
        up = op.startswith('upconv') or (op.startswith('s2') and ks == 1)
        kind = 'upconv3x3' if up else 'poolconv3x3'
        D.fit(B * H * W * 16, headroom=4)                 # a 3 x 3 tap folds up to 4 of the 16 products per low-resolution pixel
        p0 = D(B, Cin, H, W, seed=4) if up else D(B, Cin, 2 * H, 2 * W)
        p1 = D(B, Cout, 2 * H, 2 * W, seed=5, filt=True) if up else D(B, Cout, H, W, seed=3, filt=True)
        if op.endswith('_wgrad'):
            nbytes = getattr(K, op + '_workspace')(*d5)
            return go([p0, p1, torch.zeros(Cout, Cin, 3, 3), workspace(nbytes), nbytes] + d5 + [0, torch.zeros(Cout) if bias else None],
                      [2, 11] if bias else [2])
        first = op.endswith('partials')
        return two_steps(K, kind, p0, p1, d5, 1 if up else 0, bias, pl if first else 'aligned', 'aligned' if first else pl, tol, atol, D)
    if op in ('upconv3x3_weights', 'upconv3x3_weights_t', 'upconv3x3_weights_pair', 'poolconv3x3_weights', 'poolconv3x3_weights_batch'):
        w = D(Cout, Cin, 3, 3, filt=True)
        wp, w4t = torch.zeros(4, Cout, Cin, 2, 2), torch.zeros(Cin, Cout, 4, 4)
        w4, wpp = torch.zeros(Cout, Cin, 4, 4), torch.zeros(4, Cin, Cout, 2, 2)
        if op == 'poolconv3x3_weights_batch':
            got = run_both(K, op, [HostTable([[w, w4, wpp, Cout, Cin]], outs=[(0, 1), (0, 2)]), 1], [], tol=tol, atol=atol, placement=pl, emulator=E)
            return [got[0][(0, 1)], got[0][(0, 2)]]
        args, outs = {'upconv3x3_weights': ([w, wp], [1]), 'upconv3x3_weights_t': ([w, w4t], [1]), 'upconv3x3_weights_pair': ([w, wp, w4t], [1, 2]),
                      'poolconv3x3_weights': ([w, w4, wpp], [1, 2])}[op]
        return go(args + [Cout, Cin], outs)
    if op in ('rgb_compose_fwd', 'rgb_compose_bwd'):
        C, Cimg = Cin, ks
        D.fit(max(C, Cout * 9))
        w1, b1, w3 = D(C, Cimg), D(C, seed=1), D(Cout, C, 3, 3, seed=2, filt=True)
        if op == 'rgb_compose_fwd':
            return go([w1, b1, w3, torch.zeros(Cout, Cimg + 1, 3, 3), Cout, C, Cimg], [3])
        return go([D(Cout, Cimg + 1, 3, 3, seed=3, filt=True), w1, b1, w3, torch.zeros(C, Cimg), torch.zeros(C), torch.zeros(Cout, C, 3, 3),
                   Cout, C, Cimg, 0], [4, 5, 6])
    cs = [c for c in (Cout, c1, c2) if c]
    C = sum(cs)
    if op == 'conv1x1_multi_fwd':
        D.fit(Cin)
        return go([D(B, Cin, H, W), D(C, Cin, scale=0.2, filt=True)] + [torch.zeros(B, c, H, W) for c in cs] + cs + [B, Cin, H, W], [2, 3, 4])
    gys = [D(B, c, H, W, seed=3 + k, filt=True) for k, c in enumerate(cs)]
    if op == 'conv1x1_multi_dgrad':
        D.fit(C)
        return go([D(B, c, H, W, seed=3 + k) for k, c in enumerate(cs)] + [D(C, Cin, scale=0.2, filt=True), torch.zeros(B, Cin, H, W)] + cs + [B, Cin, H, W], [4])
    D.fit(B * H * W)
    x = D(B, Cin, H, W)
    if op == 'conv1x1_multi_wgrad':
        nbytes = K.conv1x1_multi_wgrad_workspace(*cs, B, Cin, H, W)
        return go([x] + gys + [torch.zeros(C, Cin), workspace(nbytes), nbytes] + cs + [B, Cin, H, W, 0], [4])
    assert op == 'conv1x1_wgrad_partials_batch'
    nbytes, nb_e = K.conv2d_wgrad_workspace(B, Cin, C, H, W, 1), E.conv2d_wgrad_workspace(B, Cin, C, H, W, 1)
    tail = list(cs) + [0] * (3 - len(cs)) + [B, Cin, H, W, 1, bias]
    ws_e = workspace(nb_e)
    gy_e = gys + [None] * (3 - len(cs))
    E.conv1x1_wgrad_partials_batch(torch.tensor([[t.data_ptr() if torch.is_tensor(t) else 0 for t in [x] + gy_e] + [ws_e.data_ptr(), nb_e] + tail],
                                                dtype=torch.int64), 1)
    dev = run_both(K, op, [HostTable([[x] + gy_e + [workspace(nbytes), nbytes] + tail], scratch=[(0, 4)]), 1], [], placement=pl, emulator=E)[0]
    row = [Per(ws_e, dev[(0, 4)].cpu()), torch.zeros(C, Cin), torch.zeros(C) if bias else None, B, Cin, C, H, W, 1, 0]
    outs = [(0, 1)] + ([(0, 2)] if bias else [])
    got = run_both(K, 'conv2d_wgrad_reduce_batch', [HostTable([row], outs=outs), 1], [], tol=tol, atol=atol, emulator=E)
    return [got[0][pos] for pos in outs]


@pytest.mark.parametrize('i', ROWS, ids=[f'{i}-{CASES[i][0][0]}-{"x".join(map(str, CASES[i][0][1][:6]))}' for i in ROWS])
def test_row(K, i):
    case, record, nbytes = CASES[i]
    assert S.query(case, (-1, -1, -1)) == record, f'{case}: this process ({ACTIVE}) would not launch what the ledger says'
    poison_lds(K)
    run_row(K, case, exact=False)
    for out in run_row(K, case, exact=True):
        assert float(out.abs().max()) < EXACT            # (the a-priori bound of Data.fit, seen on the result)


_FAILED_CHILD = []


@pytest.mark.parametrize('knob', [k for k in S.KNOBS if k != 'default'])
def test_other_knob_sets_in_a_child_each(knob):
    if ACTIVE != 'default':
        return                                            # (a child: its own rows are test_row above)
    assert not _FAILED_CHILD, f'not started: the child for {_FAILED_CHILD[0]} failed'
    _FAILED_CHILD.append(knob)
    n = sum(1 for case, _, _ in CASES if case[5] == knob)
    assert n > 0
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-x', '-q', '-k', 'test_row', '-p', 'no:cacheprovider'],
                       env=dict(os.environ, **S.KNOB_ENV[knob]), cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=60 + 2 * n)
    assert r.returncode == 0, r.stdout[-4000:]
    assert re.search(rf'^{n} passed[, ]', r.stdout, re.M), r.stdout[-500:]
    _FAILED_CHILD.clear()
