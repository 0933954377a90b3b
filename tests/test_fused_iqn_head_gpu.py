"""tg_iqn_head_fwd / tg_iqn_head_bwd (csrc/iqnhead.hip) on the GPU, every call behind guard bands (guarded.run_both), aligned and one
element off, against float64 autograd of the head restated in plain torch ops (shared_iqn_cases.head_ref).

Tolerance, per case and per output: let e32 be the error the SAME ATen ops make in float32 on the CPU against the float64 result
(largest absolute difference over the largest absolute reference value).  The kernel may be off by at most 4 * e32 and never has
to beat 2.4e-7, four fp32 roundoffs (shared_cases.limit).  Each case prints e32, the kernel's error and its share of the limit
(pytest -s; the table is in DESIGN.md, f8).

(This file sorts in front of test_guard_bands_gpu.py on purpose: that file's completeness test wants every entry point with a
pointer parameter to have gone through the guarded harness earlier in the same process.)"""

import pytest
import torch

import guarded
import shared_iqn_cases as SI
from guarded import run_both

pytestmark = pytest.mark.gpu
EMU = SI.SharedIQNEmulator()

# (G, B, Q, C, D)
SHAPES = [(1, 1, 1, 1, 1),
          (1, 1, 8, 1, 20),
          (2, 1, 8, 3, 20),
          (1, 3, 8, 65, 20),         # one channel past a wave
          (1, 5, 3, 257, 7),         # odd everything, one channel past a 256-thread workgroup
          (2, 4, 8, 64, 20),         # config '16'
          (2, 64, 8, 128, 20),       # the benched size
          (2, 8, 8, 1024, 20)]       # '128big'
COTANGENTS = [(True, False), (False, True), (True, True)]          # (gl, gpt)
_id = lambda s: 'x'.join(map(str, s))


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(None)
    yield backend.get()
    backend._set_backend_for_testing(prev)


def _fwd_args(K, c, targets=True):
    G, B, Q, C, D = (c[n] for n in 'GBQCD')
    return [c['f'], c['taus'], c['t'] if targets else None, c['W1'], c['b1'], c['w2'], c['b2'], c['range'], c['k'], torch.zeros(G * B, 1),
            torch.zeros(()) if targets else None, torch.zeros(G * Q * B) if targets else None,
            guarded.workspace(K.iqn_head_workspace(G, B)) if targets else None, G, B, Q, C, D]


def _bwd_args(c, use_gl, use_gpt, params=True, accumulate=0):
    G, B, Q, C, D = (c[n] for n in 'GBQCD')
    dpreds = c['variants'][True, True][0]['dpreds'].float()          # (fp32 of the float64 truth: an input here)
    grads = [torch.zeros(C, D), torch.zeros(C), torch.zeros(1, C), torch.zeros(1)] if params else [None] * 4
    return [c['gl'] if use_gl else None, c['gpt'] if use_gpt else None, dpreds if use_gl else None, c['f'], c['taus'], c['W1'], c['b1'],
            c['w2'], c['range'], torch.zeros(G * B, C), *grads, G, B, Q, C, D, accumulate]


def _report(tag, shape, what, placement, pairs):
    """pairs: (label, got, want, e32) -> failures; prints the table line of each."""
    failures = []
    for label, got, want, e32 in pairs:
        err, lim = SI._rel(got.cpu().double().reshape(-1), want.reshape(-1)), SI.limit(e32)
        print(f'IQNHEAD {tag} {_id(shape)} {what} [{placement}] {label}: e32 {e32:.2e} kernel {err:.2e} limit {lim:.2e} share {err / lim:.2f}')
        if err > lim:
            failures.append(f'{label}: {err:.3e} > {lim:.3e} (e32 {e32:.3e})')
    return failures


@pytest.mark.parametrize('placement', ['aligned', 'shifted'])
@pytest.mark.parametrize('targets', [True, False], ids=['targets', 'sampling'])
@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_head_forward(K, shape, targets, placement):
    c = SI.head_case(*shape)
    want, e32 = c['variants'][True, True]
    names = SI.OUTPUTS_FWD if targets else ('pt',)
    loosest = max(SI.limit(e32[n]) for n in names)
    dev = run_both(K, 'iqn_head_fwd', _fwd_args(K, c, targets), [9, 10, 11] if targets else [9], tol=2 * loosest + 1e-5,
                   placement=placement, emulator=EMU)
    failures = _report('fwd', shape, 'targets' if targets else 'sampling', placement,
                       [(n, dev[i], want[n], e32[n]) for n, i in zip(names, (9, 10, 11))])
    assert not failures, (shape, targets, placement, failures)


@pytest.mark.parametrize('placement', ['aligned', 'shifted'])
@pytest.mark.parametrize('params', [True, False], ids=['params', 'df-only'])
@pytest.mark.parametrize('cot', COTANGENTS, ids=['gl', 'gpt', 'gl+gpt'])
@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_head_backward(K, shape, cot, params, placement):
    c = SI.head_case(*shape)
    want, e32 = c['variants'][cot]
    names = SI.OUTPUTS_BWD if params else ('df',)
    outs = [9, 10, 11, 12, 13] if params else [9]
    loosest = max(SI.limit(e32[n]) for n in names)
    dev = run_both(K, 'iqn_head_bwd', _bwd_args(c, *cot, params=params), outs, tol=2 * loosest + 1e-5, placement=placement, emulator=EMU)
    what = ('gl' if cot[0] else '') + ('+' if all(cot) else '') + ('gpt' if cot[1] else '') + ('' if params else ' df-only')
    failures = _report('bwd', shape, what, placement, [(n, dev[i], want[n], e32[n]) for n, i in zip(names, outs)])
    assert not failures, (shape, cot, params, placement, failures)


@pytest.mark.parametrize('shape', SHAPES[:3], ids=_id)
def test_smallest_shapes_with_each_pointer_shifted_alone(K, shape):
    c = SI.head_case(*shape)
    tol = 2 * max(SI.limit(e) for e in c['e32'].values()) + 1e-5
    run_both(K, 'iqn_head_fwd', _fwd_args(K, c), [9, 10, 11], tol=tol, placement=[0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12], emulator=EMU)
    run_both(K, 'iqn_head_bwd', _bwd_args(c, True, True), [9, 10, 11, 12, 13], tol=tol, placement=list(range(14)), emulator=EMU)


@pytest.mark.parametrize('shape', [SHAPES[2], SHAPES[5]], ids=_id)
def test_accumulate_adds_to_the_parameter_gradients_and_overwrites_df(K, shape):
    c = SI.head_case(*shape)
    args = _bwd_args(c, True, True, accumulate=1)
    for i, seed in zip((10, 11, 12, 13), range(4)):
        args[i] = guarded.rnd(*args[i].shape, seed=seed)
    tol = 2 * max(SI.limit(e) for e in c['e32'].values()) + 1e-5
    run_both(K, 'iqn_head_bwd', args, [9, 10, 11, 12, 13], tol=tol, accum=[10, 11, 12, 13], placement=['aligned', 'shifted'], emulator=EMU)


def test_huber_branch_edges_are_the_references(K):
    """w2 = 0: p = b2 exactly in any summation order; targets b2, b2 + k, b2 - k make err exactly 0, +k, -k.  |err| <= k is the
    quadratic branch (k included), err < 0 is strict (err == 0 weighs |tau - 0|)."""
    G, B, Q, C, D, k = 1, 3, 8, 5, 20, 0.5
    c = dict(SI.head_case(G, B, Q, C, D))
    b2 = torch.tensor([0.25])
    t = torch.tensor([0.25, 0.75, -0.25])
    assert (t - b2).tolist() == [0.0, k, -k]
    c.update(w2=torch.zeros(1, C), b2=b2, t=t, k=k)
    taus = c['taus'].reshape(Q, B)
    err = (t - b2).reshape(1, B).expand(Q, B).double()
    quad = 0.5 * err * err                                     # every row is on the quadratic side, k included
    assert torch.equal(quad[:, 1:], torch.full((Q, 2), 0.5 * k * k, dtype=torch.float64))
    wgt = (taus.double() - (err < 0).double()).abs()
    want_loss = (wgt * quad).sum(0).mean().reshape(1)
    want_dp = (-wgt * err / B).reshape(-1)
    dev = run_both(K, 'iqn_head_fwd', _fwd_args(K, c), [9, 10, 11], tol=1e-6, emulator=EMU)
    assert torch.equal(dev[9].cpu().reshape(-1), b2.expand(B))
    assert SI._rel(dev[10].cpu().double().reshape(1), want_loss) <= 1e-6
    assert SI._rel(dev[11].cpu().double(), want_dp) <= 1e-6
    print(f'IQNHEAD edges: loss {float(dev[10]):.8f} want {float(want_loss):.8f}')


def test_taus_at_zero_and_just_below_one(K):
    shape = (1, 3, 8, 65, 20)
    c = dict(SI.head_case(*shape))
    top = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
    assert top < 1.0
    taus = c['taus'].clone()
    taus[::2], taus[1::2] = 0.0, top
    c['taus'] = taus
    c['variants'] = {}
    want, r32 = SI.head_outputs(c, torch.float64), SI.head_outputs(c, torch.float32)
    e32 = {n: SI._rel(r32[n], want[n]) for n in want}
    c['variants'][True, True] = (want, e32)
    tol = 2 * max(SI.limit(e) for e in e32.values()) + 1e-5
    dev = run_both(K, 'iqn_head_fwd', _fwd_args(K, c), [9, 10, 11], tol=tol, emulator=EMU)
    failures = _report('fwd', shape, 'taus 0 | 1-', 'aligned', [(n, dev[i], want[n], e32[n]) for n, i in zip(SI.OUTPUTS_FWD, (9, 10, 11))])
    dev = run_both(K, 'iqn_head_bwd', _bwd_args(c, True, True), [9, 10, 11, 12, 13], tol=tol, emulator=EMU)
    failures += _report('bwd', shape, 'taus 0 | 1-', 'aligned', [(n, dev[i], want[n], e32[n]) for n, i in zip(SI.OUTPUTS_BWD, range(9, 14))])
    assert not failures, failures


@pytest.mark.parametrize('shape', SHAPES[-2:], ids=_id)
def test_two_runs_are_bit_identical(K, shape):
    G, B, Q, C, D = shape
    c = SI.head_case(*shape)
    dv = {n: c[n].cuda() for n in ('f', 'taus', 't', 'W1', 'b1', 'w2', 'b2', 'range', 'gl', 'gpt')}
    ws = torch.empty((K.iqn_head_workspace(G, B) + 3) // 4, device='cuda')
    nan = lambda *s: torch.full(s, float('nan'), device='cuda')
    runs = []
    for _ in range(2):
        pt, loss, dpreds = nan(G * B, 1), nan(1), nan(G * Q * B)
        ws.fill_(float('nan'))
        K.iqn_head_fwd(dv['f'], dv['taus'], dv['t'], dv['W1'], dv['b1'], dv['w2'], dv['b2'], dv['range'], 1.0, pt, loss, dpreds, ws, *shape)
        df, dW1, db1, dw2, db2 = nan(G * B, C), nan(C, D), nan(C), nan(1, C), nan(1)
        K.iqn_head_bwd(dv['gl'], dv['gpt'], dpreds, dv['f'], dv['taus'], dv['W1'], dv['b1'], dv['w2'], dv['range'], df, dW1, db1, dw2, db2,
                       *shape, 0)
        torch.cuda.synchronize()
        flat = torch.cat([t.reshape(-1) for t in (pt, loss, dpreds, df, dW1, db1, dw2, db2)]).cpu()
        assert not bool(torch.isnan(flat).any())
        runs.append(flat.view(torch.int32))
    assert torch.equal(*runs)


FWD_BAD = ['G0', 'G3', 'B0', 'Q0', 'C0', 'D0', 'D21', 'null f', 'null taus', 'null W1', 'null b1', 'null w2', 'null range', 'null pt',
           'targets without loss', 'targets without dpreds']
BWD_BAD = ['G0', 'G3', 'B0', 'Q0', 'C0', 'D0', 'D21', 'null f', 'null taus', 'null W1', 'null b1', 'null w2', 'null range', 'gl without dpreds']


def _bad_dims(form, shape):
    G, B, Q, C, D = shape
    return {'G0': (0, B, Q, C, D), 'G3': (3, B, Q, C, D), 'B0': (G, 0, Q, C, D), 'Q0': (G, B, 0, C, D), 'C0': (G, B, Q, 0, D),
            'D0': (G, B, Q, C, 0), 'D21': (G, B, Q, C, 21)}.get(form, shape)


@pytest.mark.parametrize('form', FWD_BAD)
def test_forward_rejects_bad_arguments_with_nothing_written(K, form):
    shape = (2, 1, 8, 3, 20)
    args = _fwd_args(K, SI.head_case(*shape))
    names = [p[1] for p in guarded.params_of('iqn_head_fwd')]
    if form.startswith('null '):
        args[names.index(form[5:])] = None
    if form.startswith('targets without '):
        args[names.index(form[16:])] = None
    args[13:18] = _bad_dims(form, shape)
    run_both(K, 'iqn_head_fwd', args, [i for i in (9, 10, 11) if args[i] is not None], expect='rejected', emulator=EMU)


@pytest.mark.parametrize('form', BWD_BAD)
def test_backward_rejects_bad_arguments_with_nothing_written(K, form):
    shape = (2, 1, 8, 3, 20)
    args = _bwd_args(SI.head_case(*shape), True, True)
    names = [p[1] for p in guarded.params_of('iqn_head_bwd')]
    if form.startswith('null '):
        args[names.index(form[5:])] = None
    if form == 'gl without dpreds':
        args[2] = None
    args[14:19] = _bad_dims(form, shape)
    run_both(K, 'iqn_head_bwd', args, [9, 10, 11, 12, 13], expect='rejected', emulator=EMU)


# ------------------------------------------------------------------------------------------- functional.iqn_head on the device
def _device_function_outputs(c, paired, misalign=False):
    from tartangan_amd import functional as TF
    G, B, Q, C = c['G'], c['B'], c['Q'], c['C']
    if misalign:
        buf = torch.zeros(G * B * C + 1, device='cuda')
        buf[1:] = c['f'].cuda().reshape(-1)
        f = buf[1:].view(G * B, C).requires_grad_(True)
        assert f.data_ptr() % 16 == 4
    else:
        f = c['f'].cuda().requires_grad_(True)
    W1, b1, w2, b2 = (c[n].cuda().requires_grad_(True) for n in ('W1', 'b1', 'w2', 'b2'))
    gpt = c['gpt'].cuda().reshape(G * B, 1).requires_grad_(True)
    t, taus, rng = c['t'].cuda().reshape(G * B, 1), c['taus'].cuda(), c['range'].cuda()
    if paired:
        pt, loss = TF.iqn_head(TF.Pair(f[:B], f[B:]), TF.Pair(taus[:Q * B].reshape(-1, 1), taus[Q * B:].reshape(-1, 1)), t, W1, b1, w2, b2, rng, Q, c['k'])
        weighted = (gpt[:B] * pt.r).sum() + (gpt[B:] * pt.f).sum()
        pt = torch.cat([pt.r, pt.f])
    else:
        pt, loss = TF.iqn_head(f, taus.reshape(-1, 1), t, W1, b1, w2, b2, rng, Q, c['k'])
        weighted = (gpt * pt).sum()
    df, dW1, db1, dw2, db2 = torch.autograd.grad(c['gl'].cuda() * loss + weighted, (f, W1, b1, w2, b2), create_graph=True)
    second = torch.autograd.grad((c['v'].cuda() * df).sum(), (gpt, W1, b1, w2))
    out = dict(pt=pt, loss=loss, df=df, dW1=dW1, db1=db1, dw2=dw2, db2=db2)
    out.update(zip(SI.OUTPUTS_DBWD, second))
    return out


@pytest.mark.parametrize('shape,misalign', [((1, 3, 8, 65, 20), False), ((1, 5, 3, 257, 7), True), ((2, 4, 8, 64, 20), False),
                                            ((2, 64, 8, 128, 20), False)], ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_function_first_and_second_order_on_the_device(K, shape, misalign):
    c = SI.head_case(*shape)
    want, e32 = c['variants'][True, True]
    got = _device_function_outputs(c, paired=shape[0] == 2, misalign=misalign)
    failures = _report('TF', shape, 'misaligned f' if misalign else 'function', 'device', [(n, g.detach(), want[n], e32[n]) for n, g in got.items()])
    assert not failures, failures


def test_function_on_a_pair_whose_real_half_alone_is_differentiated(K):
    """The R1 pattern: grad(pt.r.sum(), f_r, create_graph) and the parameter gradients of a function of it, against float64 of the
    real half as an evaluation of its own (G = 1)."""
    from tartangan_amd import functional as TF
    G, B, Q, C, D = shape = (2, 4, 8, 64, 20)
    c = SI.head_case(*shape)
    f_r, f_f = (x.cuda().requires_grad_(True) for x in (c['f'][:B], c['f'][B:]))
    W1, b1, w2, b2 = (c[n].cuda().requires_grad_(True) for n in ('W1', 'b1', 'w2', 'b2'))
    taus = c['taus'].cuda()
    pt, loss = TF.iqn_head(TF.Pair(f_r, f_f), TF.Pair(taus[:Q * B].reshape(-1, 1), taus[Q * B:].reshape(-1, 1)), c['t'].cuda().reshape(-1, 1),
                           W1, b1, w2, b2, c['range'].cuda(), Q)
    g_r, = torch.autograd.grad(pt.r.sum(), f_r, create_graph=True)
    assert f_f.grad is None
    got = torch.autograd.grad(g_r.pow(2).sum(), (W1, b1, w2))

    def both(dtype):
        fr, W, b, w, bb = (c[n][:B].to(dtype).requires_grad_(True) if n == 'f' else c[n].to(dtype).requires_grad_(True)
                           for n in ('f', 'W1', 'b1', 'w2', 'b2'))
        _, ptr = SI.head_ref(fr, c['taus'][:Q * B].to(dtype), W, b, w, bb, c['range'].to(dtype), 1, B, Q)
        g, = torch.autograd.grad(ptr.sum(), fr, create_graph=True)
        return [g.detach().double()] + [x.double() for x in torch.autograd.grad(g.pow(2).sum(), (W, b, w))]
    want, r32 = both(torch.float64), both(torch.float32)
    pairs = [(n, g.detach(), w_, SI._rel(r, w_)) for n, g, w_, r in zip(('df_r', 'd_W1', 'd_b1', 'd_w2'), (g_r,) + tuple(got), want, r32)]
    failures = _report('TF', shape, 'real half alone', 'device', pairs)
    assert not failures, failures


def test_both_entry_points_went_through_the_guarded_harness():
    assert {'iqn_head_fwd', 'iqn_head_bwd'} <= guarded.SEEN
