"""tg_sn_batch_workspace / tg_sn_batch_fwd / tg_sn_batch_bwd (csrc/spectral.hip) on the GPU, every call behind guard bands
(guarded.run_both: outputs and workspaces handed over NaN-filled), aligned and one element off, the smallest case with each pointer
shifted alone.  Truth is float64 torch (``F.normalize``, ``mv``, ``dot``, autograd through ``W / dot(u, W v)``); ``e32`` is what the
same ops are off in fp32 on the CPU; the limit is the house rule ``e_op <= 4 max(e32, 2.4e-7)`` relative to the tensor's largest
magnitude, for u, v, sigma, w_sn and g_orig.

One call covers six layers of unequal size, so the (layer, tile) mapping of every stage is exercised.  The kernels tile by 64-row
slabs and 256-column chunks (W^T u) and by 2048-element chunks (the element-wise stages): 70 x 333 has two slabs with a ragged last
one and two column chunks with a ragged tail on the scalar path (cols % 4 != 0), 128 x 1152 and 256 x 2304 several whole slabs and
a ragged column tail on the float4 path, 72 x 260 (a case of its own) the ragged slab and tail on the float4 path."""
import pytest
import torch

import guarded
from guarded import HostTable, run_both, workspace
from spectral_cases import EMU, SHAPES, SN_COLS, SN_ELEMS, SN_SLAB, bwd_formula, limit, low_rank, make_layers, reference_fwd, rel

pytestmark = pytest.mark.gpu
EPS = 1e-12


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    backend._set_backend_for_testing(None)
    return backend.get()


def nbytes_of(K, layers):
    t = torch.tensor([[256] * 6 + [L['rows'], L['cols']] for L in layers], dtype=torch.int64)
    return K.sn_batch_workspace(t, len(layers))


def run_fwd(K, layers, update, placement='aligned'):
    """-> per layer (u, v, w_sn) and sigma as the device left them (CPU copies)."""
    n = len(layers)
    rows = [[L['W'], L['u'], L['v'], torch.zeros_like(L['W']), None, None, L['rows'], L['cols']] for L in layers]
    rmw = [(r, c) for r in range(n) for c in (1, 2)] if update else []
    tab = HostTable(rows, outs=rmw + [(r, 3) for r in range(n)], accum=rmw, tol=1e-5)
    nbytes = nbytes_of(K, layers)
    out = run_both(K, 'sn_batch_fwd', [tab, n, torch.zeros(n), workspace(nbytes), nbytes, update, EPS], [2], tol=1e-5,
                   placement=placement, emulator=EMU)
    return [tuple(out[0][(r, c)].cpu() for c in (1, 2, 3)) for r in range(n)], out[2].cpu()


def run_bwd(K, layers, truth, clear, placement='aligned'):
    """-> per layer (g_sn, g_orig) as the device left them; w_sn and sigma are the float64 truth rounded to fp32."""
    n = len(layers)
    rows = [[L['W'], T['u'].float(), T['v'].float(), T['w_sn'].float(), L['g_sn'], L['g_orig'], L['rows'], L['cols']]
            for L, T in zip(layers, truth)]
    rmw = [(r, 5) for r in range(n)] + ([(r, 4) for r in range(n)] if clear else [])
    tab = HostTable(rows, outs=rmw, accum=rmw, tol=1e-5)
    nbytes = nbytes_of(K, layers)
    sigma = torch.stack([T['sigma'] for T in truth]).float()
    out = run_both(K, 'sn_batch_bwd', [tab, n, sigma, workspace(nbytes), nbytes, clear], [], tol=1e-5, placement=placement, emulator=EMU)
    return [tuple(out[0][(r, c)].cpu() for c in (4, 5)) for r in range(n)]


def truths(layers, update):
    out = []
    for L in layers:
        t64 = dict(zip(('u', 'v', 'sigma', 'w_sn'), reference_fwd(L['W'], L['u'], L['v'], update, EPS, torch.float64)))
        t32 = dict(zip(('u', 'v', 'sigma', 'w_sn'), reference_fwd(L['W'], L['u'], L['v'], update, EPS, torch.float32)))
        t64['e32'] = {k: rel(t32[k].reshape(-1), t64[k].reshape(-1)) for k in t32}
        # the backward of exactly what the kernel is handed: the fp32-rounded truth of the forward
        args = (L['g_sn'], t64['w_sn'].float(), t64['u'].float(), t64['v'].float(), t64['sigma'].float())
        g64 = L['g_orig'].double() + bwd_formula(*args, torch.float64)
        g32 = L['g_orig'] + bwd_formula(*args, torch.float32)
        t64['g_orig'], t64['e32']['g_orig'] = g64, rel(g32, g64)
        out.append(t64)
    return out


def check(tag, L, T, got):
    for k, g in got.items():
        e, e32 = rel(g.reshape(-1), T[k].reshape(-1)), T['e32'][k]
        print(f'SN {tag} {L["rows"]}x{L["cols"]} {k}: e32 {e32:.2e} kernel {e:.2e} limit {limit(e32):.2e}')
        assert e <= limit(e32), (tag, L['rows'], L['cols'], k, e, e32)


@pytest.fixture(scope='module')
def six():
    layers = make_layers(SHAPES)
    t1 = truths(layers, 1)
    # without an update the kernel reads STORED u and v, which have been iterated: sigma = u^T W v of a random pair is a sum that
    # cancels to ~1/sqrt(cols) of its terms, a case that no forward of a network produces
    stored = [dict(L, u=T['u'].float(), v=T['v'].float()) for L, T in zip(layers, t1)]
    return layers, t1, (stored, truths(stored, 0))


def test_tile_coverage_of_the_case_set():
    assert (SN_SLAB, SN_COLS, SN_ELEMS) == (64, 256, 2048)
    assert any(r > SN_SLAB and r % SN_SLAB for r, c in SHAPES) and any(c > SN_COLS and c % SN_COLS for r, c in SHAPES)
    assert any(c % 4 for r, c in SHAPES) and any(r * c > SN_ELEMS and (r * c) % SN_ELEMS for r, c in SHAPES)


@pytest.mark.parametrize('placement', ['aligned', 'shifted'])
def test_forward_with_update_six_layers_in_one_call(K, six, placement):
    layers, t1, _ = six
    got, sigma = run_fwd(K, layers, 1, placement)
    for i, (L, T) in enumerate(zip(layers, t1)):
        check(f'fwd update=1 {placement}', L, T, dict(u=got[i][0], v=got[i][1], w_sn=got[i][2], sigma=sigma[i]))


@pytest.mark.parametrize('placement', ['aligned', 'shifted'])
def test_forward_without_update_reads_u_and_v_only(K, six, placement):
    """run_both fails the call if an input (here u and v) is not bit-identical afterwards."""
    _, _, (layers, t0) = six
    got, sigma = run_fwd(K, layers, 0, placement)
    for i, (L, T) in enumerate(zip(layers, t0)):
        check(f'fwd update=0 {placement}', L, T, dict(w_sn=got[i][2], sigma=sigma[i]))


@pytest.mark.parametrize('clear', [1, 0])
@pytest.mark.parametrize('placement', ['aligned', 'shifted'])
def test_backward_accumulates_into_a_nonzero_gradient(K, six, placement, clear):
    """clear = 1 leaves g_sn exact zeros; clear = 0 leaves it untouched (an input to run_both: compared bit for bit)."""
    layers, t1, _ = six
    got = run_bwd(K, layers, t1, clear, placement)
    for i, (L, T) in enumerate(zip(layers, t1)):
        check(f'bwd clear={clear} {placement}', L, T, dict(g_orig=got[i][1]))
        if clear:
            assert not got[i][0].view(torch.int32).any(), 'g_sn is not all (positive) zeros'


def test_two_runs_and_the_two_paths_are_bit_identical(K, six):
    layers, t1, _ = six
    runs = [run_fwd(K, layers, 1, p) for p in ('aligned', 'aligned', 'shifted')]
    grads = [run_bwd(K, layers, t1, 1, p) for p in ('aligned', 'aligned', 'shifted')]
    for other in (1, 2):
        assert torch.equal(runs[0][1].view(torch.int32), runs[other][1].view(torch.int32))
        for a, b in zip(runs[0][0] + grads[0], runs[other][0] + grads[other]):
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_single_item_of_one_by_one_each_pointer_shifted_alone(K):
    layers = make_layers([(1, 1)], seed=3)
    t1 = truths(layers, 1)
    pls = ['aligned', 'shifted', 2, 3]
    for pl in pls:
        got, sigma = run_fwd(K, layers, 1, pl)
        check(f'fwd 1x1 {pl}', layers[0], t1[0], dict(u=got[0][0], v=got[0][1], w_sn=got[0][2], sigma=sigma[0]))
        g = run_bwd(K, layers, t1, 1, pl)
        check(f'bwd 1x1 {pl}', layers[0], t1[0], dict(g_orig=g[0][1]))
    tab = HostTable([[L['W'], L['u'], L['v'], torch.zeros_like(L['W']), None, None, 1, 1] for L in layers])
    run_both(K, 'sn_batch_workspace', [tab, 1], [], emulator=EMU)
    assert nbytes_of(K, layers) >= 12


def test_float4_path_with_a_ragged_slab_and_a_ragged_column_tail(K):
    layers = make_layers([(72, 260), (5, 8)], seed=5)
    t1 = truths(layers, 1)
    got, sigma = run_fwd(K, layers, 1)
    grads = run_bwd(K, layers, t1, 1)
    for i, (L, T) in enumerate(zip(layers, t1)):
        check('fwd ragged float4', L, T, dict(u=got[i][0], v=got[i][1], w_sn=got[i][2], sigma=sigma[i], g_orig=grads[i][1]))


@pytest.mark.parametrize('rows,cols', [(16, 27), (128, 1152)])
def test_three_updates_reach_the_largest_singular_value(K, rows, cols):
    W = low_rank(rows, cols)
    L = make_layers([(rows, cols)], seed=9)[0]
    top = torch.linalg.svdvals(W.double())[0]
    u32, v32, s32 = L['u'], L['v'], None
    for _ in range(3):
        u32, v32, s32, _ = reference_fwd(W, u32, v32, 1, EPS, torch.float32)
    e32 = abs(float(s32) - float(top)) / float(top)
    dev = dict(W=W.cuda(), u=L['u'].cuda(), v=L['v'].cuda(), w_sn=torch.empty(rows, cols, device='cuda'))
    items = torch.tensor([[dev['W'].data_ptr(), dev['u'].data_ptr(), dev['v'].data_ptr(), dev['w_sn'].data_ptr(), 0, 0, rows, cols]],
                         dtype=torch.int64)
    nbytes = K.sn_batch_workspace(items, 1)
    ws, sigma = torch.empty(nbytes // 4 + 1, device='cuda'), torch.zeros(1, device='cuda')
    for _ in range(3):
        K.sn_batch_fwd(items, 1, sigma, ws, nbytes, 1, EPS)
    e = abs(float(sigma[0]) - float(top)) / float(top)
    print(f'SN convergence {rows}x{cols}: top {float(top):.6f} e32 {e32:.2e} kernel {e:.2e} limit {limit(e32):.2e}')
    assert e <= limit(e32)


def test_covered():
    assert {'sn_batch_workspace', 'sn_batch_fwd', 'sn_batch_bwd'} <= guarded.SEEN
