"""tg_skipgram_step, tg_embed_gather_t and tg_embed_lookup (csrc/text.hip) on the GPU, every call behind guard bands
(guarded.run_both), aligned and one element off, the smallest case with each pointer shifted alone.

The skip-gram step is compared with the reference's own formulas in float64 (embedding, bmm, logsigmoid, autograd, dense SGD with
the padding row masked: text_cases.skipgram_reference).  Tolerance, for the loss and for either table after the update: 4 * e32,
never below 2.4e-7, e32 being what the same ops are off in float32 on the CPU (text_cases.limit).  Every case runs at lr 4e-4 (the
trainer's) and at lr 1.0: at the small rate a wrong gradient hides under the table's own roundoff.

(This file sorts in front of test_guard_bands_gpu.py on purpose: that file's completeness test wants every entry point with a
pointer parameter to have gone through the guarded harness earlier in the same process.)"""
import math

import pytest
import torch

import guarded
import text_cases as TC
from guarded import run_both, workspace

pytestmark = pytest.mark.gpu
EMU = TC.TextEmulator()
LRS = (4e-4, 1.0)
OUTPUTS = ((7, 'loss'), (0, 'U'), (1, 'V'))


@pytest.fixture(scope='module')
def K():
    from tartangan_amd import backend
    prev = backend._set_backend_for_testing(None)
    yield backend.get()
    backend._set_backend_for_testing(prev)


def _args(K, c, lr, B, C2, E, vocab):
    nbytes = K.skipgram_workspace(B, C2, E)
    assert nbytes > 0
    return [c['U'], c['V'], c['words'], c['contexts'], c['negatives'], lr, c['padding_idx'], torch.zeros(()), workspace(nbytes), nbytes,
            B, C2, E, vocab]


def _run(K, c, lr, shape, placement, tag):
    B, C2, E, vocab = shape
    dev = run_both(K, 'skipgram_step', _args(K, c, lr, *shape), [0, 1, 7], accum=[0, 1], tol=2 * max(TC.limit(e) for e in c['e32']),
                   placement=placement, emulator=EMU)
    failures = []
    for (i, label), want, e32 in zip(OUTPUTS, c['want'], c['e32']):
        got = dev[i].cpu().double().reshape(want.shape)
        assert bool(torch.isfinite(got).all()), f'{tag} {label}: not finite'
        err, lim = TC.rel(got, want), TC.limit(e32)
        print(f'SKIPGRAM {tag} [{placement}] {label}: e32 {e32:.2e} kernel {err:.2e} limit {lim:.2e} share {err / lim:.2f}')
        if err > lim:
            failures.append(f'{label}: {err:.3e} > {lim:.3e} (e32 {e32:.3e})')
    tu, tv = TC.untouched_rows(c, vocab)
    for name, before, after, keep in (('U', c['U'], dev[0], tu), ('V', c['V'], dev[1], tv)):
        same = torch.equal(after.cpu().view(torch.int32)[keep], before.view(torch.int32)[keep])
        if not same:
            failures.append(f'{name}: a row that no index names (or the padding row) changed')
    assert not failures, (tag, placement, failures)


@pytest.mark.parametrize('lr', LRS)
@pytest.mark.parametrize('shape', TC.SKIPGRAM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_step_against_the_reference_formulas(K, shape, lr):
    c = TC.skipgram_case(*shape, lr)
    for pl in ['aligned', 'shifted'] + ([0, 1, 2, 3, 4, 7, 8] if shape == TC.SKIPGRAM_SHAPES[0] else []):
        _run(K, c, lr, shape, pl, f'{shape} lr={lr}')


@pytest.mark.parametrize('lr', LRS)
@pytest.mark.parametrize('variant,shape', [('same_word', (16, 4, 8, 23)), ('padding', (6, 4, 8, 23)), ('planted', (5, 2, 8, 23))])
def test_step_on_duplicates_padding_rows_and_saturated_scores(K, variant, shape, lr):
    c = TC.skipgram_case(*shape, lr, variant)
    if variant == 'planted':
        assert math.isfinite(float(c['want'][0]))
    for pl in ('aligned', 'shifted'):
        _run(K, c, lr, shape, pl, f'{variant} {shape} lr={lr}')


def test_two_runs_are_bit_identical(K):
    shape = (5, 4, 100, 7)
    B, C2, E, vocab = shape
    c = TC.skipgram_case(*shape, 1.0)
    nbytes = K.skipgram_workspace(B, C2, E)
    runs = []
    for _ in range(2):
        U, V = c['U'].cuda(), c['V'].cuda()
        loss, ws = torch.full((), float('nan'), device='cuda'), torch.full(((nbytes + 3) // 4,), float('nan'), device='cuda')
        K.skipgram_step(U, V, c['words'].cuda(), c['contexts'].cuda(), c['negatives'].cuda(), 1.0, -1, loss, ws, nbytes, B, C2, E, vocab)
        torch.cuda.synchronize()
        runs.append(torch.cat([U.view(-1), V.view(-1), loss.view(1)]).cpu().view(torch.int32))
    assert torch.equal(*runs)


def test_refusals_leave_everything_untouched(K):
    shape = (4, 6, 8, 23)
    B, C2, E, vocab = shape
    c = TC.skipgram_case(*shape, 1.0)
    args = _args(K, c, 1.0, *shape)
    short = list(args)
    short[8], short[9] = workspace(args[9] - 4), args[9] - 4
    run_both(K, 'skipgram_step', short, [0, 1, 7], accum=[0, 1], expect='rejected', emulator=EMU)
    assert K.skipgram_workspace(B, C2, 1025) == 0
    wide = [torch.zeros(vocab, 1025), torch.zeros(vocab, 1025)] + args[2:8] + [workspace(1 << 16), 1 << 16, B, C2, 1025, vocab]
    run_both(K, 'skipgram_step', wide, [0, 1, 7], accum=[0, 1], expect='rejected', emulator=EMU)


@pytest.mark.parametrize('B,L,E', [(1, 1, 1), (3, 7, 5), (4, 16, 64), (2, 40, 70)])
def test_gather_transposed_is_copy_exact(K, B, L, E):
    vocab = 11
    U = guarded.rnd(vocab, E, seed=4)
    idx = torch.randint(0, vocab, (B, L), generator=torch.Generator().manual_seed(B + L + E))
    pls = ['aligned', 'shifted'] + ([0, 1, 2] if (B, L, E) == (1, 1, 1) else [])
    run_both(K, 'embed_gather_t', [U, idx, torch.zeros(B, E, L), B, L, E, vocab], [2], atol=0.0, placement=pls, emulator=EMU)


@pytest.mark.parametrize('B,L,E,vocab', [(1, 1, 1, 2), (3, 7, 8, 23), (2, 16, 64, 1000)])
def test_lookup_against_float64_under_the_margin_condition(K, B, L, E, vocab):
    c = TC.lookup_case(B, L, E, vocab) if vocab > 2 else dict(U=torch.tensor([[1.], [2.]]), z=torch.tensor([[[3.]]]), want=torch.zeros(1, 1, dtype=torch.int64))
    if vocab > 2:
        assert TC.lookup_margin(c['U'], c['z']) >= TC.LOOKUP_MARGIN
    pls = ['aligned', 'shifted'] + ([0, 1, 2] if vocab == 2 else [])
    dev = run_both(K, 'embed_lookup', [c['U'], c['z'], torch.zeros(B, L, dtype=torch.int64), B, L, E, vocab], [2], atol=0.0, placement=pls,
                   emulator=EMU)
    assert torch.equal(dev[2].cpu(), c['want'])


def test_functional_layer_on_the_device(K):
    """functional.skipgram_step / embed_gather_t / embed_lookup and models.text.SkipGram over the same kernels."""
    from tartangan_amd.models.text import SkipGram
    shape = (4, 6, 8, 23)
    B, C2, E, vocab = shape
    c = TC.skipgram_case(*shape, 1.0, 'plain')
    m = SkipGram(vocab, E, sparse=True, padding_idx=0).cuda()
    assert list(m.state_dict()) == ['embedding_u.weight', 'embedding_v.weight']
    m.load_state_dict({'embedding_u.weight': c['U'], 'embedding_v.weight': c['V']})
    want = TC.skipgram_reference(c['U'], c['V'], c['words'], c['contexts'], c['negatives'], 1.0, 0, torch.float64)
    loss = m.train_step(c['words'], c['contexts'], c['negatives'], 1.0)
    assert abs(float(loss) - float(want[0])) <= 1e-5 * abs(float(want[0]))
    assert TC.rel(m.embedding_u.weight.detach().cpu(), want[1]) <= 1e-5 and TC.rel(m.embedding_v.weight.detach().cpu(), want[2]) <= 1e-5
    idx = torch.randint(0, vocab, (3, 5), generator=torch.Generator().manual_seed(1))
    assert torch.equal(m.gather_t(idx.cuda()).cpu(), m.embedding_u.weight.detach().cpu()[idx].permute(0, 2, 1))
    lc = TC.lookup_case(3, 7, E, vocab)
    m.embedding_u.weight.data.copy_(lc['U'])
    assert torch.equal(torch.stack(m.lookup(lc['z'].cuda())).cpu(), lc['want'])


def test_the_entry_points_went_through_the_guarded_harness():
    assert {'skipgram_step', 'embed_gather_t', 'embed_lookup'} <= guarded.SEEN
