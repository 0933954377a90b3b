"""Helpers of the text kernels' tests (not collected).

* ``TextEmulator``: ``tests/emulator.Emulator`` plus float64 forms (rounded to the output's dtype) of the entry points of
  csrc/conv1d.hip and csrc/text.hip, written from the header's formulas and the reference's ops (``F.conv1d``, ``F.embedding``,
  ``bmm``, ``logsigmoid``, dense SGD -- what the sparse gradient + ``coalesce`` + ``optim.SGD`` compute).
* ``conv_case`` / ``skipgram_case`` / ``lookup_case``: inputs of one case, the float64 truth and ``e32``, the error the same
  ATen ops make in float32 on the CPU on the same inputs; ``limit``: the house rule of ``shared_cases.limit``.
* ``text_trainer`` / ``load_text_fixture`` / ``load_procedural`` / ``documents``: the trainer and the batches a
  ``tests/golden/text_*.json`` fixture describes."""
import functools
import json
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from emulator import Emulator


def limit(e32):
    """At most 4 x what the same ATen ops are off in fp32 on the same inputs (relative to the largest reference value), and
    never less than 4 fp32 roundoffs."""
    return max(4 * e32, 2.4e-7)


def rel(got, want):
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    return err / scale if scale > 0 else err


# ------------------------------------------------------------------------------------------------------------- emulator
def _logsigmoid(s):
    return torch.clamp(s, max=0) - torch.log1p(torch.exp(-s.abs()))


def skipgram_reference(U, V, words, contexts, negatives, lr, padding_idx, dtype):
    """-> loss, U', V' with the reference's ops in ``dtype``: embedding, bmm, logsigmoid, autograd, dense SGD; the rows equal to
    padding_idx get no gradient (nn.Embedding(padding_idx=...))."""
    u = U.detach().to(dtype).clone().requires_grad_(True)
    v = V.detach().to(dtype).clone().requires_grad_(True)
    pad = padding_idx if padding_idx is not None and padding_idx >= 0 else None
    with torch.enable_grad():
        emb_u = F.embedding(words, u, padding_idx=pad)
        pos = torch.bmm(F.embedding(contexts, v, padding_idx=pad), emb_u.unsqueeze(-1)).squeeze(-1)
        neg = torch.bmm(F.embedding(negatives, v, padding_idx=pad), emb_u.unsqueeze(-1)).squeeze(-1)
        loss = -(F.logsigmoid(pos).sum(1) + F.logsigmoid(-neg).sum(1)).mean()
        gu, gv = torch.autograd.grad(loss, (u, v))
    return loss.detach(), (u - lr * gu).detach(), (v - lr * gv).detach()


def lookup_reference(U, z, dtype=torch.float64):
    w = U.to(dtype)
    w_norm = w.pow(2).sum(1).sqrt()[..., None]
    scores = torch.stack([torch.mm(w, zi) / w_norm for zi in z.to(dtype)])          # (B, vocab, L)
    return scores[:, 1:]


class TextEmulator(Emulator):
    def conv1d_supported(self, B, Cin, Cout, L, ks):
        return int(min(B, Cin, Cout, L) > 0 and ks in (1, 3))

    def conv1d_fwd(self, x, w, bias, residual, y, B, Cin, Cout, L, ks):
        r = F.conv1d(x.view(B, Cin, L).double(), w.view(Cout, Cin, ks).double(), None if bias is None else bias.double(), padding=ks // 2)
        if residual is not None:
            r = r + residual.view(B, Cout, L).double()
        y.copy_(r.to(y.dtype).view(y.shape))
        return 0

    def conv1d_dgrad(self, gy, w, gx, B, Cin, Cout, L, ks):
        r = F.conv_transpose1d(gy.view(B, Cout, L).double(), w.view(Cout, Cin, ks).double(), padding=ks // 2)
        gx.copy_(r.to(gx.dtype).view(gx.shape))
        return 0

    def conv1d_wgrad_workspace(self, B, Cin, Cout, L, ks):
        return 4 * Cout * (Cin * ks + 1) if ks in (1, 3) else 0

    def conv1d_wgrad(self, x, gy, gw, gbias, ws, ws_bytes, B, Cin, Cout, L, ks, accumulate):
        xp = F.pad(x.view(B, Cin, L).double(), (ks // 2, ks // 2))
        g = gy.view(B, Cout, L).double()
        r = torch.stack([torch.einsum('bol,bil->oi', g, xp[:, :, t:t + L]) for t in range(ks)], dim=2)
        gw.copy_(((gw.double().view(Cout, Cin, ks) if accumulate else 0) + r).to(gw.dtype).view(gw.shape))
        if gbias is not None:
            gbias.copy_(((gbias.double() if accumulate else 0) + g.sum((0, 2))).to(gbias.dtype))
        return 0

    def up2x1d(self, x, y, alpha, BC, L):
        # alpha as the fp32 value the C ABI receives, one rounding: bit-exact against the kernel
        a = float(torch.tensor(alpha, dtype=torch.float32)) if x.dtype == torch.float32 else alpha
        y.copy_((x.view(BC, L) * a).repeat_interleave(2, dim=1).view(y.shape))
        return 0

    def pool2_1d(self, x, residual, y, BC, L):
        p = 0.5 * (x.view(BC, L, 2).double()[:, :, 0] + x.view(BC, L, 2).double()[:, :, 1])
        if residual is not None:
            p = p + residual.view(BC, L).double()
        y.copy_(p.to(y.dtype).view(y.shape))
        return 0

    def skipgram_workspace(self, B, C2, E):
        return 4 * (B + 2 * B * C2 + 2 * B * E)

    def skipgram_step(self, U, V, words, contexts, negatives, lr, padding_idx, loss_out, ws, ws_bytes, B, C2, E, vocab):
        loss, u, v = skipgram_reference(U.view(vocab, E), V.view(vocab, E), words.view(B), contexts.view(B, C2), negatives.view(B, C2),
                                        lr, padding_idx, torch.float64)
        touched_u = torch.zeros(vocab, dtype=torch.bool)
        touched_u[words.view(-1)] = True
        touched_v = torch.zeros(vocab, dtype=torch.bool)
        touched_v[contexts.view(-1)] = True
        touched_v[negatives.view(-1)] = True
        if padding_idx >= 0:
            touched_u[padding_idx] = touched_v[padding_idx] = False
        with torch.no_grad():            # untouched rows stay bit-unchanged (no float64 round trip)
            U.view(vocab, E)[touched_u] = u[touched_u].to(U.dtype)
            V.view(vocab, E)[touched_v] = v[touched_v].to(V.dtype)
            loss_out.copy_(loss.to(loss_out.dtype))
        return 0

    def embed_gather_t(self, U, idx, out, B, L, E, vocab):
        out.copy_(F.embedding(idx.view(B, L), U.view(vocab, E)).permute(0, 2, 1))
        return 0

    def embed_lookup(self, U, z, out, B, L, E, vocab):
        out.copy_(torch.argmax(lookup_reference(U.view(vocab, E), z.view(B, E, L)), dim=1))
        return 0


# ----------------------------------------------------------------------------------------------------------- conv cases
CONV_SHAPES = [(3, 5, 7, 1),          # both outer taps are padding
               (2, 3, 64, 4),
               (5, 33, 17, 5),        # ragged everywhere: a tile spans several sequences
               (7, 128, 128, 4),
               (2, 64, 128, 64),
               (1, 8, 8, 300)]        # one sequence longer than a tile


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def conv_case(B, Cin, Cout, L, ks):
    """dict(x, w, bias, residual, gy, gw0, gb0; want = float64 results; e32 = the fp32 ATen errors) for one shape."""
    g = _gen(B, Cin, Cout, L, ks)
    x, gy = torch.randn(B, Cin, L, generator=g), torch.randn(B, Cout, L, generator=g)
    w = torch.randn(Cout, Cin, ks, generator=g) * (2.0 / (Cin * ks)) ** 0.5
    bias, residual = torch.randn(Cout, generator=g), torch.randn(B, Cout, L, generator=g)
    gw0, gb0 = torch.randn(Cout, Cin, ks, generator=g), torch.randn(Cout, generator=g)

    def both(dtype):
        xd, wd, bd = (t.clone().to(dtype).requires_grad_(True) for t in (x, w, bias))
        plain = F.conv1d(xd, wd, None, padding=ks // 2)
        full = F.conv1d(xd, wd, bd, padding=ks // 2) + residual.to(dtype)
        gx, gw, gb = torch.autograd.grad(full, (xd, wd, bd), gy.to(dtype))
        return dict(plain=plain.detach().double(), full=full.detach().double(), gx=gx.double(), gw=gw.double(), gb=gb.double(),
                    gw_acc=(gw0.to(dtype) + gw).double(), gb_acc=(gb0.to(dtype) + gb).double())
    want, r32 = both(torch.float64), both(torch.float32)
    return dict(x=x, w=w, bias=bias, residual=residual, gy=gy, gw0=gw0, gb0=gb0, want=want, e32={k: rel(r32[k], want[k]) for k in want})


# ------------------------------------------------------------------------------------------------------ skip-gram cases
SKIPGRAM_SHAPES = [(1, 2, 1, 2), (4, 6, 8, 23), (5, 4, 100, 7), (128, 6, 64, 1000)]
PLANTED = (0., 30., -30., 90., -90.)


@functools.lru_cache(maxsize=None)
def skipgram_case(B, C2, E, vocab, lr, variant='plain'):
    """variant: 'plain' | 'same_word' (every word equal) | 'padding' (padding_idx 0 is hit by words, contexts and negatives) |
    'planted' (scores of exactly 0, +-30, +-90 on both the context and the negative side; needs B = 5, vocab >= 12)."""
    g = _gen(B, C2, E, vocab, variant)
    U, V = torch.randn(vocab, E, generator=g) * 0.5, torch.randn(vocab, E, generator=g) * 0.5
    words = torch.randint(0, vocab, (B,), generator=g)
    contexts, negatives = torch.randint(0, vocab, (B, C2), generator=g), torch.randint(0, vocab, (B, C2), generator=g)
    padding_idx = -1
    if variant == 'same_word':
        words[:] = int(words[0])
    elif variant == 'padding':
        padding_idx = 0
        U[0] = 0.
        V[0] = 0.                      # (nn.Embedding(padding_idx=0) starts its row at zero; nothing ever moves it)
        words[0] = 0
        contexts[:, -1] = 0
        negatives[0, 0] = 0
    elif variant == 'planted':
        assert B == len(PLANTED) and vocab >= 12
        words = torch.arange(1, B + 1)
        U[1:B + 1] = 0.
        U[1:B + 1, 0] = torch.tensor(PLANTED)
        V[10], V[11] = 0., 0.
        V[10, 0] = V[11, 0] = 1.
        contexts[:], negatives[:] = 10, 11
    want = skipgram_reference(U, V, words, contexts, negatives, lr, padding_idx, torch.float64)
    r32 = skipgram_reference(U, V, words, contexts, negatives, lr, padding_idx, torch.float32)
    return dict(U=U, V=V, words=words, contexts=contexts, negatives=negatives, padding_idx=padding_idx,
                want=tuple(t.double() for t in want), e32=tuple(rel(r, t.double()) for r, t in zip(r32, want)))


def untouched_rows(c, vocab):
    """(rows of U, rows of V) that no index names or that are the padding row: they must come back bit-unchanged."""
    tu, tv = torch.ones(vocab, dtype=torch.bool), torch.ones(vocab, dtype=torch.bool)
    tu[c['words']] = False
    tv[c['contexts'].view(-1)] = False
    tv[c['negatives'].view(-1)] = False
    if c['padding_idx'] >= 0:
        tu[c['padding_idx']] = tv[c['padding_idx']] = True
    return tu, tv


# ---------------------------------------------------------------------------------------------------------- lookup cases
LOOKUP_MARGIN = 1e-3


def lookup_margin(U, z):
    """Smallest relative float64 gap between the best and the second-best score over all columns."""
    top = lookup_reference(U, z).topk(2, dim=1).values
    return float(((top[:, 0] - top[:, 1]) / top[:, 0].abs()).min())


@functools.lru_cache(maxsize=None)
def lookup_case(B, L, E, vocab):
    """Inputs whose float64 top-1 margin is at least LOOKUP_MARGIN relative in every column (the seed is searched for that: a
    property of the inputs alone), and the float64 answer."""
    for attempt in range(64):
        g = _gen(B, L, E, vocab, attempt)
        U, z = torch.randn(vocab, E, generator=g), torch.randn(B, E, L, generator=g)
        if lookup_margin(U, z) >= 2 * LOOKUP_MARGIN:
            return dict(U=U, z=z, want=torch.argmax(lookup_reference(U, z), dim=1))
    raise AssertionError('no seed with the required margin')


# -------------------------------------------------------------------------------------------------------------- fixtures
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TEXT_CASES = ('text_c16_e8_b4', 'text_c32_e16_b4_id', 'text_c16_e64_b2_elu_nogp')
LOSS_KEYS = ('g_loss', 'd_loss', 'gp', 'embedding_loss')


def load_text_fixture(name):
    with open(os.path.join(GOLDEN_DIR, name + '.json')) as f:
        return json.load(f)


def documents(fx, k):
    """The batch of step k: (batch, size) int64 word indexes in [1, vocab) from a seeded RandomState, every second row with a tail
    of zeros (the padding index) of a third of its length."""
    rs = np.random.RandomState(fx['doc_seed'] + k)
    docs = rs.randint(1, fx['flags']['vocab'], (fx['batch'], fx['size'])).astype(np.int64)
    docs[1::2, -(fx['size'] // 3):] = 0
    return torch.from_numpy(docs)


def text_trainer(fx, device, seed=0, **overrides):
    from tartangan_amd.trainers.text_cnn import TextCNNTrainer
    flags = {k: v for k, v in fx['flags'].items() if k != 'vocab'}
    tr = TextCNNTrainer(TextCNNTrainer.default_args(config=fx['config'], batch_size=fx['batch'], device=device, **{**flags, **overrides}))
    torch.manual_seed(seed)
    tr.build_models()
    tr.build_embedding(fx['flags']['vocab'], padding_idx=0)
    return tr


def load_procedural(tr, fx):
    from oracle.procedural import procedural_state
    seed = fx['weight_seed']
    tr.g.load_state_dict(procedural_state(tr.g.state_dict(), seed))
    tr.target_g.load_state_dict(procedural_state(tr.target_g.state_dict(), seed + 1))
    tr.d.load_state_dict(procedural_state(tr.d.state_dict(), seed + 2))
    state = procedural_state(tr.embedding.state_dict(), seed + 3)
    for v in state.values():
        v[0] = 0.
    tr.embedding.load_state_dict(state)


def seed_step_streams(fx):
    torch.manual_seed(fx['rng_seed'])
    np.random.seed(fx['np_seed'])


def total_l2(tensors, grads=False):
    s = 0.
    for p in tensors:
        t = p.grad if grads else p
        if t is not None:
            t = t.coalesce().values() if t.is_sparse else t
            s += float(t.detach().double().pow(2).sum())
    return s ** 0.5


def step_entry(tr, logs):
    """The four losses, the L2 of G, D, the target and both tables, and the gradient L2 of G, D and -- where the trainer keeps
    them (the reference's sparse ``.grad``; this package's fused step has none) -- of both tables."""
    entry = {k: float(logs[k]) for k in LOSS_KEYS}
    u, v = tr.embedding.embedding_u.weight, tr.embedding.embedding_v.weight
    entry.update(g_l2=total_l2(tr.g.parameters()), d_l2=total_l2(tr.d.parameters()), target_g_l2=total_l2(tr.target_g.parameters()),
                 u_l2=total_l2([u]), v_l2=total_l2([v]),
                 g_grad_l2=total_l2(tr.g.parameters(), True), d_grad_l2=total_l2(tr.d.parameters(), True))
    if u.grad is not None:
        entry.update(u_grad_l2=total_l2([u], True), v_grad_l2=total_l2([v], True))
    return entry
